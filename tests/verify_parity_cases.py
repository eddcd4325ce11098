"""Inputs and oracle-side expectations of the verification parity tests.

tests/test_verify_parity_gpu.py feeds these cases to the engine;
tests/test_verify_parity_cpu.py pins, without a GPU, that the expectations
are what `oracle.verify` says and that the cases hold the verdicts they are
meant to hold.  Every expected value is computed by the oracle (`aes128`,
`aes128_dec`, `cipher_key`, `oracle_proving_difficulty`, `verify`,
`verify_vrf_nonce`, `scan_hits`); nothing here imports the engine except
`slots_child`, the body of the child process of the scratch-slot test.

A proof here need not win anything: it is k2 indices, a nonce and a pow
valid for (challenge, nonce / 16).  Labels are made at scrypt N = 2.
"""
import functools
import json
import os

import numpy as np

from oracle import Oracle, Proof, make_meta

POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31  # accepts one pow in 16
N = 2
K2 = 37
ALL_FF = (1 << 64) - 1
MAINNET_K1, MAINNET_TOTAL = 26, 1 << 34
D_MAINNET = 26 << 30  # floor(26 * 2^64 / 2^34)
T = 256  # threads per block of the predicate kernel

# oracle_verify's codes -> the engine's Status values
ST_OK, ST_ARGS, ST_POW, ST_INDEX = 0, 2, 7, 8
FROM_ORACLE = {0: ST_OK, 1: ST_INDEX, 2: ST_POW, 3: ST_ARGS}

IDENTITIES = [(bytes([0xA5]) * 32, bytes([0x5A]) * 32),
              (bytes(range(32)), bytes(range(32, 64))),
              (bytes([0x11]) * 32, bytes([0xEE]) * 32)]
CHALLENGES = [bytes(32), bytes(range(100, 132))]


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


def difficulty(k1, num_labels):
    return oracle().lib.oracle_proving_difficulty(k1, num_labels)


def pred(key, label16, half, D):
    """The predicate restated: the nonce's little-endian u64 of
    AES(key, label[:16]) is below the difficulty."""
    ct = oracle().aes128(key, label16)
    return int.from_bytes(ct[8 * half:8 * half + 8], "little") < D


@functools.lru_cache(maxsize=None)
def find_pow(challenge, group, start=0):
    p = start
    while oracle().lib.oracle_k2pow_verify(challenge, group, p, POW_DIFF):
        p += 1
    return p


def proof_key(challenge, nonce, pow_):
    return oracle().cipher_key(challenge, nonce // 2, pow_)


@functools.lru_cache(maxsize=None)
def label_table(ident, count):
    """The first `count` 16-byte labels of an identity."""
    node, atx = IDENTITIES[ident]
    labels, _ = oracle().init_range(oracle().commitment(node, atx), 0, count,
                                    N, with_nonce=False)
    return labels


def pack(indices, num_labels):
    bpi = oracle().lib.oracle_bits_per_index(num_labels)
    from ctypes import c_uint64, create_string_buffer
    out = create_string_buffer(800)
    n = oracle().lib.oracle_pack_indices(
        (c_uint64 * len(indices))(*indices), len(indices), bpi, out)
    assert n == (len(indices) * bpi + 7) // 8
    return out.raw[:n]


class Case:
    """One proof with its metadata, in the plain form both sides build
    their structs from."""

    def __init__(self, ident, challenge, num_units, lpu, nonce, pow_, packed,
                 num_indices=K2):
        self.ident, self.challenge = ident, challenge
        self.num_units, self.lpu = num_units, lpu
        self.nonce, self.pow, self.packed = nonce, pow_, packed
        self.num_indices = num_indices

    def o_proof(self):
        p = Proof()
        p.nonce, p.pow = self.nonce, self.pow
        p.num_indices = self.num_indices
        p.indices_len = len(self.packed)
        for i, b in enumerate(self.packed):
            p.indices[i] = b
        return p

    def o_meta(self):
        node, atx = IDENTITIES[self.ident]
        return make_meta(node, atx, self.challenge, self.num_units, self.lpu)

    def expect(self, k1, k2=K2, k3=K2, seed=None, selected=-1):
        """(engine status, invalid_index or None) as `oracle.verify` has
        it.  The position is compared only where the oracle reports one."""
        rc, inv = oracle().verify(self.o_proof(), self.o_meta(), N, k1, k2,
                                  k3, seed, selected, POW_DIFF)
        return FROM_ORACLE[rc], (inv if rc == 1 else None)


def passing_and_failing(ident, challenge, nonce, pow_, num_labels, k1):
    """Indices of the identity whose label passes / fails this proof's
    predicate."""
    tab = label_table(ident, num_labels)
    key = proof_key(challenge, nonce, pow_)
    D = difficulty(k1, num_labels)
    ok = [pred(key, tab[16 * i:16 * i + 16], nonce % 2, D)
          for i in range(num_labels)]
    return ([i for i in range(num_labels) if ok[i]],
            [i for i in range(num_labels) if not ok[i]])


# --------------------- predicate kernel: crafted blocks ---------------------

def _bswap64(v):
    return int.from_bytes(v.to_bytes(8, "little"), "big")


def _wswap64(v):
    return (v & 0xFFFFFFFF) << 32 | v >> 32


def crafted_values():
    """Values of the selected u64 around D = 0x6_80000000.  Bytes 0-2 of D
    are zero, so no single value makes one of them decide alone; their
    traps pass only while the byte stays below byte 3, and the byte- and
    word-swapped forms of every passing trap fail unless the order is
    wrong.  Byte 3: 0x7F / 0x80 under byte 4 = 6.  Byte 4: 5 over all-ones,
    7 over zeros.  Bytes 5-7: D - 1 with one bit set in that byte."""
    D = D_MAINNET
    vals = [D - 1, D, D + 1, 0, ALL_FF]
    low = [0x6_7F000000 | 0xFF << 8 * i for i in range(3)]      # bytes 0-2
    vals += low
    vals += [0x6_7FFFFFFF, 0x6_80000000]                        # byte 3
    vals += [0x5_FFFFFFFF, 0x7_00000000]                        # byte 4
    vals += [(D - 1) | 1 << 8 * i for i in (5, 6, 7)]           # bytes 5-7
    passing = low + [D - 1, 0x5_FFFFFFFF]
    vals += [_bswap64(v) for v in passing]
    vals += [_wswap64(v) for v in passing]
    vals += [ALL_FF - 1]
    return vals


@functools.lru_cache(maxsize=None)
def crafted_case():
    """8 keys x 2 halves x {mainnet D, the UINT64_MAX clamp} as 32 proofs;
    one task per (proof, value).  The label is the decryption of a block
    whose selected half is LE64(value) and whose other half holds the
    opposite verdict, followed by 16 junk bytes.
    Returns (labels, keys, halves, diffs, task_proof, values)."""
    o = oracle()
    rng = np.random.default_rng(0xC4AF)
    pow_ = find_pow(CHALLENGES[0], 0)
    ckeys = [o.cipher_key(CHALLENGES[0], c, pow_) for c in range(8)]
    keys, halves, diffs = [], [], []
    for D in (D_MAINNET, ALL_FF):
        for k in ckeys:
            for h in (0, 1):
                keys.append(k)
                halves.append(h)
                diffs.append(D)
    tasks = [(p, v) for p in range(len(keys)) for v in crafted_values()]
    order = rng.permutation(len(tasks))
    labels, task_proof, values = [], [], []
    for t in order:
        p, v = tasks[t]
        D = diffs[p]
        if v < D:  # the other half fails
            other = ALL_FF if D == ALL_FF else \
                int(rng.integers(0, 1 << 56)) | 0xFF << 56
        else:      # the other half passes
            other = int(rng.integers(0, D_MAINNET))
        sel, oth = v.to_bytes(8, "little"), other.to_bytes(8, "little")
        ct = sel + oth if halves[p] == 0 else oth + sel
        junk = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        labels.append(o.aes128_dec(keys[p], ct) + junk)
        task_proof.append(p)
        values.append(v)
    return b"".join(labels), keys, halves, diffs, task_proof, values


def pred_expected(labels, keys, halves, diffs, task_proof):
    return bytes(
        1 if pred(keys[p], labels[32 * t:32 * t + 16], halves[p], diffs[p])
        else 0 for t, p in enumerate(task_proof))


# --------------------- predicate kernel: per-proof tables ---------------------

TABLE_SHAPES = [2048, 2100, 2049, 5000, 4000000001]  # num_labels; k1 < 2^32


@functools.lru_cache(maxsize=None)
def tables_case():
    """300 proofs with their own key, half and difficulty (all near 2^63,
    from `oracle_proving_difficulty` at k1 about num_labels / 2; only 2048
    gives zero low bytes), 3000 random labels, a shuffled task -> proof map
    in which every proof has ten tasks.
    Returns (labels, keys, halves, diffs, task_proof, expected)."""
    rng = np.random.default_rng(0x7AB1E5)
    n, count = 300, 3000
    keys = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            for _ in range(n)]
    assert len(set(keys)) == n
    halves = [int(h) for h in rng.integers(0, 2, n)]
    diffs = []
    for p in range(n):
        nl = TABLE_SHAPES[p % len(TABLE_SHAPES)]
        k1 = nl // 2 + int(rng.integers(-nl // 64, nl // 64 + 1))
        diffs.append(difficulty(k1, nl))
    labels = rng.integers(0, 256, count * 32, dtype=np.uint8).tobytes()
    task_proof = [int(p) for p in rng.permutation(np.arange(count) % n)]
    want = pred_expected(labels, keys, halves, diffs, task_proof)
    return labels, keys, halves, diffs, task_proof, want


STRIDE_COUNTS = [1, T - 1, T + 1, 2 * T, 2 * T + 1, 5 * 2 * T + 37]


# --------------------------- batch path: proofs ---------------------------

# (num_units, labels_per_unit): 10, 11 and 12 bits per index, the middle
# one not a power of two
SHAPES = [(2, 510), (5, 206), (3, 683)]
HET_K1 = 600  # D / 2^64 = 0.59, 0.58, 0.29
NONCES = [0, 1, 2, 3, 5, 16, 19, 30]  # both halves, 6 ciphers, 2 pow groups


def _random_case(rng, kind):
    ident = int(rng.integers(0, len(IDENTITIES)))
    challenge = CHALLENGES[int(rng.integers(0, len(CHALLENGES)))]
    nu, lpu = SHAPES[int(rng.integers(0, len(SHAPES)))]
    nl = nu * lpu
    nonce = NONCES[int(rng.integers(0, len(NONCES)))]
    pow_ = find_pow(challenge, nonce // 16, int(rng.integers(0, 4)) * 1000)
    if kind in ("passing", "late"):
        ok, bad = passing_and_failing(ident, challenge, nonce, pow_, nl,
                                      HET_K1)
        idx = [ok[int(i)] for i in rng.integers(0, len(ok), K2)]
        if kind == "late":
            for pos in rng.choice(K2, 2, replace=False):
                idx[int(pos)] = bad[int(rng.integers(0, len(bad)))]
    else:
        idx = [int(i) for i in rng.integers(0, nl, K2)]
    c = Case(ident, challenge, nu, lpu, nonce, pow_, pack(idx, nl))
    if kind == "pow":
        c.pow += 1
        while oracle().lib.oracle_k2pow_verify(challenge, nonce // 16, c.pow,
                                               POW_DIFF) == 0:
            c.pow += 1
    elif kind == "shape_len":      # packed for another bits-per-index
        c.packed = pack(idx, 4 * nl)
    elif kind == "shape_count":
        c.num_indices = K2 - 1
    elif kind == "zero_units":
        c.num_units = 0
    elif kind == "zero_lpu":
        c.lpu = 0
    return c


@functools.lru_cache(maxsize=None)
def heterogeneous_batch():
    """200 proofs, interleaved: random indices, all-passing indices,
    passing with two failures planted, and rejects by pow, by shape and by
    num_labels == 0."""
    rng = np.random.default_rng(0x4E7E)
    kinds = (["random"] * 8 + ["passing"] * 3 + ["late"] * 3 +
             ["pow", "shape_len", "shape_count", "zero_units", "zero_lpu",
              "pow"])
    return [_random_case(rng, kinds[int(rng.integers(0, len(kinds)))])
            for _ in range(200)]


@functools.lru_cache(maxsize=None)
def position_case():
    """One proof of random indices under D = 2^63."""
    rng = np.random.default_rng(0x9051)
    nl = 2048
    idx = [int(i) for i in rng.integers(0, nl, K2)]
    pow_ = find_pow(CHALLENGES[1], 1)
    return Case(1, CHALLENGES[1], 2, 1024, 19, pow_, pack(idx, nl)), nl // 2


SUBSET_K3 = [1, 3, K2 - 1]
SUBSET_SEEDS = [bytes([s]) * 8 + b"peer" for s in range(8)]


@functools.lru_cache(maxsize=None)
def subset_batch():
    """Eight proofs (one per seed), each all-passing but for three
    failures planted at random positions; returns (cases, k1)."""
    rng = np.random.default_rng(0x5B5E7)
    nu, lpu = SHAPES[1]
    cases = []
    for s in range(len(SUBSET_SEEDS)):
        ident = s % len(IDENTITIES)
        challenge = CHALLENGES[s % 2]
        nonce = NONCES[s % len(NONCES)]
        pow_ = find_pow(challenge, nonce // 16)
        ok, bad = passing_and_failing(ident, challenge, nonce, pow_,
                                      nu * lpu, HET_K1)
        idx = [ok[int(i)] for i in rng.integers(0, len(ok), K2)]
        for pos in rng.choice(K2, 3, replace=False):
            idx[int(pos)] = bad[int(rng.integers(0, len(bad)))]
        cases.append(Case(ident, challenge, nu, lpu, nonce, pow_,
                          pack(idx, nu * lpu)))
    return cases, HET_K1


def subset_positions(k3, seed):
    from ctypes import c_uint32
    out = (c_uint32 * K2)()
    oracle().lib.oracle_subset(K2, k3, seed, len(seed), out)
    return list(out[:k3])


def failing_positions(case, k1):
    return [pos for pos in range(K2)
            if case.expect(k1, selected=pos)[0] != ST_OK]


# order of failure: (positions failing the threshold, positions out of range)
ORDER_PLANS = [([1], [5]),        # threshold first
               ([9], [2]),        # out of range first
               ([], [4, 20]),     # two out of range
               ([], [0]),         # nothing before it
               ([36], [35]),      # both at the end
               ([3, 30], [17])]
ORDER_SEEDS = [b"order-%d" % s for s in range(6)]


@functools.lru_cache(maxsize=None)
def order_batch():
    """All-passing proofs over 5 * 206 = 1030 labels (11 bits per index, so
    1030..2047 are out of range) with the plan's failures planted."""
    rng = np.random.default_rng(0x0DE4)
    nu, lpu = SHAPES[1]
    nl = nu * lpu
    cases = []
    for n, (aes_bad, oor) in enumerate(ORDER_PLANS):
        ident, challenge = n % len(IDENTITIES), CHALLENGES[n % 2]
        nonce = NONCES[(n + 3) % len(NONCES)]
        pow_ = find_pow(challenge, nonce // 16)
        ok, bad = passing_and_failing(ident, challenge, nonce, pow_, nl,
                                      HET_K1)
        idx = [ok[int(i)] for i in rng.integers(0, len(ok), K2)]
        for pos in aes_bad:
            idx[pos] = bad[int(rng.integers(0, len(bad)))]
        for pos in oor:
            idx[pos] = int(rng.integers(nl, 2048))
        cases.append(Case(ident, challenge, nu, lpu, nonce, pow_,
                          pack(idx, nl)))
    return cases, HET_K1


# ------------------- batch path: more tasks than scratch slots -------------------

SLOTS_K2 = 8
SLOTS_TASKS = 140 * 1024
SLOTS_NONCES = 16


def slots_batch(tasks):
    """tasks / 8 proofs over one identity and one challenge; proof p holds
    the contiguous indices [8p, 8p + 8) and nonce p % 16.
    Returns (cases, k1, num_labels)."""
    assert tasks % SLOTS_K2 == 0
    pow_ = find_pow(CHALLENGES[0], 0)
    k1 = 3 * tasks // 4  # three labels in four pass, one proof in ten
    cases = [Case(0, CHALLENGES[0], 1, tasks, p % SLOTS_NONCES, pow_,
                  pack(list(range(SLOTS_K2 * p, SLOTS_K2 * p + SLOTS_K2)),
                       tasks), SLOTS_K2)
             for p in range(tasks // SLOTS_K2)]
    return cases, k1, tasks


def slots_expected(tasks):
    """(statuses, invalid positions) of `slots_batch(tasks)` from one
    `init_range` and one `scan_hits`: a proof fails at the first of its
    labels that is no hit for its nonce."""
    o = oracle()
    pow_ = find_pow(CHALLENGES[0], 0)
    labels = label_table(0, tasks)
    hits = o.scan_hits(labels, 0, tasks, CHALLENGES[0], 3 * tasks // 4,
                       SLOTS_NONCES, [pow_])
    hit = np.zeros((tasks, SLOTS_NONCES), dtype=bool)
    arr = np.array(hits, dtype=np.int64).reshape(-1, 2)
    hit[arr[:, 0], arr[:, 1]] = True
    n = tasks // SLOTS_K2
    nonce = np.arange(n) % SLOTS_NONCES
    mine = hit.reshape(n, SLOTS_K2, SLOTS_NONCES)[np.arange(n), :, nonce]
    miss = ~mine
    status = np.where(miss.any(axis=1), ST_INDEX, ST_OK)
    return status.tolist(), miss.argmax(axis=1).tolist()


def engine_verify(cases, k1, k2=K2, k3=None, seeds=None, selected=-1,
                  seed=None):
    """[(status, invalid_index)] from `post_verify_batch[_seeded]`."""
    import gsm_amd
    cfg = gsm_amd.PostConfig(k1=k1, k2=k2, k3=k2 if k3 is None else k3,
                             pow_difficulty=POW_DIFF)
    ver = gsm_amd.PostVerifier(cfg, scrypt_n=N)
    proofs = [gsm_amd.PostProof(c.nonce, c.packed, c.pow) for c in cases]
    metas = [gsm_amd.PostProofMetadata(*IDENTITIES[c.ident], c.challenge,
                                       c.num_units, c.lpu) for c in cases]
    cps, cms, n = ver.marshal_batch(proofs, metas)
    for i, c in enumerate(cases):
        cps[i].num_indices = c.num_indices
    opts = gsm_amd.VerifyOpts(subset_seed=seed, selected_index=selected)
    got = ver.verify_batch(None, None, opts, seeds=seeds,
                           marshalled=(cps, cms, n))
    return [(int(s), int(i)) for s, i in got]


def slots_child():
    """Body of the child process: verify the batch, print the verdicts."""
    cases, k1, _ = slots_batch(int(os.environ["VERIFY_PARITY_TASKS"]))
    got = engine_verify(cases, k1, k2=SLOTS_K2)
    print("VERDICTS " + json.dumps(got))


# ------------------------------ VRF nonce ------------------------------

VRF_NUM_LABELS = [16, 32, 64, 4096]


@functools.lru_cache(maxsize=None)
def vrf_cases():
    """{num_labels: (identity, [(index, oracle verdict)] * 64)}: every
    passing index below 4096 (the first 32 of them), filled up with the
    lowest failing ones, and one index past 2^32."""
    o = oracle()
    out = {}
    for n, nl in enumerate(VRF_NUM_LABELS):
        ident = n % len(IDENTITIES)
        node, atx = IDENTITIES[ident]
        meta = make_meta(node, atx, bytes(32), 1, nl)
        verdict = {i: o.verify_vrf_nonce(meta, i, N)
                   for i in list(range(4096)) + [(1 << 32) + 17]}
        ok = [i for i in range(4096) if verdict[i] == 0][:32]
        bad = [i for i in range(4096) if verdict[i] != 0]
        picked = sorted(ok + bad[:63 - len(ok)]) + [(1 << 32) + 17]
        if len(picked) < 64:  # everything passes
            picked = list(range(63)) + [(1 << 32) + 17]
        out[nl] = (ident, [(i, verdict[i]) for i in picked])
    return out
