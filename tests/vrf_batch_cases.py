"""Inputs and oracle-side expectations of the batched VRF-nonce tests.

tests/test_vrf_batch_gpu.py feeds these cases to the engine;
tests/test_vrf_batch_cpu.py pins, without a GPU, that the expectations are
what the oracle says and that every group holds both verdicts.  A threshold
is `oracle_vrf_difficulty`, a label is `oracle.label`, a verdict is
`oracle.verify_vrf_nonce` or `label < threshold` on `bytes`; nothing here
imports the engine except `engine_verify_mixed` and `lanes_child`, which
only carry cases to it.
"""
import functools
import json
import os
from ctypes import create_string_buffer

import numpy as np

from oracle import make_meta

import verify_parity_cases as vc

N = vc.N
ST_OK, ST_ARGS, ST_INDEX = vc.ST_OK, vc.ST_ARGS, vc.ST_INDEX
FROM_ORACLE = {0: ST_OK, 1: ST_INDEX}
ALL_00, ALL_FF = bytes(32), bytes([0xFF]) * 32


def threshold(num_labels):
    out = create_string_buffer(32)
    vc.oracle().lib.oracle_vrf_difficulty(num_labels, out)
    return out.raw


def pred(label, thr):
    """The predicate restated: strictly below, as 32-byte big-endian
    numbers (which is how Python orders `bytes` of equal length)."""
    assert len(label) == 32 and len(thr) == 32
    return label < thr


# --------------------- predicate kernel: crafted labels ---------------------

# mainnet (00 00 00 04 00...), one with no zero byte pattern, the clamp
CRAFTED_NUM_LABELS = [1 << 34, 4000000001, 16]


def swap_bytes_in_words(b):
    return b"".join(b[i:i + 4][::-1] for i in range(0, 32, 4))


def swap_words_in_u64(b):
    return b"".join(b[i + 4:i + 8] + b[i:i + 4] for i in range(0, 32, 8))


def swap_halves(b):
    return b[16:] + b[:16]


SWAPS = [swap_bytes_in_words, swap_words_in_u64, swap_halves]


def crafted_base(thr):
    """Labels around one threshold: the threshold itself, its neighbours as
    numbers, and for every byte position a label that equals the threshold
    before it and is lower (higher) at it, with every later byte at the
    opposite extreme; all-zero and all-0xFF."""
    t = int.from_bytes(thr, "big")
    out = [thr, ALL_00, ALL_FF]
    if t > 0:
        out.append((t - 1).to_bytes(32, "big"))
    if t < (1 << 256) - 1:
        out.append((t + 1).to_bytes(32, "big"))
    for b in range(32):
        if thr[b] > 0:
            out.append(thr[:b] + bytes([thr[b] - 1]) + b"\xFF" * (31 - b))
        if thr[b] < 255:
            out.append(thr[:b] + bytes([thr[b] + 1]) + b"\x00" * (31 - b))
    return out


def swapped_traps(thr):
    """(swap, label) for every base label and its swapped form for which a
    compare made in that swapped byte order gives the opposite verdict."""
    out = []
    for f in SWAPS:
        for lab in crafted_base(thr):
            for cand in (lab, f(lab)):
                if pred(f(cand), f(thr)) != pred(cand, thr):
                    out.append((f, cand))
    return out


@functools.lru_cache(maxsize=None)
def crafted_case():
    """(labels, thresholds, task_thr, expected) over the three thresholds,
    tasks shuffled."""
    thrs = [threshold(nl) for nl in CRAFTED_NUM_LABELS]
    tasks = []
    for s, thr in enumerate(thrs):
        labs = crafted_base(thr) + [lab for _, lab in swapped_traps(thr)]
        tasks += [(s, lab) for lab in dict.fromkeys(labs)]
    rng = np.random.default_rng(0x7F1)
    tasks = [tasks[int(i)] for i in rng.permutation(len(tasks))]
    labels = b"".join(lab for _, lab in tasks)
    task_thr = [s for s, _ in tasks]
    want = bytes(1 if pred(lab, thrs[s]) else 0 for s, lab in tasks)
    return labels, thrs, task_thr, want


# --------------------- predicate kernel: map and grid ---------------------

TABLE_NUM_LABELS = list(range(3, 303))  # 14 clamped, most no power of two


@functools.lru_cache(maxsize=None)
def tables_case():
    """300 thresholds of distinct num_labels (a random label passes one in
    16 / num_labels times), 3000 random labels, a shuffled task -> threshold
    map in which every threshold has ten tasks.
    Returns (labels, thresholds, task_thr, expected)."""
    rng = np.random.default_rng(0x7AB1E6)
    n, count = len(TABLE_NUM_LABELS), 3000
    thrs = [threshold(nl) for nl in TABLE_NUM_LABELS]
    labels = rng.integers(0, 256, count * 32, dtype=np.uint8).tobytes()
    task_thr = [int(p) for p in rng.permutation(np.arange(count) % n)]
    want = bytes(1 if pred(labels[32 * t:32 * t + 32], thrs[s]) else 0
                 for t, s in enumerate(task_thr))
    return labels, thrs, task_thr, want


STRIDE_COUNTS = vc.STRIDE_COUNTS  # 1, 255, 257, 512, 513, 5 * 512 + 37


# ------------------------------ batch path ------------------------------

@functools.lru_cache(maxsize=None)
def vrf_items():
    """All 4 x 64 picks of `vrf_cases()` as (identity, num_labels, index,
    engine status), in the order of VRF_NUM_LABELS."""
    cases = vc.vrf_cases()
    return [(cases[nl][0], nl, i, FROM_ORACLE[v])
            for nl in vc.VRF_NUM_LABELS for i, v in cases[nl][1]]


def interleaved(items):
    """One item of each quarter in turn."""
    q = len(items) // 4
    return [items[k * q + i] for i in range(q) for k in range(4)]


def o_meta(ident, num_labels):
    node, atx = vc.IDENTITIES[ident]
    return make_meta(node, atx, bytes(32), 1, num_labels)


def e_meta(ident, num_labels):
    import gsm_amd
    return gsm_amd.PostProofMetadata(*vc.IDENTITIES[ident], bytes(32), 1,
                                     num_labels)


def e_vrf(items):
    """(metas, indices) of items for the engine's Python mirror."""
    return ([e_meta(ident, nl) for ident, nl, _, _ in items],
            [i for _, _, i, _ in items])


def bad_pow_batch():
    """The heterogeneous batch with every pow made invalid: no proof gets as
    far as a label."""
    out = []
    for c in vc.heterogeneous_batch():
        pow_ = c.pow + 1
        while vc.oracle().lib.oracle_k2pow_verify(
                c.challenge, c.nonce // 16, pow_, vc.POW_DIFF) == 0:
            pow_ += 1
        out.append(vc.Case(c.ident, c.challenge, c.num_units, c.lpu, c.nonce,
                           pow_, c.packed, c.num_indices))
    return out


def engine_verify_mixed(cases, k1, vrf, k2=vc.K2, seeds=None):
    """([(status, invalid_index)], [vrf status]) from
    `post_verify_batch_vrf`; `vrf` is (metas, indices) or a marshalled
    triple."""
    import gsm_amd
    cfg = gsm_amd.PostConfig(k1=k1, k2=k2, k3=k2, pow_difficulty=vc.POW_DIFF)
    ver = gsm_amd.PostVerifier(cfg, scrypt_n=N)
    proofs = [gsm_amd.PostProof(c.nonce, c.packed, c.pow) for c in cases]
    metas = [gsm_amd.PostProofMetadata(*vc.IDENTITIES[c.ident], c.challenge,
                                       c.num_units, c.lpu) for c in cases]
    cps, cms, n = ver.marshal_batch(proofs, metas)
    for i, c in enumerate(cases):
        cps[i].num_indices = c.num_indices
    got, vgot = ver.verify_batch(None, None, gsm_amd.VerifyOpts(),
                                 seeds=seeds, marshalled=(cps, cms, n),
                                 vrf=vrf)
    return [(int(s), int(i)) for s, i in got], [int(s) for s in vgot]


# ------------------- batch path: more tasks than scratch lanes -------------------

LANES_PROOF_TASKS = 64          # 8 proofs of vc.slots_batch
LANES_VRF_ITEMS = 140 * 1024    # as many as vc.SLOTS_TASKS: past every lane
LANES_IDENT, LANES_NUM_LABELS = 1, 64   # threshold 0x40 00...: one in four


def lanes_expected(count):
    """Oracle verdicts of indices 0 .. count - 1."""
    o, meta = vc.oracle(), o_meta(LANES_IDENT, LANES_NUM_LABELS)
    return [FROM_ORACLE[o.verify_vrf_nonce(meta, i, N)] for i in range(count)]


def lanes_child():
    """Body of the child process: verify the batch, print the verdicts."""
    import ctypes
    import gsm_amd
    count = int(os.environ["VRF_BATCH_ITEMS"])
    cases, k1, _ = vc.slots_batch(LANES_PROOF_TASKS)
    one = e_meta(LANES_IDENT, LANES_NUM_LABELS).to_c()
    cms = (gsm_amd.api.CProofMetadata * count).from_buffer_copy(
        bytes(one) * count)
    idx = (ctypes.c_uint64 * count)(*range(count))
    got, vgot = engine_verify_mixed(cases, k1, (cms, idx, count),
                                    k2=vc.SLOTS_K2)
    print("VERDICTS " + json.dumps([got, vgot]))
