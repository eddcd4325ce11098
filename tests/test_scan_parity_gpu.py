"""Proving-scan hit-set parity: every scan kernel's full (index, nonce) hit
list against the oracle's, at the configurations production runs.

The proof tests elsewhere scan at most 2^21 labels per launch, which keeps
every lane on ILP chain 0 for one loop iteration, use a difficulty that
about 8 bits of the compare decide, and see only the winning nonce's first
k2 indices.  Here POST_SCAN_MAX_BLOCKS caps the grid at two blocks, so a
few thousand labels make every chain live and the grid-stride loop iterate;
crafted ciphertexts sit on both sides of the mainnet difficulty in every
byte lane; the chunked pipeline is crossed with POST_PROVE_CHUNK_LABELS;
and the comparison is the whole sorted hit list, as lists, so a missed,
duplicated or misattributed hit for any nonce fails.

The scan depends on the labels alone, so they are seeded random bytes and
no init session is needed.
"""
import contextlib
import functools
import importlib
import os

import numpy as np
import pytest

import gsm_amd
from oracle import Oracle

proving = importlib.import_module("go-spacemesh_amd.proving")

pytestmark = pytest.mark.gpu

NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
CHALLENGE = bytes(32)
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
NONCES = 16
INDEX_BASE = (1 << 33) + 12345  # the 64-bit add in index_base + ts[u]

# mode -> (threads of a launch capped at 2 blocks, ILP chains per lane).
# tt4 falls back to bankrep's geometry where 128 KiB of dynamic LDS is
# refused; the result is checked against the oracle either way.
MODES = {
    "shared": (512, 2),
    "bankrep": (512, 2),
    "bankrepbg": (512, 2),
    "bankrep512": (1024, 2),
    "bankrep512bg": (1024, 2),
    "tt4": (2048, 4),
}
MODE_IDS = list(MODES)


@contextlib.contextmanager
def scan_env(mode, max_blocks=None, chunk_labels=None):
    want = {"POST_SCAN_MODE": mode,
            "POST_SCAN_MAX_BLOCKS": max_blocks,
            "POST_PROVE_CHUNK_LABELS": chunk_labels}
    saved = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def group_pows():
    return tuple(proving.group_pows(CHALLENGE, NONCES, POW_DIFF))


def random_labels(count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, count * 16, dtype=np.uint8).tobytes()


def gpu_hits(labels, total_labels, k1, cap, index_base=INDEX_BASE):
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total_labels,
                             k1=k1, k2=8, pow_difficulty=POW_DIFF)
    return proving.scan_shard(labels, index_base, total_labels, CHALLENGE,
                              cfg, NONCES, list(group_pows()), cap=cap)


def ref_hits(labels, total_labels, k1, index_base=INDEX_BASE):
    return _oracle().scan_hits(labels, index_base, total_labels, CHALLENGE,
                               k1, NONCES, list(group_pows()))


def segments(count, T, L):
    """[lo, hi) label ranges that one chain covers in one loop iteration of
    a T-thread launch with L chains per lane: iteration k, chain u covers
    k*L*T + u*T + lane for lane < T."""
    out = []
    lo = 0
    while lo < count:
        out.append((lo, min(lo + T, count)))
        lo += T
    return out


# ------------------- a. live chains and loop iterations -------------------

def chain_counts(T, L):
    return [1, T - 1, T + 1, L * T,
            L * T + 1,                    # 2nd iteration: one lane, live = 1
            L * T + T + 37,               # 2nd iteration: ragged chain 1
            3 * L * T + (L - 1) * T + 5]  # 4 iterations, last chain partial


@functools.lru_cache(maxsize=None)
def chain_case(count):
    """(labels, k1, reference hits) for one count; shared by the modes with
    the same geometry and computed once."""
    labels = random_labels(count, 0x5CA0 + count)
    k1 = max(1, count // 8)
    return labels, k1, ref_hits(labels, count, k1)


CHAIN_CASES = [(m, i) for m in MODE_IDS for i in range(7)]


@pytest.mark.parametrize("mode,case", CHAIN_CASES,
                         ids=[f"{m}-{i}" for m, i in CHAIN_CASES])
def test_live_chains_and_iterations(mode, case):
    T, L = MODES[mode]
    count = chain_counts(T, L)[case]
    labels, k1, want = chain_case(count)
    # the input itself: about one (label, nonce) pair in eight hits, and
    # every chain of every iteration contributes at least one hit, so a
    # case cannot pass without that chain's labels having been scanned
    assert len(want) > count
    idx = np.array([h[0] - INDEX_BASE for h in want], dtype=np.int64)
    for lo, hi in segments(count, T, L):
        assert np.any((idx >= lo) & (idx < hi)), (count, lo, hi)
    with scan_env(mode, max_blocks=2):
        got = gpu_hits(labels, count, k1, cap=len(want) + 1024)
    assert sorted(got) == want


# --------------- b. mainnet difficulty on crafted ciphertexts ---------------

MAINNET_K1, MAINNET_TOTAL = 26, 1 << 34
D = 26 << 30  # floor(26 * 2^64 / 2^34)
ALL_FF = (1 << 64) - 1


def _bswap64(v):
    return int.from_bytes(v.to_bytes(8, "little"), "big")


CRAFTED_V = [
    D - 1, D, D + 1, 0,
    (D - 1) | (1 << 40), (D - 1) | (1 << 48), (D - 1) | (1 << 56),
    0x5_FFFFFFFF,
    0x6_7FFFFFFF, 0x6_80000000,
    _bswap64(D - 1),
    ((D - 1) & 0xFFFFFFFF) << 32 | (D - 1) >> 32,
    ALL_FF,  # the only value that misses when the difficulty clamps
]


@functools.lru_cache(maxsize=None)
def crafted_case(T, L):
    """Random filler with one crafted label per (cipher, half, value): the
    label is the decryption, under that cipher's key, of a block whose
    target half is LE64(value) and whose other half is random with its top
    byte 0xFF (a miss at mainnet difficulty).  One crafted label falls in
    each of len(crafted) equal strata of the buffer, narrower than the
    shortest chain segment, so every chain of every iteration gets some.
    Returns (labels, {position: (cipher, half, value)})."""
    o = _oracle()
    count = 2 * L * T + 99
    rng = np.random.default_rng(0xC4AF + T)
    buf = bytearray(random_labels(count, 0xF111 + T))
    keys = [o.cipher_key(CHALLENGE, c, group_pows()[0])
            for c in range(NONCES // 2)]
    crafted = [(c, j, v) for c in range(NONCES // 2) for j in (0, 1)
               for v in CRAFTED_V]
    order = rng.permutation(len(crafted))
    placed = {}
    for s, k in enumerate(order):
        c, j, v = crafted[k]
        lo = count * s // len(crafted)
        hi = count * (s + 1) // len(crafted)
        pos = int(rng.integers(lo, hi))
        other = bytearray(rng.integers(0, 256, 8, dtype=np.uint8).tobytes())
        other[7] = 0xFF
        half = v.to_bytes(8, "little")
        ct = half + bytes(other) if j == 0 else bytes(other) + half
        buf[16 * pos:16 * pos + 16] = o.aes128_dec(keys[c], ct)
        placed[pos] = (c, j, v)
    return bytes(buf), placed


@functools.lru_cache(maxsize=None)
def crafted_ref(T, L, k1, total):
    labels, _ = crafted_case(T, L)
    return ref_hits(labels, total, k1)


@pytest.mark.parametrize("mode", MODE_IDS)
def test_mainnet_difficulty_crafted(mode):
    T, L = MODES[mode]
    labels, placed = crafted_case(T, L)
    count = len(labels) // 16
    assert _oracle().lib.oracle_proving_difficulty(MAINNET_K1,
                                                   MAINNET_TOTAL) == D
    for lo, hi in segments(count, T, L):
        assert any(lo <= p < hi for p in placed), (lo, hi)
    want = crafted_ref(T, L, MAINNET_K1, MAINNET_TOTAL)
    # the test's own design: on the crafted (position, nonce) pairs the
    # reference hits exactly where value < D
    want_set = set(want)
    assert len(want_set) == len(want)
    for pos, (c, j, v) in placed.items():
        assert ((INDEX_BASE + pos, 2 * c + j) in want_set) == (v < D), \
            (pos, c, j, hex(v))
    assert len(want) >= 4 * NONCES
    with scan_env(mode, max_blocks=2):
        got = gpu_hits(labels, MAINNET_TOTAL, MAINNET_K1,
                       cap=len(want) + 1024)
    assert sorted(got) == want


@pytest.mark.parametrize("mode", MODE_IDS)
def test_clamped_difficulty_crafted(mode):
    """k1 == total_labels clamps the difficulty to UINT64_MAX: only an
    all-0xFF half misses."""
    T, L = MODES[mode]
    labels, placed = crafted_case(T, L)
    count = len(labels) // 16
    assert _oracle().lib.oracle_proving_difficulty(37, 37) == ALL_FF
    want = crafted_ref(T, L, 37, 37)
    misses = {(INDEX_BASE + pos, 2 * c + j)
              for pos, (c, j, v) in placed.items() if v == ALL_FF}
    assert len(misses) == NONCES
    assert want == [(INDEX_BASE + i, n) for i in range(count)
                    for n in range(NONCES)
                    if (INDEX_BASE + i, n) not in misses]
    with scan_env(mode, max_blocks=2):
        got = gpu_hits(labels, 37, 37, cap=count * NONCES + 1024)
    assert sorted(got) == want


# ----------------------- c. production grid, uncapped -----------------------

@pytest.fixture(scope="module")
def full_grid_case():
    count = (1 << 21) + (1 << 10) + 37  # chain 1 live in the first 1061 lanes
    labels = random_labels(count, 0xF0071)
    k1 = count // 64
    return labels, count, k1, ref_hits(labels, count, k1)


@pytest.mark.parametrize("mode", ["shared", "bankrep", "tt4"])
def test_production_grid_uncapped(mode, full_grid_case):
    labels, count, k1, want = full_grid_case
    idx = np.array([h[0] - INDEX_BASE for h in want], dtype=np.int64)
    assert np.any(idx >= 1 << 21) and np.any(idx < 1 << 21)
    with scan_env(mode):
        got = gpu_hits(labels, count, k1, cap=len(want) + 1024)
    assert sorted(got) == want


# --------------------------- d. chunked pipeline ---------------------------

CHUNK = 4096
CHUNKED_COUNT = 4 * CHUNK + 1500


@functools.lru_cache(maxsize=None)
def chunked_case():
    labels = random_labels(CHUNKED_COUNT, 0xC40C)
    want = _oracle().scan_hits(labels, 0, CHUNKED_COUNT, CHALLENGE, 12,
                               NONCES, list(group_pows()))
    proof = _oracle().prove(labels, CHUNKED_COUNT, CHALLENGE, 12, 8, NONCES,
                            POW_DIFF)  # raises if no nonce reached k2
    return labels, want, proof


@pytest.mark.parametrize("mode", MODE_IDS)
def test_chunked_scan_and_prove(mode):
    labels, want, op = chunked_case()
    # hits in every one of the five chunks, or a chunk could go unscanned
    assert {h[0] // CHUNK for h in want} == set(range(5))
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=CHUNKED_COUNT,
                             k1=12, k2=8, pow_difficulty=POW_DIFF)
    with scan_env(mode, chunk_labels=CHUNK):
        got = gpu_hits(labels, CHUNKED_COUNT, 12, cap=len(want) + 1024,
                       index_base=0)
        proof = gsm_amd.api.prove_buffer(labels, CHUNKED_COUNT, NODE, ATX,
                                         CHALLENGE, cfg,
                                         gsm_amd.ProveOpts(nonces=NONCES))
    assert sorted(got) == want
    assert (proof.nonce, proof.pow) == (op.nonce, op.pow)
    assert proof.indices == bytes(op.indices[:op.indices_len])


# -------------------------------- e. hit cap --------------------------------

@pytest.mark.parametrize("mode", MODE_IDS)
def test_hit_cap_overflow_leaves_no_state(mode):
    count = 3001
    labels, k1, want = chain_case(count)
    assert len(want) > 8
    with scan_env(mode, max_blocks=2):
        with pytest.raises(gsm_amd.EngineError) as ei:
            gpu_hits(labels, count, k1, cap=8)
        assert "overflow" in str(ei.value)
        got = gpu_hits(labels, count, k1, cap=len(want) + 1024)
    assert sorted(got) == want


# ----------------------------- f. unknown mode -----------------------------

def test_unknown_mode_runs_the_fallback():
    """A POST_SCAN_MODE that is none of the six names runs the default
    fallback (bankrep)."""
    labels, k1, want = chain_case(3001)
    with scan_env("fastest", max_blocks=2):
        got = gpu_hits(labels, 3001, k1, cap=len(want) + 1024)
    assert sorted(got) == want
