"""Lean lookup-gap-1 ROMix kernel vs the CPU oracle, byte for byte.

The gap-1 kernel addresses its scratch with 24-bit multiplies off a per-quad
base pointer and folds `X ^= V` into the first salsa input; the generic
kernel serves POST_GAP_SHIFT > 0 and scratch geometries outside the lean
kernel's range.  Shapes are the smallest at which each of those can go
wrong.  All label comparisons are over every byte the engine returns.
"""
import ctypes
import os
import subprocess
import sys

import pytest

import gsm_amd
from oracle import Oracle, Proof, make_meta

gpu = pytest.mark.gpu

NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
NODE2 = bytes([0x3C]) * 32
CHALLENGE = bytes(32)
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_labels(count, scrypt_n, num_units=1, lpu=None, **kw):
    cfg = gsm_amd.PostConfig(min_num_units=1,
                             labels_per_unit=lpu if lpu else count,
                             k1=12, k2=8, k3=4, pow_difficulty=POW_DIFF)
    kw.setdefault("scratch_bytes", 1 << 30)
    opts = gsm_amd.PostSetupOpts(num_units=num_units, scrypt_n=scrypt_n, **kw)
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
    mgr.prepare_initializer()
    mgr.start_session()
    try:
        return mgr.copy_labels(0, count), mgr.vrf_nonce()
    finally:
        mgr.reset()


@gpu
@pytest.mark.parametrize("scrypt_n", [2, 4, 64])
@pytest.mark.parametrize("count", [1, 3, 257])
def test_smallest_n_gap1(scrypt_n, count):
    """mask = 1 is the smallest Integerify range; 257 labels cross a
    workgroup's 64 quads and leave the second workgroup one live quad."""
    o = Oracle()
    want, _ = o.init_range(o.commitment(NODE, ATX), 0, count, scrypt_n)
    got, _ = gpu_labels(count, scrypt_n)
    assert got == want


@gpu
@pytest.mark.parametrize("count", [3 * 128, 3 * 128 + 37, 5 * 128 + 1])
def test_scratch_slot_reuse(count):
    """1 MiB of scratch is 128 slots at N=64, so every quad runs three or
    more tasks over the same scratch column, the last round ragged."""
    n = 64
    o = Oracle()
    want, _ = o.init_range(o.commitment(NODE, ATX), 0, count, n)
    got, _ = gpu_labels(count, n, scratch_bytes=128 * n * 128)
    assert got == want


@gpu
def test_index_range_crossing_2_32():
    n, start = 64, 2**32 - 5
    o = Oracle()
    want, _ = o.init_range(o.commitment(NODE, ATX), start, start + 16, n)
    got, _ = gpu_labels(16, n, num_units=2, lpu=2**32, index_start=start,
                        index_end=start + 16)
    assert got == want


def _unpack(packed, k, bpi):
    v = int.from_bytes(packed, "little")
    return [(v >> (i * bpi)) & ((1 << bpi) - 1) for i in range(k)]


def _pack(idx, bpi):
    v = 0
    for i, x in enumerate(idx):
        v |= x << (i * bpi)
    return v.to_bytes((len(idx) * bpi + 7) // 8, "little")


def _o_proof(p, k2):
    op = Proof()
    op.nonce, op.pow, op.num_indices = p.nonce, p.pow, k2
    op.indices_len = len(p.indices)
    for i, b in enumerate(p.indices):
        op.indices[i] = b
    return op


@gpu
def test_index_list_mode_two_commitments():
    """The verification entry point recomputes labels in index-list mode
    with one commitment per task.  It returns verdicts, not labels: a proof
    passes only if every recomputed label passes its AES threshold, so the
    verdicts (and the rejected position) are held to the oracle's over two
    identities, unsorted indices and one index swapped for a failing one."""
    n, total, k1, k2, bpi = 64, 2048, 12, 8, 11
    o = Oracle()
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total, k1=k1,
                             k2=k2, k3=k2, pow_difficulty=POW_DIFF)
    ver = gsm_amd.PostVerifier(cfg, scrypt_n=n)
    proofs, metas, ometas = [], [], []
    for node in (NODE, NODE2):
        labels, _ = o.init_range(o.commitment(node, ATX), 0, total, n,
                                 with_nonce=False)
        op = o.prove(labels, total, CHALLENGE, k1, k2, 16, POW_DIFF)
        idx = _unpack(bytes(op.indices[:op.indices_len]), k2, bpi)
        mixed = [idx[i] for i in (5, 0, 7, 2, 1, 6, 3, 4)]
        assert mixed != sorted(mixed)
        for cand in (mixed, [mixed[0], mixed[1], (mixed[2] + 1) % total] +
                     mixed[3:]):
            proofs.append(gsm_amd.PostProof(op.nonce, _pack(cand, bpi),
                                            op.pow))
            metas.append(gsm_amd.PostProofMetadata(node, ATX, CHALLENGE, 1,
                                                   total))
            ometas.append(make_meta(node, ATX, CHALLENGE, 1, total))
    # interleave the identities so neighbouring tasks differ in commitment
    order = [0, 2, 1, 3]
    res = ver.verify_batch([proofs[i] for i in order],
                           [metas[i] for i in order])
    want_ok = 0
    for (st, inv), i in zip(res, order):
        orc, oinv = o.verify(_o_proof(proofs[i], k2), ometas[i], n, k1, k2,
                             k2, None, -1, POW_DIFF)
        assert (st == gsm_amd.api.Status.OK) == (orc == 0), (i, st, orc)
        if orc != 0:
            assert st == gsm_amd.api.Status.INVALID_INDEX and inv == oinv
        else:
            want_ok += 1
    assert want_ok >= 2  # both shuffled, untampered proofs are accepted


_CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import gsm_amd
from oracle import Oracle
NODE, ATX = bytes([0xA5])*32, bytes([0x5A])*32
POW = bytes([0x0F]) + bytes([0xFF])*31
cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=300, k1=12,
                         k2=8, k3=4, pow_difficulty=POW)
opts = gsm_amd.PostSetupOpts(num_units=1, scrypt_n=64,
                             scratch_bytes=1 << 30)
mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
mgr.prepare_initializer()
mgr.start_session()
got = mgr.copy_labels(0, 300)
o = Oracle()
want, best = o.init_range(o.commitment(NODE, ATX), 0, 300, 64)
assert got == want, "labels mismatch"
n = mgr.vrf_nonce()
assert n is not None and n[0] == best.index
mgr.reset()
print("gap parity OK")
"""


@gpu
@pytest.mark.parametrize("gap_shift", [1, 2])
def test_generic_kernel_still_exact(gap_shift):
    """POST_GAP_SHIFT is read by the engine at session creation; a fresh
    process keeps it away from the other tests."""
    env = dict(os.environ, POST_GAP_SHIFT=str(gap_shift))
    r = subprocess.run(
        [sys.executable, "-c", _CHILD % (REPO, os.path.join(REPO, "oracle"))],
        capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gap parity OK" in r.stdout


def test_launcher_falls_back_outside_lean_range():
    """Host only: the predicate the launcher branches on.  The lean kernel
    multiplies j < scrypt_n by scratch_lanes * 8 in 24 bits."""
    lib = gsm_amd.load_engine()
    ok = lib.poste_label_romix_lean_ok
    ok.restype = ctypes.c_int
    ok.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    assert ok(8192, 0, 1 << 17) == 1          # mainnet
    assert ok(2, 0, 128) == 1
    assert ok(8192, 1, 1 << 17) == 0          # lookup-gap 2
    assert ok(8192, 0, (1 << 21) - 128) == 0  # block index reaches 2^32
    assert ok(2, 0, (1 << 21) - 128) == 1
    assert ok(2, 0, 1 << 21) == 0             # stride leaves 24 bits
    assert ok(2, 0, 1 << 24) == 0
    assert ok(1 << 24, 0, 128) == 1
    assert ok(1 << 25, 0, 64) == 0            # j leaves 24 bits
    assert ok(1 << 15, 0, 1 << 17) == 0       # 2^15 * 2^17 = 2^32
    assert ok(1 << 14, 0, 1 << 17) == 1
