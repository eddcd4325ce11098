"""Phase-mixed init path (split fill/mix ROMix kernels on two streams) vs the
CPU oracle, byte for byte.

The lean gap-1 ROMix runs as a fill kernel (phase 1) and a mix kernel
(phase 2); the init path gives each half of the scratch slots a stream and
keeps the second stream one phase behind the first.  128 slots (two halves
of one 64-quad workgroup each) is the smallest geometry with both streams
live, so the counts below are chosen around 64 and 128: stream B empty,
B with one label, one full unit each, and several units per stream with a
ragged last one.  Every label comparison is over every byte.
"""
import functools
import os
import subprocess
import sys

import pytest

import gsm_amd
from oracle import Oracle

gpu = pytest.mark.gpu

NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
SLOTS128 = 128 * N * 128  # scratch bytes of 128 slots at N=64


@functools.lru_cache(maxsize=None)
def oracle_range(start, count, scrypt_n):
    """(labels, best index, best label) of [start, start+count), computed
    once per range and shared."""
    o = Oracle()
    want, best = o.init_range(o.commitment(NODE, ATX), start, start + count,
                              scrypt_n)
    return want, best.index, bytes(best.label)


def make_mgr(count, scrypt_n, num_units=1, lpu=None, **kw):
    cfg = gsm_amd.PostConfig(min_num_units=1,
                             labels_per_unit=lpu if lpu else count,
                             k1=12, k2=8, k3=4, pow_difficulty=POW_DIFF)
    kw.setdefault("scratch_bytes", 1 << 30)
    opts = gsm_amd.PostSetupOpts(num_units=num_units, scrypt_n=scrypt_n, **kw)
    return gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)


def gpu_labels(count, scrypt_n, **kw):
    mgr = make_mgr(count, scrypt_n, **kw)
    mgr.prepare_initializer()
    mgr.start_session()
    try:
        return mgr.copy_labels(0, count), mgr.vrf_nonce()
    finally:
        mgr.reset()


@gpu
@pytest.mark.parametrize("scrypt_n", [2, 4, 64])
@pytest.mark.parametrize("count", [1, 3, 257])
def test_smallest_n(scrypt_n, count):
    """Count 1 leaves stream B without work; 257 gives the second stream's
    unit a ragged second workgroup."""
    want, best_idx, best_lab = oracle_range(0, count, scrypt_n)
    got, nonce = gpu_labels(count, scrypt_n)
    assert got == want
    assert nonce == (best_idx, best_lab)


@gpu
@pytest.mark.parametrize("count",
                         [64, 65, 128, 129, 3 * 128 + 37, 5 * 128 + 1])
def test_two_halves_of_one_workgroup(count):
    """128 slots: units of 64 labels alternate between the streams and
    reuse their half of the scratch over several units."""
    want, best_idx, best_lab = oracle_range(0, count, N)
    got, nonce = gpu_labels(count, N, scratch_bytes=SLOTS128)
    assert got == want
    assert nonce == (best_idx, best_lab)


@gpu
def test_uneven_steps_drain_and_restart():
    """Each step() call drains the pipeline at its end and the next starts
    it again, on whichever label the last one stopped at."""
    total = 384
    want, best_idx, best_lab = oracle_range(0, total, N)
    mgr = make_mgr(total, N, scratch_bytes=SLOTS128)
    mgr.prepare_initializer()
    try:
        written = 0
        for ask in (100, 1, 283):
            done, kms = mgr.step(ask)
            assert done == ask
            assert kms > 0
            written += ask
            assert mgr.status()["num_labels_written"] == written
        done, _ = mgr.step(10)
        assert done == 0  # the range is complete
        assert mgr.copy_labels(0, total) == want
        assert mgr.vrf_nonce() == (best_idx, best_lab)
    finally:
        mgr.reset()


def _read_files(d):
    files = sorted((f for f in os.listdir(d)
                    if f.startswith("postdata_") and f.endswith(".bin")),
                   key=lambda f: int(f[len("postdata_"):-len(".bin")]))
    return b"".join(open(os.path.join(d, f), "rb").read() for f in files)


@gpu
def test_file_mode_and_resume(tmp_path):
    """File mode at the 128-slot geometry: a partial run leaves exactly the
    labels it reports, a fresh session resumes there, and the files end up
    byte-equal to the oracle's labels."""
    d = str(tmp_path)
    total, part = 5 * 128 + 1, 300
    want, best_idx, best_lab = oracle_range(0, total, N)
    kw = dict(scratch_bytes=SLOTS128, data_dir=d, max_file_size=256 * 16)

    mgr = make_mgr(total, N, **kw)
    mgr.prepare_initializer()
    done, _ = mgr.step(part)
    assert done == part
    assert mgr.status()["num_labels_written"] == part
    mgr.reset()
    assert _read_files(d) == want[:part * 16]

    mgr2 = make_mgr(total, N, **kw)
    mgr2.prepare_initializer()
    assert mgr2.status()["num_labels_written"] == part
    mgr2.start_session()
    try:
        assert _read_files(d) == want
        assert mgr2.vrf_nonce() == (best_idx, best_lab)
    finally:
        mgr2.reset()


@gpu
def test_index_range_crossing_2_32():
    start, count = 2**32 - 70, 200  # the crossing falls inside unit 1
    want, best_idx, best_lab = oracle_range(start, count, N)
    got, nonce = gpu_labels(count, N, num_units=2, lpu=2**32,
                            index_start=start, index_end=start + count,
                            scratch_bytes=SLOTS128)
    assert got == want
    assert nonce == (best_idx, best_lab)


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import gsm_amd
NODE, ATX = bytes([0xA5])*32, bytes([0x5A])*32
POW = bytes([0x0F]) + bytes([0xFF])*31
count = %d
cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=count, k1=12,
                         k2=8, k3=4, pow_difficulty=POW)
opts = gsm_amd.PostSetupOpts(num_units=1, scrypt_n=64,
                             scratch_bytes=%d)
mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
mgr.prepare_initializer()
mgr.start_session()
got = mgr.copy_labels(0, count)
idx, lab = mgr.vrf_nonce()
mgr.reset()
print("LABELS", got.hex())
print("NONCE", idx, lab.hex())
"""


@gpu
@pytest.mark.parametrize("mode", ["0", "seq"])
def test_other_paths_give_the_same_bytes(mode):
    """POST_ROMIX_MIX is read at session creation: 0 is the monolithic
    single-stream path, seq the split kernels on one stream.  A fresh
    process keeps the setting away from the other tests."""
    count = 3 * 128 + 37
    want, best_idx, best_lab = oracle_range(0, count, N)
    env = dict(os.environ, POST_ROMIX_MIX=mode)
    r = subprocess.run(
        [sys.executable, "-c", _CHILD % (REPO, count, SLOTS128)],
        capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(" ", 1) for l in r.stdout.splitlines()
                 if l.startswith(("LABELS", "NONCE")))
    assert bytes.fromhex(lines["LABELS"]) == want
    assert lines["NONCE"] == "%d %s" % (best_idx, best_lab.hex())
    got, nonce = gpu_labels(count, N, scratch_bytes=SLOTS128)
    assert got == want and nonce == (best_idx, best_lab)
