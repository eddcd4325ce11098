"""Free-running phase-mixed init path vs the CPU oracle, byte for byte.

The split fill/mix ROMix kernels run on three streams (two below 192
scratch slots, or with POST_ROMIX_MIX=free2 or chain), each over its own
share of the slots, and no ROMix kernel waits for another stream.  What the streams share is ordered by
events: the batch's candidate count is zeroed on the stream of the batch's
first unit and every other stream waits for that before its first tail of
the batch.  Units go round the streams across batches and across step()
calls, and the two output sets alternate likewise.

128 slots (192 with three streams) is the smallest geometry with every
stream live; a unit is then one 64-quad workgroup and a batch holds at most
4 x slots labels.  Every label comparison is over every byte, and the VRF
nonce is compared with the oracle's minimum over the labels written so far.

The tail appends a candidate only for a label below the threshold it was
given, which is the host's running minimum (it lags by the batch in flight;
pow_difficulty has no part in it).  So the first batch of a session appends
one candidate per workgroup and a later batch appends where it improves the
minimum; the nonce check after each call sees a candidate lost in either.
"""
import functools
import json
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
SLOTS192 = 192 * N * 128

# six calls of three units each at 128 slots: the batches start on streams
# A, B, A, ... and use output sets 0, 1, 0, ...  From this start index the
# oracle's running minimum improves in each of the first five batches, in
# the second and the fourth by a label of the batch's middle unit, which
# runs on the stream that did not zero the batch's candidate count.
THREE_UNIT_STEPS = (192,) * 6
THREE_UNIT_START = 294 * 192


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
@pytest.mark.parametrize("count", [1, 64, 65, 128, 129, 128 * 5 + 3])
def test_single_call_counts(count):
    """The other stream empty (1, 64), one label on it (65), one full unit
    each (128), a second unit on the first stream (129), and two batches
    with a ragged last unit (643 = 512 + 131)."""
    want, best_idx, best_lab = oracle_range(0, count, N)
    got, nonce = gpu_labels(count, N, scratch_bytes=SLOTS128)
    assert got == want
    assert nonce == (best_idx, best_lab)


@gpu
def test_three_unit_batches_alternate_streams_and_sets():
    """Each call is one batch of three units, so consecutive batches start
    on alternating streams and reuse both output sets; the count reset of a
    batch that starts on stream B must reach stream A's tail of it."""
    total, start = sum(THREE_UNIT_STEPS), THREE_UNIT_START
    want, _, _ = oracle_range(start, total, N)
    mgr = make_mgr(total, N, num_units=2, lpu=2**32, index_start=start,
                   index_end=start + total, scratch_bytes=SLOTS128)
    mgr.prepare_initializer()
    try:
        written = 0
        for ask in THREE_UNIT_STEPS:
            done, kms = mgr.step(ask)
            assert done == ask
            assert kms > 0
            written += ask
            assert mgr.status()["num_labels_written"] == written
            _, best_idx, best_lab = oracle_range(start, written, N)
            assert mgr.vrf_nonce() == (best_idx, best_lab), written
        assert mgr.copy_labels(0, total) == want
    finally:
        mgr.reset()


def _read_files(d):
    files = sorted((f for f in os.listdir(d)
                    if f.startswith("postdata_") and f.endswith(".bin")),
                   key=lambda f: int(f[len("postdata_"):-len(".bin")]))
    return b"".join(open(os.path.join(d, f), "rb").read() for f in files)


@gpu
def test_cancel_between_calls_and_resume(tmp_path):
    """A call that ends after an odd number of units leaves the cursor on
    stream B; cancel then stops the session before anything more is issued,
    and a fresh session resumes at the label the files end at."""
    d = str(tmp_path)
    total, part = 128 * 5 + 3, 192
    want, best_idx, best_lab = oracle_range(0, total, N)
    kw = dict(scratch_bytes=SLOTS128, data_dir=d, max_file_size=256 * 16)

    mgr = make_mgr(total, N, **kw)
    mgr.prepare_initializer()
    done, _ = mgr.step(part)
    assert done == part
    mgr.stop()
    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.step(part)
    assert ei.value.code == gsm_amd.api.Status.CANCELLED
    assert mgr.status()["num_labels_written"] == part
    _, part_idx, part_lab = oracle_range(0, part, N)
    assert mgr.vrf_nonce() == (part_idx, part_lab)
    mgr.reset()
    assert _read_files(d) == want[:part * 16]

    mgr2 = make_mgr(total, N, **kw)
    mgr2.prepare_initializer()
    assert mgr2.status()["num_labels_written"] == part
    mgr2.start_session()
    try:
        assert _read_files(d)[part * 16:] == want[part * 16:]
        assert mgr2.vrf_nonce() == (best_idx, best_lab)
    finally:
        mgr2.reset()


_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import gsm_amd
NODE, ATX = bytes([0xA5])*32, bytes([0x5A])*32
POW = bytes([0x0F]) + bytes([0xFF])*31
steps, scratch, start = %r, %d, %d
count = sum(steps)
cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=2**32, k1=12,
                         k2=8, k3=4, pow_difficulty=POW)
opts = gsm_amd.PostSetupOpts(num_units=2, scrypt_n=64, scratch_bytes=scratch,
                             index_start=start, index_end=start + count)
mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
mgr.prepare_initializer()
nonces = []
for ask in steps:
    done, _ = mgr.step(ask)
    assert done == ask, (done, ask)
    idx, lab = mgr.vrf_nonce()
    nonces.append([idx, lab.hex()])
got = mgr.copy_labels(0, count)
mgr.reset()
print("RESULT", json.dumps({"labels": got.hex(), "nonces": nonces}))
"""


def run_arm(mode, steps, scratch, start=0):
    """One session in a fresh process (POST_ROMIX_MIX is read at session
    creation): labels of the whole range and the nonce after each call."""
    env = dict(os.environ)
    env.pop("POST_ROMIX_MIX", None)
    if mode is not None:
        env["POST_ROMIX_MIX"] = mode
    r = subprocess.run(
        [sys.executable, "-c", _CHILD % (REPO, tuple(steps), scratch, start)],
        capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))
    res = json.loads(line[len("RESULT "):])
    return bytes.fromhex(res["labels"]), [(i, l) for i, l in res["nonces"]]


def want_nonces(steps, start=0):
    out, written = [], 0
    for ask in steps:
        written += ask
        _, idx, lab = oracle_range(start, written, N)
        out.append((idx, lab.hex()))
    return out


@gpu
def test_three_streams_tail():
    """192 slots, three streams, a batch is 12 units.  The first call is a
    full batch and a batch of two units, which leaves one stream without
    work; the second is a single ragged unit, which leaves two."""
    steps = (768 + 128, 37)
    want, _, _ = oracle_range(0, sum(steps), N)
    got, nonces = run_arm("free3", steps, SLOTS192)
    assert got == want
    assert nonces == want_nonces(steps)


@gpu
def test_arms_give_identical_bytes():
    """The chained two-stream schedule, three free-running streams and the
    default produce the same labels and the same nonce after every call of
    the three-unit-batch case."""
    steps, start = THREE_UNIT_STEPS, THREE_UNIT_START
    want, _, _ = oracle_range(start, sum(steps), N)
    wn = want_nonces(steps, start)
    for mode, scratch in (("chain", SLOTS128), ("free3", SLOTS192),
                          (None, SLOTS128)):
        got, nonces = run_arm(mode, steps, scratch, start)
        assert got == want, mode
        assert nonces == wn, mode


@gpu
def test_monolithic_uneven_steps_match_oracle_and_default():
    """POST_ROMIX_MIX=0, the monolithic kernel, which shares the host half
    of a batch (candidate merge, self-check, bookkeeping) with the split
    path.  Three uneven calls from a non-zero start: a full batch of 512
    and a part of one, less than a workgroup, and a ragged 3 * 128 + 37.
    Labels and the nonce after every call against the oracle, and the
    default arm gives the same over the same range."""
    steps, start = (512 + 192, 65, 3 * 128 + 37), THREE_UNIT_START
    want, _, _ = oracle_range(start, sum(steps), N)
    wn = want_nonces(steps, start)
    for mode in ("0", None):
        got, nonces = run_arm(mode, steps, SLOTS128, start)
        assert got == want, mode
        assert nonces == wn, mode
