"""Seal during init on a real MI355X.

Every expectation is hashlib per page over the CPU oracle's labels (seal.py),
never something the engine computed.  Fixture as in the seal and heal tests:
3*1024+517 oracle labels at N=32 (4 pages, the last ragged) in files of 1500
labels.  128 scratch lanes give the two-stream schedule and batches of 512
labels, 192 lanes the three-stream schedule and batches of 768: neither is a
multiple of the page, and every batch is shorter than one.

Cancellation stays what it was: post_init_cancel is not taken back, so a
session that was stopped answers CANCELLED from then on and the open page is
continued by a new session from the page boundary.
"""
import base64
import json
import os
import shutil
import subprocess
import sys

import pytest

import gsm_amd
from gsm_amd import seal
Status = gsm_amd.api.Status

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
N = 32
PAGE = 1024 * 16
PER_FILE = 1500
TOTAL = 3 * 1024 + 517
SCRATCH_128 = 128 * N * 128
SCRATCH_192 = 192 * N * 128
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
CHALLENGE = bytes([0x07]) * 32      # proves at postcli's K1/K2 (heal tests)


@pytest.fixture(scope="module")
def clean(oracle):
    """(labels, best index, best label) of the fixture; never modified."""
    labels, best = oracle.init_range(oracle.commitment(NODE, ATX), 0, TOTAL,
                                     N)
    return labels, best.index, bytes(best.label)


@pytest.fixture(scope="module")
def labels(clean):
    return clean[0]


@pytest.fixture(scope="module")
def sidecar(labels):
    return seal.sidecar_bytes(labels)


def make_mgr(d, seal_on=True, scratch=SCRATCH_128, start=0, end=0):
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=TOTAL, k1=12,
                             k2=8, k3=4, pow_difficulty=POW_DIFF)
    opts = gsm_amd.PostSetupOpts(
        data_dir=str(d), num_units=1, scrypt_n=N,
        max_file_size=PER_FILE * 16, scratch_bytes=scratch,
        index_start=start, index_end=end, seal=seal_on)
    return gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)


def read_dir(d):
    return seal.read_stream(str(d))


def read_sidecar(d):
    with open(os.path.join(str(d), seal.SIDECAR), "rb") as f:
        return f.read()


def parts(d):
    return sorted(f for f in os.listdir(str(d))
                  if f.startswith(seal.PART_PREFIX))


def leftovers(d):
    """Anything in the dir that is neither labels, metadata nor sidecar."""
    return [f for f in os.listdir(str(d))
            if not (f.startswith("postdata_") and f.endswith(".bin")
                    and f[len("postdata_"):-len(".bin")].isdigit())
            and f != "postdata_metadata.json"]


def flip(d, label, bit=3):
    path = os.path.join(str(d), f"postdata_{label // PER_FILE}.bin")
    with open(path, "r+b") as f:
        f.seek(label % PER_FILE * 16 + 5)
        b = f.read(1)[0]
        f.seek(label % PER_FILE * 16 + 5)
        f.write(bytes([b ^ (1 << bit)]))


# ------------------------- the kernel, through seal_digest_stream --------

CUTS = [
    [],
    [1], [3], [4], [5],
    [1023], [1024], [1025],
    [511, 512, 513],
    [1, 2, 3, 4, 5, 6, 7, 8, 9],
    [1022, 1023, 1024, 1026],
    [700, 2900],
    [3 * 1024 + 516],
    list(range(256, TOTAL, 256)),
    list(range(768, TOTAL, 768)),
]


def cuts_id(c):
    return "none" if not c else (
        "-".join(map(str, c)) if len(c) < 10 else f"every{c[0]}")


@pytest.fixture(scope="module")
def buffer_digests(labels):
    """post_seal_kernel over the same buffer, computed once."""
    return gsm_amd.seal_digest_buffer(labels)


@pytest.mark.parametrize("cuts", CUTS, ids=cuts_id)
def test_stream_digests_do_not_depend_on_the_cuts(labels, buffer_digests,
                                                  cuts):
    want = seal.stream_digests(labels, cuts)
    assert len(want) == 4 * 16
    got = gsm_amd.seal_digest_stream(labels, 0, cuts)
    assert got == want
    assert got == buffer_digests


@pytest.mark.parametrize("cuts", [[], [700, 2900], [3 * 1024, 3 * 1024 + 1],
                                  list(range(256, TOTAL, 256))], ids=cuts_id)
def test_open_last_page_has_no_digest(labels, cuts):
    want = seal.stream_digests(labels, cuts, stream_end=False)
    assert len(want) == 3 * 16
    assert gsm_amd.seal_digest_stream(labels, 0, cuts,
                                      stream_end=False) == want


@pytest.mark.parametrize("cuts", [[], [5], [700, 2900]], ids=cuts_id)
def test_stream_high_first_index(labels, cuts):
    first = 2**33 + 5 * 1024
    assert gsm_amd.seal_digest_stream(labels, first, cuts) == \
        seal.page_digests(labels)


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_stream_tiny_counts(labels, count):
    data = labels[:count * 16]
    want = seal.page_digests(data)
    assert gsm_amd.seal_digest_stream(data) == want
    assert gsm_amd.seal_digest_stream(data, 1024,
                                      list(range(1, count))) == want
    assert gsm_amd.seal_digest_buffer(data) == want
    assert gsm_amd.seal_digest_stream(data, stream_end=False) == b""


def test_stream_constant_pages():
    data = bytes([0x5C]) * (2 * PAGE + 3 * 16)
    want = seal.page_digests(data)
    assert want[:16] == want[16:32]
    for cuts in ([], [1023, 1025], [2, 2047, 2049]):
        assert gsm_amd.seal_digest_stream(data, 0, cuts) == want


def test_stream_argument_checks(labels):
    for kw in (dict(first_index=5), dict(cuts=[5, 4]),
               dict(cuts=[TOTAL + 1])):
        with pytest.raises(gsm_amd.EngineError) as ei:
            gsm_amd.seal_digest_stream(labels, **kw)
        assert ei.value.code == Status.INVALID_ARGS


# ------------------------- sealed init of a dir -------------------------

def check_sealed_dir(d, labels, sidecar):
    assert read_dir(d) == labels
    assert read_sidecar(d) == sidecar
    assert leftovers(d) == [seal.SIDECAR]       # parts and temporaries gone
    rep = gsm_amd.check_seal(str(d))
    assert rep.clean and (rep.total_labels, rep.pages) == (TOTAL, 4)


@pytest.mark.parametrize("arm", ["two-stream", "three-stream", "monolithic"])
def test_sealed_init(clean, sidecar, tmp_path, monkeypatch, arm):
    labels, best_idx, best_lab = clean
    if arm == "monolithic":
        monkeypatch.setenv("POST_ROMIX_MIX", "0")
    scratch = SCRATCH_192 if arm == "three-stream" else SCRATCH_128
    mgr = make_mgr(tmp_path, scratch=scratch)
    mgr.prepare_initializer()
    assert parts(tmp_path) == [seal.part_name(0)]
    mgr.start_session()
    nonce = mgr.vrf_nonce()
    mgr.reset()
    check_sealed_dir(tmp_path, labels, sidecar)
    assert nonce == (best_idx, best_lab)

    plain = tmp_path / "plain"
    mgr = make_mgr(plain, seal_on=False, scratch=scratch)
    mgr.prepare_initializer()
    mgr.start_session()
    assert mgr.vrf_nonce() == nonce
    mgr.reset()
    assert read_dir(plain) == labels
    assert leftovers(plain) == []               # the seal is off by default


def test_steps_that_end_anywhere(labels, sidecar, tmp_path):
    mgr = make_mgr(tmp_path)
    mgr.prepare_initializer()
    written = 0
    for ask in (1000, 1, 23):
        done, _ = mgr.step(ask)
        written += ask
        assert done == ask
        assert mgr.status()["num_labels_written"] == written
        with open(tmp_path / seal.part_name(0), "rb") as f:
            part = f.read()
        assert part == seal.part_bytes(labels, 0, TOTAL, written // 1024)
    done, _ = mgr.step(TOTAL)
    assert done == TOTAL - written
    mgr.reset()
    check_sealed_dir(tmp_path, labels, sidecar)


def test_stop_between_steps_then_a_new_session(labels, sidecar, tmp_path):
    mgr = make_mgr(tmp_path)
    mgr.prepare_initializer()
    assert mgr.step(1300)[0] == 1300
    mgr.stop()
    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.step(100)
    assert ei.value.code == Status.CANCELLED
    assert mgr.status()["num_labels_written"] == 1300
    mgr.reset()
    assert read_dir(tmp_path) == labels[:1300 * 16]
    with open(tmp_path / seal.part_name(0), "rb") as f:
        assert f.read() == seal.part_bytes(labels, 0, TOTAL, 1)

    mgr = make_mgr(tmp_path)
    mgr.prepare_initializer()
    assert mgr.status()["num_labels_written"] == 1024   # the page boundary
    mgr.start_session()
    mgr.reset()
    check_sealed_dir(tmp_path, labels, sidecar)


# ------------------------- kill and resume -------------------------

_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import gsm_amd
cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=%d, k1=12, k2=8,
                         k3=4, pow_difficulty=bytes([0x0F]) + bytes([0xFF])*31)
opts = gsm_amd.PostSetupOpts(data_dir=%r, num_units=1, scrypt_n=%d,
                             max_file_size=%d, scratch_bytes=%d, seal=True)
mgr = gsm_amd.PostSetupManager(bytes([0xA5])*32, bytes([0x5A])*32, cfg, opts)
mgr.prepare_initializer()
for ask in (1000, 1300):
    done, _ = mgr.step(ask)
    assert done == ask
print("STOPPED", mgr.status()["num_labels_written"], flush=True)
os._exit(0)     # no reset, no completion: the process just ends
"""


@pytest.fixture(scope="module")
def killed(labels, tmp_path_factory):
    """A sealed init whose process ended after 2300 labels."""
    d = str(tmp_path_factory.mktemp("killed"))
    r = subprocess.run(
        [sys.executable, "-c",
         _CHILD % (REPO, TOTAL, d, N, PER_FILE * 16, SCRATCH_128)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "STOPPED 2300" in r.stdout, \
        r.stdout + r.stderr
    assert read_dir(d) == labels[:2300 * 16]
    with open(os.path.join(d, seal.part_name(0)), "rb") as f:
        assert f.read() == seal.part_bytes(labels, 0, TOTAL, 2)
    return d


def labels_truncated_unevenly(d):
    # 2101 labels and a torn one: not a multiple of 4, nor of 1024
    os.truncate(os.path.join(d, "postdata_1.bin"), 601 * 16 + 7)
    return 2048


def part_lost_a_digest(d):
    os.truncate(os.path.join(d, seal.part_name(0)), 32 + 16)
    return 1024


def part_ahead_of_labels(d):
    # 1800 labels on disk, the part vouches for 2048
    os.truncate(os.path.join(d, "postdata_1.bin"), 300 * 16)
    return 1024


@pytest.mark.parametrize("alter", [labels_truncated_unevenly,
                                   part_lost_a_digest, part_ahead_of_labels])
def test_kill_and_resume(labels, sidecar, killed, tmp_path, alter):
    d = shutil.copytree(killed, str(tmp_path / "d"))
    resume_at = alter(d)
    mgr = make_mgr(d)
    mgr.prepare_initializer()
    assert mgr.status()["num_labels_written"] == resume_at
    with open(os.path.join(d, seal.part_name(0)), "rb") as f:
        assert f.read() == seal.part_bytes(labels, 0, TOTAL,
                                           resume_at // 1024)
    mgr.start_session()
    mgr.reset()
    check_sealed_dir(d, labels, sidecar)


def test_part_of_another_geometry_is_refused(killed, tmp_path):
    d = shutil.copytree(killed, str(tmp_path / "d"))
    with open(os.path.join(d, seal.part_name(0)), "r+b") as f:
        f.write(seal.pack_part_header(0, 5))
    mgr = make_mgr(d)
    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.prepare_initializer()
    assert ei.value.code == Status.IO
    assert "disagrees with the session" in str(ei.value)


# ------------------------- two shards -------------------------

SHARDS = [(0, 2048), (2048, TOTAL)]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_shards_in_either_order(labels, sidecar, tmp_path, order):
    first, second = SHARDS[order[0]], SHARDS[order[1]]
    mgr = make_mgr(tmp_path, start=first[0], end=first[1])
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    # the first to finish leaves its part and no sidecar
    assert parts(tmp_path) == [seal.part_name(first[0])]
    with open(tmp_path / seal.part_name(first[0]), "rb") as f:
        assert f.read() == seal.part_bytes(labels, *first)
    assert not os.path.exists(tmp_path / seal.SIDECAR)
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.seal_assemble(str(tmp_path))
    assert ei.value.code == Status.IO
    missing = "pages [2, 4) are missing" if order == (0, 1) \
        else "pages [0, 2) are missing"
    assert missing in str(ei.value)

    mgr = make_mgr(tmp_path, start=second[0], end=second[1])
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    check_sealed_dir(tmp_path, labels, sidecar)
    assert gsm_amd.seal_assemble(str(tmp_path)) == 4


def test_unaligned_shard_is_refused(tmp_path):
    for start, end in ((1500, TOTAL), (0, 1500)):
        mgr = make_mgr(tmp_path, start=start, end=end)
        with pytest.raises(gsm_amd.EngineError) as ei:
            mgr.prepare_initializer()
        assert ei.value.code == Status.UNSUPPORTED
        assert "1024" in str(ei.value)
    assert parts(tmp_path) == []


def test_file_size_that_tears_labels_is_refused(tmp_path):
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=TOTAL)
    opts = gsm_amd.PostSetupOpts(data_dir=str(tmp_path), num_units=1,
                                 scrypt_n=N, max_file_size=PER_FILE * 16 + 8,
                                 scratch_bytes=SCRATCH_128, seal=True)
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.PostSetupManager(NODE, ATX, cfg, opts).prepare_initializer()
    assert ei.value.code == Status.UNSUPPORTED
    assert "MaxFileSize" in str(ei.value)


def test_dir_started_without_a_seal_is_refused(labels, tmp_path):
    mgr = make_mgr(tmp_path, seal_on=False)
    mgr.prepare_initializer()
    assert mgr.step(600)[0] == 600
    mgr.reset()
    mgr = make_mgr(tmp_path)
    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.prepare_initializer()
    assert ei.value.code == Status.UNSUPPORTED
    assert "dir was started without a seal; finish init and run `seal`" in \
        str(ei.value)
    assert parts(tmp_path) == []


def test_enable_seal_after_the_first_step_is_refused(tmp_path):
    mgr = make_mgr(tmp_path, seal_on=False)
    mgr.prepare_initializer()
    lib = mgr.engine.lib
    assert mgr.step(10)[0] == 10
    assert lib.post_init_enable_seal(mgr._session) == Status.INVALID_ARGS
    assert "before the first step" in lib.post_last_error().decode()
    mgr.reset()
    # and a session without a data dir
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=TOTAL)
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, gsm_amd.PostSetupOpts(
        num_units=1, scrypt_n=N, scratch_bytes=SCRATCH_128, seal=True))
    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.prepare_initializer()
    assert ei.value.code == Status.INVALID_ARGS


# ------------------------- the point of the feature -------------------------

def test_seal_from_the_device_lets_repair_confirm(labels, sidecar, tmp_path):
    """The digests were taken before the labels went through host memory and
    the disk, so a page damaged on disk is found by check-seal and repair can
    confirm its recomputation against the seal and write it back.

    The weakness this removes: `seal` run over the damaged dir hashes the
    bytes as they lie, and check-seal is then clean over bad labels."""
    d = tmp_path / "sealed"
    mgr = make_mgr(d)
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    flip(d, 1024 + 77)
    late = shutil.copytree(str(d), str(tmp_path / "late"))

    rep = gsm_amd.check_seal(str(d))
    assert rep.bad_pages == [1] and rep.pages_bad == 1
    rep = gsm_amd.repair_data(str(d),
                              gsm_amd.HealOpts(scratch_bytes=SCRATCH_128))
    assert (rep.pages_bad, rep.pages_healed, rep.pages_unconfirmed,
            rep.pages_written, rep.labels_repaired) == (1, 1, 0, 1, 1)
    check_sealed_dir(d, labels, sidecar)

    os.remove(os.path.join(late, seal.SIDECAR))
    gsm_amd.seal_data(late)
    assert gsm_amd.check_seal(late).clean
    assert read_dir(late) != labels


# ------------------------- end to end, child processes -------------------

def cli(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "postcli.py"),
                           *argv], cwd=REPO, capture_output=True, text=True,
                          timeout=120)


def test_cli_init_seal_check_prove_verify(labels, sidecar, tmp_path):
    d = str(tmp_path / "d")
    init = ("init", "--datadir", d, "--node-id", NODE.hex(), "--atx-id",
            ATX.hex(), "--num-units", "1", "--labels-per-unit", str(TOTAL),
            "--scrypt-n", str(N), "--max-file-size", str(PER_FILE * 16),
            "--seal")
    r = cli(*init, "--shard", "1/3")
    assert r.returncode == 2 and r.stdout == "", r.stdout + r.stderr
    assert "1024" in r.stderr
    r = cli(*init)
    assert r.returncode == 0, r.stderr
    check_sealed_dir(d, labels, sidecar)
    r = cli("seal", "--datadir", d, "--assemble")
    assert r.returncode == 0 and json.loads(r.stdout)["pages"] == 4, r.stderr
    r = cli("check-seal", "--datadir", d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout)["pages_bad"] == 0
    r = cli("prove", "--datadir", d, "--challenge", CHALLENGE.hex(),
            "--pow-difficulty", POW_DIFF.hex(), "--check-seal")
    assert r.returncode == 0, r.stderr
    path = str(tmp_path / "proof.json")
    with open(path, "w") as fh:
        fh.write(r.stdout)
    r = cli("verify", "--datadir", d, "--proof", path, "--pow-difficulty",
            POW_DIFF.hex())
    assert r.returncode == 0 and json.loads(r.stdout) == {"valid": True}, \
        r.stdout + r.stderr
