"""Initial proof during init on a real MI355X.

Every expectation comes from the CPU oracle: the labels are oracle.init_range,
the hit records of the parts (markers taken out) are oracle.scan_hits over
the same range, compared as lists, and the proof is oracle.prove over the
clean labels.  Fixture as in tests/test_heal_gpu.py: 3*1024+517 labels at
N=32 in files of 1500 labels.  128 scratch lanes give the two-stream schedule
and batches of 512 labels, 192 lanes the three-stream schedule and batches of
768.  The host gets the first 1024 records of a batch with its count.  By the
oracle no batch of the fixture has more than 88 hits, so they stay inside
that window; the batch of the overflow test has 65376 and goes back to the
device for the rest: both ways of bringing the hits home are taken."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import gsm_amd
from gsm_amd import initproof, seal, wire
Status = gsm_amd.api.Status

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
N = 32
PER_FILE = 1500
TOTAL = 3 * 1024 + 517
SCRATCH_128 = 128 * N * 128
SCRATCH_192 = 192 * N * 128
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
K1, K2 = 12, 8
ZERO = bytes(32)
SEVEN = bytes([0x07]) * 32
CASES = [(ZERO, 16), (SEVEN, 16), (ZERO, 32), (SEVEN, 32)]


def case_id(c):
    return "ch%02x-%d" % (c[0][0], c[1])


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
def hits_of(oracle, labels):
    """(challenge, nonces) -> oracle.scan_hits over the whole space."""
    cache = {}

    def get(challenge, nonces):
        key = (challenge, nonces)
        if key not in cache:
            pows = [oracle.lib.oracle_k2pow(challenge, g, POW_DIFF)
                    for g in range(nonces // 16)]
            cache[key] = [(int(i), int(n)) for i, n in oracle.scan_hits(
                labels, 0, TOTAL, challenge, K1, nonces, pows)]
        return cache[key]
    return get


@pytest.fixture(scope="module")
def proof_of(oracle, labels):
    cache = {}

    def get(challenge, nonces):
        key = (challenge, nonces)
        if key not in cache:
            op = oracle.prove(labels, TOTAL, challenge, K1, K2, nonces,
                              POW_DIFF)
            cache[key] = gsm_amd.PostProof(
                op.nonce, bytes(op.indices[:op.indices_len]), op.pow)
        return cache[key]
    return get


def pcfg(k2=K2, k1=K1):
    return gsm_amd.PostConfig(min_num_units=1, labels_per_unit=TOTAL, k1=k1,
                              k2=k2, k3=k2, pow_difficulty=POW_DIFF)


def make_mgr(d, challenge=ZERO, nonces=16, proof=True, seal_on=False,
             scratch=SCRATCH_128, start=0, end=0, k2=K2, k1=K1):
    ip = gsm_amd.InitialProofOpts.of(
        pcfg(k2, k1), gsm_amd.ProveOpts(nonces=nonces), challenge) \
        if proof else None
    opts = gsm_amd.PostSetupOpts(
        data_dir=str(d), num_units=1, scrypt_n=N,
        max_file_size=PER_FILE * 16, scratch_bytes=scratch,
        index_start=start, index_end=end, seal=seal_on, initial_proof=ip)
    return gsm_amd.PostSetupManager(NODE, ATX, pcfg(k2, k1), opts)


def read_dir(d):
    return seal.read_stream(str(d))


def part_path(d, start=0):
    return os.path.join(str(d), initproof.part_name(start))


def read_part(d, start=0):
    with open(part_path(d, start), "rb") as f:
        return initproof.read_part(f.read())


def parts(d):
    return sorted(f for f in os.listdir(str(d))
                  if f.startswith(initproof.PART_PREFIX))


def check_part(d, hits, upto, start=0, end=TOTAL):
    """The part of [start, end) is complete up to `upto` and holds exactly
    the oracle's hits below it, in order."""
    h, got, complete_to = read_part(d, start)
    assert (h.index_start, h.index_end, h.total_labels) == (start, end, TOTAL)
    assert complete_to == upto
    assert got == [x for x in hits if start <= x[0] < upto]


def check_proved_dir(d, labels, hits, want, challenge, nonces):
    assert read_dir(d) == labels
    got, rep = gsm_amd.init_proof_assemble(str(d))
    assert got == want
    assert (rep.total_labels, rep.labels_covered, rep.hits) == \
        (TOTAL, TOTAL, len(hits))
    assert gsm_amd.api.prove_dir(str(d), challenge, pcfg(),
                                 gsm_amd.ProveOpts(nonces=nonces)) == want
    gsm_amd.PostVerifier(pcfg(), scrypt_n=N).verify(
        got, gsm_amd.PostProofMetadata(NODE, ATX, challenge, 1, TOTAL))


# ------------------------- schedules and variants -------------------------

def select_arm(monkeypatch, arm):
    if arm == "monolithic":
        monkeypatch.setenv("POST_ROMIX_MIX", "0")
    return SCRATCH_192 if arm == "three-stream" else SCRATCH_128


@pytest.fixture(scope="module")
def plain_nonce():
    """VRF nonce of an init without the scan, per scratch size."""
    cache = {}

    def get(d, scratch):
        if scratch not in cache:
            mgr = make_mgr(d, proof=False, scratch=scratch)
            mgr.prepare_initializer()
            mgr.start_session()
            cache[scratch] = mgr.vrf_nonce()
            mgr.reset()
            assert parts(d) == []           # the scan is off by default
        return cache[scratch]
    return get


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("arm", ["two-stream", "three-stream", "monolithic"])
def test_init_with_the_scan_on(clean, hits_of, proof_of, plain_nonce,
                               tmp_path, monkeypatch, arm, case):
    labels, best_idx, best_lab = clean
    challenge, nonces = case
    scratch = select_arm(monkeypatch, arm)
    d = tmp_path / "d"
    mgr = make_mgr(d, challenge, nonces, scratch=scratch)
    mgr.prepare_initializer()
    assert parts(d) == [initproof.part_name(0)]
    mgr.start_session()
    nonce = mgr.vrf_nonce()
    mgr.reset()
    assert nonce == (best_idx, best_lab)
    assert nonce == plain_nonce(tmp_path / "plain", scratch)
    hits = hits_of(challenge, nonces)
    check_part(d, hits, TOTAL)
    check_proved_dir(d, labels, hits, proof_of(challenge, nonces), challenge,
                     nonces)


@pytest.mark.parametrize("max_blocks", [None, "2"])
def test_scan_variants_leave_identical_parts(labels, hits_of, proof_of,
                                             tmp_path, monkeypatch,
                                             max_blocks):
    """Each variant the session can be made to choose; with a cap of two
    blocks every ILP chain is live and the grid-stride loop iterates."""
    if max_blocks:
        monkeypatch.setenv("POST_SCAN_MAX_BLOCKS", max_blocks)
    hits = hits_of(ZERO, 32)
    blobs = []
    for variant in ("bankrep", "tt4"):
        monkeypatch.setenv("POST_INIT_PROOF_SCAN", variant)
        d = tmp_path / variant
        mgr = make_mgr(d, ZERO, 32)
        mgr.prepare_initializer()
        mgr.start_session()
        mgr.reset()
        check_part(d, hits, TOTAL)
        assert gsm_amd.init_proof_assemble(str(d))[0] == proof_of(ZERO, 32)
        with open(part_path(d), "rb") as f:
            blobs.append(f.read())
    assert blobs[0] == blobs[1]
    monkeypatch.setenv("POST_INIT_PROOF_SCAN", "fastest")
    with pytest.raises(gsm_amd.EngineError) as ei:
        make_mgr(tmp_path / "x").prepare_initializer()
    assert ei.value.code == Status.INVALID_ARGS
    assert parts(tmp_path / "x") == []      # a refused enable leaves no part


def test_a_second_enable_must_bring_the_same_config(tmp_path):
    mgr = make_mgr(tmp_path)
    mgr.prepare_initializer()
    lib = mgr.engine.lib
    pc = gsm_amd.InitialProofOpts.of(pcfg(), gsm_amd.ProveOpts(nonces=16)
                                     ).to_c()
    assert lib.post_init_enable_proof(mgr._session, pc) == Status.OK
    pc.k1 = K1 + 1
    assert lib.post_init_enable_proof(mgr._session, pc) == Status.INVALID_ARGS
    assert "another proving config" in lib.post_last_error().decode()
    pc.k1 = K1
    pc.challenge[0] = 1
    assert lib.post_init_enable_proof(mgr._session, pc) == Status.INVALID_ARGS
    mgr.reset()


# ------------------------- steps, stop, resume -------------------------

def test_steps_that_end_anywhere(labels, hits_of, proof_of, tmp_path):
    hits = hits_of(ZERO, 16)
    mgr = make_mgr(tmp_path)
    mgr.prepare_initializer()
    check_part(tmp_path, hits, 0)
    written = 0
    for ask in (1000, 1, 23):
        done, _ = mgr.step(ask)
        written += ask
        assert done == ask
        assert mgr.status()["num_labels_written"] == written
        check_part(tmp_path, hits, written)
    done, _ = mgr.step(TOTAL)
    assert done == TOTAL - written
    mgr.reset()
    # the whole file: the hits of a batch, then its marker, batch by batch
    marks = [512, 1000, 1001, 1024] + list(range(1536, TOTAL, 512)) + [TOTAL]
    header = initproof.PartHeader(16, K1, K2, ZERO, POW_DIFF, 0, TOTAL, TOTAL)
    with open(part_path(tmp_path), "rb") as f:
        assert f.read() == initproof.build_part(header, hits, marks)
    check_proved_dir(tmp_path, labels, hits, proof_of(ZERO, 16), ZERO, 16)


def test_stop_between_steps_then_a_new_session(labels, hits_of, proof_of,
                                               tmp_path):
    hits = hits_of(ZERO, 16)
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
    check_part(tmp_path, hits, 1300)
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.init_proof_assemble(str(tmp_path))
    assert ei.value.code == Status.IO
    assert "labels [1300, 3589) are missing" in str(ei.value)

    mgr = make_mgr(tmp_path)
    mgr.prepare_initializer()
    assert mgr.status()["num_labels_written"] == 1300
    mgr.start_session()
    mgr.reset()
    check_part(tmp_path, hits, TOTAL)
    check_proved_dir(tmp_path, labels, hits, proof_of(ZERO, 16), ZERO, 16)


_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import gsm_amd
cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=%d, k1=12, k2=8,
                         k3=8, pow_difficulty=bytes([0x0F]) + bytes([0xFF])*31)
ip = gsm_amd.InitialProofOpts.of(cfg, gsm_amd.ProveOpts(nonces=16))
opts = gsm_amd.PostSetupOpts(data_dir=%r, num_units=1, scrypt_n=%d,
                             max_file_size=%d, scratch_bytes=%d, seal=%r,
                             initial_proof=ip)
mgr = gsm_amd.PostSetupManager(bytes([0xA5])*32, bytes([0x5A])*32, cfg, opts)
mgr.prepare_initializer()
for ask in (1000, 1300):
    done, _ = mgr.step(ask)
    assert done == ask
print("STOPPED", mgr.status()["num_labels_written"], flush=True)
os._exit(0)     # no reset, no completion: the process just ends
"""


def run_child(d, seal_on):
    r = subprocess.run(
        [sys.executable, "-c",
         _CHILD % (REPO, TOTAL, d, N, PER_FILE * 16, SCRATCH_128, seal_on)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "STOPPED 2300" in r.stdout, \
        r.stdout + r.stderr


@pytest.fixture(scope="module")
def killed(labels, hits_of, tmp_path_factory):
    """An init with the scan on whose process ended after 2300 labels: the
    batches ended at 512, 1000, 1512, 2024 and 2300."""
    d = str(tmp_path_factory.mktemp("killed"))
    run_child(d, False)
    assert read_dir(d) == labels[:2300 * 16]
    check_part(d, hits_of(ZERO, 16), 2300)
    return d


def labels_truncated_unevenly(d, hits):
    # 2101 labels and a torn one
    os.truncate(os.path.join(d, "postdata_1.bin"), 601 * 16 + 7)
    return 2101


def part_cut_inside_a_record(d, hits):
    os.truncate(part_path(d), os.path.getsize(part_path(d)) - 7)
    return 2024


def part_cut_before_its_marker(d, hits):
    assert any(2024 <= i < 2300 for i, _ in hits)
    os.truncate(part_path(d), os.path.getsize(part_path(d)) - 16)
    with open(part_path(d), "rb") as f:
        last = f.read()[-16:]
    assert last[12:] == bytes(4)            # a hit, its marker gone
    return 2024


def part_ahead_of_labels(d, hits):
    os.truncate(os.path.join(d, "postdata_1.bin"), 300 * 16)
    return 1800


@pytest.mark.parametrize("alter", [
    labels_truncated_unevenly, part_cut_inside_a_record,
    part_cut_before_its_marker, part_ahead_of_labels])
def test_kill_and_resume(labels, hits_of, proof_of, killed, tmp_path, alter):
    hits = hits_of(ZERO, 16)
    d = shutil.copytree(killed, str(tmp_path / "d"))
    resume_at = alter(d, hits)
    mgr = make_mgr(d)
    mgr.prepare_initializer()
    assert mgr.status()["num_labels_written"] == resume_at
    check_part(d, hits, resume_at)
    assert os.path.getsize(part_path(d)) == 128 + 16 * (
        len(read_part(d)[1]) + initproof_markers(d))
    mgr.start_session()
    mgr.reset()
    check_part(d, hits, TOTAL)
    check_proved_dir(d, labels, hits, proof_of(ZERO, 16), ZERO, 16)


def initproof_markers(d):
    with open(part_path(d), "rb") as f:
        raw = f.read()[128:]
    return sum(raw[o + 8:o + 16] == b"\xff\xff\xff\xffMARK"
               for o in range(0, len(raw), 16))


# ------------------------- with the seal -------------------------

def cut_part_behind_marker(d, index):
    with open(part_path(d), "rb") as f:
        raw = f.read()
    at = raw.index(initproof.marker(index), 128)
    assert (at - 128) % 16 == 0
    os.truncate(part_path(d), at + 16)


def test_seal_and_scan_together(labels, hits_of, proof_of, tmp_path):
    hits = hits_of(ZERO, 16)
    d = str(tmp_path / "d")
    run_child(d, True)
    assert read_dir(d) == labels[:2300 * 16]
    check_part(d, hits, 2300)
    with open(os.path.join(d, seal.part_name(0)), "rb") as f:
        assert f.read() == seal.part_bytes(labels, 0, TOTAL, 2)
    late = shutil.copytree(d, str(tmp_path / "late"))

    # the seal's point is the lower one: the page boundary below 2300
    mgr = make_mgr(d, seal_on=True)
    mgr.prepare_initializer()
    assert mgr.status()["num_labels_written"] == 2048
    check_part(d, hits, 2048)
    mgr.start_session()
    mgr.reset()
    # the part's point is the lower one: the seal goes back below it
    cut_part_behind_marker(late, 1512)
    mgr = make_mgr(late, seal_on=True)
    mgr.prepare_initializer()
    assert mgr.status()["num_labels_written"] == 1024
    check_part(late, hits, 1024)
    with open(os.path.join(late, seal.part_name(0)), "rb") as f:
        assert f.read() == seal.part_bytes(labels, 0, TOTAL, 1)
    mgr.start_session()
    mgr.reset()
    for x in (d, late):
        with open(os.path.join(x, seal.SIDECAR), "rb") as f:
            assert f.read() == seal.sidecar_bytes(labels)
        assert gsm_amd.check_seal(x).clean
        check_part(x, hits, TOTAL)
        check_proved_dir(x, labels, hits, proof_of(ZERO, 16), ZERO, 16)


# ------------------------- two shards -------------------------

SHARDS = [(0, 2048), (2048, TOTAL)]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_two_shards_in_either_order(labels, hits_of, proof_of, tmp_path,
                                    order):
    hits = hits_of(SEVEN, 16)
    first, second = SHARDS[order[0]], SHARDS[order[1]]
    mgr = make_mgr(tmp_path, SEVEN, start=first[0], end=first[1])
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    assert parts(tmp_path) == [initproof.part_name(first[0])]
    check_part(tmp_path, hits, first[1], *first)
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.init_proof_assemble(str(tmp_path))
    assert ei.value.code == Status.IO
    missing = "labels [2048, 3589) are missing" if order == (0, 1) \
        else "labels [0, 2048) are missing"
    assert missing in str(ei.value)

    mgr = make_mgr(tmp_path, SEVEN, start=second[0], end=second[1])
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    check_part(tmp_path, hits, second[1], *second)
    check_proved_dir(tmp_path, labels, hits, proof_of(SEVEN, 16), SEVEN, 16)
    assert gsm_amd.init_proof_assemble(str(tmp_path))[1].parts == 2


# ------------------------- no nonce, refusals, overflow -------------------

def test_no_nonce_reaches_k2(oracle, labels, tmp_path):
    with pytest.raises(ValueError):
        oracle.prove(labels, TOTAL, ZERO, K1, 40, 16, POW_DIFF)
    mgr = make_mgr(tmp_path, k2=40)
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.init_proof_assemble(str(tmp_path))
    assert ei.value.code == Status.NO_NONCE
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.api.prove_dir(str(tmp_path), ZERO, pcfg(k2=40),
                              gsm_amd.ProveOpts(nonces=16))
    assert ei.value.code == Status.NO_NONCE


def test_enable_after_the_first_step_is_refused(tmp_path):
    mgr = make_mgr(tmp_path, proof=False)
    mgr.prepare_initializer()
    lib = mgr.engine.lib
    assert mgr.step(10)[0] == 10
    pc = gsm_amd.InitialProofOpts.of(pcfg()).to_c()
    assert lib.post_init_enable_proof(mgr._session, pc) == Status.INVALID_ARGS
    assert "before the first step" in lib.post_last_error().decode()
    mgr.reset()
    assert parts(tmp_path) == []


def test_dir_started_without_the_scan_is_refused(tmp_path):
    mgr = make_mgr(tmp_path, proof=False)
    mgr.prepare_initializer()
    assert mgr.step(600)[0] == 600
    mgr.reset()
    with pytest.raises(gsm_amd.EngineError) as ei:
        make_mgr(tmp_path).prepare_initializer()
    assert ei.value.code == Status.UNSUPPORTED
    assert "dir was started without the proof scan; finish init and run " \
        "prove" in str(ei.value)
    assert parts(tmp_path) == []


def test_part_of_another_k1_is_refused(killed, tmp_path):
    d = shutil.copytree(killed, str(tmp_path / "d"))
    before = os.path.getsize(part_path(d))
    with pytest.raises(gsm_amd.EngineError) as ei:
        make_mgr(d, k1=K1 + 1).prepare_initializer()
    assert ei.value.code == Status.IO
    assert "disagrees with the session or with the proving config" in \
        str(ei.value)
    assert os.path.getsize(part_path(d)) == before


def test_bad_proving_configs_are_refused(tmp_path):
    mgr = make_mgr(tmp_path, proof=False)
    mgr.prepare_initializer()
    lib = mgr.engine.lib
    pc = gsm_amd.InitialProofOpts.of(pcfg()).to_c()
    assert lib.post_init_enable_proof(mgr._session, None) == \
        Status.INVALID_ARGS
    for nonces in (0, 8, 24):
        pc.nonces = nonces
        assert lib.post_init_enable_proof(mgr._session, pc) == \
            Status.INVALID_ARGS
        assert "multiple of 16" in lib.post_last_error().decode()
    pc.nonces = 16
    pc.pow_mode = gsm_amd.api.POW_MODE_RANDOMX
    assert lib.post_init_enable_proof(mgr._session, pc) == Status.UNSUPPORTED
    assert "RandomX" in lib.post_last_error().decode()
    mgr.reset()
    assert parts(tmp_path) == []
    # and a session without a data dir
    opts = gsm_amd.PostSetupOpts(
        num_units=1, scrypt_n=N, scratch_bytes=SCRATCH_128,
        initial_proof=gsm_amd.InitialProofOpts.of(pcfg()))
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.PostSetupManager(NODE, ATX, pcfg(), opts).prepare_initializer()
    assert ei.value.code == Status.INVALID_ARGS


def test_a_batch_with_more_hits_than_room_fails_its_step(oracle, tmp_path):
    """N = 2 and K1 = the label count: every label is a hit for every nonce.
    A batch is 512 labels, so the session chose the upper bound of 65536
    records; 227 labels at 288 nonces are 65376 records and fit, 228 are the
    smallest count * nonces above it."""
    total, nonces, n = 1024, 288, 2
    cap = initproof.hit_capacity(512, nonces, total, total)
    assert cap == 65536 and 227 * nonces <= cap < 228 * nonces
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total,
                             k1=total, k2=K2, pow_difficulty=POW_DIFF)
    opts = gsm_amd.PostSetupOpts(
        data_dir=str(tmp_path), num_units=1, scrypt_n=n,
        max_file_size=PER_FILE * 16, scratch_bytes=128 * n * 128,
        initial_proof=gsm_amd.InitialProofOpts.of(
            cfg, gsm_amd.ProveOpts(nonces=nonces)))
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
    mgr.prepare_initializer()
    assert mgr.step(227)[0] == 227
    labels = oracle.init_range(oracle.commitment(NODE, ATX), 0, 227, n,
                               with_nonce=False)[0]
    pows = [oracle.lib.oracle_k2pow(ZERO, g, POW_DIFF)
            for g in range(nonces // 16)]
    want = [(int(i), int(x)) for i, x in oracle.scan_hits(
        labels, 0, total, ZERO, total, nonces, pows)]
    assert len(want) == 227 * nonces
    h, got, complete_to = read_part(tmp_path)
    assert complete_to == 227 and got == want
    size = os.path.getsize(part_path(tmp_path))

    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.step(228)
    assert ei.value.code == Status.ERR
    assert "scan hit buffer overflow" in str(ei.value)
    assert "labels written stays at 227" in str(ei.value)
    assert mgr.status()["num_labels_written"] == 227
    mgr.reset()
    assert os.path.getsize(part_path(tmp_path)) == size
    assert seal.read_stream(str(tmp_path)) == labels


# ------------------------- end to end, child processes -------------------

def cli(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "postcli.py"),
                           *argv], cwd=REPO, capture_output=True, text=True,
                          timeout=120)


def test_cli_init_initial_proof_verify_prove(oracle, labels, tmp_path):
    """postcli's own K1, K2 and nonce count: 26, 37, 288."""
    op = oracle.prove(labels, TOTAL, ZERO, 26, 37, 288, POW_DIFF)
    d = str(tmp_path / "d")
    r = cli("init", "--datadir", d, "--node-id", NODE.hex(), "--atx-id",
            ATX.hex(), "--num-units", "1", "--labels-per-unit", str(TOTAL),
            "--scrypt-n", str(N), "--max-file-size", str(PER_FILE * 16),
            "--pow-difficulty", POW_DIFF.hex(), "--initial-proof")
    assert r.returncode == 0, r.stderr
    assert read_dir(d) == labels
    with open(os.path.join(d, "initial_proof.json")) as f:
        written = json.load(f)
    r = cli("initial-proof", "--datadir", d)
    assert r.returncode == 0, r.stderr
    pj = json.loads(r.stdout)
    assert pj["nonce"] == op.nonce and pj["pow"] == op.pow
    assert bytes.fromhex(pj["scale_encoded_postv1"]) == \
        wire.PostV1(op.nonce, bytes(op.indices[:op.indices_len]),
                            op.pow).encode()
    for key in ("nonce", "indices", "pow", "challenge"):
        assert written[key] == pj[key]
    path = str(tmp_path / "proof.json")
    with open(path, "w") as fh:
        fh.write(r.stdout)
    r = cli("verify", "--datadir", d, "--proof", path, "--pow-difficulty",
            POW_DIFF.hex())
    assert r.returncode == 0 and json.loads(r.stdout) == {"valid": True}, \
        r.stdout + r.stderr
    r = cli("prove", "--datadir", d, "--challenge", ZERO.hex(),
            "--pow-difficulty", POW_DIFF.hex())
    assert r.returncode == 0, r.stderr
    proved = json.loads(r.stdout)
    for key in ("nonce", "indices", "pow", "challenge",
                "scale_encoded_postv1"):
        assert proved[key] == pj[key]
