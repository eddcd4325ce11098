"""Initial proof during init, the part that needs no GPU: the
part format restated in initproof.py, post_init_proof_assemble over parts
built by initproof.py from oracle.scan_hits, the rungs of
post_init_enable_proof that need no session, and postcli's flags and exit
codes over a stubbed engine.

Fixture as in tests/test_heal_gpu.py: 3*1024+517 oracle labels at N=32.  Every
expected proof is oracle.prove over those labels."""
import base64
import ctypes
import dataclasses
import json
import os

import pytest

import gsm_amd
from gsm_amd import initproof
Status = gsm_amd.api.Status

NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
N = 32
TOTAL = 3 * 1024 + 517
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
K1, K2 = 12, 8
CHALLENGES = [bytes(32), bytes([0x07]) * 32, bytes([0x01]) * 32]
# the winner oracle.prove picks (K1, K2 = 12, 8), found once on the CPU
WINNERS = {(0x00, 16): 6, (0x07, 16): 8, (0x01, 16): 0, (0x00, 32): 19}
TILINGS = [[(0, TOTAL)],
           [(0, 2048), (2048, TOTAL)],
           [(3072, TOTAL), (1000, 2048), (0, 1000), (2048, 3072)]]


@pytest.fixture(scope="module")
def labels(oracle):
    return oracle.init_range(oracle.commitment(NODE, ATX), 0, TOTAL, N,
                             with_nonce=False)[0]


@pytest.fixture(scope="module")
def hits_of(oracle, labels):
    """(challenge, nonces) -> oracle.scan_hits over the whole space."""
    cache = {}

    def get(challenge, nonces, k1=K1):
        key = (challenge, nonces, k1)
        if key not in cache:
            pows = [oracle.lib.oracle_k2pow(challenge, g, POW_DIFF)
                    for g in range(nonces // 16)]
            cache[key] = [(int(i), int(n)) for i, n in oracle.scan_hits(
                labels, 0, TOTAL, challenge, k1, nonces, pows)]
        return cache[key]
    return get


def oracle_proof(oracle, labels, challenge, nonces, k2=K2):
    op = oracle.prove(labels, TOTAL, challenge, K1, k2, nonces, POW_DIFF)
    return gsm_amd.PostProof(op.nonce, bytes(op.indices[:op.indices_len]),
                             op.pow)


def write_metadata(d, total=TOTAL):
    md = {"NodeId": base64.b64encode(NODE).decode(),
          "CommitmentAtxId": base64.b64encode(ATX).decode(),
          "LabelsPerUnit": total, "NumUnits": 1, "MaxFileSize": 1500 * 16,
          "Scrypt": {"N": N, "R": 1, "P": 1}}
    with open(os.path.join(str(d), "postdata_metadata.json"), "w") as f:
        json.dump(md, f, indent=2)


def header(start, end, challenge=CHALLENGES[0], nonces=16, k1=K1, k2=K2,
           **kw):
    return initproof.PartHeader(nonces, k1, k2, challenge, POW_DIFF, start,
                                end, TOTAL, **kw)


def put_part(d, hits, start, end, name_start=None, marks=None, blob=None,
             **kw):
    if blob is None:
        blob = initproof.build_part(
            header(start, end, **kw),
            [h for h in hits if start <= h[0] < end], marks)
    name = initproof.part_name(start if name_start is None else name_start)
    with open(os.path.join(str(d), name), "wb") as f:
        f.write(blob)
    return blob


def assemble(d):
    lib = gsm_amd.load_engine()
    out = gsm_amd.api.CProof()
    rep = gsm_amd.api._CInitProofReport()
    rc = lib.post_init_proof_assemble(str(d).encode(), ctypes.byref(out),
                                      ctypes.byref(rep))
    return Status(rc), lib.post_last_error().decode(), out, rep


def listing(d):
    return sorted((f, os.stat(os.path.join(str(d), f)).st_size,
                   os.stat(os.path.join(str(d), f)).st_mtime_ns)
                  for f in os.listdir(str(d)))


# ------------------------- symbols and format -------------------------

def test_the_new_symbols_are_exported():
    lib = gsm_amd.load_engine()
    for name in ("post_init_enable_proof", "post_init_proof_assemble"):
        assert hasattr(lib, name), name
    assert callable(gsm_amd.init_proof_assemble)
    # two u64, a third, two u32: as declared in spacemesh_post.h
    assert ctypes.sizeof(gsm_amd.api._CInitProofReport) == 32
    assert gsm_amd.PostSetupOpts().initial_proof is None
    ip = gsm_amd.InitialProofOpts.of(gsm_amd.PostConfig(k1=12, k2=8),
                                     gsm_amd.ProveOpts(nonces=32))
    assert (ip.k1, ip.k2, ip.nonces, ip.challenge) == (12, 8, 32, bytes(32))


def test_part_header_and_records_round_trip():
    h = header(2048, TOTAL, challenge=CHALLENGES[1], nonces=32)
    raw = h.pack()
    assert len(raw) == 128 and raw[:8] == b"PSTHITSP"
    assert raw[8:24] == b"".join(v.to_bytes(4, "little")
                                 for v in (16, 32, K1, K2))
    assert raw[24:56] == CHALLENGES[1] and raw[56:88] == POW_DIFF
    assert raw[88:112] == b"".join(v.to_bytes(8, "little")
                                   for v in (2048, TOTAL, TOTAL))
    assert raw[112:] == bytes(16)
    assert initproof.unpack_header(raw) == h
    with pytest.raises(ValueError):
        initproof.unpack_header(b"PSTSEALP" + raw[8:])
    with pytest.raises(ValueError):
        initproof.unpack_header(raw[:127])
    assert initproof.marker(7) == (7).to_bytes(8, "little") + \
        b"\xff\xff\xff\xff" + b"MARK"
    assert initproof.hit(9, 3) == (9).to_bytes(8, "little") + \
        (3).to_bytes(4, "little") + bytes(4)
    assert initproof.part_name(2048) == "postdata_hits.part-2048"

    hits = [(2100, 3), (2050, 1), (2100, 2), (3000, 0)]
    part = initproof.build_part(h, hits, marks=[2500, TOTAL])
    assert initproof.read_part(part) == (h, sorted(hits), TOTAL)
    # what lies behind the last marker does not count, nor does a torn record
    assert initproof.read_part(part[:-16] + b"\x01") == \
        (h, sorted(hits)[:3], 2500)
    assert initproof.hit_capacity(512, 16, 12, TOTAL) == 4096
    assert initproof.hit_capacity(512, 288, 1024, 1024) == 1 << 16


# ------------------------- post_init_enable_proof -------------------------

def test_enable_proof_refuses_null_arguments():
    lib = gsm_amd.load_engine()
    pc = gsm_amd.InitialProofOpts().to_c()
    assert lib.post_init_enable_proof(None, ctypes.byref(pc)) == \
        Status.INVALID_ARGS
    assert "data dir" in lib.post_last_error().decode()
    assert lib.post_init_enable_proof(None, None) == Status.INVALID_ARGS


# ------------------------- post_init_proof_assemble -------------------------

def test_assemble_null_args_and_missing_metadata(tmp_path, hits_of):
    lib = gsm_amd.load_engine()
    assert lib.post_init_proof_assemble(None, None, None) == \
        Status.INVALID_ARGS
    put_part(tmp_path, hits_of(CHALLENGES[0], 16), 0, TOTAL)
    code, msg, _, _ = assemble(tmp_path)
    assert code == Status.IO and "postdata_metadata.json" in msg


@pytest.mark.parametrize("tiling", TILINGS, ids=["one", "two", "four"])
@pytest.mark.parametrize("challenge,nonces", [
    (CHALLENGES[0], 16), (CHALLENGES[1], 16), (CHALLENGES[2], 16),
    (CHALLENGES[0], 32)], ids=["ch00", "ch07", "ch01", "ch00-32"])
def test_clean_tiling_gives_the_oracle_proof(oracle, labels, hits_of,
                                             tmp_path, tiling, challenge,
                                             nonces):
    want = oracle_proof(oracle, labels, challenge, nonces)
    assert want.nonce == WINNERS[(challenge[0], nonces)]
    hits = hits_of(challenge, nonces)
    write_metadata(tmp_path)
    for start, end in tiling:               # file order: as listed
        put_part(tmp_path, hits, start, end, challenge=challenge,
                 nonces=nonces, marks=[(start + end) // 2, end])
    before = listing(tmp_path)
    got, rep = gsm_amd.init_proof_assemble(str(tmp_path))
    assert got == want
    assert (rep.total_labels, rep.labels_covered, rep.hits, rep.parts) == \
        (TOTAL, TOTAL, len(hits), len(tiling))
    assert gsm_amd.init_proof_assemble(str(tmp_path))[0] == want
    assert listing(tmp_path) == before      # reads only


def test_no_nonce_reaches_k2(oracle, labels, hits_of, tmp_path):
    for ch in CHALLENGES:
        with pytest.raises(ValueError):
            oracle.prove(labels, TOTAL, ch, K1, 40, 16, POW_DIFF)
    write_metadata(tmp_path)
    hits = hits_of(CHALLENGES[0], 16)
    put_part(tmp_path, hits, 0, 2048, k2=40)
    put_part(tmp_path, hits, 2048, TOTAL, k2=40)
    code, msg, _, rep = assemble(tmp_path)
    assert code == Status.NO_NONCE and "no nonce reached k2" in msg
    assert (rep.labels_covered, rep.hits, rep.parts) == (TOTAL, len(hits), 2)
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.init_proof_assemble(str(tmp_path))
    assert ei.value.code == Status.NO_NONCE


def bad_gap(d, hits):
    put_part(d, hits, 0, 1000)
    put_part(d, hits, 2048, TOTAL)


def bad_tail_gap(d, hits):
    put_part(d, hits, 0, 2048)
    put_part(d, hits, 2048, TOTAL, marks=[3000])


def bad_last_shard_absent(d, hits):
    put_part(d, hits, 0, 2048)


def bad_overlap(d, hits):
    put_part(d, hits, 0, 2048)
    put_part(d, hits, 1024, TOTAL)


def bad_k1(d, hits):
    put_part(d, hits, 0, 2048)
    put_part(d, hits, 2048, TOTAL, k1=K1 + 1)


def bad_challenge(d, hits):
    put_part(d, hits, 0, 2048)
    put_part(d, hits, 2048, TOTAL, challenge=CHALLENGES[1])


def bad_magic(d, hits):
    put_part(d, hits, 0, 2048)
    put_part(d, hits, 2048, TOTAL, magic=b"PSTSEALP")


def bad_name(d, hits):
    put_part(d, hits, 0, 2048)
    put_part(d, hits, 2048, TOTAL, name_start=1024)


def bad_torn(d, hits):
    put_part(d, hits, 0, 2048)
    blob = put_part(d, hits, 2048, TOTAL)
    put_part(d, hits, 2048, TOTAL, blob=blob[:-7])


def bad_none(d, hits):
    pass


@pytest.mark.parametrize("make,says", [
    (bad_gap, "gap: labels [1000, 2048) are missing"),
    (bad_tail_gap, "postdata_hits.part-2048 is short, its shard is not "
                   "finished: labels [3000, 3589) are missing"),
    (bad_last_shard_absent, "gap: labels [2048, 3589) are missing"),
    (bad_overlap, "overlap: labels [1024, 2048)"),
    (bad_k1, "postdata_hits.part-2048 differs from postdata_hits.part-0 in "
             "k1"),
    (bad_challenge, "differs from postdata_hits.part-0 in challenge"),
    (bad_magic, "postdata_hits.part-2048 has a wrong magic"),
    (bad_name, "index_start 2048 disagrees with the file name"),
    (bad_torn, "postdata_hits.part-2048 ends inside a record"),
    (bad_none, "no postdata_hits.part-*"),
])
def test_each_assembly_fault_is_io_with_its_own_message(tmp_path, hits_of,
                                                        make, says):
    write_metadata(tmp_path)
    make(tmp_path, hits_of(CHALLENGES[0], 16))
    before = listing(tmp_path)
    code, msg, _, _ = assemble(tmp_path)
    assert code == Status.IO
    assert says in msg, msg
    if make is bad_none:
        assert "labels [0, 3589) are missing" in msg
    assert listing(tmp_path) == before      # nothing written, nothing removed
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.init_proof_assemble(str(tmp_path))
    assert ei.value.code == Status.IO


def test_records_behind_the_last_marker_do_not_count(oracle, labels, hits_of,
                                                     tmp_path):
    """A part is only as complete as its last well-formed marker: hits that
    follow it (a session ended between hits and marker) make the part short,
    and a record out of order ends the reading."""
    hits = hits_of(CHALLENGES[0], 16)
    write_metadata(tmp_path)
    blob = put_part(tmp_path, hits, 0, TOTAL, marks=[2300])
    tail = [h for h in hits if h[0] >= 2300][:3]
    put_part(tmp_path, hits, 0, TOTAL,
             blob=blob + b"".join(initproof.hit(*h) for h in tail))
    code, msg, _, _ = assemble(tmp_path)
    assert code == Status.IO and "labels [2300, 3589) are missing" in msg
    # a hit below the marker in front of it: everything from there is dropped
    put_part(tmp_path, hits, 0, TOTAL,
             blob=blob + initproof.hit(5, 0) + initproof.marker(TOTAL))
    code, msg, _, _ = assemble(tmp_path)
    assert code == Status.IO and "labels [2300, 3589) are missing" in msg


# ------------------------- postcli over a stubbed engine -------------------

def run_cli(monkeypatch, capsys, argv, **stubs):
    import postcli
    for name, fn in stubs.items():
        monkeypatch.setattr(gsm_amd, name, fn)
    args = postcli.build_parser().parse_args(argv)
    rc = args.fn(args)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


class StubManager:
    """PostSetupManager as cmd_init uses it."""
    made = []
    refuse = None

    def __init__(self, node, atx, cfg, opts):
        self.opts = opts
        StubManager.made.append(self)

    def prepare_initializer(self):
        if StubManager.refuse and self.opts.initial_proof is not None:
            raise gsm_amd.EngineError(*StubManager.refuse)

    def status(self):
        return {"state": 2, "num_labels_written": 0}

    def start_session(self):
        pass

    def vrf_nonce(self):
        return 7, bytes(32)

    def reset(self):
        pass


PROOF = gsm_amd.PostProof(6, bytes(range(12)), 99)
REPORT = gsm_amd.InitProofReport(TOTAL, TOTAL, 200, 1)


def init_argv(d):
    return ["init", "--datadir", str(d), "--node-id", NODE.hex(), "--atx-id",
            ATX.hex(), "--num-units", "1", "--labels-per-unit", str(TOTAL),
            "--scrypt-n", str(N), "--pow-difficulty", POW_DIFF.hex()]


def no_assembly(d):
    raise AssertionError("a plain init must not try the assembly")


def test_cli_init_flag_mapping(monkeypatch, capsys, tmp_path):
    StubManager.made, StubManager.refuse = [], None
    rc, out, _ = run_cli(monkeypatch, capsys, init_argv(tmp_path),
                         PostSetupManager=StubManager,
                         init_proof_assemble=no_assembly)
    assert not rc and StubManager.made[-1].opts.initial_proof is None
    assert os.listdir(tmp_path) == []

    rc, out, err = run_cli(
        monkeypatch, capsys, init_argv(tmp_path) + ["--initial-proof"],
        PostSetupManager=StubManager,
        init_proof_assemble=lambda d: (PROOF, REPORT))
    assert not rc
    ip = StubManager.made[-1].opts.initial_proof
    assert dataclasses.asdict(ip) == dataclasses.asdict(
        gsm_amd.InitialProofOpts(pow_difficulty=POW_DIFF))
    assert (ip.k1, ip.k2, ip.nonces, ip.challenge) == (26, 37, 288, bytes(32))
    assert json.loads(out)["labels"] == TOTAL
    with open(tmp_path / "initial_proof.json") as f:
        pj = json.load(f)
    assert (pj["nonce"], pj["pow"], pj["challenge"]) == (6, 99, "00" * 32)
    assert base64.b64decode(pj["indices"]) == PROOF.indices
    assert "scale_encoded_postv1" in pj

    rc, _, _ = run_cli(
        monkeypatch, capsys, init_argv(tmp_path) + [
            "--initial-proof", "--k1", "12", "--k2", "8", "--nonces", "32",
            "--seal"],
        PostSetupManager=StubManager,
        init_proof_assemble=lambda d: (PROOF, REPORT))
    opts = StubManager.made[-1].opts
    ip = opts.initial_proof
    assert not rc and opts.seal is True
    assert (ip.k1, ip.k2, ip.nonces, ip.pow_difficulty) == \
        (12, 8, 32, POW_DIFF)

    with pytest.raises(SystemExit):
        run_cli(monkeypatch, capsys, init_argv(tmp_path) + ["--k1", "12"],
                PostSetupManager=StubManager)


def test_cli_init_outstanding_range_exits_0(monkeypatch, capsys, tmp_path):
    StubManager.made, StubManager.refuse = [], None

    def outstanding(d):
        raise gsm_amd.EngineError(
            Status.IO, "the parts leave a gap: labels [2048, 3589) are "
                       "missing")

    rc, out, err = run_cli(
        monkeypatch, capsys,
        init_argv(tmp_path) + ["--initial-proof", "--shard", "0/2"],
        PostSetupManager=StubManager, init_proof_assemble=outstanding)
    assert rc == 0 and json.loads(out)["labels"] == 1795
    assert "labels [2048, 3589) are missing" in err
    assert os.listdir(tmp_path) == []


def test_cli_init_refusal_exits_2(monkeypatch, capsys, tmp_path):
    StubManager.made = []
    StubManager.refuse = (Status.UNSUPPORTED,
                          "dir was started without the proof scan; finish "
                          "init and run prove")
    rc, out, err = run_cli(monkeypatch, capsys,
                           init_argv(tmp_path) + ["--initial-proof"],
                           PostSetupManager=StubManager,
                           init_proof_assemble=no_assembly)
    StubManager.refuse = None
    assert rc == 2 and out == ""
    assert "started without the proof scan" in err


def test_cli_initial_proof_exit_codes(monkeypatch, capsys):
    seen = []

    def ok(d):
        seen.append(d)
        return PROOF, REPORT

    rc, out, _ = run_cli(monkeypatch, capsys,
                         ["initial-proof", "--datadir", "D"],
                         init_proof_assemble=ok)
    pj = json.loads(out)
    assert rc == 0 and seen == ["D"]
    assert (pj["nonce"], pj["pow"], pj["challenge"]) == (6, 99, "00" * 32)
    assert base64.b64decode(pj["indices"]) == PROOF.indices

    for code, text in ((Status.IO, "labels [2048, 3589) are missing"),
                       (Status.NO_NONCE, "no nonce reached k2")):
        def fails(d, code=code, text=text):
            raise gsm_amd.EngineError(code, text)
        rc, out, err = run_cli(monkeypatch, capsys,
                               ["initial-proof", "--datadir", "D"],
                               init_proof_assemble=fails)
        assert rc == 1 and out == "" and text in err
