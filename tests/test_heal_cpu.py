"""Self-healing prove, the parts that need no GPU: the exported
symbols, the validation order of post_prove_healed / post_repair_data
(arguments, the sidecar, the metadata, the stream layout, then the GPU
requirement), and postcli's flag mapping and exit codes over a stubbed
engine."""
import base64
import ctypes
import hashlib
import json
import os
import struct

import pytest

import gsm_amd
from gsm_amd import seal
Status = gsm_amd.api.Status

NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
PER_FILE = 1500
TOTAL = 1500 + 1500 + 700       # three files, four pages


def has_gpu():
    import torch
    return torch.cuda.is_available()


def stream(count, salt=b"heal"):
    out = bytearray()
    i = 0
    while len(out) < count * 16:
        out += hashlib.sha256(salt + struct.pack("<Q", i)).digest()
        i += 1
    return bytes(out[:count * 16])


def write_md(d, lpu=TOTAL, units=1, max_file=PER_FILE * 16, drop=None):
    md = {"NodeId": base64.b64encode(NODE).decode(),
          "CommitmentAtxId": base64.b64encode(ATX).decode(),
          "LabelsPerUnit": lpu, "NumUnits": units, "MaxFileSize": max_file,
          "Scrypt": {"N": 32, "R": 1, "P": 1}}
    if drop:
        del md[drop]
    with open(os.path.join(str(d), "postdata_metadata.json"), "w") as f:
        json.dump(md, f, indent=2)


def make_dir(d, sidecar="good", sizes=(1500, 1500, 700), metadata=True,
             **md):
    """Files of `sizes` labels, the sidecar of exactly that stream (or a
    faulty one), and metadata for files of 1500 labels."""
    d = str(d)
    data = stream(sum(sizes))
    at = 0
    for i, n in enumerate(sizes):
        with open(os.path.join(d, f"postdata_{i}.bin"), "wb") as f:
            f.write(data[at * 16:(at + n) * 16])
        at += n
    good = seal.sidecar_bytes(data)
    body = good[32:]
    total = sum(sizes)
    blob = {
        "absent": None,
        "good": good,
        "short_header": good[:31],
        "short_digests": good[:-1],
        "magic": seal.pack_header(total, magic=b"PSTSEAL0") + body,
        "page_labels": seal.pack_header(total, page_labels=2048) + body,
        "digest_bytes": seal.pack_header(total, digest_bytes=32) + body,
        "stale": seal.sidecar_bytes(data + bytes(16)),
    }[sidecar]
    if blob is not None:
        with open(os.path.join(d, seal.SIDECAR), "wb") as f:
            f.write(blob)
    if metadata:
        write_md(d, **md)
    return d


def prove_cfg(nonces=16):
    pc = gsm_amd.api._CProveConfig()
    pc.k1, pc.k2, pc.nonces = 12, 8, nonces
    ctypes.memmove(pc.pow_difficulty, bytes([0x0F]) + bytes([0xFF]) * 31, 32)
    pc.pow_mode = gsm_amd.api.POW_MODE_BLAKE3
    return pc


def raw_healed(d, cfg="cfg", heal="heal", out="out", bad="buf", cap=4,
               rep="rep", nonces=16):
    lib = gsm_amd.load_engine()
    buf = (ctypes.c_uint64 * 4)()
    r = gsm_amd.api._CHealReport()
    pc, hc = prove_cfg(nonces), gsm_amd.api._CHealConfig(0, 1, 0)
    proof = gsm_amd.api.CProof()
    rc = lib.post_prove_healed(
        d.encode() if d is not None else None,
        ctypes.byref(pc) if cfg == "cfg" else None,
        ctypes.byref(hc) if heal == "heal" else None,
        ctypes.byref(proof) if out == "out" else None,
        buf if bad == "buf" else None, cap,
        ctypes.byref(r) if rep == "rep" else None)
    return Status(rc), lib.post_last_error().decode()


def raw_repair(d, heal="heal", bad="buf", cap=4, rep="rep", **_):
    lib = gsm_amd.load_engine()
    buf = (ctypes.c_uint64 * 4)()
    r = gsm_amd.api._CHealReport()
    hc = gsm_amd.api._CHealConfig(0, 0, 0)
    rc = lib.post_repair_data(
        d.encode() if d is not None else None, 0,
        ctypes.byref(hc) if heal == "heal" else None,
        buf if bad == "buf" else None, cap,
        ctypes.byref(r) if rep == "rep" else None)
    return Status(rc), lib.post_last_error().decode()


BOTH = pytest.mark.parametrize("call", [raw_healed, raw_repair])


def snapshot(d):
    return {n: open(os.path.join(d, n), "rb").read()
            for n in sorted(os.listdir(d))}


# ------------------------- exported symbols -------------------------

def test_the_two_symbols_and_the_api_names_are_exported():
    lib = gsm_amd.load_engine()
    for name in ("post_prove_healed", "post_repair_data"):
        assert hasattr(lib, name), name
    for name in ("prove_healed", "repair_data", "HealOpts", "HealReport"):
        assert callable(getattr(gsm_amd, name)), name
    assert ctypes.sizeof(gsm_amd.api._CHealConfig) == 16
    assert ctypes.sizeof(gsm_amd.api._CHealReport) == 88
    h = gsm_amd.HealOpts()
    assert (h.max_pages, h.write_back, h.scratch_bytes) == (0, False, 0)


# ------------------------- validation order -------------------------

def test_null_arguments_come_first(tmp_path):
    d = make_dir(tmp_path, "absent", metadata=False)   # IO if it were read
    assert raw_healed(None)[0] == Status.INVALID_ARGS
    for arg in ("cfg", "heal", "out", "rep"):
        assert raw_healed(d, **{arg: None})[0] == Status.INVALID_ARGS, arg
    assert raw_healed(d, bad=None, cap=1)[0] == Status.INVALID_ARGS
    assert raw_repair(None)[0] == Status.INVALID_ARGS
    for arg in ("heal", "rep"):
        assert raw_repair(d, **{arg: None})[0] == Status.INVALID_ARGS, arg
    assert raw_repair(d, bad=None, cap=1)[0] == Status.INVALID_ARGS
    # bad_pages may be NULL when cap is 0: the next rung answers
    for call in (raw_healed, raw_repair):
        code, msg = call(d, bad=None, cap=0)
        assert code == Status.IO and "cannot open" in msg


@pytest.mark.parametrize("sidecar,says", [
    ("absent", "cannot open"),
    ("short_header", "shorter"),
    ("short_digests", "shorter"),
    ("magic", "magic"),
    ("page_labels", "page_labels"),
    ("digest_bytes", "digest_bytes"),
    ("stale", "postdata length changed since seal"),
])
@BOTH
def test_sidecar_faults_come_before_the_metadata(tmp_path, call, sidecar,
                                                 says):
    # no metadata at all: were it read first, the message would name it
    code, msg = call(make_dir(tmp_path, sidecar, metadata=False))
    assert code == Status.IO
    assert says in msg and "metadata" not in msg, msg


@BOTH
def test_metadata_comes_before_the_layout(tmp_path, call):
    # a short middle file as well: UNSUPPORTED if the layout were looked at
    d = make_dir(tmp_path, "good", sizes=(1500, 1400, 700), metadata=False)
    code, msg = call(d)
    assert code == Status.IO and "postdata_metadata.json" in msg, msg
    for field in ("NodeId", "LabelsPerUnit", "MaxFileSize", "Scrypt"):
        write_md(d, drop=field)
        code, msg = call(d)
        assert code == Status.IO, (field, msg)
        assert "lacks a valid " + ("N" if field == "Scrypt" else field) \
            in msg, msg


@BOTH
def test_layout_comes_before_the_gpu_and_the_prove_config(tmp_path, call):
    # nonces = 7 is INVALID_ARGS for post_prove; the layout comes first
    d = make_dir(tmp_path, "good", sizes=(1500, 1400, 700))
    before = snapshot(d)
    code, msg = call(d, nonces=7)
    assert code == Status.UNSUPPORTED
    assert "global-index" in msg and "postdata_1.bin" in msg, msg
    assert snapshot(d) == before


@BOTH
def test_other_layouts_that_are_refused(tmp_path, call):
    # a last file longer than MaxFileSize / 16
    (tmp_path / "a").mkdir()
    d = make_dir(tmp_path / "a", "good", sizes=(1500, 1501))
    code, msg = call(d)
    assert code == Status.UNSUPPORTED and "postdata_1.bin" in msg, msg
    # a stream longer than the label space of the metadata (a shard's dir
    # would also have its first label at another global index)
    (tmp_path / "b").mkdir()
    d = make_dir(tmp_path / "b", "good", lpu=3000)
    code, msg = call(d)
    assert code == Status.UNSUPPORTED
    assert "NumUnits*LabelsPerUnit" in msg, msg


@BOTH
def test_a_well_formed_dir_reaches_the_gpu_check(tmp_path, call):
    d = make_dir(tmp_path, "good")
    before = snapshot(d)
    code, msg = call(d)
    assert code == (Status.OK if has_gpu() else Status.NO_GPU), msg
    assert snapshot(d) == before     # nothing bad: nothing written
    if call is raw_healed:
        # the prove config is looked at as post_prove looks at it
        assert raw_healed(d, nonces=7)[0] == Status.INVALID_ARGS


# ------------------------- postcli over a stubbed engine -------------------

def report(pages_bad=0, bad_pages=(), total=3 * 1024 + 517, **kw):
    return gsm_amd.HealReport(total, -(-total // 1024), pages_bad,
                              kw.pop("touches_bad", False), list(bad_pages),
                              **kw)


def test_report_properties():
    assert report().publishable and report().repaired and report().clean
    healed = report(2, [1, 3], pages_healed=2, pages_written=2)
    assert healed.publishable and healed.repaired and not healed.clean
    assert healed.bad_label_ranges() == [(1024, 2048), (3072, 3589)]
    assert not report(2, [1, 3], pages_healed=2, pages_written=1,
                      pages_unconfirmed=1).repaired
    assert not report(1, [1], pages_healed=1, pages_unconfirmed=1,
                      proof_touches_unconfirmed_page=True).publishable
    assert not report(2, [1, 3], heal_skipped=True).publishable
    assert not report(2, [1, 3], heal_skipped=True,
                      touches_bad=True).publishable


def run_cli(monkeypatch, capsys, argv, **stubs):
    import postcli
    for name, fn in stubs.items():
        monkeypatch.setattr(gsm_amd, name, fn)
    args = postcli.build_parser().parse_args(argv)
    rc = args.fn(args)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


def test_cli_prove_heal(monkeypatch, capsys, tmp_path):
    write_md(tmp_path, lpu=3589)
    d = str(tmp_path)
    proof = gsm_amd.PostProof(5, b"\x01\x02\x03", 77)
    seen = []

    def stub(rep):
        def prove_healed(data_dir, challenge, cfg, opts, heal=None,
                         max_report=64):
            seen.append((data_dir, challenge, cfg.labels_per_unit,
                         opts.nonces, heal.max_pages, heal.write_back,
                         heal.scratch_bytes, max_report))
            if isinstance(rep, Exception):
                raise rep
            return proof, rep
        return prove_healed

    def not_this(*a, **k):
        raise AssertionError("--heal must go through prove_healed alone")
    monkeypatch.setattr(gsm_amd.api, "prove_dir", not_this)
    monkeypatch.setattr(gsm_amd, "prove_checked", not_this)
    argv = ["prove", "--datadir", d, "--challenge", "07" * 32, "--nonces",
            "32", "--check-seal", "--heal"]

    # clean dir: the proof, nothing on stderr, the defaults mapped
    rc, out, err = run_cli(monkeypatch, capsys, argv,
                           prove_healed=stub(report()))
    assert not rc and seen == [(d, bytes([7]) * 32, 3589, 32, 0, False, 0,
                                64)]
    assert json.loads(out)["nonce"] == 5 and json.loads(out)["pow"] == 77
    assert err == ""

    # everything healed: status 0, the proof, one line per healed range
    rc, out, err = run_cli(
        monkeypatch, capsys,
        argv + ["--write-back", "--max-heal-pages", "9", "--max-report",
                "7"],
        prove_healed=stub(report(2, [1, 3], pages_healed=2, pages_written=2,
                                 labels_repaired=3)))
    assert not rc and seen[-1][4:] == (9, True, 0, 7)
    assert json.loads(out)["nonce"] == 5
    lines = err.splitlines()
    assert lines[:2] == ["healed labels [1024, 2048)",
                         "healed labels [3072, 3589)"]
    assert "2 written back" in lines[2] and "verify-data" not in err

    # an unconfirmed page the proof keeps away from: still status 0
    rc, out, err = run_cli(
        monkeypatch, capsys, argv,
        prove_healed=stub(report(1, [2], pages_healed=1,
                                 pages_unconfirmed=1)))
    assert not rc and json.loads(out)["nonce"] == 5
    assert "1 not confirmed by the seal" in err

    # the proof touches an unconfirmed page: status 1, no proof
    rc, out, err = run_cli(
        monkeypatch, capsys, argv,
        prove_healed=stub(report(1, [2], pages_healed=1, pages_unconfirmed=1,
                                 proof_touches_unconfirmed_page=True)))
    assert rc == 1 and out == ""
    assert "not printed, do not publish" in err

    # healing skipped: status 1, no proof, the verify-data commands
    rc, out, err = run_cli(
        monkeypatch, capsys, argv + ["--max-heal-pages", "1"],
        prove_healed=stub(report(2, [0, 3], heal_skipped=True)))
    assert rc == 1 and out == "" and seen[-1][4] == 1
    assert f"verify-data --datadir {d} --every 1 --from 3072 --to 3589" in err
    assert "do not publish" in err and "healed labels" not in err

    # an engine error: status 2, no proof
    rc, out, err = run_cli(
        monkeypatch, capsys, argv,
        prove_healed=stub(gsm_amd.EngineError(
            Status.UNSUPPORTED, "healing needs the label stream in "
                                "global-index terms")))
    assert rc == 2 and out == "" and "global-index" in err


def test_cli_heal_flags_need_their_parents(monkeypatch, capsys, tmp_path):
    write_md(tmp_path, lpu=3589)

    def not_this(*a, **k):
        raise AssertionError("a usage error must not reach the engine")
    stubs = dict(prove_healed=not_this, prove_checked=not_this)
    monkeypatch.setattr(gsm_amd.api, "prove_dir", not_this)
    base = ["prove", "--datadir", str(tmp_path), "--challenge", "00" * 32]
    for extra in (["--heal"], ["--heal", "--write-back"],
                  ["--check-seal", "--write-back"],
                  ["--check-seal", "--max-heal-pages", "3"]):
        with pytest.raises(SystemExit) as ei:
            run_cli(monkeypatch, capsys, base + extra, **stubs)
        assert "need" in str(ei.value.code), extra


def test_cli_repair(monkeypatch, capsys):
    seen = []

    def stub(rep):
        def repair_data(d, heal=None, provider_id=0, max_report=64):
            seen.append((d, heal.max_pages, provider_id, max_report))
            if isinstance(rep, Exception):
                raise rep
            return rep
        return repair_data

    rc, out, _ = run_cli(monkeypatch, capsys, ["repair", "--datadir", "D"],
                         repair_data=stub(report()))
    assert rc == 0 and seen == [("D", 0, 0, 64)]
    j = json.loads(out)
    assert (j["pages_bad"], j["pages_healed"], j["pages_written"],
            j["pages_unconfirmed"]) == (0, 0, 0, 0)

    rc, out, _ = run_cli(
        monkeypatch, capsys,
        ["repair", "--datadir", "D", "--max-heal-pages", "8", "--provider",
         "2", "--max-report", "3"],
        repair_data=stub(report(2, [1, 3], pages_healed=2, pages_written=2,
                                labels_repaired=5)))
    assert rc == 0 and seen[-1] == ("D", 8, 2, 3)
    j = json.loads(out)
    assert (j["pages_bad"], j["pages_healed"], j["pages_written"],
            j["pages_unconfirmed"], j["labels_repaired"]) == (2, 2, 2, 0, 5)
    assert j["bad"] == [{"page": 1, "from": 1024, "to": 2048},
                        {"page": 3, "from": 3072, "to": 3589}]

    # an unconfirmed page stays bad on disk: check-seal would not be clean
    rc, out, _ = run_cli(
        monkeypatch, capsys, ["repair", "--datadir", "D"],
        repair_data=stub(report(2, [1, 3], pages_healed=2, pages_written=1,
                                pages_unconfirmed=1)))
    assert rc == 1 and json.loads(out)["pages_unconfirmed"] == 1
    rc, out, _ = run_cli(
        monkeypatch, capsys, ["repair", "--datadir", "D"],
        repair_data=stub(report(9, [1, 3], heal_skipped=True)))
    assert rc == 1 and json.loads(out)["heal_skipped"] is True

    rc, out, err = run_cli(
        monkeypatch, capsys, ["repair", "--datadir", "D"],
        repair_data=stub(gsm_amd.EngineError(Status.IO, "cannot open X")))
    assert rc == 2 and out == "" and "cannot open" in err
