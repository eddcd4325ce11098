"""Postdata seal, the parts that need no GPU: the host-only
restatement of the format in seal.py, the exported symbols, the validation
order of post_check_seal / post_prove_checked (arguments, then the sidecar,
then the GPU requirement), and postcli's mapping and exit codes over a
stubbed engine."""
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

COUNTS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2048, 3 * 1024 + 517]
NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32


def has_gpu():
    import torch
    return torch.cuda.is_available()


def stream(count, salt=b"seal"):
    """count deterministic pseudo-random labels."""
    out = bytearray()
    i = 0
    while len(out) < count * 16:
        out += hashlib.sha256(salt + struct.pack("<Q", i)).digest()
        i += 1
    return bytes(out[:count * 16])


# ------------------------- format restatement -------------------------

def test_header_round_trip():
    for total in (0, 1, 1024, 1025, (1 << 34) + 3, (1 << 64) - 1):
        h = seal.pack_header(total)
        assert len(h) == seal.HEADER_SIZE == 32
        assert h[:8] == b"PSTSEAL1"
        assert h[8:12] == (1024).to_bytes(4, "little")
        assert h[12:16] == (16).to_bytes(4, "little")
        assert h[16:24] == total.to_bytes(8, "little")
        assert h[24:32] == bytes(8)
        assert seal.unpack_header(h) == {
            "page_labels": 1024, "digest_bytes": 16, "total_labels": total,
            "reserved": 0}


def test_header_refuses_what_the_engine_refuses():
    good = seal.pack_header(5)
    for bad in (good[:31], seal.pack_header(5, magic=b"PSTSEAL2"),
                seal.pack_header(5, page_labels=512),
                seal.pack_header(5, digest_bytes=32)):
        with pytest.raises(ValueError):
            seal.unpack_header(bad)


@pytest.mark.parametrize("count", COUNTS)
def test_page_digests_restate_sha256_per_page(count):
    data = stream(count)
    got = seal.page_digests(data)
    pages = -(-count // 1024)
    assert seal.num_pages(count) == pages and len(got) == 16 * pages
    for p in range(pages):
        page = data[p * 16384:(p + 1) * 16384]
        assert len(page) == 16 * min(1024, count - 1024 * p)
        assert got[16 * p:16 * p + 16] == hashlib.sha256(page).digest()[:16]
    # bytes short of a whole label are not part of the stream
    assert seal.page_digests(data + b"\x01" * 15) == got
    assert seal.sidecar_bytes(data) == seal.pack_header(count) + got


def test_read_stream_stops_at_the_first_absent_file(tmp_path):
    parts = [stream(1500, b"a"), stream(7, b"b") + b"xyz", stream(9, b"c")]
    for i, name in enumerate(["postdata_0.bin", "postdata_1.bin",
                              "postdata_3.bin"]):
        (tmp_path / name).write_bytes(parts[i])
    assert seal.read_stream(str(tmp_path)) == parts[0] + parts[1][:7 * 16]


# ------------------------- exported symbols -------------------------

def test_the_four_symbols_are_exported():
    lib = gsm_amd.load_engine()
    for name in ("post_seal_digest_buffer", "post_seal_data",
                 "post_check_seal", "post_prove_checked"):
        assert hasattr(lib, name), name
    for name in ("seal_data", "check_seal", "prove_checked",
                 "seal_digest_buffer"):
        assert callable(getattr(gsm_amd, name))
    assert ctypes.sizeof(gsm_amd.api._CSealReport) == 32


# ------------------------- validation order -------------------------

TOTAL = 1500 + 700          # two files, three pages


def make_dir(d, sidecar="good"):
    d = str(d)
    data = stream(TOTAL)
    with open(os.path.join(d, "postdata_0.bin"), "wb") as f:
        f.write(data[:1500 * 16])
    with open(os.path.join(d, "postdata_1.bin"), "wb") as f:
        f.write(data[1500 * 16:])
    good = seal.sidecar_bytes(data)
    body = good[32:]
    blob = {
        "absent": None,
        "good": good,
        "short_header": good[:31],
        "short_digests": good[:-1],
        "magic": seal.pack_header(TOTAL, magic=b"PSTSEAL0") + body,
        "page_labels": seal.pack_header(TOTAL, page_labels=2048) + body,
        "digest_bytes": seal.pack_header(TOTAL, digest_bytes=32) + body,
        # a well-formed sidecar of a dir that was 16 bytes longer
        "stale": seal.sidecar_bytes(data + bytes(16)),
    }[sidecar]
    if blob is not None:
        with open(os.path.join(d, seal.SIDECAR), "wb") as f:
            f.write(blob)
    return d


def prove_cfg(nonces=16):
    pc = gsm_amd.api._CProveConfig()
    pc.k1, pc.k2, pc.nonces = 12, 8, nonces
    ctypes.memmove(pc.pow_difficulty, bytes([0x0F]) + bytes([0xFF]) * 31, 32)
    pc.pow_mode = gsm_amd.api.POW_MODE_BLAKE3
    return pc


def raw_check(d, bad="buf", cap=4, rep="rep"):
    lib = gsm_amd.load_engine()
    buf = (ctypes.c_uint64 * 4)()
    r = gsm_amd.api._CSealReport()
    rc = lib.post_check_seal(
        d.encode() if d is not None else None, 0,
        buf if bad == "buf" else None, cap,
        ctypes.byref(r) if rep == "rep" else None)
    return Status(rc), lib.post_last_error().decode()


def raw_prove_checked(d, cfg="cfg", out="out", bad="buf", cap=4, rep="rep"):
    lib = gsm_amd.load_engine()
    buf = (ctypes.c_uint64 * 4)()
    r = gsm_amd.api._CSealReport()
    pc, proof = prove_cfg(), gsm_amd.api.CProof()
    rc = lib.post_prove_checked(
        d.encode() if d is not None else None,
        ctypes.byref(pc) if cfg == "cfg" else None,
        ctypes.byref(proof) if out == "out" else None,
        buf if bad == "buf" else None, cap,
        ctypes.byref(r) if rep == "rep" else None)
    return Status(rc), lib.post_last_error().decode()


def test_null_arguments_are_invalid_args_before_anything_is_read(tmp_path):
    d = make_dir(tmp_path, "absent")      # no sidecar: IO if it were read
    assert raw_check(None)[0] == Status.INVALID_ARGS
    assert raw_check(d, rep=None)[0] == Status.INVALID_ARGS
    assert raw_check(d, bad=None, cap=1)[0] == Status.INVALID_ARGS
    assert raw_prove_checked(None)[0] == Status.INVALID_ARGS
    assert raw_prove_checked(d, cfg=None)[0] == Status.INVALID_ARGS
    assert raw_prove_checked(d, out=None)[0] == Status.INVALID_ARGS
    assert raw_prove_checked(d, rep=None)[0] == Status.INVALID_ARGS
    assert raw_prove_checked(d, bad=None, cap=1)[0] == Status.INVALID_ARGS
    # bad_pages may be NULL when cap is 0: the next rung answers
    assert raw_check(d, bad=None, cap=0)[0] == Status.IO
    assert raw_prove_checked(d, bad=None, cap=0)[0] == Status.IO
    lib = gsm_amd.load_engine()
    r = gsm_amd.api._CSealReport()
    assert lib.post_seal_data(None, 0, ctypes.byref(r)) == Status.INVALID_ARGS
    assert lib.post_seal_data(d.encode(), 0, None) == Status.INVALID_ARGS
    n = ctypes.c_uint64(0)
    out = ctypes.create_string_buffer(32)
    lab = stream(1025)
    for args in ((None, 1025, 0, out, 2, ctypes.byref(n)),
                 (lab, 1025, 0, None, 2, ctypes.byref(n)),
                 (lab, 1025, 0, out, 2, None),
                 (lab, 0, 0, out, 2, ctypes.byref(n)),
                 (lab, 1025, 0, out, 1, ctypes.byref(n))):   # cap too small
        assert lib.post_seal_digest_buffer(*args) == Status.INVALID_ARGS


@pytest.mark.parametrize("sidecar,says", [
    ("absent", "cannot open"),
    ("short_header", "shorter"),
    ("short_digests", "shorter"),
    ("magic", "magic"),
    ("page_labels", "page_labels"),
    ("digest_bytes", "digest_bytes"),
    ("stale", "postdata length changed since seal"),
])
@pytest.mark.parametrize("call", [raw_check, raw_prove_checked])
def test_each_sidecar_rung_is_io_with_its_own_message(tmp_path, call,
                                                      sidecar, says):
    code, msg = call(make_dir(tmp_path, sidecar))
    assert code == Status.IO
    assert says in msg, msg


@pytest.mark.parametrize("call", [raw_check, raw_prove_checked])
def test_truncated_and_removed_files_are_a_changed_length(tmp_path, call):
    d = make_dir(tmp_path, "good")
    p1 = os.path.join(d, "postdata_1.bin")
    os.truncate(p1, os.path.getsize(p1) - 16)
    code, msg = call(d)
    assert code == Status.IO and "length changed since seal" in msg
    os.remove(p1)
    code, msg = call(d)
    assert code == Status.IO and "length changed since seal" in msg


def test_sidecar_is_validated_before_the_prove_config(tmp_path):
    # nonces = 7 is INVALID_ARGS for post_prove; the stale seal comes first
    lib = gsm_amd.load_engine()
    r = gsm_amd.api._CSealReport()
    pc, proof = prove_cfg(nonces=7), gsm_amd.api.CProof()
    d = make_dir(tmp_path, "stale")
    rc = lib.post_prove_checked(d.encode(), ctypes.byref(pc),
                                ctypes.byref(proof), None, 0,
                                ctypes.byref(r))
    assert rc == Status.IO


def test_well_formed_sidecar_reaches_the_gpu_check(tmp_path):
    d = make_dir(tmp_path, "good")
    want = Status.OK if has_gpu() else Status.NO_GPU
    assert raw_check(d)[0] == want
    if not has_gpu():
        assert raw_prove_checked(d)[0] == Status.NO_GPU
        lib = gsm_amd.load_engine()
        r = gsm_amd.api._CSealReport()
        assert lib.post_seal_data(d.encode(), 0,
                                  ctypes.byref(r)) == Status.NO_GPU
        with pytest.raises(gsm_amd.EngineError) as ei:
            gsm_amd.seal_digest_buffer(stream(5))
        assert ei.value.code == Status.NO_GPU
        # nothing was written, nothing is left behind
        assert sorted(os.listdir(d)) == ["postdata_0.bin", "postdata_1.bin",
                                         seal.SIDECAR]


# ------------------------- postcli over a stubbed engine -------------------

def report(pages_bad, bad_pages, touches=False, total=3 * 1024 + 517):
    return gsm_amd.SealReport(total, -(-total // 1024), pages_bad, touches,
                              bad_pages)


def test_report_ranges_clip_the_ragged_last_page():
    rep = report(3, [0, 2, 3])
    assert rep.bad_label_ranges() == [(0, 1024), (2048, 3072), (3072, 3589)]
    assert not rep.clean and report(0, []).clean


def run_cli(monkeypatch, capsys, argv, **stubs):
    import postcli
    for name, fn in stubs.items():
        monkeypatch.setattr(gsm_amd, name, fn)
    args = postcli.build_parser().parse_args(argv)
    rc = args.fn(args)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


def test_cli_seal_maps_arguments(monkeypatch, capsys):
    seen = []

    def seal_data(d, provider):
        seen.append((d, provider))
        return report(0, [])
    rc, out, _ = run_cli(monkeypatch, capsys,
                         ["seal", "--datadir", "D", "--provider", "3"],
                         seal_data=seal_data)
    assert rc == 0 and seen == [("D", 3)]
    j = json.loads(out)
    assert j["total_labels"] == 3589 and j["pages"] == 4


def test_cli_check_seal_exit_codes_and_ranges(monkeypatch, capsys):
    seen = []

    def clean(d, provider, max_report):
        seen.append((d, provider, max_report))
        return report(0, [])
    rc, out, _ = run_cli(monkeypatch, capsys,
                         ["check-seal", "--datadir", "D"], check_seal=clean)
    assert rc == 0 and seen == [("D", 0, 64)]
    assert json.loads(out)["pages_bad"] == 0 and json.loads(out)["bad"] == []

    def dirty(d, provider, max_report):
        seen.append((d, provider, max_report))
        return report(3, [1, 3][:max_report])
    rc, out, _ = run_cli(monkeypatch, capsys,
                         ["check-seal", "--datadir", "D", "--max-report", "2",
                          "--provider", "1"], check_seal=dirty)
    assert rc == 1 and seen[-1] == ("D", 1, 2)
    j = json.loads(out)
    assert j["pages_bad"] == 3          # the full count, whatever the cap
    assert j["bad"] == [{"page": 1, "from": 1024, "to": 2048},
                        {"page": 3, "from": 3072, "to": 3589}]

    def broken(d, provider, max_report):
        raise gsm_amd.EngineError(Status.IO, "postdata length changed since "
                                             "seal")
    rc, out, err = run_cli(monkeypatch, capsys,
                           ["check-seal", "--datadir", "D"],
                           check_seal=broken)
    assert rc == 2 and out == "" and "length changed" in err


def write_md(d):
    with open(os.path.join(str(d), "postdata_metadata.json"), "w") as f:
        json.dump({"NodeId": base64.b64encode(NODE).decode(),
                   "CommitmentAtxId": base64.b64encode(ATX).decode(),
                   "LabelsPerUnit": 3589, "NumUnits": 1,
                   "MaxFileSize": 1500 * 16,
                   "Scrypt": {"N": 32, "R": 1, "P": 1}}, f)


def test_cli_prove_check_seal(monkeypatch, capsys, tmp_path):
    write_md(tmp_path)
    d = str(tmp_path)
    proof = gsm_amd.PostProof(5, b"\x01\x02\x03", 77)
    seen = []

    def stub(rep):
        def prove_checked(data_dir, challenge, cfg, opts, max_report=64):
            seen.append((data_dir, challenge, cfg.labels_per_unit,
                         opts.nonces, max_report))
            return proof, rep
        return prove_checked

    def no_plain_prove(*a, **k):
        raise AssertionError("--check-seal must not call post_prove")
    monkeypatch.setattr(gsm_amd.api, "prove_dir", no_plain_prove)
    argv = ["prove", "--datadir", d, "--challenge", "07" * 32, "--nonces",
            "32", "--check-seal"]

    rc, out, err = run_cli(monkeypatch, capsys, argv,
                           prove_checked=stub(report(0, [])))
    assert not rc and seen == [(d, bytes([7]) * 32, 3589, 32, 64)]
    assert json.loads(out)["nonce"] == 5 and json.loads(out)["pow"] == 77
    assert "verify-data" not in err

    # bad pages the proof does not touch: proof printed, ranges on stderr
    rc, out, err = run_cli(monkeypatch, capsys, argv + ["--max-report", "9"],
                           prove_checked=stub(report(2, [0, 3])))
    assert not rc and seen[-1][-1] == 9
    assert json.loads(out)["nonce"] == 5
    assert f"verify-data --datadir {d} --every 1 --from 0 --to 1024" in err
    assert f"verify-data --datadir {d} --every 1 --from 3072 --to 3589" in err

    # the proof touches a bad page: status 1, no proof
    rc, out, err = run_cli(monkeypatch, capsys, argv,
                           prove_checked=stub(report(1, [2], touches=True)))
    assert rc == 1 and out == ""
    assert "--from 2048 --to 3072" in err and "do not publish" in err


def test_cli_prove_without_check_seal_is_unchanged(monkeypatch, capsys,
                                                   tmp_path):
    write_md(tmp_path)
    proof = gsm_amd.PostProof(5, b"\x01\x02\x03", 77)
    monkeypatch.setattr(gsm_amd.api, "prove_dir",
                        lambda d, ch, cfg, opts: proof)

    def no_checked(*a, **k):
        raise AssertionError("prove without --check-seal must use post_prove")
    rc, out, _ = run_cli(monkeypatch, capsys,
                         ["prove", "--datadir", str(tmp_path), "--challenge",
                          "00" * 32], prove_checked=no_checked)
    assert not rc and json.loads(out)["nonce"] == 5
