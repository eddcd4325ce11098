"""Seal during init, the part that needs no GPU: the part-file
format restated in seal.py, post_seal_assemble over part files built by
seal.py, the first rung of post_init_enable_seal, and postcli's flags and
exit codes over a stubbed engine."""
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
TOTAL = 3 * 1024 + 517          # four pages, the last ragged


def stream(count, salt=b"seal-init"):
    """count deterministic pseudo-random labels."""
    out = bytearray()
    i = 0
    while len(out) < count * 16:
        out += hashlib.sha256(salt + struct.pack("<Q", i)).digest()
        i += 1
    return bytes(out[:count * 16])


DATA = stream(TOTAL)


def write_metadata(d, total=TOTAL):
    md = {"NodeId": base64.b64encode(NODE).decode(),
          "CommitmentAtxId": base64.b64encode(ATX).decode(),
          "LabelsPerUnit": total, "NumUnits": 1, "MaxFileSize": 1500 * 16,
          "Scrypt": {"N": 32, "R": 1, "P": 1}}
    with open(os.path.join(d, "postdata_metadata.json"), "w") as f:
        json.dump(md, f, indent=2)


def put_part(d, start, end, pages_done=None, name_start=None, blob=None):
    blob = seal.part_bytes(DATA, start, end, pages_done) if blob is None \
        else blob
    name = seal.part_name(start if name_start is None else name_start)
    with open(os.path.join(d, name), "wb") as f:
        f.write(blob)


def assemble(d):
    lib = gsm_amd.load_engine()
    pages = ctypes.c_uint64(0)
    rc = lib.post_seal_assemble(str(d).encode(), ctypes.byref(pages))
    return Status(rc), lib.post_last_error().decode(), pages.value


# ------------------------- symbols and format -------------------------

def test_the_new_symbols_are_exported():
    lib = gsm_amd.load_engine()
    for name in ("post_init_enable_seal", "post_seal_assemble",
                 "post_seal_digest_stream"):
        assert hasattr(lib, name), name
    for name in ("seal_assemble", "seal_digest_stream"):
        assert callable(getattr(gsm_amd, name))
    fields = [f.name for f in
              __import__("dataclasses").fields(gsm_amd.PostSetupOpts)]
    assert fields[-1] == "seal"
    assert gsm_amd.PostSetupOpts().seal is False


def test_part_header_round_trip():
    h = seal.pack_part_header(5, (1 << 40) + 3)
    assert len(h) == 32 and h[:8] == b"PSTSEALP"
    assert h[8:12] == (1024).to_bytes(4, "little")
    assert h[12:16] == (16).to_bytes(4, "little")
    assert h[16:24] == (5).to_bytes(8, "little")
    assert h[24:32] == ((1 << 40) + 3).to_bytes(8, "little")
    assert seal.unpack_part_header(h) == {
        "page_labels": 1024, "digest_bytes": 16, "first_page": 5,
        "end_page": (1 << 40) + 3}
    with pytest.raises(ValueError):
        seal.unpack_part_header(seal.pack_header(7))   # the sidecar's magic
    with pytest.raises(ValueError):
        seal.unpack_part_header(h[:31])
    assert seal.part_name(2048) == "postdata_seal.part-2048"


def test_part_bytes_and_stream_digests_restate_sha256_per_page():
    want = [hashlib.sha256(DATA[p * 16384:(p + 1) * 16384]).digest()[:16]
            for p in range(4)]
    assert seal.stream_digests(DATA, cuts=[1, 700, 2900]) == b"".join(want)
    assert seal.stream_digests(DATA, stream_end=False) == b"".join(want[:3])
    part = seal.part_bytes(DATA, 2048, TOTAL)
    assert seal.unpack_part_header(part) == {
        "page_labels": 1024, "digest_bytes": 16, "first_page": 2,
        "end_page": 4}
    assert part[32:] == b"".join(want[2:])
    assert seal.part_bytes(DATA, 0, 2048, pages_done=1)[32:] == want[0]


# ------------------------- post_init_enable_seal -------------------------

def test_enable_seal_refuses_a_null_session():
    lib = gsm_amd.load_engine()
    assert lib.post_init_enable_seal(None) == Status.INVALID_ARGS
    assert "data dir" in lib.post_last_error().decode()


# ------------------------- post_seal_assemble -------------------------

def test_assemble_null_dir_and_missing_metadata(tmp_path):
    lib = gsm_amd.load_engine()
    assert lib.post_seal_assemble(None, None) == Status.INVALID_ARGS
    put_part(tmp_path, 0, TOTAL)
    code, msg, _ = assemble(tmp_path)
    assert code == Status.IO and "postdata_metadata.json" in msg


@pytest.mark.parametrize("shards", [
    [(0, TOTAL)],
    [(0, 2048), (2048, TOTAL)],
    [(0, 1024), (1024, 2048), (2048, 3072), (3072, TOTAL)],
])
def test_clean_tiling_gives_the_sidecar_and_removes_the_parts(tmp_path,
                                                               shards):
    d = str(tmp_path)
    write_metadata(d)
    for a, b in shards:
        put_part(d, a, b)
    code, msg, pages = assemble(d)
    assert code == Status.OK, msg
    assert pages == 4
    with open(os.path.join(d, seal.SIDECAR), "rb") as f:
        assert f.read() == seal.sidecar_bytes(DATA)   # ragged last page too
    assert sorted(os.listdir(d)) == ["postdata_metadata.json", seal.SIDECAR]
    # a second run finds the parts gone and the sidecar present
    code, msg, pages = assemble(d)
    assert code == Status.OK and pages == 4
    assert gsm_amd.seal_assemble(d) == 4


def test_whole_pages_only_dir(tmp_path):
    d = str(tmp_path)
    write_metadata(d, total=2048)
    with open(os.path.join(d, seal.part_name(0)), "wb") as f:
        f.write(seal.pack_part_header(0, 2) + seal.page_digests(
            DATA[:2048 * 16]))
    assert assemble(d)[0] == Status.OK
    with open(os.path.join(d, seal.SIDECAR), "rb") as f:
        assert f.read() == seal.sidecar_bytes(DATA[:2048 * 16])


def bad_gap(d):
    put_part(d, 0, 1024)
    put_part(d, 2048, TOTAL)


def bad_tail_gap(d):
    put_part(d, 0, 2048)


def bad_overlap(d):
    put_part(d, 0, 2048)
    put_part(d, 1024, TOTAL)


def bad_short(d):
    put_part(d, 0, 2048, pages_done=1)
    put_part(d, 2048, TOTAL)


def bad_magic(d):
    put_part(d, 0, 2048)
    put_part(d, 2048, TOTAL, blob=seal.pack_part_header(
        2, 4, magic=b"PSTSEAL1") + bytes(32))


def bad_name(d):
    put_part(d, 0, 2048)
    put_part(d, 2048, TOTAL, name_start=1024)


def bad_none(d):
    pass


@pytest.mark.parametrize("make,says", [
    (bad_gap, "gap: pages [1, 2) are missing"),
    (bad_tail_gap, "gap: pages [2, 4) are missing"),
    (bad_overlap, "overlap: pages [1, 2)"),
    (bad_short, "is short, its shard is not finished: pages [1, 2) are "
                "missing"),
    (bad_magic, "wrong magic"),
    (bad_name, "first_page 2 disagrees with the file name"),
    (bad_none, "pages [0, 4) are missing"),
])
def test_each_bad_tiling_is_io_with_its_own_message(tmp_path, make, says):
    d = str(tmp_path)
    write_metadata(d)
    make(d)
    before = sorted(os.listdir(d))
    code, msg, _ = assemble(d)
    assert code == Status.IO
    assert says in msg, msg
    # nothing written, nothing removed
    assert sorted(os.listdir(d)) == before
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.seal_assemble(d)
    assert ei.value.code == Status.IO


# ------------------------- postcli over a stubbed engine -------------------

def run_cli(monkeypatch, capsys, argv, **stubs):
    import postcli
    for name, fn in stubs.items():
        monkeypatch.setattr(gsm_amd, name, fn)
    args = postcli.build_parser().parse_args(argv)
    rc = args.fn(args)
    cap = capsys.readouterr()
    return rc, cap.out, cap.err


def test_cli_seal_assemble(monkeypatch, capsys):
    seen = []

    def no_pass(*a):
        raise AssertionError("seal --assemble must not run the GPU pass")

    def ok(d):
        seen.append(d)
        return 4

    rc, out, _ = run_cli(monkeypatch, capsys,
                         ["seal", "--datadir", "D", "--assemble"],
                         seal_assemble=ok, seal_data=no_pass)
    assert rc == 0 and seen == ["D"]
    assert json.loads(out)["pages"] == 4

    def missing(d):
        raise gsm_amd.EngineError(Status.IO, "pages [2, 4) are missing")

    rc, out, err = run_cli(monkeypatch, capsys,
                           ["seal", "--datadir", "D", "--assemble"],
                           seal_assemble=missing, seal_data=no_pass)
    assert rc == 2 and out == ""
    assert "pages [2, 4) are missing" in err


def test_cli_seal_without_assemble_is_unchanged(monkeypatch, capsys):
    def no_assemble(d):
        raise AssertionError("plain seal must not assemble")

    rc, out, _ = run_cli(
        monkeypatch, capsys, ["seal", "--datadir", "D"],
        seal_assemble=no_assemble,
        seal_data=lambda d, p: gsm_amd.SealReport(3589, 4, 0, False, []))
    assert rc == 0 and json.loads(out)["pages"] == 4


class StubManager:
    """PostSetupManager as cmd_init uses it."""
    made = []
    refuse = None

    def __init__(self, node, atx, cfg, opts):
        self.opts = opts
        StubManager.made.append(self)

    def prepare_initializer(self):
        if StubManager.refuse and self.opts.seal:
            raise gsm_amd.EngineError(*StubManager.refuse)

    def status(self):
        return {"state": 2, "num_labels_written": 0}

    def start_session(self):
        pass

    def vrf_nonce(self):
        return 7, bytes(32)

    def reset(self):
        pass


INIT_ARGV = ["init", "--datadir", "D", "--node-id", NODE.hex(), "--atx-id",
             ATX.hex(), "--num-units", "1", "--labels-per-unit", "3589",
             "--scrypt-n", "32"]


def test_cli_init_seal_flag_reaches_the_opts(monkeypatch, capsys):
    StubManager.made, StubManager.refuse = [], None
    rc, out, _ = run_cli(monkeypatch, capsys, INIT_ARGV,
                         PostSetupManager=StubManager)
    assert not rc and StubManager.made[-1].opts.seal is False
    rc, out, _ = run_cli(monkeypatch, capsys, INIT_ARGV + ["--seal"],
                         PostSetupManager=StubManager)
    assert not rc and StubManager.made[-1].opts.seal is True
    assert json.loads(out)["labels"] == 3589


def test_cli_init_seal_unaligned_shard_exits_2(monkeypatch, capsys):
    StubManager.made = []
    StubManager.refuse = (Status.UNSUPPORTED,
                          "seal during init needs a range of whole "
                          "1024-label pages")
    rc, out, err = run_cli(monkeypatch, capsys,
                           INIT_ARGV + ["--seal", "--shard", "1/2"],
                           PostSetupManager=StubManager)
    StubManager.refuse = None
    assert rc == 2 and out == ""
    assert "whole 1024-label pages" in err
    opts = StubManager.made[-1].opts
    assert (opts.index_start, opts.index_end) != (0, 0)
