"""Postdata seal on a real MI355X.

Every expected digest comes from hashlib through the host-only restatement
in seal.py, every expected proof from the CPU oracle.  Label bytes are
pseudo-random: hashing and the proving scan do not care what they hold, so
the tests write their dirs themselves.

Base dir: 3*1024+517 labels (4 pages, the last one ragged) in files of 1500
labels, so the file boundaries 1500 and 3000 fall inside pages 1 and 2.
Chunk dir: 4*4096+1500 labels, run at POST_PROVE_CHUNK_LABELS 4096 (pages
align with chunks, both pipeline buffers reused) and 1500 (rounded up to
2048 on the seal paths)."""
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys

import pytest

import gsm_amd
from gsm_amd import seal
Status = gsm_amd.api.Status

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 1024 * 16
PER_FILE = 1500
TOTAL = 3 * 1024 + 517
CHUNK_TOTAL = 4 * 4096 + 1500
COUNTS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2048, TOTAL]
CHALLENGE = bytes([0x07]) * 32
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
K1, K2, NONCES = 12, 8, 16


def stream(count, salt=b"seal"):
    out = bytearray()
    i = 0
    while len(out) < count * 16:
        out += hashlib.sha256(salt + struct.pack("<Q", i)).digest()
        i += 1
    return bytes(out[:count * 16])


def write_dir(d, data):
    d = str(d)
    os.makedirs(d, exist_ok=True)
    step = PER_FILE * 16
    for f in range(-(-len(data) // step)):
        with open(os.path.join(d, f"postdata_{f}.bin"), "wb") as fh:
            fh.write(data[f * step:(f + 1) * step])
    return d


def flip(d, offsets, bit=None):
    """Flip one bit at each byte offset of the dir's label stream: `bit`, or
    bit k mod 8 at the k-th offset."""
    step = PER_FILE * 16
    for k, off in enumerate(offsets):
        with open(os.path.join(d, f"postdata_{off // step}.bin"),
                  "r+b") as fh:
            fh.seek(off % step)
            b = fh.read(1)[0]
            fh.seek(off % step)
            fh.write(bytes([b ^ (1 << (k % 8 if bit is None else bit))]))


def copy_of(src, tmp_path):
    return shutil.copytree(src, str(tmp_path / "copy"))


@pytest.fixture(scope="module")
def base():
    """The base dir's label stream; never modified."""
    return stream(TOTAL)


@pytest.fixture(scope="module")
def sealed(base, tmp_path_factory):
    """The base dir, sealed on the GPU once; tests copy it."""
    d = write_dir(tmp_path_factory.mktemp("sealed"), base)
    gsm_amd.seal_data(d)
    return d


@pytest.fixture(scope="module")
def chunky():
    return stream(CHUNK_TOTAL, b"chunks")


# ------------------------- the kernel -------------------------

@pytest.mark.parametrize("count", COUNTS)
def test_digests_match_hashlib(base, count):
    data = base[:count * 16]
    assert gsm_amd.seal_digest_buffer(data) == seal.page_digests(data)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
@pytest.mark.parametrize("count", [1024, 1027])
def test_digests_of_constant_pages(byte, count):
    data = bytes([byte]) * (count * 16)
    assert gsm_amd.seal_digest_buffer(data) == seal.page_digests(data)


# ------------------------- seal, then check -------------------------

def test_seal_then_check_clean(base, sealed):
    with open(os.path.join(sealed, seal.SIDECAR), "rb") as f:
        assert f.read() == seal.sidecar_bytes(base)
    # nothing but the label files and the sidecar: no temporary file
    assert sorted(os.listdir(sealed)) == [
        "postdata_0.bin", "postdata_1.bin", "postdata_2.bin", seal.SIDECAR]
    rep = gsm_amd.check_seal(sealed)
    assert (rep.total_labels, rep.pages, rep.pages_bad) == (TOTAL, 4, 0)
    assert rep.bad_pages == [] and rep.clean
    # sealing again replaces the sidecar in place
    rep = gsm_amd.seal_data(sealed)
    assert (rep.total_labels, rep.pages) == (TOTAL, 4)
    assert len(os.listdir(sealed)) == 4


@pytest.mark.parametrize("offsets,pages", [
    ([0], [0]),                             # byte 0 of page 0
    ([PAGE - 1], [0]),                      # last byte of a page
    ([PAGE], [1]),                          # first byte of the next page
    ([TOTAL * 16 - 1], [3]),                # last byte of the ragged page
    ([PER_FILE * 16 - 1], [1]),             # last byte of file 0, in page 1
    ([PER_FILE * 16], [1]),                 # first byte of file 1, in page 1
    ([2 * PER_FILE * 16 - 1, 2 * PER_FILE * 16], [2]),  # files 1|2, page 2
    ([PAGE - 1, PAGE, 3 * PAGE], [0, 1, 3]),
])
def test_one_bit_flips_are_located(sealed, tmp_path, offsets, pages):
    d = copy_of(sealed, tmp_path)
    flip(d, offsets)
    rep = gsm_amd.check_seal(d)
    assert rep.bad_pages == pages
    assert rep.pages_bad == len(pages) and rep.pages == 4


def test_cap_below_the_count_keeps_the_smallest_pages(sealed, tmp_path):
    d = copy_of(sealed, tmp_path)
    flip(d, [3 * PAGE + 5, 0, 2 * PAGE + 1, PAGE + 77])
    for cap, want in [(0, []), (1, [0]), (2, [0, 1]), (3, [0, 1, 2]),
                      (4, [0, 1, 2, 3]), (9, [0, 1, 2, 3])]:
        rep = gsm_amd.check_seal(d, max_report=cap)
        assert rep.bad_pages == want
        assert rep.pages_bad == 4


# ------------------------- chunk crossings -------------------------

# first and last byte of the chunks at 4096 labels, of those at 2048, the
# label 1500 an unrounded chunk would end at, and the ragged last page
CHUNK_FLIPS = [0, 1500 * 16 - 1, 1500 * 16, 2048 * 16 - 1, 2048 * 16,
               4096 * 16 - 1, 4096 * 16, 3 * 4096 * 16 - 1, 4 * 4096 * 16,
               CHUNK_TOTAL * 16 - 1]
CHUNK_BAD = sorted({o // PAGE for o in CHUNK_FLIPS})


@pytest.mark.parametrize("chunk", ["4096", "1500"])
def test_chunk_crossings_change_nothing(chunky, tmp_path, monkeypatch,
                                        chunk):
    monkeypatch.setenv("POST_PROVE_CHUNK_LABELS", chunk)
    want = seal.page_digests(chunky)
    assert len(want) == 16 * 18
    assert gsm_amd.seal_digest_buffer(chunky) == want
    d = write_dir(tmp_path / "d", chunky)
    rep = gsm_amd.seal_data(d)
    assert (rep.total_labels, rep.pages) == (CHUNK_TOTAL, 18)
    with open(os.path.join(d, seal.SIDECAR), "rb") as f:
        assert f.read() == seal.pack_header(CHUNK_TOTAL) + want
    assert gsm_amd.check_seal(d).bad_pages == []
    flip(d, CHUNK_FLIPS)
    rep = gsm_amd.check_seal(d)
    assert rep.bad_pages == CHUNK_BAD == [0, 1, 2, 3, 4, 11, 16, 17]
    assert rep.pages_bad == len(CHUNK_BAD)
    # a seal written at one chunk size is checked at the other
    monkeypatch.setenv("POST_PROVE_CHUNK_LABELS",
                       "1500" if chunk == "4096" else "4096")
    assert gsm_amd.check_seal(d).bad_pages == CHUNK_BAD


# ------------------------- prove_checked -------------------------

def pcfg():
    return gsm_amd.PostConfig(min_num_units=1, labels_per_unit=CHUNK_TOTAL,
                              k1=K1, k2=K2, pow_difficulty=POW_DIFF)


def proof_indices(proof, total):
    bpi = max(1, (total - 1).bit_length())
    v = int.from_bytes(proof.indices, "little")
    return [(v >> (i * bpi)) & ((1 << bpi) - 1) for i in range(K2)]


@pytest.fixture(scope="module")
def proved(oracle, chunky, tmp_path_factory):
    """The chunk dir sealed, and the proof of it from the CPU oracle."""
    d = write_dir(tmp_path_factory.mktemp("proved"), chunky)
    gsm_amd.seal_data(d)
    op = oracle.prove(chunky, CHUNK_TOTAL, CHALLENGE, K1, K2, NONCES,
                      POW_DIFF)
    want = gsm_amd.PostProof(op.nonce, bytes(op.indices[:op.indices_len]),
                             op.pow)
    return d, want


@pytest.mark.parametrize("chunk", [None, "4096", "1500"])
def test_prove_checked_clean_equals_prove_and_oracle(proved, monkeypatch,
                                                     chunk):
    d, want = proved
    if chunk:
        monkeypatch.setenv("POST_PROVE_CHUNK_LABELS", chunk)
    opts = gsm_amd.ProveOpts(nonces=NONCES)
    proof, rep = gsm_amd.prove_checked(d, CHALLENGE, pcfg(), opts)
    assert proof == want
    assert proof == gsm_amd.api.prove_dir(d, CHALLENGE, pcfg(), opts)
    assert (rep.total_labels, rep.pages, rep.pages_bad) == \
        (CHUNK_TOTAL, 18, 0)
    assert rep.bad_pages == [] and not rep.proof_touches_bad_page


def test_prove_checked_flip_away_from_the_proof(proved, tmp_path,
                                                monkeypatch):
    monkeypatch.setenv("POST_PROVE_CHUNK_LABELS", "4096")
    src, want = proved
    idx = proof_indices(want, CHUNK_TOTAL)
    # the last page lies behind every index of the winner: a label changed
    # there can neither remove one of its hits nor let another nonce reach
    # K2 earlier, so the proof is determined
    assert max(idx) < 17 * 1024
    d = copy_of(src, tmp_path)
    flip(d, [17 * PAGE + 40])
    proof, rep = gsm_amd.prove_checked(d, CHALLENGE, pcfg(),
                                       gsm_amd.ProveOpts(nonces=NONCES))
    assert proof == want
    assert rep.pages_bad == 1 and rep.bad_pages == [17]
    assert not rep.proof_touches_bad_page


@pytest.mark.parametrize("byte,bit", [(0, 0), (15, 7)])
def test_prove_checked_flip_inside_a_winning_label(proved, tmp_path,
                                                   monkeypatch, byte, bit):
    monkeypatch.setenv("POST_PROVE_CHUNK_LABELS", "4096")
    src, want = proved
    target = proof_indices(want, CHUNK_TOTAL)[0]
    page = target // 1024
    d = copy_of(src, tmp_path)
    flip(d, [target * 16 + byte], bit=bit)
    proof, rep = gsm_amd.prove_checked(d, CHALLENGE, pcfg(),
                                       gsm_amd.ProveOpts(nonces=NONCES))
    # whether the changed label still passes, and which nonce then wins, is
    # not determined; that the page is reported and what the flag says are
    assert rep.pages_bad == 1 and rep.bad_pages == [page]
    touches = any(i // 1024 == page
                  for i in proof_indices(proof, CHUNK_TOTAL))
    assert rep.proof_touches_bad_page == touches


def test_stale_seal_is_io(sealed, tmp_path):
    d = copy_of(sealed, tmp_path)
    p = os.path.join(d, "postdata_2.bin")
    os.truncate(p, os.path.getsize(p) - 16)
    for call in (lambda: gsm_amd.check_seal(d),
                 lambda: gsm_amd.prove_checked(
                     d, CHALLENGE, pcfg(), gsm_amd.ProveOpts(nonces=NONCES))):
        with pytest.raises(gsm_amd.EngineError) as ei:
            call()
        assert ei.value.code == Status.IO
        assert "postdata length changed since seal" in str(ei.value)


# ------------------------- end to end, child processes -------------------

def cli(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "postcli.py"),
                           *argv], cwd=REPO, capture_output=True, text=True,
                          timeout=120)


def test_cli_seal_flip_check_then_audit_confirms(tmp_path):
    d = str(tmp_path / "d")
    r = cli("init", "--datadir", d, "--node-id", "a5" * 32, "--atx-id",
            "5a" * 32, "--num-units", "2", "--labels-per-unit", "1500",
            "--scrypt-n", "2", "--max-file-size", str(PER_FILE * 16))
    assert r.returncode == 0, r.stderr
    r = cli("seal", "--datadir", d)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["pages"] == 3
    r = cli("check-seal", "--datadir", d)
    assert r.returncode == 0, r.stderr
    flip(d, [2500 * 16 + 3])                # label 2500: file 1, page 2
    r = cli("check-seal", "--datadir", d)
    assert r.returncode == 1, r.stderr
    rep = json.loads(r.stdout)
    assert rep["pages_bad"] == 1
    assert rep["bad"] == [{"page": 2, "from": 2048, "to": 3000}]
    r = cli("verify-data", "--datadir", d, "--every", "1", "--from",
            str(rep["bad"][0]["from"]), "--to", str(rep["bad"][0]["to"]))
    assert r.returncode == 1, r.stderr
    audit = json.loads(r.stdout)
    assert audit["labels_checked"] == 3000 - 2048
    assert audit["labels_bad"] == 1 and audit["bad"][0]["index"] == 2500
