"""Self-healing prove on a real MI355X.

Nothing expected comes from the engine.  The labels are the CPU oracle's,
the dir and its metadata are written by the test, every expected proof is
oracle.prove over the clean labels, and the expected hits_dropped /
hits_added are oracle.scan_hits over the corrupt and the clean bytes of the
bad pages.

Fixture: 3*1024+517 oracle labels at N=32 (4 pages, the last one ragged) in
files of 1500 labels, so the file edges 1500 and 3000 fall inside pages 1
and 2.  Scratch is pinned to 128 lanes: a recompute batch is 512 labels and
a one-page heal already spans two of them.  The dir is sealed once; tests
copy it."""
import base64
import json
import os
import shutil
import subprocess
import sys

import pytest

import gsm_amd
Status = gsm_amd.api.Status

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
N = 32
PAGE = 1024 * 16
PER_FILE = 1500
TOTAL = 3 * 1024 + 517
SCRATCH_128 = 128 * N * 128     # budget for exactly 128 lanes at this N
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
K1, K2, NONCES = 12, 8, 16
# picked on the CPU: oracle.prove succeeds on the clean labels for each; the
# winner of 0x01 lies in page 0 alone, the others reach into page 1 and
# across the file edge at label 1500
CHALLENGES = [bytes([c]) * 32 for c in (0x07, 0x01, 0x16, 0x27)]


def ch_id(ch):
    return "ch%02x" % ch[0]


def write_dir(d, data):
    d = str(d)
    os.makedirs(d, exist_ok=True)
    step = PER_FILE * 16
    for f in range(-(-len(data) // step)):
        with open(os.path.join(d, f"postdata_{f}.bin"), "wb") as fh:
            fh.write(data[f * step:(f + 1) * step])
    with open(os.path.join(d, "postdata_metadata.json"), "w") as fh:
        json.dump({"NodeId": base64.b64encode(NODE).decode(),
                   "CommitmentAtxId": base64.b64encode(ATX).decode(),
                   "LabelsPerUnit": TOTAL, "NumUnits": 1,
                   "MaxFileSize": PER_FILE * 16,
                   "Scrypt": {"N": N, "R": 1, "P": 1}}, fh, indent=2)
    return d


def read_dir(d):
    out = b""
    for f in range(-(-TOTAL // PER_FILE)):
        with open(os.path.join(d, f"postdata_{f}.bin"), "rb") as fh:
            out += fh.read()
    return out


def flipped(data, offsets, bit=None):
    """One bit flipped at each byte offset: `bit`, or bit k mod 8 at the
    k-th offset."""
    buf = bytearray(data)
    for k, off in enumerate(offsets):
        buf[off] ^= 1 << (k % 8 if bit is None else bit)
    return bytes(buf)


def put(d, data):
    """Overwrite the dir's label files with `data` (seal and metadata stay)."""
    step = PER_FILE * 16
    for f in range(-(-len(data) // step)):
        with open(os.path.join(d, f"postdata_{f}.bin"), "r+b") as fh:
            fh.write(data[f * step:(f + 1) * step])


def pages_of(offsets):
    return sorted({o // PAGE for o in offsets})


def labels_differing(a, b):
    return sum(a[i:i + 16] != b[i:i + 16] for i in range(0, len(a), 16))


def pcfg():
    return gsm_amd.PostConfig(min_num_units=1, labels_per_unit=TOTAL,
                              k1=K1, k2=K2, pow_difficulty=POW_DIFF)


def popts():
    return gsm_amd.ProveOpts(nonces=NONCES)


def heal(**kw):
    kw.setdefault("scratch_bytes", SCRATCH_128)
    return gsm_amd.HealOpts(**kw)


def proof_indices(proof, k2=K2):
    bpi = max(1, (TOTAL - 1).bit_length())
    v = int.from_bytes(proof.indices, "little")
    return [(v >> (i * bpi)) & ((1 << bpi) - 1) for i in range(k2)]


def oracle_proof(oracle, labels, challenge, k1=K1, k2=K2, nonces=NONCES):
    """oracle.prove as a PostProof, or None when no nonce reaches k2."""
    try:
        op = oracle.prove(labels, TOTAL, challenge, k1, k2, nonces, POW_DIFF)
    except ValueError:
        return None
    return gsm_amd.PostProof(op.nonce, bytes(op.indices[:op.indices_len]),
                             op.pow)


def oracle_hits(oracle, labels, pages, challenge):
    """Hits of the proving scan inside `pages` of `labels`."""
    pows = [oracle.lib.oracle_k2pow(challenge, g, POW_DIFF)
            for g in range(NONCES // 16)]
    return sum(len(oracle.scan_hits(labels[p * PAGE:(p + 1) * PAGE],
                                    p * 1024, TOTAL, challenge, K1, NONCES,
                                    pows)) for p in pages)


@pytest.fixture(scope="module")
def clean(oracle):
    """The oracle labels of the fixture; never modified."""
    labels, _ = oracle.init_range(oracle.commitment(NODE, ATX), 0, TOTAL, N,
                                  with_nonce=False)
    return labels


@pytest.fixture(scope="module")
def want(oracle, clean):
    """challenge -> the oracle's proof over the clean labels (None: none)."""
    return {ch: oracle_proof(oracle, clean, ch) for ch in CHALLENGES}


@pytest.fixture(scope="module")
def sealed(clean, tmp_path_factory):
    d = write_dir(tmp_path_factory.mktemp("sealed"), clean)
    gsm_amd.seal_data(d)
    return d


def corrupt_copy(sealed, tmp_path, data, name="copy"):
    d = shutil.copytree(sealed, str(tmp_path / name))
    put(d, data)
    return d


def check_healed(oracle, clean, corrupt, bad, ch, want, proof, rep,
                 written=0, unconfirmed=0):
    """A healed call over `corrupt` whose bad pages are `bad`."""
    assert want[ch] is not None, "precondition: the oracle proves this one"
    assert proof == want[ch]
    assert (rep.total_labels, rep.pages) == (TOTAL, 4)
    assert rep.pages_bad == len(bad) and rep.bad_pages == bad
    assert not rep.heal_skipped and not rep.proof_touches_bad_page
    assert rep.pages_healed == len(bad)
    assert rep.pages_unconfirmed == unconfirmed
    assert rep.pages_written == written
    assert rep.labels_repaired == labels_differing(corrupt, clean)
    assert rep.hits_dropped == oracle_hits(oracle, corrupt, bad, ch)
    assert rep.hits_added == oracle_hits(oracle, clean, bad, ch)


# ------------------------- nothing to heal -------------------------

def test_the_oracle_proves_every_challenge(want):
    assert all(p is not None for p in want.values())
    touched = [sorted({i // 1024 for i in proof_indices(p)})
               for p in want.values()]
    assert touched[1] == [0] and all(1 in t for t in touched[:1] +
                                     touched[2:])


@pytest.mark.parametrize("ch", CHALLENGES, ids=ch_id)
def test_clean_dir_is_post_prove_and_all_zero(sealed, want, ch):
    before = read_dir(sealed)
    proof, rep = gsm_amd.prove_healed(sealed, ch, pcfg(), popts(),
                                      heal(write_back=True))
    assert want[ch] is not None and proof == want[ch]
    assert proof == gsm_amd.api.prove_dir(sealed, ch, pcfg(), popts())
    assert (rep.total_labels, rep.pages, rep.pages_bad) == (TOTAL, 4, 0)
    assert rep.bad_pages == [] and rep.clean and rep.publishable
    assert (rep.heal_skipped, rep.pages_healed, rep.pages_unconfirmed,
            rep.labels_repaired, rep.hits_dropped, rep.hits_added,
            rep.pages_written) == (False, 0, 0, 0, 0, 0, 0)
    assert not rep.proof_touches_bad_page
    assert not rep.proof_touches_unconfirmed_page
    assert read_dir(sealed) == before


# ------------------------- one-bit flips -------------------------

@pytest.mark.parametrize("offsets", [
    [0],                                    # byte 0 of page 0
    [PAGE - 1],                             # last byte of a page
    [PER_FILE * 16 - 1, PER_FILE * 16],     # files 0|1, inside page 1
    [2 * PER_FILE * 16 - 1, 2 * PER_FILE * 16],     # files 1|2, page 2
    [TOTAL * 16 - 1],                       # last byte of the ragged page
])
def test_one_bit_flips_are_healed(oracle, clean, sealed, want, tmp_path,
                                  offsets):
    corrupt = flipped(clean, offsets)
    d = corrupt_copy(sealed, tmp_path, corrupt)
    ch = CHALLENGES[0]
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(), heal())
    check_healed(oracle, clean, corrupt, pages_of(offsets), ch, want, proof,
                 rep)
    assert rep.labels_repaired == len(offsets) and rep.publishable
    assert read_dir(d) == corrupt           # no write_back: dir as it was


@pytest.mark.parametrize("byte,bit", [(0, 0), (15, 7)])
def test_flip_inside_a_winning_label(oracle, clean, sealed, want, tmp_path,
                                     byte, bit):
    ch = CHALLENGES[0]
    target = proof_indices(want[ch])[0]
    page = target // 1024
    corrupt = flipped(clean, [target * 16 + byte], bit=bit)
    # what the damaged dir proves, from the oracle: it has an index in the
    # bad page whichever nonce wins
    damaged = oracle_proof(oracle, corrupt, ch)
    assert damaged is not None
    assert any(i // 1024 == page for i in proof_indices(damaged))
    d = corrupt_copy(sealed, tmp_path, corrupt)
    proof, rep = gsm_amd.prove_checked(d, ch, pcfg(), popts())
    assert proof == damaged and rep.bad_pages == [page]
    assert rep.proof_touches_bad_page
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(), heal())
    check_healed(oracle, clean, corrupt, [page], ch, want, proof, rep)
    assert rep.labels_repaired == 1 and rep.publishable
    assert not rep.proof_touches_unconfirmed_page


# ------------------------- whole pages -------------------------

@pytest.mark.parametrize("ch", CHALLENGES, ids=ch_id)
def test_page_1_holding_the_bytes_of_page_2(oracle, clean, sealed, want,
                                            tmp_path, ch):
    corrupt = clean[:PAGE] + clean[2 * PAGE:3 * PAGE] + clean[2 * PAGE:]
    assert len(corrupt) == len(clean)
    # dozens of spurious hits, dozens of lost ones
    assert oracle_hits(oracle, corrupt, [1], ch) >= 24
    assert oracle_hits(oracle, clean, [1], ch) >= 24
    d = corrupt_copy(sealed, tmp_path, corrupt)
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(), heal())
    check_healed(oracle, clean, corrupt, [1], ch, want, proof, rep)
    assert rep.labels_repaired == 1024


@pytest.mark.parametrize("ch", CHALLENGES[:2], ids=ch_id)
def test_first_page_and_ragged_last_page(oracle, clean, sealed, want,
                                         tmp_path, ch):
    # the compact buffer is 1024 + 517 labels: it ends short
    corrupt = bytes(PAGE) + clean[PAGE:3 * PAGE] + bytes(517 * 16)
    d = corrupt_copy(sealed, tmp_path, corrupt)
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(), heal())
    check_healed(oracle, clean, corrupt, [0, 3], ch, want, proof, rep)
    assert rep.labels_repaired == 1024 + 517


@pytest.mark.parametrize("chunk", ["2048", "1500"])
def test_bad_pages_in_both_halves_of_the_pass(oracle, clean, sealed, want,
                                              tmp_path, monkeypatch, chunk):
    # chunks of 2048 labels (1500 is rounded up to that on the seal paths):
    # page 1 arrives with the first pipeline buffer, page 3 with the second
    monkeypatch.setenv("POST_PROVE_CHUNK_LABELS", chunk)
    offsets = [PAGE + 7, 2 * PAGE - 1, 3 * PAGE, TOTAL * 16 - 1]
    corrupt = flipped(clean, offsets)
    d = corrupt_copy(sealed, tmp_path, corrupt)
    for ch in CHALLENGES[::2]:
        proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(), heal())
        check_healed(oracle, clean, corrupt, [1, 3], ch, want, proof, rep)
        assert rep.labels_repaired == 4


# ------------------------- unconfirmed pages -------------------------

def test_unconfirmed_page_is_used_but_never_written(oracle, clean, sealed,
                                                    want, tmp_path):
    # page 1: data and sidecar digest both damaged; page 3: data alone
    corrupt = flipped(clean, [1100 * 16 + 2, 3 * PAGE + 9])
    d = corrupt_copy(sealed, tmp_path, corrupt)
    side = os.path.join(d, "postdata_seal.bin")
    with open(side, "r+b") as fh:
        fh.seek(32 + 16 * 1 + 5)
        b = fh.read(1)[0]
        fh.seek(32 + 16 * 1 + 5)
        fh.write(bytes([b ^ 0x10]))
    sidecar = open(side, "rb").read()
    half_clean = flipped(clean, [1100 * 16 + 2])    # page 3 repaired
    flags = []
    for n, ch in enumerate(CHALLENGES):
        on_disk, bad = (corrupt, [1, 3]) if n == 0 else (half_clean, [1])
        proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(),
                                          heal(write_back=True))
        # the recomputed labels are used either way: the oracle's proof
        check_healed(oracle, clean, on_disk, bad, ch, want, proof, rep,
                     written=len(bad) - 1, unconfirmed=1)
        touches = any(i // 1024 == 1 for i in proof_indices(want[ch]))
        assert rep.proof_touches_unconfirmed_page == touches
        assert rep.publishable == (not touches) and not rep.repaired
        flags.append(touches)
        assert read_dir(d) == half_clean    # page 1 as it was, page 3 clean
        assert open(side, "rb").read() == sidecar
    assert True in flags and False in flags
    # repair cannot put it right either, and says so
    rep = gsm_amd.repair_data(d, heal())
    assert (rep.pages_bad, rep.pages_healed, rep.pages_unconfirmed,
            rep.pages_written) == (1, 1, 1, 0)
    assert not rep.repaired and read_dir(d) == half_clean


# ------------------------- the heal limit -------------------------

def test_more_bad_pages_than_the_limit_heals_nothing(oracle, clean, sealed,
                                                     tmp_path):
    ch = CHALLENGES[0]
    corrupt = flipped(clean, [40, 3 * PAGE + 40])
    damaged = oracle_proof(oracle, corrupt, ch)
    assert damaged is not None
    d = corrupt_copy(sealed, tmp_path, corrupt)
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(),
                                      heal(max_pages=1, write_back=True))
    assert proof == damaged
    assert rep.heal_skipped and not rep.publishable
    touches = any(i // 1024 in (0, 3) for i in proof_indices(damaged))
    assert rep.proof_touches_bad_page == touches
    assert (rep.pages_healed, rep.pages_unconfirmed, rep.labels_repaired,
            rep.hits_dropped, rep.hits_added, rep.pages_written) == (0,) * 6
    assert not rep.proof_touches_unconfirmed_page
    assert read_dir(d) == corrupt
    # the report is prove_checked's
    cproof, crep = gsm_amd.prove_checked(d, ch, pcfg(), popts())
    assert cproof == proof
    assert (rep.total_labels, rep.pages, rep.pages_bad, rep.bad_pages,
            rep.proof_touches_bad_page) == \
        (crep.total_labels, crep.pages, crep.pages_bad, crep.bad_pages,
         crep.proof_touches_bad_page) == (TOTAL, 4, 2, [0, 3], touches)
    # a limit of two heals both
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(),
                                      heal(max_pages=2))
    assert not rep.heal_skipped and rep.pages_healed == 2


# ------------------------- write-back -------------------------

def test_write_back_repairs_the_dir(oracle, clean, sealed, want, tmp_path):
    # page 1 lies in files 0 and 1; file 2 holds none of it
    offsets = [1030 * 16, (PER_FILE - 1) * 16 + 15, PER_FILE * 16,
               2047 * 16 + 15]
    corrupt = flipped(clean, offsets)
    d = corrupt_copy(sealed, tmp_path, corrupt)
    untouched = os.path.join(d, "postdata_2.bin")
    os.utime(untouched, ns=(10 ** 18, 10 ** 18))
    ch = CHALLENGES[2]
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(),
                                      heal(write_back=True))
    check_healed(oracle, clean, corrupt, [1], ch, want, proof, rep,
                 written=1)
    assert rep.labels_repaired == 4 and rep.repaired and rep.publishable
    assert read_dir(d) == clean
    assert os.stat(untouched).st_mtime_ns == 10 ** 18
    assert gsm_amd.check_seal(d).clean
    proof, rep = gsm_amd.prove_healed(d, ch, pcfg(), popts(), heal())
    assert proof == want[ch] and rep.clean and rep.pages_healed == 0


def test_repair_data_writes_without_proving(clean, sealed, tmp_path):
    corrupt = flipped(clean, [5, PAGE - 1, 3 * PAGE + 1, TOTAL * 16 - 1])
    d = corrupt_copy(sealed, tmp_path, corrupt)
    rep = gsm_amd.repair_data(d, heal(max_pages=1))
    assert rep.heal_skipped and not rep.repaired and rep.bad_pages == [0, 3]
    assert read_dir(d) == corrupt
    rep = gsm_amd.repair_data(d, heal())
    assert (rep.pages_bad, rep.pages_healed, rep.pages_written,
            rep.pages_unconfirmed, rep.labels_repaired) == (2, 2, 2, 0, 4)
    assert (rep.hits_dropped, rep.hits_added) == (0, 0)
    assert rep.repaired and rep.bad_pages == [0, 3]
    assert read_dir(d) == clean
    assert gsm_amd.check_seal(d).clean
    rep = gsm_amd.repair_data(d, heal())
    assert rep.clean and rep.repaired and rep.pages_healed == 0


# ------------------------- end to end, child processes -------------------

def cli(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "postcli.py"),
                           *argv], cwd=REPO, capture_output=True, text=True,
                          timeout=120)


def test_cli_flip_heal_verify_repair(oracle, clean, tmp_path):
    """postcli proves at its own K1 = 26, K2 = 37 and 288 nonces."""
    d = str(tmp_path / "d")
    ch = CHALLENGES[0]
    args = ("--datadir", d, "--challenge", ch.hex(), "--pow-difficulty",
            POW_DIFF.hex())
    good = oracle_proof(oracle, clean, ch, 26, 37, 288)
    spot = 2500 * 16 + 3                    # label 2500: file 1, page 2
    damaged = oracle_proof(oracle, flipped(clean, [spot]), ch, 26, 37, 288)
    assert good is not None and damaged is not None
    assert any(i // 1024 == 2 for i in proof_indices(damaged, 37))

    r = cli("init", "--datadir", d, "--node-id", NODE.hex(), "--atx-id",
            ATX.hex(), "--num-units", "1", "--labels-per-unit", str(TOTAL),
            "--scrypt-n", str(N), "--max-file-size", str(PER_FILE * 16))
    assert r.returncode == 0, r.stderr
    assert read_dir(d) == clean
    r = cli("seal", "--datadir", d)
    assert r.returncode == 0, r.stderr
    put(d, flipped(clean, [spot]))
    r = cli("prove", *args, "--check-seal")
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert "do not publish" in r.stderr

    r = cli("prove", *args, "--check-seal", "--heal", "--write-back")
    assert r.returncode == 0, r.stderr
    assert "healed labels [2048, 3072)" in r.stderr
    pj = json.loads(r.stdout)
    assert (pj["nonce"], base64.b64decode(pj["indices"]), pj["pow"]) == \
        (good.nonce, good.indices, good.pow)
    path = str(tmp_path / "proof.json")
    with open(path, "w") as fh:
        fh.write(r.stdout)
    r = cli("verify", "--datadir", d, "--proof", path, "--pow-difficulty",
            POW_DIFF.hex())
    assert r.returncode == 0 and json.loads(r.stdout) == {"valid": True}, \
        r.stdout + r.stderr
    assert read_dir(d) == clean
    r = cli("check-seal", "--datadir", d)
    assert r.returncode == 0, r.stdout + r.stderr

    put(d, flipped(clean, [40, spot]))
    r = cli("repair", "--datadir", d)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads(r.stdout)
    assert (j["pages_bad"], j["pages_healed"], j["pages_written"],
            j["pages_unconfirmed"]) == (2, 2, 2, 0)
    assert read_dir(d) == clean
