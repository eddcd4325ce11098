"""Postdata audit (verify-data) on a real MI355X.

Every expectation comes from the CPU oracle and a Python restatement of the
sampling rule, so nothing here leans on GPU init being right: the test
writes the postdata files and postdata_metadata.json itself.

Base fixture: N=32, 2 units x 1500 labels, MaxFileSize 16000 B (3 files of
1000 labels), scratch sized for lanes = 128, so a batch is 512 labels and
K=1 runs 6 batches — every quad does 4 tasks and the last batch is ragged
(440 labels)."""
import base64
import json
import os
import subprocess
import sys

import pytest

import gsm_amd
Status = gsm_amd.api.Status

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
N, LPU, UNITS, MAX_FILE = 32, 1500, 2, 16000
TOTAL, PER_FILE = LPU * UNITS, MAX_FILE // 16
SCRATCH_128 = 128 * N * 128     # budget for exactly 128 lanes at this N
SEED = 2

# batch edges (511|512, 1023, 2559|2560), file edges (999|1000, 1999|2000),
# first and last label
CORRUPT16 = [0, 1, 257, 511, 512, 999, 1000, 1023, 1500, 1999, 2000, 2048,
             2559, 2560, 2998, 2999]


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_sample(seed, k, start, end):
    s = splitmix64(seed)
    out = []
    for w in range(-(-(end - start) // k)):
        first = start + w * k
        out.append(first + splitmix64((s + w) & M64) % min(k, end - first))
    return out


def label_at(buf, i, base=0):
    return bytes(buf[(i - base) * 16:(i - base) * 16 + 16])


def corrupt(labels, indices, base=0):
    """Flip one bit in byte position b of the b-th index (b mod 16)."""
    buf = bytearray(labels)
    for b, i in enumerate(indices):
        buf[(i - base) * 16 + b % 16] ^= 1 << (b % 8)
    return bytes(buf)


def write_dir(d, labels, node=NODE, scrypt_n=N):
    d = str(d)
    os.makedirs(d, exist_ok=True)
    for f in range(-(-len(labels) // MAX_FILE)):
        with open(os.path.join(d, f"postdata_{f}.bin"), "wb") as fh:
            fh.write(labels[f * MAX_FILE:(f + 1) * MAX_FILE])
    with open(os.path.join(d, "postdata_metadata.json"), "w") as fh:
        json.dump({"NodeId": base64.b64encode(node).decode(),
                   "CommitmentAtxId": base64.b64encode(ATX).decode(),
                   "LabelsPerUnit": LPU, "NumUnits": UNITS,
                   "MaxFileSize": MAX_FILE,
                   "Scrypt": {"N": scrypt_n, "R": 1, "P": 1}}, fh, indent=2)
    return d


def opts(**kw):
    kw.setdefault("scratch_bytes", SCRATCH_128)
    kw.setdefault("seed", SEED)
    return gsm_amd.AuditOpts(**kw)


@pytest.fixture(scope="module")
def commit(oracle):
    return oracle.commitment(NODE, ATX)


@pytest.fixture(scope="module")
def good(oracle, commit):
    """The 3000 oracle labels of the base fixture; never modified."""
    labels, _ = oracle.init_range(commit, 0, TOTAL, N, with_nonce=False)
    return labels


@pytest.fixture(scope="module")
def bad16_dir(good, tmp_path_factory):
    return write_dir(tmp_path_factory.mktemp("bad16"),
                     corrupt(good, CORRUPT16))


def check_bad(rep, on_disk_buf, good_buf, want_indices, base=0):
    assert rep.labels_bad == len(want_indices)
    assert [b[0] for b in rep.bad] == sorted(want_indices)
    for idx, on_disk, expected in rep.bad:
        assert on_disk == label_at(on_disk_buf, idx, base)
        assert expected == label_at(good_buf, idx, base)
        assert on_disk != expected


def test_clean_dir_every_label(good, tmp_path):
    rep = gsm_amd.verify_data(write_dir(tmp_path, good), opts(sample_every=1))
    assert rep.labels_in_range == rep.labels_sampled == TOTAL
    assert rep.labels_checked == TOTAL
    assert rep.labels_bad == 0 and rep.labels_missing == 0 and rep.bad == []
    assert rep.clean


def test_sixteen_corrupted_labels_every_byte_position(good, bad16_dir):
    assert len(set(CORRUPT16)) == 16
    rep = gsm_amd.verify_data(bad16_dir, opts(sample_every=1))
    assert rep.labels_checked == TOTAL and rep.labels_missing == 0
    check_bad(rep, corrupt(good, CORRUPT16), good, CORRUPT16)


def test_sampled_audit_k7(good, bad16_dir):
    sample = py_sample(SEED, 7, 0, TOTAL)
    hit = sorted(set(CORRUPT16) & set(sample))
    assert hit and len(hit) < len(CORRUPT16)   # precondition on the seed
    rep = gsm_amd.verify_data(bad16_dir, opts(sample_every=7))
    assert rep.labels_sampled == rep.labels_checked == len(sample) == 429
    check_bad(rep, corrupt(good, CORRUPT16), good, hit)


def test_sub_range_k3_crosses_both_file_boundaries(good, bad16_dir):
    start, end = 937, 2101
    sample = py_sample(SEED, 3, start, end)
    inside = [c for c in CORRUPT16 if start <= c < end]
    hit = sorted(set(inside) & set(sample))
    assert hit and len(hit) < len(inside)      # precondition on the seed
    rep = gsm_amd.verify_data(bad16_dir, opts(sample_every=3,
                                              index_start=start,
                                              index_end=end))
    assert rep.labels_in_range == end - start
    assert rep.labels_sampled == rep.labels_checked == len(sample) == 388
    check_bad(rep, corrupt(good, CORRUPT16), good, hit)
    # the same range at K=1 finds all of them
    rep = gsm_amd.verify_data(bad16_dir, opts(sample_every=1,
                                              index_start=start,
                                              index_end=end))
    assert rep.labels_checked == end - start
    check_bad(rep, corrupt(good, CORRUPT16), good, inside)


def test_cap_returns_the_smallest_and_counts_all(good, tmp_path):
    forty = [(i * 73 + 5) % TOTAL for i in range(40)]
    assert len(set(forty)) == 40
    disk = corrupt(good, forty)
    d = write_dir(tmp_path, disk)
    rep = gsm_amd.verify_data(d, opts(sample_every=1, max_report=8))
    assert rep.labels_bad == 40
    assert [b[0] for b in rep.bad] == sorted(forty)[:8]
    for idx, on_disk, expected in rep.bad:
        assert on_disk == label_at(disk, idx)
        assert expected == label_at(good, idx)
    # cap 0 with no list at all still counts
    rep = gsm_amd.verify_data(d, opts(sample_every=1, max_report=0))
    assert rep.labels_bad == 40 and rep.bad == []


def py_missing(sample, sizes):
    """sizes: bytes of postdata_i.bin, None when absent."""
    def gone(g):
        size = sizes[g // PER_FILE]
        return size is None or (g % PER_FILE) * 16 + 16 > size
    return [g for g in sample if gone(g)]


def test_truncated_last_file_is_missing_not_bad(good, tmp_path):
    d = write_dir(tmp_path, good)
    cut = 100 * 16 + 5
    with open(os.path.join(d, "postdata_2.bin"), "r+b") as fh:
        fh.truncate(MAX_FILE - cut)
    sizes = [MAX_FILE, MAX_FILE, MAX_FILE - cut]
    for k in (1, 7):
        sample = py_sample(SEED, k, 0, TOTAL)
        missing = py_missing(sample, sizes)
        assert missing
        rep = gsm_amd.verify_data(d, opts(sample_every=k))
        assert rep.labels_sampled == len(sample)
        assert rep.labels_missing == len(missing)
        assert rep.labels_bad == 0 and rep.bad == []
        assert rep.labels_checked + rep.labels_missing == rep.labels_sampled
        assert not rep.clean
    assert len(py_missing(py_sample(SEED, 1, 0, TOTAL), sizes)) == 101


def test_removed_middle_file_is_missing_not_bad(good, tmp_path):
    d = write_dir(tmp_path, corrupt(good, CORRUPT16))
    os.remove(os.path.join(d, "postdata_1.bin"))
    sizes = [MAX_FILE, None, MAX_FILE]
    for k in (1, 7):
        sample = py_sample(SEED, k, 0, TOTAL)
        missing = py_missing(sample, sizes)
        rep = gsm_amd.verify_data(d, opts(sample_every=k))
        assert rep.labels_missing == len(missing) > 0
        assert rep.labels_checked + rep.labels_missing == rep.labels_sampled
        # corrupted labels of the files that remain are still found
        want = sorted(c for c in set(CORRUPT16) & set(sample)
                      if c not in missing)
        assert [b[0] for b in rep.bad] == want
        assert rep.labels_bad == len(want)


def test_wrong_identity_makes_every_checked_label_bad(good, tmp_path):
    other = bytes([NODE[0] ^ 1]) + NODE[1:]
    d = write_dir(tmp_path, good, node=other)
    sample = py_sample(SEED, 7, 0, TOTAL)
    rep = gsm_amd.verify_data(d, opts(sample_every=7, max_report=1000))
    assert rep.labels_checked == rep.labels_bad == len(sample)
    assert [b[0] for b in rep.bad] == sample
    assert all(on_disk == label_at(good, i) and expected != on_disk
               for i, on_disk, expected in rep.bad)


def test_high_indices_buffer(oracle, commit):
    base, count = (1 << 33) + 12345, 1061
    want, _ = oracle.init_range(commit, base, base + count, N,
                                with_nonce=False)
    hurt = [base, base + 530, base + count - 1]
    disk = corrupt(want, hurt, base)
    for k in (1, 5):
        sample = py_sample(SEED, k, base, base + count)
        hit = sorted(set(hurt) & set(sample))
        # precondition on the seed: the sampled leg finds some, not all
        assert hit and (k == 1 or len(hit) < len(hurt))
        rep = gsm_amd.verify_data_buffer(disk, base, NODE, ATX, N,
                                         opts(sample_every=k))
        assert rep.labels_in_range == count
        assert rep.labels_checked == len(sample)
        assert rep.labels_missing == 0
        check_bad(rep, disk, want, hit, base)
    assert len(py_sample(SEED, 1, base, base + count)) == count


def test_mainnet_n_buffer_lean_romix(oracle, commit):
    n, count = 8192, 150
    want, _ = oracle.init_range(commit, 0, count, n, with_nonce=False)
    hurt = [0, 77, count - 1]
    disk = corrupt(want, hurt)
    rep = gsm_amd.verify_data_buffer(disk, 0, NODE, ATX, n,
                                     gsm_amd.AuditOpts(sample_every=1))
    assert rep.labels_checked == count
    check_bad(rep, disk, want, hurt)


def test_fastnet_n2_buffer(oracle, commit):
    n, count = 2, 300
    want, _ = oracle.init_range(commit, 0, count, n, with_nonce=False)
    hurt = [3, 128, 299]
    disk = corrupt(want, hurt)
    rep = gsm_amd.verify_data_buffer(disk, 0, NODE, ATX, n,
                                     gsm_amd.AuditOpts(sample_every=1))
    assert rep.labels_checked == count
    check_bad(rep, disk, want, hurt)


def test_progress_and_cancel(good, tmp_path):
    d = write_dir(tmp_path, good)
    calls = []
    rep = gsm_amd.verify_data(d, opts(sample_every=1),
                              lambda c, t: calls.append((c, t)))
    assert [c for c, _ in calls] == [512, 1024, 1536, 2048, 2560, 3000]
    assert all(t == TOTAL for _, t in calls)
    assert calls[-1][0] == rep.labels_checked

    seen = []

    def stop_on_second(c, t):
        seen.append(c)
        return len(seen) == 2

    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.verify_data(d, opts(sample_every=1), stop_on_second)
    assert ei.value.code == Status.CANCELLED
    assert seen == [512, 1024]

    # an exception in the callback stops the audit and reaches the caller
    def boom(c, t):
        raise KeyError("from progress")

    with pytest.raises(KeyError, match="from progress"):
        gsm_amd.verify_data(d, opts(sample_every=1), boom)
    # the engine is still usable in this process
    rep = gsm_amd.verify_data(d, opts(sample_every=1))
    assert rep.clean and rep.labels_checked == TOTAL


def test_end_to_end_init_then_postcli(tmp_path):
    d = str(tmp_path / "post")
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=LPU)
    mgr = gsm_amd.PostSetupManager(
        NODE, ATX, cfg,
        gsm_amd.PostSetupOpts(data_dir=d, num_units=UNITS, scrypt_n=N,
                              max_file_size=MAX_FILE,
                              scratch_bytes=SCRATCH_128))
    mgr.prepare_initializer()
    mgr.start_session()
    mgr.reset()
    rep = gsm_amd.verify_data(d, opts(sample_every=1))
    assert rep.clean and rep.labels_checked == TOTAL

    victim = 1234
    with open(os.path.join(d, "postdata_1.bin"), "r+b") as fh:
        fh.seek((victim % PER_FILE) * 16 + 9)
        byte = fh.read(1)
        fh.seek(-1, os.SEEK_CUR)
        fh.write(bytes([byte[0] ^ 0x40]))
    r = subprocess.run([sys.executable, os.path.join(REPO, "postcli.py"),
                        "verify-data", "--datadir", d, "--every", "1"],
                       cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["labels_checked"] == TOTAL and out["labels_missing"] == 0
    assert out["labels_bad"] == 1
    assert [b["index"] for b in out["bad"]] == [victim]
    assert out["bad"][0]["on_disk"] != out["bad"][0]["expected"]
