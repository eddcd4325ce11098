"""Postdata audit (verify-data), the parts that need no GPU: the sampling
rule against a pure-Python restatement of DESIGN §3.4, the validation order
of post_verify_data / post_verify_data_buffer (arguments, then metadata, then
the GPU requirement), and postcli's argument mapping."""
import base64
import json
import os

import pytest

import gsm_amd
Status = gsm_amd.api.Status

M64 = (1 << 64) - 1
NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_sample(seed, k, start, end):
    """The rule of DESIGN §3.4, restated."""
    out = []
    s = splitmix64(seed)
    windows = -(-(end - start) // k)
    for w in range(windows):
        first = start + w * k
        length = min(k, end - first)
        out.append(first + splitmix64((s + w) & M64) % length)
    return out


def has_gpu():
    import torch
    return torch.cuda.is_available()


# ------------------------- sampling rule -------------------------

@pytest.mark.parametrize("k", [1, 2, 7, 1000])
@pytest.mark.parametrize("seed", [0, M64, 0x1234_5678_9ABC_DEF0])
@pytest.mark.parametrize("start,end", [
    (0, 3000),                           # k=7, 1000: ragged last window
    (937, 2101),                         # unaligned both ends
    ((1 << 33) - 5, (1 << 33) + 2048),   # crosses 2^33
    ((1 << 33) + 12345, (1 << 33) + 12345 + 1061),
    (10, 11),                            # one label
])
def test_sample_matches_python_rule(k, seed, start, end):
    got = gsm_amd.sample_indices(seed, k, start, end)
    want = py_sample(seed, k, start, end)
    assert got == want
    # exactly one index per window, inside its window
    assert len(got) == -(-(end - start) // k)
    for w, g in enumerate(got):
        assert start + w * k <= g < min(start + (w + 1) * k, end)


def test_sample_k1_is_every_label():
    assert gsm_amd.sample_indices(99, 1, 100, 164) == list(range(100, 164))


def test_sample_paging_stitches_to_the_unpaged_list():
    seed, k, start, end = 7, 7, 937, 2101
    whole = gsm_amd.sample_indices(seed, k, start, end)
    assert whole == py_sample(seed, k, start, end)
    stitched, w = [], 0
    for page in (1, 5, 64, 13, 1000):
        part = gsm_amd.sample_indices(seed, k, start, end, first_window=w,
                                      max_count=page)
        assert len(part) == min(page, len(whole) - w)
        stitched += part
        w += len(part)
    assert stitched == whole
    # past the last window: nothing, not an error
    assert gsm_amd.sample_indices(seed, k, start, end,
                                  first_window=len(whole)) == []


def test_sample_seeds_differ_and_are_deterministic():
    a = gsm_amd.sample_indices(1, 1000, 0, 1 << 20)
    assert a == gsm_amd.sample_indices(1, 1000, 0, 1 << 20)
    assert a != gsm_amd.sample_indices(2, 1000, 0, 1 << 20)


def test_sample_rejects_bad_arguments():
    for k, start, end in [(0, 0, 10), (3, 10, 10), (3, 11, 10)]:
        with pytest.raises(gsm_amd.EngineError) as ei:
            gsm_amd.sample_indices(0, k, start, end)
        assert ei.value.code == Status.INVALID_ARGS


# ------------------------- validation order -------------------------

FIELDS = {
    "NodeId": base64.b64encode(NODE).decode(),
    "CommitmentAtxId": base64.b64encode(ATX).decode(),
    "LabelsPerUnit": 1500,
    "NumUnits": 2,
    "MaxFileSize": 16000,
    "Scrypt": {"N": 32, "R": 1, "P": 1},
}


def write_md(d, drop=None):
    md = {k: v for k, v in FIELDS.items() if k != drop}
    with open(os.path.join(d, "postdata_metadata.json"), "w") as f:
        json.dump(md, f, indent=2)


def audit_code(d, **kw):
    try:
        gsm_amd.verify_data(str(d), gsm_amd.AuditOpts(**kw))
    except gsm_amd.EngineError as e:
        return e.code, str(e)
    return Status.OK, ""


@pytest.mark.parametrize("kw", [
    dict(sample_every=0),
    dict(sample_every=1, index_start=5, index_end=5),      # empty
    dict(sample_every=1, index_start=9, index_end=3),      # inverted
    dict(sample_every=1, index_start=9, index_end=0),      # inverted
    dict(sample_every=1, index_start=0, index_end=3001),   # beyond space
    dict(sample_every=1, index_start=2999, index_end=1 << 40),
])
def test_bad_arguments_are_invalid_args(tmp_path, kw):
    write_md(str(tmp_path))
    assert audit_code(tmp_path, **kw)[0] == Status.INVALID_ARGS


def test_argument_checks_precede_metadata(tmp_path):
    # no metadata at all: a bad period is still INVALID_ARGS, a good one IO
    assert audit_code(tmp_path, sample_every=0)[0] == Status.INVALID_ARGS
    code, msg = audit_code(tmp_path, sample_every=1)
    assert code == Status.IO and "postdata_metadata.json" in msg


@pytest.mark.parametrize("field,named", [
    ("NodeId", "NodeId"), ("CommitmentAtxId", "CommitmentAtxId"),
    ("LabelsPerUnit", "LabelsPerUnit"), ("NumUnits", "NumUnits"),
    ("Scrypt", "N"), ("MaxFileSize", "MaxFileSize"),
])
def test_missing_metadata_field_is_io_and_named(tmp_path, field, named):
    write_md(str(tmp_path), drop=field)
    code, msg = audit_code(tmp_path, sample_every=1)
    assert code == Status.IO
    assert msg.rstrip().endswith(named), msg


@pytest.mark.parametrize("field,value,named", [
    ("LabelsPerUnit", "many", "LabelsPerUnit"),      # not a number
    ("LabelsPerUnit", -5, "LabelsPerUnit"),
    ("NumUnits", 0, "NumUnits"),
    ("MaxFileSize", 1 << 70, "MaxFileSize"),         # does not fit 64 bits
    ("Scrypt", {"N": 48, "R": 1, "P": 1}, "N"),      # not a power of two
    ("NodeId", "AAAA", "NodeId"),                    # not 32 bytes
    ("LabelsPerUnit", 1 << 63, "overflows"),         # times NumUnits = 2
])
def test_damaged_metadata_value_is_io_and_named(tmp_path, field, value,
                                                named):
    md = dict(FIELDS)
    md[field] = value
    with open(os.path.join(str(tmp_path), "postdata_metadata.json"),
              "w") as f:
        json.dump(md, f, indent=2)
    code, msg = audit_code(tmp_path, sample_every=1)
    assert code == Status.IO
    assert msg.rstrip().endswith(named), msg


def test_long_data_dir_path_is_not_truncated(tmp_path):
    # deeper than 4096 bytes in total would exceed PATH_MAX; stay below it
    # but well past any short fixed buffer
    d = str(tmp_path)
    for _ in range(12):
        d = os.path.join(d, "x" * 200)
    os.makedirs(d)
    write_md(d)
    code, _ = audit_code(d, sample_every=1)
    assert code == (Status.OK if has_gpu() else Status.NO_GPU)


def test_well_formed_dir_call_reaches_the_gpu_check(tmp_path):
    write_md(str(tmp_path))
    code, _ = audit_code(tmp_path, sample_every=7, index_start=937,
                         index_end=2101)
    # no label files here: with a GPU every sampled label is missing
    assert code == (Status.OK if has_gpu() else Status.NO_GPU)
    if has_gpu():
        rep = gsm_amd.verify_data(str(tmp_path),
                                  gsm_amd.AuditOpts(sample_every=7))
        assert rep.labels_missing == rep.labels_sampled == 429
        assert rep.labels_checked == rep.labels_bad == 0


def buffer_code(labels, base, n, **kw):
    try:
        gsm_amd.verify_data_buffer(labels, base, NODE, ATX, n,
                                   gsm_amd.AuditOpts(**kw))
    except gsm_amd.EngineError as e:
        return e.code
    return Status.OK


def test_buffer_validation_order(oracle):
    labels, _ = oracle.init_range(oracle.commitment(NODE, ATX), 100, 164, 2,
                                  with_nonce=False)
    assert buffer_code(labels, 100, 2, sample_every=0) == Status.INVALID_ARGS
    assert buffer_code(b"", 100, 2, sample_every=1) == Status.INVALID_ARGS
    assert buffer_code(labels, 100, 3, sample_every=1) == Status.INVALID_ARGS
    for s, e in [(120, 120), (130, 120), (99, 120), (100, 165), (0, 64)]:
        assert buffer_code(labels, 100, 2, sample_every=1, index_start=s,
                           index_end=e) == Status.INVALID_ARGS
    # well-formed: only now is a GPU required
    want = Status.OK if has_gpu() else Status.NO_GPU
    assert buffer_code(labels, 100, 2, sample_every=1) == want
    assert buffer_code(labels, 100, 2, sample_every=3, index_start=101,
                       index_end=164) == want


# ------------------------- postcli mapping -------------------------

def cli_args(*argv):
    import postcli
    return postcli, postcli.build_parser().parse_args(
        ["verify-data", "--datadir", "d", *argv])


@pytest.mark.parametrize("argv,k", [
    ([], 100),                          # default: --fraction 1
    (["--fraction", "1"], 100),
    (["--fraction", "100"], 1),
    (["--fraction", "50"], 2),
    (["--fraction", "0.1"], 1000),
    (["--fraction", "30"], 3),          # round(3.33)
    (["--fraction", "80"], 1),          # round(1.25)
    (["--every", "1"], 1),
    (["--every", "4096"], 4096),
])
def test_cli_fraction_and_every_map_to_period(argv, k):
    postcli, args = cli_args(*argv)
    assert postcli.audit_period(args) == k


def test_cli_shard_and_from_to_map_to_range():
    from importlib import import_module
    sharding = import_module("go-spacemesh_amd.sharding")
    total = 3001
    postcli, args = cli_args()
    assert postcli.audit_range(args, total) == (0, 0)
    for r in range(4):
        postcli, args = cli_args("--shard", f"{r}/4")
        assert postcli.audit_range(args, total) == \
            sharding.shard_range(total, 4, r)
    postcli, args = cli_args("--from", "937", "--to", "2101")
    assert postcli.audit_range(args, total) == (937, 2101)
    postcli, args = cli_args("--from", "937")
    assert postcli.audit_range(args, total) == (937, total)
    postcli, args = cli_args("--to", "50")
    assert postcli.audit_range(args, total) == (0, 50)
    postcli, args = cli_args("--seed", "0xffffffffffffffff")
    assert args.seed == M64


def test_cli_rejects_conflicting_or_bad_options():
    import postcli
    ap = postcli.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["verify-data", "--datadir", "d", "--every", "2",
                       "--fraction", "1"])
    for argv in (["--every", "0"], ["--fraction", "0"],
                 ["--fraction", "101"]):
        _, args = cli_args(*argv)
        with pytest.raises(SystemExit):
            postcli.audit_period(args)
    _, args = cli_args("--shard", "0/2", "--from", "3")
    with pytest.raises(SystemExit):
        postcli.audit_range(args, 100)


def test_cli_damaged_metadata_exits_2_without_traceback(tmp_path):
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(repo, "postcli.py")
    write_md(str(tmp_path), drop="NumUnits")
    for argv in (["--every", "3"], ["--shard", "0/2"]):
        r = subprocess.run([sys.executable, cli, "verify-data", "--datadir",
                            str(tmp_path), *argv], cwd=repo,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (r.stdout, r.stderr)
        assert "NumUnits" in r.stderr and "Traceback" not in r.stderr
        assert r.stdout == ""
