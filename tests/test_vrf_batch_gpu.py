"""Batched VRF-nonce verification on a real MI355X: the VRF predicate kernel
driven directly (`post_selftest_vrf_pred`: the production kernel and
launcher over caller-made labels), `post_verify_vrf_nonce_batch` and
`post_verify_batch_vrf` across the C ABI, BatchingVerifier over the real
PostVerifier, and `postcli verify --vrf-nonce` as child processes.

Every expected value is the oracle's (`verify_vrf_nonce`, `verify`,
`oracle_vrf_difficulty`) or a `bytes` comparison in Python; the cases are
built in vrf_batch_cases.py and pinned without a GPU by
tests/test_vrf_batch_cpu.py.  Labels are made at scrypt N = 2 except in the
one mainnet-N case.
"""
import json
import os
import re
import subprocess
import sys
import threading

import pytest

import gsm_amd

import verify_parity_cases as vc
import vrf_batch_cases as vb

pytestmark = pytest.mark.gpu

Status = gsm_amd.api.Status
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "golden.json")))


@pytest.fixture(scope="module")
def eng():
    return gsm_amd.Engine()


@pytest.fixture(scope="module")
def ver():
    return gsm_amd.PostVerifier(gsm_amd.PostConfig(), scrypt_n=vb.N)


# ------------------------- predicate kernel -------------------------

def test_pred_crafted_labels(eng):
    labels, thrs, task_thr, want = vb.crafted_case()
    got = eng.selftest_vrf_pred(labels, thrs, task_thr)
    bad = [(t, task_thr[t], labels[32 * t:32 * t + 32].hex(), got[t])
           for t in range(len(want)) if got[t] != want[t]]
    assert not bad, bad[:8]


def test_pred_threshold_map(eng):
    labels, thrs, task_thr, want = vb.tables_case()
    assert eng.selftest_vrf_pred(labels, thrs, task_thr) == want


@pytest.mark.parametrize("count", vb.STRIDE_COUNTS)
def test_pred_grid_stride(eng, count):
    labels, thrs, task_thr, want = vb.tables_case()
    got = eng.selftest_vrf_pred(labels[:32 * count], thrs, task_thr[:count],
                                max_blocks=2)
    assert got == want[:count]


# ------------------------- VRF-only batch -------------------------

def single_verdict(ver, meta, index):
    try:
        ver.verify_vrf_nonce(meta, index)
        return vb.ST_OK
    except gsm_amd.EngineError as e:
        return int(e.code)


@pytest.fixture(scope="module")
def vrf_only(ver):
    """Statuses of the 256 items in one call."""
    items = vb.vrf_items()
    return [int(s) for s in ver.verify_vrf_nonce_batch(*vb.e_vrf(items))]


def test_vrf_batch_equals_oracle_and_looped_single(ver, vrf_only):
    items = vb.vrf_items()
    assert vrf_only == [w for _, _, _, w in items]
    metas, indices = vb.e_vrf(items)
    assert [single_verdict(ver, m, i)
            for m, i in zip(metas, indices)] == vrf_only


@pytest.mark.parametrize("order", ["reversed", "interleaved"])
def test_vrf_batch_in_another_order(ver, order):
    items = vb.vrf_items()
    items = items[::-1] if order == "reversed" else vb.interleaved(items)
    got = ver.verify_vrf_nonce_batch(*vb.e_vrf(items))
    assert [int(s) for s in got] == [w for _, _, _, w in items]


def test_vrf_batch_zero_labels_item_disturbs_nothing(ver, vrf_only):
    items = vb.vrf_items()
    metas, indices = vb.e_vrf(items)
    for nu, lpu in ((0, 64), (3, 0)):
        bad = gsm_amd.PostProofMetadata(*vc.IDENTITIES[0], bytes(32), nu, lpu)
        got = ver.verify_vrf_nonce_batch(metas[:100] + [bad] + metas[100:],
                                         indices[:100] + [5] + indices[100:])
        got = [int(s) for s in got]
        assert got[100] == vb.ST_ARGS
        assert got[:100] + got[101:] == vrf_only
        with pytest.raises(gsm_amd.EngineError) as ei:
            ver.verify_vrf_nonce(bad, 5)
        assert ei.value.code == Status.INVALID_ARGS
        assert "labels_per_unit is zero" in str(ei.value)


# ------------------------- mixed call -------------------------

def test_mixed_call_equals_each_kind_alone(vrf_only):
    cases = vc.heterogeneous_batch()
    alone = vc.engine_verify(cases, vc.HET_K1)
    want = [c.expect(vc.HET_K1) for c in cases]
    got, vgot = vb.engine_verify_mixed(cases, vc.HET_K1,
                                       vb.e_vrf(vb.vrf_items()))
    assert got == alone                 # status and invalid_index, exactly
    for (gs, gi), (ws, wi) in zip(got, want):
        assert gs == ws and (wi is None or gi == wi)
    assert vgot == vrf_only == [w for _, _, _, w in vb.vrf_items()]


def test_mixed_call_with_every_proof_rejected_early(vrf_only):
    """No proof task at all: the VRF tail starts at offset 0."""
    cases = vb.bad_pow_batch()
    want = [c.expect(vc.HET_K1)[0] for c in cases]
    got, vgot = vb.engine_verify_mixed(cases, vc.HET_K1,
                                       vb.e_vrf(vb.vrf_items()))
    assert [s for s, _ in got] == want
    assert set(want) == {vc.ST_POW, vc.ST_ARGS}
    assert vgot == vrf_only


def test_mixed_call_without_vrf_items():
    cases = vc.heterogeneous_batch()
    got, vgot = vb.engine_verify_mixed(cases, vc.HET_K1, ([], []))
    assert got == vc.engine_verify(cases, vc.HET_K1) and vgot == []


def test_mixed_call_more_tasks_than_scratch_lanes():
    child = ("import sys; sys.path[:0] = [%r, %r, %r]; "
             "import torch, vrf_batch_cases as vb; vb.lanes_child()"
             % (os.path.join(REPO, "tests"), REPO,
                os.path.join(REPO, "oracle")))
    env = dict(os.environ, POST_VERIFY_DEBUG="1",
               VRF_BATCH_ITEMS=str(vb.LANES_VRF_ITEMS))
    r = subprocess.run([sys.executable, "-c", child], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"\[verify\] reserve .*tasks=(\d+) lanes=(\d+) vrf=(\d+)",
                  r.stderr)
    assert m, r.stderr[-2000:]
    tasks, lanes, n_vrf = (int(x) for x in m.groups())
    assert n_vrf == vb.LANES_VRF_ITEMS
    assert tasks == vb.LANES_PROOF_TASKS + vb.LANES_VRF_ITEMS
    assert lanes < n_vrf, "every VRF task had a scratch lane of its own"
    line = next(x for x in r.stdout.splitlines() if x.startswith("VERDICTS "))
    got, vgot = json.loads(line[len("VERDICTS "):])
    status, inv = vc.slots_expected(vb.LANES_PROOF_TASKS)
    assert [g[0] for g in got] == status
    assert [g[1] for g, s in zip(got, status) if s == vc.ST_INDEX] == \
        [i for i, s in zip(inv, status) if s == vc.ST_INDEX]
    want = vb.lanes_expected(vb.LANES_VRF_ITEMS)
    wrong = [i for i in range(len(want)) if vgot[i] != want[i]]
    assert len(vgot) == len(want) and not wrong, wrong[:8]
    # both verdicts on either side of the wrap
    assert set(want[:lanes]) == set(want[lanes:]) == {vb.ST_OK, vb.ST_INDEX}


# ------------------------- mainnet N -------------------------

def test_vrf_batch_mainnet_n_golden():
    """Index 1000 of the OpenSSL-made labels at N = 8192 starts 0xba7c: below
    16 * 2^256 / 20, above 16 * 2^256 / 24.  Both in one batch call."""
    lv = GOLDEN["labels_openssl"]
    node, atx = bytes.fromhex(lv["node_id"]), bytes.fromhex(lv["atx_id"])
    v = next(x for x in lv["labels"] if x["N"] == 8192 and x["index"] == 1000)
    full = bytes.fromhex(v["full"])
    assert [vb.pred(full, vb.threshold(nl)) for nl in (20, 24)] == [True,
                                                                    False]
    for nl, want in ((20, 0), (24, 1)):
        ometa = vc.make_meta(node, atx, bytes(32), 1, nl)
        assert vc.oracle().verify_vrf_nonce(ometa, 1000, 8192) == want
    ver = gsm_amd.PostVerifier(gsm_amd.PostConfig(), scrypt_n=8192)
    metas = [gsm_amd.PostProofMetadata(node, atx, bytes(32), 1, nl)
             for nl in (20, 24)]
    got = ver.verify_vrf_nonce_batch(metas, [1000, 1000])
    assert [int(s) for s in got] == [vb.ST_OK, vb.ST_INDEX]


# ------------------------- BatchingVerifier -------------------------

def test_batching_verifier_mixed_jobs_over_the_engine():
    cases, k1 = vc.subset_batch()
    k3 = vc.SUBSET_K3[1]
    want_p = [c.expect(k1, k3=k3, seed=s)[0]
              for c, s in zip(cases, vc.SUBSET_SEEDS)]
    items = vb.interleaved(vb.vrf_items())[:16]
    want_v = [w for _, _, _, w in items]
    assert set(want_v) == {vb.ST_OK, vb.ST_INDEX}
    cfg = gsm_amd.PostConfig(k1=k1, k2=vc.K2, k3=k3,
                             pow_difficulty=vc.POW_DIFF)
    bv = gsm_amd.BatchingVerifier(
        gsm_amd.PostVerifier(cfg, scrypt_n=vb.N), max_batch=64,
        max_wait_s=0.05, seed_len=len(vc.SUBSET_SEEDS[0]))
    vmetas, vidx = vb.e_vrf(items)
    got_p, got_v = [None] * 8, [None] * 16

    def verdict(call, *args):
        try:
            call(*args)
            return vb.ST_OK
        except gsm_amd.EngineError as e:
            return int(e.code)

    def work(t):
        c = cases[t]
        proof = gsm_amd.PostProof(c.nonce, c.packed, c.pow)
        meta = gsm_amd.PostProofMetadata(*vc.IDENTITIES[c.ident],
                                         c.challenge, c.num_units, c.lpu)
        got_v[2 * t] = verdict(bv.verify_vrf_nonce, vmetas[2 * t],
                               vidx[2 * t])
        got_p[t] = verdict(bv.verify, proof, meta, vc.SUBSET_SEEDS[t])
        got_v[2 * t + 1] = verdict(bv.verify_vrf_nonce, vmetas[2 * t + 1],
                                   vidx[2 * t + 1])

    ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(60)
    bv.close()
    assert got_p == want_p and got_v == want_v


# ------------------------- postcli children -------------------------

CLI_NODE, CLI_ATX = bytes([0xA5]) * 32, bytes([0x5A]) * 32
CLI_TOTAL, CLI_N = 3 * 1024 + 517, 32
CLI_CHALLENGE = bytes([0x07]) * 32  # proves at postcli's K1 = 26, K2 = 37


def cli(*argv):
    return subprocess.run([sys.executable, os.path.join(REPO, "postcli.py"),
                           *argv], cwd=REPO, capture_output=True, text=True,
                          timeout=120)


def test_cli_init_prove_verify_with_vrf_nonce(tmp_path):
    d = str(tmp_path / "d")
    r = cli("init", "--datadir", d, "--node-id", CLI_NODE.hex(), "--atx-id",
            CLI_ATX.hex(), "--num-units", "1", "--labels-per-unit",
            str(CLI_TOTAL), "--scrypt-n", str(CLI_N))
    assert r.returncode == 0, r.stderr
    nonce = json.loads(r.stdout.splitlines()[-1])["vrf_nonce"]
    o = vc.oracle()
    ometa = vc.make_meta(CLI_NODE, CLI_ATX, bytes(32), 1, CLI_TOTAL)
    assert o.verify_vrf_nonce(ometa, nonce, CLI_N) == 0
    failing = next(i for i in range(CLI_TOTAL)
                   if o.verify_vrf_nonce(ometa, i, CLI_N) != 0)
    r = cli("prove", "--datadir", d, "--challenge", CLI_CHALLENGE.hex(),
            "--pow-difficulty", vc.POW_DIFF.hex())
    assert r.returncode == 0, r.stderr
    path = str(tmp_path / "proof.json")
    with open(path, "w") as fh:
        fh.write(r.stdout)
    args = ("verify", "--datadir", d, "--proof", path, "--pow-difficulty",
            vc.POW_DIFF.hex())

    r = cli(*args, "--vrf-nonce")
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout) == {
        "valid": True, "vrf_nonce": {"index": nonce, "valid": True}}

    r = cli(*args, "--vrf-nonce", str(failing))
    assert r.returncode == 1, r.stdout + r.stderr
    assert json.loads(r.stdout) == {
        "valid": True, "vrf_nonce": {"index": failing, "valid": False}}
