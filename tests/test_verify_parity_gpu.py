"""Verification parity: the predicate kernel and `post_verify_batch[_seeded]`
against the oracle.

The verify cases elsewhere all check one proof under one nonce at a
difficulty that the top byte of the compared u64 decides.  Here the
predicate kernel is driven directly (`post_selftest_verify_pred`: the
production kernel and launcher over caller-made labels) with crafted
ciphertexts either side of the mainnet difficulty in both halves, with 300
proofs that each have their own key, half and difficulty, and with a
two-block grid that has to stride; and the batch path is driven across the C
ABI with heterogeneous batches of 200 proofs, per-position and subset
verdicts, failures of both kinds in either order, and one batch with more
tasks than the label kernel has scratch slots.  Status and `invalid_index`
are compared exactly.

The cases and their expectations are built in verify_parity_cases.py from
the oracle alone; tests/test_verify_parity_cpu.py pins them without a GPU.
"""
import json
import os
import re
import subprocess
import sys

import pytest

import gsm_amd

import verify_parity_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "golden.json")))


@pytest.fixture(scope="module")
def eng():
    return gsm_amd.Engine()


def assert_verdicts(got, want):
    """Exact status; the position wherever the oracle reports one."""
    assert len(got) == len(want)
    for n, ((gs, gi), (ws, wi)) in enumerate(zip(got, want)):
        assert gs == ws, (n, got[n], want[n])
        if wi is not None:
            assert gi == wi, (n, got[n], want[n])


# ------------------------- predicate kernel -------------------------

def test_pred_crafted_ciphertexts(eng):
    labels, keys, halves, diffs, task_proof, values = vc.crafted_case()
    want = vc.pred_expected(labels, keys, halves, diffs, task_proof)
    # the design of the inputs: the verdict is value < D, nothing else
    assert want == bytes(1 if v < diffs[p] else 0
                         for p, v in zip(task_proof, values))
    got = eng.selftest_verify_pred(labels, keys, halves, diffs, task_proof)
    bad = [(t, task_proof[t], halves[task_proof[t]], hex(values[t]))
           for t in range(len(want)) if got[t] != want[t]]
    assert not bad, bad[:8]


def test_pred_per_proof_tables(eng):
    labels, keys, halves, diffs, task_proof, want = vc.tables_case()
    assert 4 * sum(want) >= len(want) and 4 * sum(want) <= 3 * len(want)
    got = eng.selftest_verify_pred(labels, keys, halves, diffs, task_proof)
    assert got == want


@pytest.mark.parametrize("count", vc.STRIDE_COUNTS)
def test_pred_grid_stride(eng, count):
    labels, keys, halves, diffs, task_proof, want = vc.tables_case()
    got = eng.selftest_verify_pred(labels[:32 * count], keys, halves, diffs,
                                   task_proof[:count], max_blocks=2)
    assert got == want[:count]


def test_pred_selftest_rejects_bad_map(eng):
    """The entry checks its task -> proof map before anything is launched."""
    labels, keys, halves, diffs, task_proof, _ = vc.tables_case()
    with pytest.raises(gsm_amd.EngineError) as ei:
        eng.selftest_verify_pred(labels[:64], keys, halves, diffs,
                                 [0, len(keys)])
    assert ei.value.code == gsm_amd.api.Status.INVALID_ARGS


# ------------------------- batch path -------------------------

def test_batch_heterogeneous():
    cases = vc.heterogeneous_batch()
    want = [c.expect(vc.HET_K1) for c in cases]
    assert {s for s, _ in want} == {vc.ST_OK, vc.ST_ARGS, vc.ST_POW,
                                    vc.ST_INDEX}
    got = vc.engine_verify(cases, vc.HET_K1)
    assert_verdicts(got, want)


def test_batch_per_position_verdicts():
    case, k1 = vc.position_case()
    want = [case.expect(k1, selected=pos) for pos in range(vc.K2 + 1)]
    assert want[vc.K2] == (vc.ST_ARGS, None)
    assert {s for s, _ in want[:vc.K2]} == {vc.ST_OK, vc.ST_INDEX}
    got = [vc.engine_verify([case], k1, selected=pos)[0]
           for pos in range(vc.K2 + 1)]
    assert_verdicts(got, want)


@pytest.mark.parametrize("k3", vc.SUBSET_K3)
def test_batch_subsets(k3):
    cases, k1 = vc.subset_batch()
    want = [c.expect(k1, k3=k3, seed=s)
            for c, s in zip(cases, vc.SUBSET_SEEDS)]
    got = vc.engine_verify(cases, k1, k3=k3, seeds=vc.SUBSET_SEEDS)
    assert_verdicts(got, want)


@pytest.mark.parametrize("mode", ["full", "k3=3", "k3=36", "selected"])
def test_batch_order_of_failure(mode):
    """A proof's verdict is the first failure in the order the positions
    are checked, whether that is an index out of range or a label above
    the difficulty."""
    cases, k1 = vc.order_batch()
    if mode == "full":
        want = [c.expect(k1) for c in cases]
        # as planned: threshold at 1 before range at 5, range at 2 before
        # threshold at 9, the first of two out of range
        assert [i for _, i in want] == [1, 2, 4, 0, 35, 3]
        assert_verdicts(vc.engine_verify(cases, k1), want)
    elif mode == "selected":
        for pos in (1, 2, 4, 5, 17, 35, 36):
            want = [c.expect(k1, selected=pos) for c in cases]
            assert_verdicts(vc.engine_verify(cases, k1, selected=pos), want)
    else:
        k3 = int(mode[3:])
        for seed in vc.ORDER_SEEDS:
            want = [c.expect(k1, k3=k3, seed=seed) for c in cases]
            got = vc.engine_verify(cases, k1, k3=k3,
                                   seeds=[seed] * len(cases))
            assert_verdicts(got, want)
            # the shared-seed form of the same call
            got = vc.engine_verify(cases, k1, k3=k3, seed=seed)
            assert_verdicts(got, want)


def test_batch_more_tasks_than_scratch_slots():
    child = ("import sys; sys.path[:0] = [%r, %r, %r]; "
             "import torch, verify_parity_cases as vc; vc.slots_child()"
             % (os.path.join(REPO, "tests"), REPO,
                os.path.join(REPO, "oracle")))
    env = dict(os.environ, POST_VERIFY_DEBUG="1",
               VERIFY_PARITY_TASKS=str(vc.SLOTS_TASKS))
    r = subprocess.run([sys.executable, "-c", child], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"\[verify\] reserve .*tasks=(\d+) lanes=(\d+)", r.stderr)
    assert m, r.stderr[-2000:]
    tasks, lanes = int(m.group(1)), int(m.group(2))
    assert tasks == vc.SLOTS_TASKS
    assert lanes < tasks, "every task had a scratch slot of its own"
    line = next(x for x in r.stdout.splitlines() if x.startswith("VERDICTS "))
    got = [tuple(x) for x in json.loads(line[len("VERDICTS "):])]
    status, inv = vc.slots_expected(vc.SLOTS_TASKS)
    assert len(got) == len(status)
    assert [g[0] for g in got] == status
    assert [g[1] for g, s in zip(got, status) if s == vc.ST_INDEX] == \
        [i for i, s in zip(inv, status) if s == vc.ST_INDEX]
    share = status.count(vc.ST_OK) / len(status)
    assert 0.02 < share < 0.5, share


# ------------------------- VRF nonce -------------------------

def vrf_verdict(ver, meta, index):
    try:
        ver.verify_vrf_nonce(meta, index)
        return 0
    except gsm_amd.EngineError as e:
        assert e.code == gsm_amd.api.Status.INVALID_INDEX
        return 1


@pytest.mark.parametrize("num_labels", vc.VRF_NUM_LABELS)
def test_vrf_nonce_verdicts(num_labels):
    ident, picked = vc.vrf_cases()[num_labels]
    assert len(picked) == 64
    want = [v for _, v in picked]
    assert set(want) == ({0} if num_labels <= 16 else {0, 1})
    ver = gsm_amd.PostVerifier(gsm_amd.PostConfig(), scrypt_n=vc.N)
    meta = gsm_amd.PostProofMetadata(*vc.IDENTITIES[ident], bytes(32), 1,
                                     num_labels)
    assert [vrf_verdict(ver, meta, i) for i, _ in picked] == want


def test_vrf_nonce_mainnet_n_golden():
    """Index 1000 of the OpenSSL-made labels at N = 8192 starts 0xba7c: below
    16 * 2^256 / 20, above 16 * 2^256 / 24."""
    lv = GOLDEN["labels_openssl"]
    node, atx = bytes.fromhex(lv["node_id"]), bytes.fromhex(lv["atx_id"])
    v = next(x for x in lv["labels"] if x["N"] == 8192 and x["index"] == 1000)
    full = int(v["full"], 16)
    ver = gsm_amd.PostVerifier(gsm_amd.PostConfig(), scrypt_n=8192)
    for num_labels, want in ((20, 0), (24, 1)):
        assert (0 if full * num_labels < 16 << 256 else 1) == want
        ometa = vc.make_meta(node, atx, bytes(32), 1, num_labels)
        assert vc.oracle().verify_vrf_nonce(ometa, 1000, 8192) == want
        meta = gsm_amd.PostProofMetadata(node, atx, bytes(32), 1, num_labels)
        assert vrf_verdict(ver, meta, 1000) == want
