"""Batched VRF-nonce verification, the parts that need no GPU: the exported
symbols, the validation order of post_verify_batch_vrf /
post_verify_vrf_nonce_batch / post_selftest_vrf_pred, the expectations of
tests/test_vrf_batch_gpu.py pinned against the oracle, BatchingVerifier's
routing over a stub inner verifier, and `postcli verify --vrf-nonce` over a
stubbed engine."""
import base64
import ctypes
import json
import os
import threading
from ctypes import byref, c_int, c_uint32, c_uint64

import pytest

import gsm_amd

import verify_parity_cases as vc
import vrf_batch_cases as vb

Status = gsm_amd.api.Status
CProof, CProofMetadata = gsm_amd.api.CProof, gsm_amd.api.CProofMetadata
_CVerifyConfig = gsm_amd.api._CVerifyConfig


def has_gpu():
    import torch
    return torch.cuda.is_available()


# the last rung of every validation order
NEEDS_GPU = Status.OK if has_gpu() else Status.NO_GPU


@pytest.fixture(scope="module")
def lib():
    return gsm_amd.load_engine()


def test_symbols_exported(lib):
    for name in ("post_verify_batch_vrf", "post_verify_vrf_nonce_batch",
                 "post_selftest_vrf_pred"):
        assert hasattr(lib, name), name


# ------------------------- validation order -------------------------

def batch_args(n=1, n_vrf=1, pow_mode=gsm_amd.api.POW_MODE_BLAKE3):
    cfg = _CVerifyConfig()
    cfg.k1, cfg.k2, cfg.k3 = 26, 37, 37
    cfg.selected_index = -1
    cfg.pow_mode = pow_mode
    cfg.scrypt_n = 2
    a = {"proofs": (CProof * max(n, 1))(),
         "metas": (CProofMetadata * max(n, 1))(), "n": n, "cfg": byref(cfg),
         "seeds": None, "seed_len": 0,
         "vrf_metas": (CProofMetadata * max(n_vrf, 1))(),
         "vrf_indices": (c_uint64 * max(n_vrf, 1))(), "n_vrf": n_vrf,
         "statuses": (c_int * max(n, 1))(),
         "invalid": (c_uint32 * max(n, 1))(),
         "vrf_statuses": (c_int * max(n_vrf, 1))(), "_keep": cfg}
    for i in range(max(n, 1)):
        a["statuses"][i] = 77
    for i in range(max(n_vrf, 1)):
        a["vrf_statuses"][i] = 77
    return a


ORDER = ["proofs", "metas", "n", "cfg", "seeds", "seed_len", "vrf_metas",
         "vrf_indices", "n_vrf", "statuses", "invalid", "vrf_statuses"]


def call_batch(lib, a, **null):
    a = dict(a)
    for k in null:
        a[k] = None
    return lib.post_verify_batch_vrf(*[a[k] for k in ORDER])


def test_batch_vrf_null_arguments(lib):
    a = batch_args()
    assert call_batch(lib, a, cfg=1) == Status.INVALID_ARGS
    for k in ("proofs", "metas", "statuses", "vrf_metas", "vrf_indices",
              "vrf_statuses"):
        assert call_batch(lib, a, **{k: 1}) == Status.INVALID_ARGS, k
    # a NULL cfg comes before everything, the empty call included
    assert call_batch(lib, batch_args(0, 0), cfg=1) == Status.INVALID_ARGS
    assert a["statuses"][0] == 77 and a["vrf_statuses"][0] == 77


def test_batch_vrf_arrays_of_an_absent_kind_are_not_needed(lib):
    a = batch_args(n=0, n_vrf=1)
    a["vrf_metas"][0].num_units = 1
    a["vrf_metas"][0].labels_per_unit = 16
    assert call_batch(lib, a, proofs=1, metas=1, statuses=1,
                      invalid=1) == NEEDS_GPU
    a = batch_args(n=1, n_vrf=0)
    assert call_batch(lib, a, vrf_metas=1, vrf_indices=1,
                      vrf_statuses=1) == NEEDS_GPU
    # invalid_indices is optional, as in post_verify_batch
    assert call_batch(lib, batch_args(), invalid=1) == NEEDS_GPU


def test_batch_vrf_unsupported_pow_only_with_proofs(lib):
    rx = gsm_amd.api.POW_MODE_RANDOMX
    assert call_batch(lib, batch_args(pow_mode=rx)) == Status.UNSUPPORTED
    # NULLs are reported before the pow mode
    assert call_batch(lib, batch_args(pow_mode=rx),
                      vrf_statuses=1) == Status.INVALID_ARGS
    a = batch_args(n=0, n_vrf=1, pow_mode=rx)
    a["vrf_metas"][0].num_units = 1
    a["vrf_metas"][0].labels_per_unit = 16
    assert call_batch(lib, a) == NEEDS_GPU
    # ... and before the empty call
    assert call_batch(lib, batch_args(0, 0, pow_mode=rx)) == Status.OK


def test_batch_vrf_empty_call_touches_nothing(lib):
    a = batch_args(0, 0)
    assert call_batch(lib, a) == Status.OK
    assert call_batch(lib, a, proofs=1, metas=1, statuses=1, invalid=1,
                      vrf_metas=1, vrf_indices=1,
                      vrf_statuses=1) == Status.OK
    assert a["statuses"][0] == 77 and a["vrf_statuses"][0] == 77


def test_batch_vrf_then_needs_a_gpu(lib):
    a = batch_args()
    assert call_batch(lib, a) == NEEDS_GPU
    if not has_gpu():
        assert b"no HIP device" in lib.post_last_error()
        assert a["statuses"][0] == 77 and a["vrf_statuses"][0] == 77
    else:   # zeroed metadata: num_labels == 0 on both sides
        assert a["statuses"][0] == Status.INVALID_ARGS
        assert a["vrf_statuses"][0] == Status.INVALID_ARGS


def test_vrf_nonce_batch_validation(lib):
    metas = (CProofMetadata * 1)()
    metas[0].num_units, metas[0].labels_per_unit = 1, 16
    idx = (c_uint64 * 1)(3)
    st = (c_int * 1)(77)
    f = lib.post_verify_vrf_nonce_batch
    assert f(None, idx, 1, 2, 0, st) == Status.INVALID_ARGS
    assert f(metas, None, 1, 2, 0, st) == Status.INVALID_ARGS
    assert f(metas, idx, 1, 2, 0, None) == Status.INVALID_ARGS
    assert f(None, None, 0, 2, 0, None) == Status.OK
    assert st[0] == 77
    assert f(metas, idx, 1, 2, 0, st) == NEEDS_GPU
    # the single entry: NULL, then the GPU
    assert lib.post_verify_vrf_nonce(None, 3, 2, 0) == Status.INVALID_ARGS
    if not has_gpu():
        assert lib.post_verify_vrf_nonce(metas, 3, 2, 0) == Status.NO_GPU


def test_selftest_vrf_pred_argument_errors(lib):
    labels = bytes(64)
    thr = vb.ALL_FF * 2
    tmap = (c_uint32 * 2)(0, 1)
    out = ctypes.create_string_buffer(2)
    f = lib.post_selftest_vrf_pred
    assert f(None, 2, thr, 2, tmap, 0, 0, out) == Status.INVALID_ARGS
    assert f(labels, 2, None, 2, tmap, 0, 0, out) == Status.INVALID_ARGS
    assert f(labels, 2, thr, 2, None, 0, 0, out) == Status.INVALID_ARGS
    assert f(labels, 2, thr, 2, tmap, 0, 0, None) == Status.INVALID_ARGS
    assert f(labels, 0, thr, 2, tmap, 0, 0, out) == Status.INVALID_ARGS
    assert f(labels, 2, thr, 1, tmap, 0, 0, out) == Status.INVALID_ARGS
    assert b"task_thr" in lib.post_last_error()
    assert f(labels, 2, thr, 2, tmap, 0, 0, out) == NEEDS_GPU
    with pytest.raises(gsm_amd.EngineError) as ei:
        gsm_amd.Engine().selftest_vrf_pred(labels, [vb.ALL_FF], [0, 1])
    assert ei.value.code == Status.INVALID_ARGS


# ------------------------- the expectations -------------------------

def test_thresholds_are_the_oracles():
    """The builder's thresholds against the formula, for every shape used:
    floor(16 * 2^256 / num_labels), all-0xFF at num_labels <= 16."""
    shapes = (vb.CRAFTED_NUM_LABELS + vb.TABLE_NUM_LABELS +
              vc.VRF_NUM_LABELS + [vb.LANES_NUM_LABELS, 20, 24])
    for nl in shapes:
        want = (vb.ALL_FF if nl <= 16 else
                ((16 << 256) // nl).to_bytes(32, "big"))
        out = ctypes.create_string_buffer(32)
        vc.oracle().lib.oracle_vrf_difficulty(nl, out)
        assert vb.threshold(nl) == out.raw == want, nl
    assert vb.threshold(1 << 34) == bytes([0, 0, 0, 4]) + bytes(28)
    assert 0 not in vb.threshold(4000000001)[4:]


def test_restated_predicate_equals_oracle_verify_vrf_nonce():
    o = vc.oracle()
    seen = set()
    for nl in vc.VRF_NUM_LABELS:
        ident, picked = vc.vrf_cases()[nl]
        commit = o.commitment(*vc.IDENTITIES[ident])
        thr = vb.threshold(nl)
        for index, verdict in picked:
            ok = vb.pred(o.label(commit, index, vb.N), thr)
            assert ok == (verdict == 0), (nl, index)
            seen.add(ok)
    assert seen == {True, False}


def test_crafted_labels_reach_every_byte():
    labels, thrs, task_thr, want = vb.crafted_case()
    assert len(thrs) == 3 and thrs[2] == vb.ALL_FF
    by_thr = {s: [(labels[32 * t:32 * t + 32], want[t])
                  for t in range(len(want)) if task_thr[t] == s]
              for s in range(3)}
    for s, thr in enumerate(thrs):
        group = dict(by_thr[s])
        assert set(group.values()) == {0, 1}
        assert group[thr] == 0                       # strict
        assert group[vb.ALL_00] == 1
        assert group[vb.ALL_FF] == 0                 # the clamp included
        t = int.from_bytes(thr, "big")
        assert group[(t - 1).to_bytes(32, "big")] == 1
        if s < 2:
            assert group[(t + 1).to_bytes(32, "big")] == 0
        for b in range(32):
            # first difference at byte b, the later bytes arguing the
            # other way
            lo = [l for l, w in group.items()
                  if l[:b] == thr[:b] and l[b] < thr[b] and w == 1 and
                  all(x == 0xFF for x in l[b + 1:])]
            hi = [l for l, w in group.items()
                  if l[:b] == thr[:b] and l[b] > thr[b] and w == 0 and
                  all(x == 0 for x in l[b + 1:])]
            assert lo or thr[b] == 0, (s, b)
            assert hi or thr[b] == 255, (s, b)
    # a compare in any of the three wrong byte orders is caught at the
    # thresholds that such a swap changes
    for s in (0, 1):
        for f in vb.SWAPS:
            assert f(thrs[s]) != thrs[s]
            wrong = [l for l, w in by_thr[s]
                     if vb.pred(f(l), f(thrs[s])) != bool(w)]
            assert len(wrong) >= 8, (s, f.__name__)
    # the verdicts are nothing but the bytes comparison
    assert want == bytes(1 if labels[32 * t:32 * t + 32] < thrs[s] else 0
                         for t, s in enumerate(task_thr))


def test_tables_case_holds_both_verdicts():
    labels, thrs, task_thr, want = vb.tables_case()
    assert len(want) == 3000 and len(set(thrs)) == 300 - 13
    assert sum(nl <= 16 for nl in vb.TABLE_NUM_LABELS) == 14
    assert sum(nl & (nl - 1) != 0 for nl in vb.TABLE_NUM_LABELS) > 250
    assert sorted(set(task_thr)) == list(range(300))
    assert task_thr != sorted(task_thr)
    assert 10 * sum(want) >= len(want) and 2 * sum(want) <= len(want)
    for count in vb.STRIDE_COUNTS:
        assert count <= len(want)
    assert set(want[2 * vc.T:]) == {0, 1}


def test_batch_items_hold_both_verdicts():
    items = vb.vrf_items()
    assert len(items) == 256 and len({i[0] for i in items}) == 3
    assert {i[1] for i in items} == {16, 32, 64, 4096}
    assert any(i[2] >= 1 << 32 for i in items)
    for order in (items, items[::-1], vb.interleaved(items)):
        assert sorted(order) == sorted(items)
        for lo in range(0, 256, 64):
            block = order[lo:lo + 64]
            if {i[1] for i in block} == {16}:
                assert {i[3] for i in block} == {vb.ST_OK}  # the clamp
            else:
                assert {i[3] for i in block} == {vb.ST_OK, vb.ST_INDEX}
    inter = vb.interleaved(items)
    assert [i[1] for i in inter[:4]] == [16, 32, 64, 4096]
    o = vc.oracle()
    for ident, nl, index, want in items[::7]:
        assert vb.FROM_ORACLE[o.verify_vrf_nonce(vb.o_meta(ident, nl), index,
                                                 vb.N)] == want


def test_bad_pow_batch_rejects_every_proof_early():
    cases = vb.bad_pow_batch()
    want = [c.expect(vc.HET_K1) for c in cases]
    assert len(want) == 200
    assert {s for s, _ in want} == {vc.ST_POW, vc.ST_ARGS}
    assert [s for s, _ in want].count(vc.ST_POW) > 150


def test_lanes_items_hold_both_verdicts():
    want = vb.lanes_expected(4096)
    share = want.count(vb.ST_OK) / len(want)
    assert 0.15 < share < 0.35 and set(want) == {vb.ST_OK, vb.ST_INDEX}
    assert vb.LANES_VRF_ITEMS >= vc.SLOTS_TASKS
    status, _ = vc.slots_expected(vb.LANES_PROOF_TASKS)
    assert len(status) == 8


# ------------------------- BatchingVerifier -------------------------

class FakeMeta:
    def __init__(self, tag):
        self.node_id = bytes([tag]) * 32
        self.tag = tag


class StubInner:
    """verify_batch as BatchingVerifier's docstring has it; proof p fails
    where p % 5 == 0, VRF index i where i % 3 == 0."""

    def __init__(self, fail=None):
        self.calls = []
        self.fail = fail
        self.gate = threading.Event()
        self.gate.set()
        self.entered = threading.Event()

    def verify_batch(self, proofs, metas, opts=None, seeds=None, **kw):
        self.entered.set()
        self.gate.wait(10)
        self.calls.append((list(proofs), [m.tag for m in metas], seeds, kw))
        if self.fail:
            raise self.fail
        res = [(8, p % 7) if p % 5 == 0 else (0, 0) for p in proofs]
        if "vrf" not in kw:
            return res
        vmetas, vidx = kw["vrf"]
        assert len(vmetas) == len(vidx)
        return res, [8 if i % 3 == 0 else 0 for i in vidx]


def run_jobs(bv, proof_jobs, vrf_jobs):
    """Start every job on its own thread; {('p'|'v', key): None or the
    exception}."""
    out = {}

    def proof(p):
        try:
            bv.verify(p, FakeMeta(p), b"s%03d" % p)
            out["p", p] = None
        except BaseException as e:  # noqa: BLE001
            out["p", p] = e

    def vrf(i):
        try:
            bv.verify_vrf_nonce(FakeMeta(i), i)
            out["v", i] = None
        except BaseException as e:  # noqa: BLE001
            out["v", i] = e

    ths = [threading.Thread(target=proof, args=(p,)) for p in proof_jobs]
    ths += [threading.Thread(target=vrf, args=(i,)) for i in vrf_jobs]
    for t in ths:
        t.start()
    return ths, out


def test_pool_merges_proofs_and_vrf_jobs_into_one_call():
    inner = StubInner()
    n_jobs = 6 + 6
    bv = gsm_amd.BatchingVerifier(inner, max_batch=n_jobs, max_wait_s=30.0,
                                  seed_len=4)
    ths, out = run_jobs(bv, range(10, 16), range(20, 26))
    for t in ths:
        t.join(20)
    bv.close()
    assert len(inner.calls) == 1
    proofs, tags, seeds, kw = inner.calls[0]
    assert sorted(proofs) == list(range(10, 16)) and tags == proofs
    assert seeds == [b"s%03d" % p for p in proofs]
    assert set(kw) == {"vrf"}
    vmetas, vidx = kw["vrf"]
    assert sorted(vidx) == list(range(20, 26))
    assert [m.tag for m in vmetas] == vidx
    # each caller its own verdict
    for p in range(10, 16):
        e = out["p", p]
        if p % 5 == 0:
            assert e.code == Status.INVALID_INDEX and \
                "position %d" % (p % 7) in str(e)
        else:
            assert e is None
    for i in range(20, 26):
        e = out["v", i]
        if i % 3 == 0:
            assert isinstance(e, gsm_amd.EngineError)
            assert e.code == Status.INVALID_INDEX
        else:
            assert e is None


def test_pool_vrf_only_and_proof_only_batches():
    inner = StubInner()
    bv = gsm_amd.BatchingVerifier(inner, max_batch=4, max_wait_s=30.0,
                                  seed_len=4)
    ths, out = run_jobs(bv, [], [1, 2, 3, 4])
    for t in ths:
        t.join(20)
    assert len(inner.calls) == 1
    proofs, tags, seeds, kw = inner.calls[0]
    assert proofs == [] and tags == [] and seeds is None
    assert sorted(kw["vrf"][1]) == [1, 2, 3, 4]
    assert out["v", 3].code == Status.INVALID_INDEX
    assert [out["v", i] for i in (1, 2, 4)] == [None] * 3

    ths, out = run_jobs(bv, [1, 2, 3, 4], [])
    for t in ths:
        t.join(20)
    bv.close()
    assert len(inner.calls) == 2
    proofs, tags, seeds, kw = inner.calls[1]
    assert sorted(proofs) == [1, 2, 3, 4] and len(seeds) == 4
    assert kw == {}, "a batch of proofs alone passes no vrf keyword"
    assert all(e is None for e in out.values())


def test_pool_proof_only_inner_without_vrf_keyword_still_works():
    """An inner verifier from before the keyword serves proof traffic."""
    calls = []

    class OldInner:
        def verify_batch(self, proofs, metas, opts=None, seeds=None):
            calls.append(len(proofs))
            return [(0, 0) for _ in proofs]

    bv = gsm_amd.BatchingVerifier(OldInner(), seed_len=1)
    bv.verify("p", FakeMeta(1), b"x")
    bv.close()
    assert calls == [1]


def test_pool_inner_exception_reaches_every_caller():
    boom = gsm_amd.EngineError(Status.OOM, "scratch")
    inner = StubInner(fail=boom)
    bv = gsm_amd.BatchingVerifier(inner, max_batch=6, max_wait_s=30.0,
                                  seed_len=4)
    ths, out = run_jobs(bv, [1, 2, 3], [4, 5, 6])
    for t in ths:
        t.join(20)
    bv.close()
    assert len(inner.calls) == 1
    assert len(out) == 6 and all(e is boom for e in out.values())


def wait_for(cond):
    import time
    deadline = time.monotonic() + 10
    while not cond() and time.monotonic() < deadline:
        time.sleep(0.001)
    assert cond()


def test_pool_close_drains_vrf_jobs():
    """Jobs queued when close() is called are still served."""
    inner = StubInner()
    bv = gsm_amd.BatchingVerifier(inner, max_batch=64, max_wait_s=0.0,
                                  seed_len=4)
    inner.gate.clear()                  # hold the collector inside a call
    first, out1 = run_jobs(bv, [], [7])
    assert inner.entered.wait(10)
    ths, out = run_jobs(bv, [1, 2], [4, 5])
    wait_for(lambda: bv._q.qsize() == 4)
    closer = threading.Thread(target=bv.close)
    closer.start()
    wait_for(lambda: bv._q.qsize() == 5)    # the pill, behind the jobs
    inner.gate.set()
    for t in first + ths + [closer]:
        t.join(20)
    assert out1 == {("v", 7): None}
    assert sorted(out) == [("p", 1), ("p", 2), ("v", 4), ("v", 5)]
    assert all(e is None for e in out.values())
    assert sum(len(c[0]) + len(c[3].get("vrf", ((), ()))[1])
               for c in inner.calls) == 5
    with pytest.raises(RuntimeError):
        bv.verify_vrf_nonce(FakeMeta(1), 1)


# ------------------------- postcli over a stubbed engine -------------------

NODE, ATX = bytes([0xA5]) * 32, bytes([0x5A]) * 32


def write_dir(d, nonce=1234):
    md = {"NodeId": base64.b64encode(NODE).decode(),
          "CommitmentAtxId": base64.b64encode(ATX).decode(),
          "LabelsPerUnit": 4096, "NumUnits": 1, "MaxFileSize": 65536,
          "Scrypt": {"N": 2, "R": 1, "P": 1}}
    if nonce is not None:
        md["Nonce"] = nonce
    with open(os.path.join(str(d), "postdata_metadata.json"), "w") as f:
        json.dump(md, f)
    path = os.path.join(str(d), "proof.json")
    with open(path, "w") as f:
        json.dump({"nonce": 5, "indices": base64.b64encode(b"abc").decode(),
                   "pow": 77, "challenge": "07" * 32}, f)
    return path


class StubVerifier:
    seen = []
    proof_status, proof_inv, vrf_status = 0, 0, 0

    def __init__(self, cfg, scrypt_n=8192):
        self.cfg, self.scrypt_n = cfg, scrypt_n

    def verify(self, proof, meta, opts=None):
        StubVerifier.seen.append(("verify", proof.nonce, opts.subset_seed))
        if self.proof_status:
            raise gsm_amd.EngineError(
                self.proof_status,
                f"invalid POST index at position {self.proof_inv}")

    def verify_batch(self, proofs, metas, opts=None, seeds=None, vrf=None):
        vm, vi = vrf
        StubVerifier.seen.append(("batch", [p.nonce for p in proofs],
                                  [m.labels_per_unit for m in metas],
                                  opts.subset_seed, seeds,
                                  [m.node_id for m in vm], list(vi)))
        return ([(Status(self.proof_status), self.proof_inv)],
                [Status(self.vrf_status)])


def run_cli(monkeypatch, capsys, argv, proof_status=0, vrf_status=0):
    import postcli
    StubVerifier.seen = []
    StubVerifier.proof_status, StubVerifier.proof_inv = proof_status, 9
    StubVerifier.vrf_status = vrf_status
    monkeypatch.setattr(gsm_amd, "PostVerifier", StubVerifier)
    args = postcli.build_parser().parse_args(argv)
    try:
        rc = args.fn(args)
    except SystemExit as e:
        rc = e.code
    cap = capsys.readouterr()
    return rc or 0, cap.out, StubVerifier.seen


def test_cli_without_the_flag_is_the_old_command(monkeypatch, capsys,
                                                 tmp_path):
    path = write_dir(tmp_path)
    argv = ["verify", "--datadir", str(tmp_path), "--proof", path]
    rc, out, seen = run_cli(monkeypatch, capsys, argv)
    assert rc == 0 and out == '{"valid": true}\n'
    assert seen == [("verify", 5, None)]
    rc, out, seen = run_cli(monkeypatch, capsys, argv, proof_status=8)
    assert rc == 1 and seen == [("verify", 5, None)]
    assert json.loads(out) == {
        "valid": False,
        "error": "INVALID_INDEX: invalid POST index at position 9"}


def test_cli_bare_flag_uses_the_metadata_nonce(monkeypatch, capsys, tmp_path):
    path = write_dir(tmp_path, nonce=1234)
    argv = ["verify", "--datadir", str(tmp_path), "--proof", path, "--seed",
            "0a0b", "--vrf-nonce"]
    rc, out, seen = run_cli(monkeypatch, capsys, argv)
    assert rc == 0
    assert json.loads(out) == {"valid": True,
                               "vrf_nonce": {"index": 1234, "valid": True}}
    # one engine call for both, for the same identity
    assert seen == [("batch", [5], [4096], b"\x0a\x0b", None, [NODE],
                     [1234])]


def test_cli_explicit_index_and_exit_codes(monkeypatch, capsys, tmp_path):
    path = write_dir(tmp_path, nonce=None)
    base = ["verify", "--datadir", str(tmp_path), "--proof", path]
    rc, out, seen = run_cli(monkeypatch, capsys,
                            base + ["--vrf-nonce", str((1 << 32) + 17)])
    assert rc == 0 and seen[0][-1] == [(1 << 32) + 17]
    assert json.loads(out)["vrf_nonce"] == {"index": (1 << 32) + 17,
                                            "valid": True}
    # index 0 is an index, not an absent flag
    rc, out, seen = run_cli(monkeypatch, capsys, base + ["--vrf-nonce", "0"])
    assert rc == 0 and seen[0][-1] == [0]

    rc, out, _ = run_cli(monkeypatch, capsys, base + ["--vrf-nonce", "7"],
                         proof_status=8)
    j = json.loads(out)
    assert rc == 1 and j["valid"] is False and "position 9" in j["error"]
    assert j["vrf_nonce"] == {"index": 7, "valid": True}

    rc, out, _ = run_cli(monkeypatch, capsys, base + ["--vrf-nonce", "7"],
                         vrf_status=8)
    assert rc == 1
    assert json.loads(out) == {"valid": True,
                               "vrf_nonce": {"index": 7, "valid": False}}

    # a bare flag needs a nonce in the metadata
    rc, out, seen = run_cli(monkeypatch, capsys, base + ["--vrf-nonce"])
    assert rc not in (0, None) and seen == []
