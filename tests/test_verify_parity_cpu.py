"""The expectations of tests/test_verify_parity_gpu.py, pinned without a GPU:
the Python restatement of the predicate and the `scan_hits`-derived verdicts
are what `oracle.verify` says, the crafted-ciphertext builder round-trips,
and every case holds the verdicts it is meant to hold."""
import numpy as np

import verify_parity_cases as vc


def test_restated_predicate_equals_oracle_verify():
    """370 (label, nonce) pairs: `oracle.verify` with `selected_index`
    accepts a position exactly where the restatement passes its label."""
    o = vc.oracle()
    rng = np.random.default_rng(0x9E57)
    seen = set()
    for n in range(10):
        nu, lpu = vc.SHAPES[n % 3]
        nl = nu * lpu
        ident, challenge = n % 3, vc.CHALLENGES[n % 2]
        nonce = vc.NONCES[n % len(vc.NONCES)]
        pow_ = vc.find_pow(challenge, nonce // 16, 500 * n)
        idx = [int(i) for i in rng.integers(0, nl, vc.K2)]
        case = vc.Case(ident, challenge, nu, lpu, nonce, pow_,
                       vc.pack(idx, nl))
        key = vc.proof_key(challenge, nonce, pow_)
        D = vc.difficulty(vc.HET_K1, nl)
        commit = o.commitment(*vc.IDENTITIES[ident])
        for pos in range(vc.K2):
            label = o.label(commit, idx[pos], vc.N)
            assert label[:16] == vc.label_table(ident, nl)[
                16 * idx[pos]:16 * idx[pos] + 16]
            ok = vc.pred(key, label[:16], nonce % 2, D)
            st, inv = case.expect(vc.HET_K1, selected=pos)
            assert (st == vc.ST_OK) == ok
            assert ok or (st, inv) == (vc.ST_INDEX, pos)
            seen.add(ok)
    assert seen == {True, False}


def test_scan_hits_expectation_equals_oracle_verify():
    tasks = 2048
    cases, k1, _ = vc.slots_batch(tasks)
    status, inv = vc.slots_expected(tasks)
    assert len(cases) == 256
    for c, s, i in zip(cases, status, inv):
        ws, wi = c.expect(k1, k2=vc.SLOTS_K2)
        assert s == ws
        if wi is not None:
            assert i == wi
    assert 0 < status.count(vc.ST_OK) < len(status)


def test_crafted_builder_round_trips():
    o = vc.oracle()
    labels, keys, halves, diffs, task_proof, values = vc.crafted_case()
    assert len(task_proof) == 32 * len(vc.crafted_values())
    assert len(set(keys)) == 8
    for t, p in enumerate(task_proof):
        ct = o.aes128(keys[p], labels[32 * t:32 * t + 16])
        assert o.aes128(keys[p], o.aes128_dec(keys[p], ct)) == ct
        sel = int.from_bytes(ct[8 * halves[p]:8 * halves[p] + 8], "little")
        oth = int.from_bytes(ct[8 - 8 * halves[p]:16 - 8 * halves[p]],
                             "little")
        assert sel == values[t]
        # the half that is not selected holds the opposite verdict
        assert (sel < diffs[p]) != (oth < diffs[p])
    want = vc.pred_expected(labels, keys, halves, diffs, task_proof)
    assert want == bytes(1 if v < diffs[p] else 0
                         for p, v in zip(task_proof, values))


def test_crafted_values_cover_the_edges():
    D = vc.D_MAINNET
    assert vc.difficulty(vc.MAINNET_K1, vc.MAINNET_TOTAL) == D
    assert vc.difficulty(37, 37) == vc.ALL_FF
    vals = vc.crafted_values()
    for v in (D - 1, D, D + 1, 0, vc.ALL_FF):
        assert v in vals
    # every byte position is set in some passing value or decides a failing
    # one, and each passing trap has its byte- and word-swapped twin failing
    for i in range(5):
        assert any(v < D and v >> 8 * i & 0xFF for v in vals)
    for i in (5, 6, 7):
        assert any(v >= D and (v & ~(0xFF << 8 * i)) < D for v in vals)
    assert sum(v < D for v in vals) >= 6 and sum(v >= D for v in vals) >= 6


def test_per_proof_tables_hold_both_verdicts():
    labels, keys, halves, diffs, task_proof, want = vc.tables_case()
    assert len(want) == 3000 and len(keys) == 300
    assert 4 * sum(want) >= len(want)
    assert 4 * (len(want) - sum(want)) >= len(want)
    assert len(set(diffs)) > 100 and set(halves) == {0, 1}
    assert all(abs(d - (1 << 63)) < 1 << 59 for d in diffs)
    assert any(d & 0xFFFFFF for d in diffs)  # low bytes that matter
    assert sorted(set(task_proof)) == list(range(300))
    assert task_proof != sorted(task_proof)
    # both verdicts beyond the first pass of a two-block grid
    for count in vc.STRIDE_COUNTS:
        assert count <= len(want)
    assert set(want[2 * vc.T:]) == {0, 1}


def test_heterogeneous_batch_holds_what_it_claims():
    cases = vc.heterogeneous_batch()
    assert len(cases) >= 200
    assert len({c.ident for c in cases}) == 3
    assert len({c.challenge for c in cases}) == 2
    shapes = {(c.num_units, c.lpu) for c in cases if c.num_units * c.lpu}
    bpis = {vc.oracle().lib.oracle_bits_per_index(u * l) for u, l in shapes}
    assert len(bpis) >= 3
    assert any(u * l & (u * l - 1) for u, l in shapes)
    assert {c.nonce % 2 for c in cases} == {0, 1}
    assert len({c.nonce // 2 for c in cases}) >= 3
    assert len({c.nonce // 16 for c in cases}) == 2
    want = [c.expect(vc.HET_K1) for c in cases]
    assert {s for s, _ in want} == {vc.ST_OK, vc.ST_ARGS, vc.ST_POW,
                                    vc.ST_INDEX}
    # failures at many positions, late ones included
    assert len({i for _, i in want if i is not None}) >= 10
    # rejects interleaved with the rest, in every block of 64
    for lo in range(0, 192, 64):
        assert len({s for s, _ in want[lo:lo + 64]}) == 4


def test_subsets_sample_a_later_failure_first():
    cases, k1 = vc.subset_batch()
    later = 0
    for k3 in vc.SUBSET_K3:
        for c, seed in zip(cases, vc.SUBSET_SEEDS):
            bad = vc.failing_positions(c, k1)
            assert len(bad) == 3
            st, inv = c.expect(k1, k3=k3, seed=seed)
            sampled = vc.subset_positions(k3, seed)
            hit = [p for p in sampled if p in bad]
            if hit:
                assert (st, inv) == (vc.ST_INDEX, hit[0])
                later += hit[0] != min(hit)
            else:
                assert st == vc.ST_OK
    assert later >= 1


def test_order_of_failure_plans():
    cases, k1 = vc.order_batch()
    want = [c.expect(k1) for c in cases]
    assert want == [(vc.ST_INDEX, 1), (vc.ST_INDEX, 2), (vc.ST_INDEX, 4),
                    (vc.ST_INDEX, 0), (vc.ST_INDEX, 35), (vc.ST_INDEX, 3)]
    for c, (aes_bad, oor) in zip(cases, vc.ORDER_PLANS):
        assert vc.failing_positions(c, k1) == sorted(aes_bad + oor)


def test_vrf_cases_hold_both_verdicts():
    cases = vc.vrf_cases()
    for nl in vc.VRF_NUM_LABELS:
        _, picked = cases[nl]
        assert len(picked) == 64 and len({i for i, _ in picked}) == 64
        verdicts = {v for _, v in picked}
        assert verdicts == ({0} if nl <= 16 else {0, 1})
