"""One-lane-per-label SHA prologue and tail vs the CPU oracle.

The prologue writes and the tails read a task's whole block in xbuf, in the
quad-z chunk layout ROMix works in; a wrong permutation changes every label.
Range mode (init: 16-B labels, VRF minimum tracked) is held to the oracle's
labels and to its minimum and the minimum's index.  A session's first batch
is given the threshold ff..ff, so every label of every workgroup qualifies
and each workgroup's reduce must hand on its true (label, index) minimum;
513 labels make three workgroups of 256 lanes, the last with one.
Index-list mode with two commitments and full 32-B labels is reached
through batch verification, which returns verdicts: they are held to the
oracle's, with one index per rejected proof swapped for a failing one.  The
audit tail is held to reporting exactly the labels altered on disk.

The candidate list itself (one entry per workgroup and launch) is not
visible through the library's interface; a workgroup that appended a wrong
or a second-best candidate shows as a wrong nonce.
"""
import functools

import pytest

import gsm_amd
from oracle import Oracle, Proof, make_meta

gpu = pytest.mark.gpu

NODE = bytes([0xA5]) * 32
NODE2 = bytes([0x3C]) * 32
ATX = bytes([0x5A]) * 32
CHALLENGE = bytes(32)
POW_DIFF = bytes([0x0F]) + bytes([0xFF]) * 31
N = 16
COUNTS = [1, 3, 63, 65, 257]


@functools.lru_cache(maxsize=None)
def oracle_range(node, start, count):
    o = Oracle()
    want, best = o.init_range(o.commitment(node, ATX), start, start + count, N)
    return want, (best.index, bytes(best.label))


def init_session(count, **kw):
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=count, k1=12,
                             k2=8, k3=4, pow_difficulty=POW_DIFF)
    kw.setdefault("scratch_bytes", 1 << 30)
    opts = gsm_amd.PostSetupOpts(num_units=1, scrypt_n=N, **kw)
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
    mgr.prepare_initializer()
    return mgr


@gpu
@pytest.mark.parametrize("count", COUNTS + [513])
def test_range_mode_labels_and_minimum(count):
    want, nonce = oracle_range(NODE, 0, count)
    mgr = init_session(count)
    mgr.start_session()
    try:
        assert mgr.copy_labels(0, count) == want
        assert mgr.vrf_nonce() == nonce
    finally:
        mgr.reset()


@gpu
def test_minimum_over_calls_with_a_lagging_threshold():
    """Several calls: a later tail is given the running minimum, so only an
    improving label qualifies, and the minimum after each call is the
    oracle's over the labels written so far."""
    steps = (300, 257, 513, 65)
    total = sum(steps)
    want, _ = oracle_range(NODE, 0, total)
    mgr = init_session(total, scratch_bytes=192 * N * 128)
    try:
        written = 0
        for ask in steps:
            done, _ = mgr.step(ask)
            assert done == ask
            written += ask
            assert mgr.vrf_nonce() == oracle_range(NODE, 0, written)[1]
        assert mgr.copy_labels(0, total) == want
    finally:
        mgr.reset()


def _unpack(packed, k, bpi):
    v = int.from_bytes(packed, "little")
    return [(v >> (i * bpi)) & ((1 << bpi) - 1) for i in range(k)]


def _pack(idx, bpi):
    v = 0
    for i, x in enumerate(idx):
        v |= x << (i * bpi)
    return v.to_bytes((len(idx) * bpi + 7) // 8, "little")


def _o_proof(p, k2):
    op = Proof()
    op.nonce, op.pow, op.num_indices = p.nonce, p.pow, k2
    op.indices_len = len(p.indices)
    for i, b in enumerate(p.indices):
        op.indices[i] = b
    return op


TOTAL, K1, BPI = 2048, 12, 11


@functools.lru_cache(maxsize=None)
def proof_pool(k2):
    """For each identity a proof the oracle made and a copy with its last
    index swapped, each with the oracle's verdict."""
    o = Oracle()
    pool = []
    for node in (NODE, NODE2):
        labels, _ = o.init_range(o.commitment(node, ATX), 0, TOTAL, N,
                                 with_nonce=False)
        op = o.prove(labels, TOTAL, CHALLENGE, K1, k2, 16, POW_DIFF)
        idx = _unpack(bytes(op.indices[:op.indices_len]), k2, BPI)
        for cand in (idx, idx[:-1] + [(idx[-1] + 1) % TOTAL]):
            p = gsm_amd.PostProof(op.nonce, _pack(cand, BPI), op.pow)
            orc, oinv = o.verify(_o_proof(p, k2),
                                 make_meta(node, ATX, CHALLENGE, 1, TOTAL),
                                 N, K1, k2, k2, None, -1, POW_DIFF)
            pool.append((p, gsm_amd.PostProofMetadata(node, ATX, CHALLENGE,
                                                      1, TOTAL), orc, oinv))
    return pool


@gpu
@pytest.mark.parametrize("k2,nproofs", [(1, 1), (3, 1), (3, 21), (1, 65),
                                        (1, 257)])
def test_index_list_two_commitments_full_labels(k2, nproofs):
    """k2 * nproofs = 1, 3, 63, 65, 257 tasks; neighbouring proofs differ
    in identity, so neighbouring tasks differ in commit_ids."""
    pool = proof_pool(k2)
    order = [(0, 2, 1, 3)[i % 4] for i in range(nproofs)]
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=TOTAL, k1=K1,
                             k2=k2, k3=k2, pow_difficulty=POW_DIFF)
    ver = gsm_amd.PostVerifier(cfg, scrypt_n=N)
    res = ver.verify_batch([pool[i][0] for i in order],
                           [pool[i][1] for i in order])
    assert any(pool[i][2] == 0 for i in order)
    for (st, inv), i in zip(res, order):
        _, _, orc, oinv = pool[i]
        assert (st == gsm_amd.api.Status.OK) == (orc == 0), (i, st, orc)
        if orc != 0:
            assert st == gsm_amd.api.Status.INVALID_INDEX and inv == oinv


@gpu
@pytest.mark.parametrize("count", COUNTS)
def test_audit_reports_the_altered_label_only(count):
    base = 2**33 + 5
    want, _ = oracle_range(NODE, base, count)
    hurt = count // 2
    disk = bytearray(want)
    disk[hurt * 16 + 9] ^= 0x40
    disk = bytes(disk)
    rep = gsm_amd.verify_data_buffer(disk, base, NODE, ATX, N,
                                     gsm_amd.AuditOpts(sample_every=1))
    assert rep.labels_checked == count
    assert rep.labels_missing == 0
    assert rep.labels_bad == 1
    assert rep.bad == [(base + hurt, disk[hurt * 16:hurt * 16 + 16],
                        want[hurt * 16:hurt * 16 + 16])]
