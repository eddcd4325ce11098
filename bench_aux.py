#!/usr/bin/env python3
"""bench_aux.py — auxiliary measurements: the proving scan (BASELINE
config 4 shape), proving over a sealed dir with the seal checked in the same
pass (against plain proving over that dir), batched verification
(config 5 shape) and batched VRF-nonce checks on one MI355X.

Prints one JSON line per measurement.  Run on a GPU box:
    python bench_aux.py [--scan-labels LOG2] [--verify-proofs N]
                        [--vrf-items N]
(--verify-proofs 0 leaves the verification legs out, --vrf-items 0 the VRF
leg.)

These are recorded alongside the main bench (profiles/aux_rNN.json); the
headline metric stays bench.py's labels/s.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import gsm_amd  # noqa: E402

NODE = bytes([0xA5]) * 32
ATX = bytes([0x5A]) * 32
MAINNET_POW_DIFF = bytes.fromhex(
    "000dfb23b0979b4b000000000000000000000000000000000000000000000000")


def bench_scan(log2_labels: int):
    """Proving index scan: 288 nonces / 144 AES-128 ciphers per 16-B label
    (config 4 shape; label count shrunk from 2^34, per-byte work identical).
    Includes k2pow (host) and H2D chunk uploads, as post_prove does."""
    total = 1 << log2_labels
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total,
                             k1=26, k2=37,
                             pow_difficulty=MAINNET_POW_DIFF)
    opts = gsm_amd.PostSetupOpts(num_units=1, scrypt_n=8192)
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
    mgr.prepare_initializer()
    t0 = time.perf_counter()
    mgr.start_session()
    init_s = time.perf_counter() - t0
    labels = mgr.copy_labels(0, total)
    mgr.reset()

    t0 = time.perf_counter()
    proof = gsm_amd.api.prove_buffer(labels, total, NODE, ATX, bytes(32),
                                     cfg, gsm_amd.ProveOpts(nonces=288))
    scan_s = time.perf_counter() - t0
    print(json.dumps({
        "metric": "prove_scan_labels_per_sec",
        "value": round(total / scan_s, 1),
        "unit": "labels/s",
        "label_bytes_per_sec": round(total * 16 / scan_s, 1),
        "seconds": round(scan_s, 3),
        "init_seconds": round(init_s, 3),
        "config": {"labels": total, "nonces": 288, "k1": 26, "k2": 37,
                   "pow": "blake3-mode, mainnet difficulty",
                   "includes": "k2pow host search + H2D chunk uploads"},
        "nonce": proof.nonce,
    }))
    return labels, cfg, proof


def bench_prove_checked(labels: bytes, cfg, proof, repeats: int = 2):
    """Proving over a data dir with the seal checked in the same pass
    (post_prove_checked), against plain post_prove over the same dir.  The
    dir holds the labels of the scan leg in /dev/shm (memory-backed, so the
    pass is bound by the pipeline and not by a disk); falls back to the
    temp dir where there is no /dev/shm."""
    import shutil
    import tempfile
    total = len(labels) // 16
    per_file = 1 << 22                          # 64 MiB files
    root = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tempfile.mkdtemp(prefix="post_bench_seal_", dir=root)
    try:
        for i in range(-(-total // per_file)):
            with open(os.path.join(d, f"postdata_{i}.bin"), "wb") as f:
                f.write(labels[i * per_file * 16:(i + 1) * per_file * 16])
        t0 = time.perf_counter()
        gsm_amd.seal_data(d)
        seal_s = time.perf_counter() - t0
        opts = gsm_amd.ProveOpts(nonces=288)
        plain, checked = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            p = gsm_amd.api.prove_dir(d, bytes(32), cfg, opts)
            plain.append(time.perf_counter() - t0)
            assert p == proof
            t0 = time.perf_counter()
            p, rep = gsm_amd.prove_checked(d, bytes(32), cfg, opts)
            checked.append(time.perf_counter() - t0)
            assert p == proof and rep.clean and rep.pages == -(-total // 1024)
        print(json.dumps({
            "metric": "prove_checked_labels_per_sec",
            "value": round(total / min(checked), 1),
            "unit": "labels/s",
            "prove_dir_labels_per_sec": round(total / min(plain), 1),
            "checked_seconds": [round(x, 4) for x in checked],
            "prove_dir_seconds": [round(x, 4) for x in plain],
            "seal_seconds": round(seal_s, 3),
            "config": {"labels": total, "nonces": 288, "k1": 26, "k2": 37,
                       "dir": "memory-backed" if root else "temp dir",
                       "seal_stream": os.environ.get("POST_SEAL_STREAM",
                                                     "second"),
                       "includes": "k2pow host search + file reads + H2D"},
        }))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def bench_verify(n_proofs: int):
    """Batched verification (config 5 shape): label space 2^20 so proofs
    generate quickly, but label recompute at mainnet scryptN=8192 — the
    dominant verification cost."""
    total = 1 << 20
    cfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total,
                             k1=26, k2=37, k3=1,
                             pow_difficulty=MAINNET_POW_DIFF)
    opts = gsm_amd.PostSetupOpts(num_units=1, scrypt_n=8192)
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
    mgr.prepare_initializer()
    mgr.start_session()
    labels = mgr.copy_labels(0, total)
    mgr.reset()

    base_proofs = []
    for c in range(4):
        challenge = bytes([c]) * 32
        base_proofs.append((challenge, gsm_amd.api.prove_buffer(
            labels, total, NODE, ATX, challenge, cfg,
            gsm_amd.ProveOpts(nonces=288))))

    proofs, metas = [], []
    for i in range(n_proofs):
        ch, pr = base_proofs[i % len(base_proofs)]
        proofs.append(pr)
        metas.append(gsm_amd.PostProofMetadata(NODE, ATX, ch, 1, total))

    for k3, seed in [(1, b"peer-seed"), (37, None)]:
        vcfg = gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total,
                                  k1=26, k2=37, k3=k3,
                                  pow_difficulty=MAINNET_POW_DIFF)
        ver = gsm_amd.PostVerifier(vcfg, scrypt_n=8192)
        vopts = gsm_amd.VerifyOpts(subset_seed=seed)
        # warmup at FULL batch size: the cached workspace reserves its
        # buffers here (a first large hipMalloc costs seconds on some
        # boxes and must not land in the timed region)
        ver.verify_batch(proofs, metas, vopts)
        t0 = time.perf_counter()
        res = ver.verify_batch(proofs, metas, vopts)
        dt = time.perf_counter() - t0
        ok = sum(1 for s, _ in res if s == gsm_amd.api.Status.OK)
        assert ok == n_proofs, f"{ok}/{n_proofs} verified"
        # ABI-boundary rate: marshal once untimed (a cgo shim holds these
        # layouts natively; the ctypes build is Python-mirror overhead)
        mar = ver.marshal_batch(proofs, metas)
        t0 = time.perf_counter()
        res2 = ver.verify_batch(proofs, metas, vopts, marshalled=mar)
        dt_abi = time.perf_counter() - t0
        assert sum(1 for s, _ in res2
                   if s == gsm_amd.api.Status.OK) == n_proofs
        print(json.dumps({
            "metric": "verify_proofs_per_sec",
            "value": round(n_proofs / dt, 1),
            "unit": "proofs/s",
            "seconds": round(dt, 3),
            "abi_boundary_proofs_per_sec": round(n_proofs / dt_abi, 1),
            "config": {"proofs": n_proofs, "k3": k3, "k2": 37,
                       "scrypt_n": 8192,
                       "mode": "full-K2" if k3 >= 37 else f"K3={k3} subset",
                       "batched": True},
        }))

    # worker-pool shape: one proof per call (the reference's inner-verifier
    # call pattern, post_verifier.go:150-160)
    ver = gsm_amd.PostVerifier(
        gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total, k1=26,
                           k2=37, k3=1, pow_difficulty=MAINNET_POW_DIFF),
        scrypt_n=8192)
    vopts = gsm_amd.VerifyOpts(subset_seed=b"peer-seed")
    n_single = min(64, n_proofs)
    t0 = time.perf_counter()
    for i in range(n_single):
        ver.verify(proofs[i], metas[i], vopts)
    dt = time.perf_counter() - t0
    print(json.dumps({
        "metric": "verify_proofs_per_sec_single_call",
        "value": round(n_single / dt, 1),
        "unit": "proofs/s",
        "config": {"proofs": n_single, "k3": 1, "batched": False},
    }))


REPEATS = 20    # timed calls per batched figure: best and mean are reported


def bench_vrf(n_items: int):
    """VRF-nonce checks at mainnet scryptN = 8192, at the C-ABI boundary
    (marshalled once, warmed at full size as bench_verify does): n_items in
    one post_verify_vrf_nonce_batch call, the single call looped over 64 of
    them, and a K3 = 1 proof batch of the same size for comparison (one
    label per proof, plus pow, unpack and the AES predicate)."""
    total = 1 << 20
    ver = gsm_amd.PostVerifier(
        gsm_amd.PostConfig(min_num_units=1, labels_per_unit=total, k1=26,
                           k2=37, k3=1, pow_difficulty=MAINNET_POW_DIFF),
        scrypt_n=8192)
    meta = gsm_amd.PostProofMetadata(NODE, ATX, bytes(32), 1, total)
    metas = [meta] * n_items
    indices = [(i * 7919) % total for i in range(n_items)]
    mar = ver.marshal_vrf(metas, indices)
    ver.verify_vrf_nonce_batch_marshalled(mar)          # warm-up, full size
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        res = ver.verify_vrf_nonce_batch_marshalled(mar)
        times.append(time.perf_counter() - t0)
    ok = sum(1 for s in res if s == gsm_amd.api.Status.OK)
    bad = sum(1 for s in res if s == gsm_amd.api.Status.INVALID_INDEX)
    assert ok + bad == n_items

    n_single = min(64, n_items)
    cm = meta.to_c()
    lib = ver.engine.lib
    from ctypes import byref
    t0 = time.perf_counter()
    single = [lib.post_verify_vrf_nonce(byref(cm), indices[i], 8192, 0)
              for i in range(n_single)]
    dt_single = time.perf_counter() - t0
    assert single == [int(s) for s in res[:n_single]]
    print(json.dumps({
        "metric": "verify_vrf_nonce_items_per_sec",
        "value": round(n_items / min(times), 1),
        "unit": "items/s",
        "mean_items_per_sec": round(n_items * len(times) / sum(times), 1),
        "seconds": [round(x, 4) for x in times],
        "single_call_items_per_sec": round(n_single / dt_single, 1),
        "config": {"items": n_items, "single_call_items": n_single,
                   "scrypt_n": 8192, "num_labels": total,
                   "passing": ok, "boundary": "C ABI, marshalled once"},
    }))

    # the K3 = 1 proof batch of the same size, same build and box
    opts = gsm_amd.PostSetupOpts(num_units=1, scrypt_n=8192)
    cfg = ver.cfg
    mgr = gsm_amd.PostSetupManager(NODE, ATX, cfg, opts)
    mgr.prepare_initializer()
    mgr.start_session()
    labels = mgr.copy_labels(0, total)
    mgr.reset()
    base = []
    for c in range(4):
        challenge = bytes([c]) * 32
        base.append((challenge, gsm_amd.api.prove_buffer(
            labels, total, NODE, ATX, challenge, cfg,
            gsm_amd.ProveOpts(nonces=288))))
    del labels
    proofs = [base[i % 4][1] for i in range(n_items)]
    pmetas = [gsm_amd.PostProofMetadata(NODE, ATX, base[i % 4][0], 1, total)
              for i in range(n_items)]
    vopts = gsm_amd.VerifyOpts(subset_seed=b"peer-seed")
    pmar = ver.marshal_batch(proofs, pmetas)
    ver.verify_batch(None, None, vopts, marshalled=pmar)
    ptimes = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        pres = ver.verify_batch(None, None, vopts, marshalled=pmar)
        ptimes.append(time.perf_counter() - t0)
    assert all(s == gsm_amd.api.Status.OK for s, _ in pres)
    # and both kinds in one call
    ver.verify_batch(None, None, vopts, marshalled=pmar, vrf=mar)
    mtimes = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ver.verify_batch(None, None, vopts, marshalled=pmar, vrf=mar)
        mtimes.append(time.perf_counter() - t0)
    print(json.dumps({
        "metric": "verify_k3_1_proofs_per_sec_same_size",
        "value": round(n_items / min(ptimes), 1),
        "unit": "proofs/s",
        "mean_proofs_per_sec": round(n_items * len(ptimes) / sum(ptimes), 1),
        "seconds": [round(x, 4) for x in ptimes],
        "mixed_call_seconds": [round(x, 4) for x in mtimes],
        "mixed_call_pairs_per_sec": round(n_items / min(mtimes), 1),
        "mixed_call_mean_pairs_per_sec": round(
            n_items * len(mtimes) / sum(mtimes), 1),
        "config": {"proofs": n_items, "k3": 1, "k2": 37, "scrypt_n": 8192,
                   "boundary": "C ABI, marshalled once",
                   "mixed_call": "the proofs and the VRF items above in "
                                 "one post_verify_batch_vrf"},
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan-labels", type=int, default=23)  # 2^23 = 128 MiB
    ap.add_argument("--verify-proofs", type=int, default=1000)
    ap.add_argument("--vrf-items", type=int, default=10000)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    labels, cfg, proof = bench_scan(args.scan_labels)
    bench_prove_checked(labels, cfg, proof)
    del labels
    if args.verify_proofs > 0:
        bench_verify(args.verify_proofs)
    if args.vrf_items > 0:
        bench_vrf(args.vrf_items)


if __name__ == "__main__":
    main()
