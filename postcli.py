#!/usr/bin/env python3
"""postcli — operator CLI over the MI355X POST engine.

Plays the role of the post-rs tooling around the reference node: data
initialization into a postdata directory, proof generation over it (the
post-service GenProof role, api/grpcserver/post_client.go:69-143), proof
verification, provider listing and benchmarking
(activation/post_supervisor.go:105-127).

    python postcli.py providers
    python postcli.py benchmark [--scrypt-n 8192]
    python postcli.py init --datadir DIR --node-id HEX32 --atx-id HEX32 \
        --num-units U [--labels-per-unit L] [--scrypt-n N] \
        [--max-file-size B] [--shard R/W] [--seal] \
        [--initial-proof [--k1 K] [--k2 K] [--nonces 288]]
    python postcli.py initial-proof --datadir DIR
    python postcli.py prove --datadir DIR --challenge HEX32 [--nonces 288] \
        [--check-seal [--max-report N] \
         [--heal [--write-back] [--max-heal-pages N]]]
    python postcli.py verify --datadir DIR --proof proof.json \
        [--k3 K] [--seed HEX] [--vrf-nonce [INDEX]]
    python postcli.py verify-data --datadir DIR [--every K | --fraction PCT] \
        [--seed S] [--shard R/W | --from I --to J] [--max-report N]
    python postcli.py seal --datadir DIR [--assemble]
    python postcli.py check-seal --datadir DIR [--max-report N]
    python postcli.py repair --datadir DIR [--max-heal-pages N]

init resumes automatically from existing postdata_*.bin
(activation/post.go:267-271); --shard R/W initializes only rank R of W
contiguous index-range shards (the multi-GPU axis).

verify --vrf-nonce also checks the VRF nonce (the Nonce of
postdata_metadata.json, or INDEX) in the same engine call as the proof and
adds "vrf_nonce": {"index", "valid"} to the output; exit status 1 when
either is invalid.

verify-data audits the labels on disk (upstream postcli -verify -fraction):
one label per window of K labels is recomputed on the GPU and compared with
the file bytes; exit status 1 when any sampled label is bad or missing.

seal writes postdata_seal.bin, one digest per 1024-label page of the dir
(DESIGN §3.5); check-seal recomputes the digests on the GPU, prints the bad
pages as label ranges and exits with status 1 when there is one; prove
--check-seal does the same check during the proving pass itself, prints the
ranges on stderr as ready verify-data commands, and withholds a proof that
has an index in a bad page (exit status 1).

init --seal produces the same sidecar during init, from the labels as they
lie in device memory: each shard appends to
postdata_seal.part-<index_start> and the last one to finish assembles
postdata_seal.bin; seal --assemble does that assembly by hand (no GPU) and
exits with status 2, naming the missing pages, while a shard is unfinished.
A shard that is not made of whole 1024-label pages is refused (status 2).

init --initial-proof runs the proving scan for the zero challenge over every
batch while it lies in device memory and appends the hits to
postdata_hits.part-<index_start>; when its range completes and the parts of
all shards are there it writes initial_proof.json into the dir, in the format
prove prints, and otherwise says which range is outstanding.  initial-proof
does that merge alone (no GPU; exit status 1 while a range is outstanding or
when no nonce reaches K2).  Either output is accepted by verify as it is.

prove --check-seal --heal puts the bad pages right in the same call (DESIGN
§3.6): they are recomputed on the GPU, their hits replaced, and the proof is
the one the undamaged dir gives; --write-back also writes the pages the seal
confirms over the file bytes.  The proof is withheld (exit status 1) when it
has an index in a page the seal could not confirm, or when more than
--max-heal-pages pages are bad and nothing was healed.  repair is the same
pass without a proof: it writes the confirmed pages back and exits with
status 0 when a following check-seal would be clean.
"""
import argparse
import base64
import json
import os
import sys
import threading
import time

sys.path.insert(0, __file__.rsplit("/", 1)[0])

import gsm_amd  # noqa: E402
from gsm_amd import wire  # noqa: E402


def cmd_providers(_args):
    provs = list(gsm_amd.Engine().providers())
    for p in provs:
        print(json.dumps(p))
    if not provs:
        print("no MI355X providers found (no GPU visible)", file=sys.stderr)
        return 1
    return 0


def cmd_benchmark(args):
    lps = gsm_amd.Engine().benchmark(args.provider, args.scrypt_n)
    print(json.dumps({"provider": args.provider, "scrypt_n": args.scrypt_n,
                      "labels_per_sec": lps}))


def _mk_cfg(args):
    if getattr(args, "preset", None):
        import importlib
        presets = importlib.import_module("go-spacemesh_amd.presets")
        cfg, popts = presets.get(args.preset)
        args.labels_per_unit = cfg.labels_per_unit
        args.scrypt_n = popts.scrypt_n
        if args.num_units is None:
            args.num_units = popts.num_units
    else:
        cfg = gsm_amd.PostConfig(labels_per_unit=args.labels_per_unit,
                                 min_num_units=1)
    if getattr(args, "pow_difficulty", None):
        cfg.pow_difficulty = bytes.fromhex(args.pow_difficulty)
    return cfg


def _proof_json(proof, challenge, seconds):
    """A proof as prove prints it and verify reads it."""
    return {"nonce": proof.nonce,
            "indices": base64.b64encode(proof.indices).decode(),
            "pow": proof.pow,
            "challenge": challenge.hex(),
            "seconds": round(seconds, 2),
            "scale_encoded_postv1": wire.PostV1(
                proof.nonce, proof.indices, proof.pow).encode().hex()}


ZERO_CHALLENGE = bytes(32)          # shared.ZeroChallenge


def cmd_initial_proof(args):
    t0 = time.time()
    try:
        proof, rep = gsm_amd.init_proof_assemble(args.datadir)
    except gsm_amd.EngineError as e:
        print(f"initial-proof failed: {e}", file=sys.stderr)
        return 1
    print(f"initial proof from {rep.parts} part(s), {rep.hits} hits over "
          f"{rep.labels_covered} labels", file=sys.stderr)
    print(json.dumps(_proof_json(proof, ZERO_CHALLENGE, time.time() - t0)))
    return 0


def cmd_init(args):
    node = bytes.fromhex(args.node_id)
    atx = bytes.fromhex(args.atx_id)
    cfg = _mk_cfg(args)
    if args.num_units is None:
        raise SystemExit("either --num-units or --preset is required")
    start = end = 0
    if args.shard:
        import importlib
        sharding = importlib.import_module("go-spacemesh_amd.sharding")
        r, w = (int(x) for x in args.shard.split("/"))
        total = args.num_units * args.labels_per_unit
        start, end = sharding.shard_range(total, w, r)
    opts = gsm_amd.PostSetupOpts(
        data_dir=args.datadir, num_units=args.num_units,
        max_file_size=args.max_file_size, provider_id=args.provider,
        scrypt_n=args.scrypt_n, index_start=start, index_end=end)
    if args.seal:
        opts.seal = True
    if not args.initial_proof and (args.k1 is not None or args.k2 is not None
                                   or args.nonces is not None):
        raise SystemExit("--k1, --k2 and --nonces need --initial-proof")
    if args.initial_proof:
        ip = gsm_amd.InitialProofOpts.of(cfg, challenge=ZERO_CHALLENGE)
        if args.k1 is not None:
            ip.k1 = args.k1
        if args.k2 is not None:
            ip.k2 = args.k2
        if args.nonces is not None:
            ip.nonces = args.nonces
        opts.initial_proof = ip
    mgr = gsm_amd.PostSetupManager(node, atx, cfg, opts)
    if args.seal or args.initial_proof:
        # what a sealed session refuses (an unaligned shard, a dir started
        # without a seal) is the operator's to put right, like a bad sidecar
        try:
            mgr.prepare_initializer()
        except gsm_amd.EngineError as e:
            flags = " ".join(f for f, on in (("--seal", args.seal),
                                             ("--initial-proof",
                                              args.initial_proof)) if on)
            print(f"init {flags} failed: {e}", file=sys.stderr)
            return 2
    else:
        mgr.prepare_initializer()
    st = mgr.status()
    total = (end or args.num_units * args.labels_per_unit) - start
    print(f"resuming at {st['num_labels_written']}/{total} labels",
          file=sys.stderr)

    stop = threading.Event()

    def progress():
        while not stop.wait(5):
            s = mgr.status()
            print(f"  {s['num_labels_written']}/{total} labels",
                  file=sys.stderr)

    t = threading.Thread(target=progress, daemon=True)
    t.start()
    resumed_at = st["num_labels_written"]
    t0 = time.time()
    mgr.start_session()
    stop.set()
    dt = time.time() - t0
    done = total - resumed_at
    nonce = mgr.vrf_nonce()
    print(json.dumps({
        "labels": total, "labels_this_session": done,
        "seconds": round(dt, 1),
        "labels_per_sec": round(done / dt, 1) if dt > 0 and done else None,
        "vrf_nonce": nonce[0] if nonce else None,
    }))
    mgr.reset()
    if args.initial_proof:
        # the range is complete: merge, when every shard's part is there
        t0 = time.time()
        try:
            proof, _ = gsm_amd.init_proof_assemble(args.datadir)
        except gsm_amd.EngineError as e:
            print(f"initial proof not written: {e}", file=sys.stderr)
            return 0
        path = os.path.join(args.datadir, "initial_proof.json")
        with open(path, "w") as f:
            json.dump(_proof_json(proof, ZERO_CHALLENGE, time.time() - t0), f)
            f.write("\n")
        print(f"initial proof written to {path}", file=sys.stderr)
    return 0


def cmd_prove(args):
    md = wire.PostMetadata.read(args.datadir)
    cfg = gsm_amd.PostConfig(labels_per_unit=md.labels_per_unit,
                             min_num_units=1)
    if args.pow_difficulty:
        cfg.pow_difficulty = bytes.fromhex(args.pow_difficulty)
    t0 = time.time()
    if not args.heal and (args.write_back or args.max_heal_pages):
        raise SystemExit("--write-back and --max-heal-pages need --heal")
    if args.heal:
        if not args.check_seal:
            raise SystemExit("--heal needs --check-seal")
        try:
            proof, rep = gsm_amd.prove_healed(
                args.datadir, bytes.fromhex(args.challenge), cfg,
                gsm_amd.ProveOpts(nonces=args.nonces),
                heal=gsm_amd.HealOpts(max_pages=args.max_heal_pages,
                                      write_back=args.write_back),
                max_report=args.max_report)
        except gsm_amd.EngineError as e:
            print(f"prove failed: {e}", file=sys.stderr)
            return 2
        if rep.heal_skipped:
            print(f"seal: {rep.pages_bad} of {rep.pages} pages differ from "
                  "postdata_seal.bin, more than --max-heal-pages: nothing "
                  "healed; confirm with", file=sys.stderr)
            for a, b in rep.bad_label_ranges():
                print(f"  verify-data --datadir {args.datadir} --every 1 "
                      f"--from {a} --to {b}", file=sys.stderr)
        elif not rep.clean:
            for a, b in rep.bad_label_ranges():
                print(f"healed labels [{a}, {b})", file=sys.stderr)
            print(f"seal: {rep.pages_bad} of {rep.pages} pages differed, "
                  f"{rep.pages_healed} recomputed "
                  f"({rep.labels_repaired} labels differed on disk), "
                  f"{rep.pages_unconfirmed} not confirmed by the seal, "
                  f"{rep.pages_written} written back", file=sys.stderr)
        if not rep.publishable:
            print("the proof has an index in a bad page: not printed, do "
                  "not publish" if not rep.heal_skipped else
                  "the bad pages were not healed: the proof is not printed, "
                  "do not publish", file=sys.stderr)
            return 1
    elif args.check_seal:
        try:
            proof, rep = gsm_amd.prove_checked(
                args.datadir, bytes.fromhex(args.challenge), cfg,
                gsm_amd.ProveOpts(nonces=args.nonces),
                max_report=args.max_report)
        except gsm_amd.EngineError as e:
            print(f"prove failed: {e}", file=sys.stderr)
            return 2
        if not rep.clean:
            print(f"seal: {rep.pages_bad} of {rep.pages} pages differ from "
                  "postdata_seal.bin; confirm with", file=sys.stderr)
            for a, b in rep.bad_label_ranges():
                print(f"  verify-data --datadir {args.datadir} --every 1 "
                      f"--from {a} --to {b}", file=sys.stderr)
        if rep.proof_touches_bad_page:
            print("the proof has an index in a bad page: not printed, do "
                  "not publish", file=sys.stderr)
            return 1
    else:
        proof = gsm_amd.api.prove_dir(args.datadir,
                                      bytes.fromhex(args.challenge), cfg,
                                      gsm_amd.ProveOpts(nonces=args.nonces))
    print(json.dumps(_proof_json(proof, bytes.fromhex(args.challenge),
                                 time.time() - t0)))


def cmd_seal(args):
    t0 = time.time()
    if args.assemble:
        try:
            pages = gsm_amd.seal_assemble(args.datadir)
        except gsm_amd.EngineError as e:
            print(f"seal --assemble failed: {e}", file=sys.stderr)
            return 2
        print(json.dumps({"pages": pages, "assembled": True,
                          "seconds": round(time.time() - t0, 2)}))
        return 0
    try:
        rep = gsm_amd.seal_data(args.datadir, args.provider)
    except gsm_amd.EngineError as e:
        print(f"seal failed: {e}", file=sys.stderr)
        return 2
    print(json.dumps({"total_labels": rep.total_labels, "pages": rep.pages,
                      "seconds": round(time.time() - t0, 2)}))
    return 0


def cmd_check_seal(args):
    t0 = time.time()
    try:
        rep = gsm_amd.check_seal(args.datadir, args.provider,
                                 args.max_report)
    except gsm_amd.EngineError as e:
        print(f"check-seal failed: {e}", file=sys.stderr)
        return 2
    print(json.dumps({
        "total_labels": rep.total_labels, "pages": rep.pages,
        "pages_bad": rep.pages_bad,
        "bad": [{"page": p, "from": a, "to": b} for p, (a, b)
                in zip(rep.bad_pages, rep.bad_label_ranges())],
        "seconds": round(time.time() - t0, 2),
    }))
    return 0 if rep.clean else 1


def cmd_repair(args):
    t0 = time.time()
    try:
        rep = gsm_amd.repair_data(
            args.datadir, gsm_amd.HealOpts(max_pages=args.max_heal_pages),
            args.provider, args.max_report)
    except gsm_amd.EngineError as e:
        print(f"repair failed: {e}", file=sys.stderr)
        return 2
    print(json.dumps({
        "total_labels": rep.total_labels, "pages": rep.pages,
        "pages_bad": rep.pages_bad, "pages_healed": rep.pages_healed,
        "pages_written": rep.pages_written,
        "pages_unconfirmed": rep.pages_unconfirmed,
        "labels_repaired": rep.labels_repaired,
        "heal_skipped": rep.heal_skipped,
        "bad": [{"page": p, "from": a, "to": b} for p, (a, b)
                in zip(rep.bad_pages, rep.bad_label_ranges())],
        "seconds": round(time.time() - t0, 2),
    }))
    return 0 if rep.repaired else 1


def cmd_verify(args):
    md = wire.PostMetadata.read(args.datadir)
    with open(args.proof) as f:
        pj = json.load(f)
    proof = gsm_amd.PostProof(pj["nonce"],
                              base64.b64decode(pj["indices"]), pj["pow"])
    cfg = gsm_amd.PostConfig(labels_per_unit=md.labels_per_unit,
                             min_num_units=1, k3=args.k3)
    if args.pow_difficulty:
        cfg.pow_difficulty = bytes.fromhex(args.pow_difficulty)
    ver = gsm_amd.PostVerifier(cfg, scrypt_n=md.scrypt_n)
    meta = gsm_amd.PostProofMetadata(
        md.node_id, md.commitment_atx_id, bytes.fromhex(pj["challenge"]),
        md.num_units, md.labels_per_unit)
    seed = bytes.fromhex(args.seed) if args.seed else None
    if args.vrf_nonce is not None:
        return verify_with_vrf_nonce(args, md, ver, proof, meta, seed)
    try:
        ver.verify(proof, meta, gsm_amd.VerifyOpts(subset_seed=seed))
        print(json.dumps({"valid": True}))
    except gsm_amd.EngineError as e:
        print(json.dumps({"valid": False, "error": str(e)}))
        sys.exit(1)


def verify_with_vrf_nonce(args, md, ver, proof, meta, seed):
    """verify --vrf-nonce: the proof and the VRF nonce (the metadata's, or
    the index given) checked in one engine call."""
    index = md.nonce if args.vrf_nonce is True else args.vrf_nonce
    if index is None:
        raise SystemExit("--vrf-nonce: postdata_metadata.json has no Nonce; "
                         "give an index")
    try:
        res, vres = ver.verify_batch(
            [proof], [meta], gsm_amd.VerifyOpts(subset_seed=seed),
            vrf=([meta], [index]))
    except gsm_amd.EngineError as e:
        print(json.dumps({"valid": False, "error": str(e)}))
        return 1
    (status, inv), vstatus = res[0], vres[0]
    Status = gsm_amd.Status
    out = {"valid": int(status) == Status.OK}
    if int(status) == Status.INVALID_INDEX:
        out["error"] = str(gsm_amd.EngineError(
            status, f"invalid POST index at position {inv}"))
    elif int(status) != Status.OK:
        out["error"] = str(gsm_amd.EngineError(status, ""))
    out["vrf_nonce"] = {"index": index,
                        "valid": int(vstatus) == Status.OK}
    print(json.dumps(out))
    return 0 if out["valid"] and out["vrf_nonce"]["valid"] else 1


def audit_period(args):
    """--every K, or --fraction PCT as K = max(1, round(100 / PCT));
    default --fraction 1."""
    if args.every is not None:
        if args.every < 1:
            raise SystemExit("--every must be >= 1")
        return args.every
    pct = 1.0 if args.fraction is None else args.fraction
    if not 0 < pct <= 100:
        raise SystemExit("--fraction must be in (0, 100]")
    return max(1, round(100 / pct))


def audit_range(args, total_labels):
    """[start, end) to audit: --shard R/W, --from/--to, or 0,0 (all)."""
    if args.shard:
        if args.index_from is not None or args.index_to is not None:
            raise SystemExit("--shard excludes --from/--to")
        import importlib
        sharding = importlib.import_module("go-spacemesh_amd.sharding")
        r, w = (int(x) for x in args.shard.split("/"))
        return sharding.shard_range(total_labels, w, r)
    if args.index_from is None and args.index_to is None:
        return 0, 0
    return (args.index_from or 0,
            total_labels if args.index_to is None else args.index_to)


def cmd_verify_data(args):
    # the engine reads and checks the dir's metadata itself; the CLI needs
    # the label count only to turn --shard or an open --from into a range
    total = 0
    if args.shard or (args.index_from is not None and args.index_to is None):
        try:
            total = wire.PostMetadata.read(args.datadir).num_labels()
        except (OSError, KeyError, ValueError, TypeError) as e:
            print(f"verify-data failed: cannot read postdata_metadata.json: "
                  f"{e!r}", file=sys.stderr)
            return 2
    start, end = audit_range(args, total)
    opts = gsm_amd.AuditOpts(
        sample_every=audit_period(args), seed=args.seed, index_start=start,
        index_end=end, provider_id=args.provider, max_report=args.max_report)
    last = [time.time()]

    def progress(checked, to_check):
        if time.time() - last[0] >= 5:
            last[0] = time.time()
            print(f"  {checked}/{to_check} labels", file=sys.stderr)

    print(f"auditing every {opts.sample_every} labels of "
          + (f"[{start}, {end})" if end else "the whole label space"),
          file=sys.stderr)
    t0 = time.time()
    try:
        rep = gsm_amd.verify_data(args.datadir, opts, progress)
    except gsm_amd.EngineError as e:
        print(f"verify-data failed: {e}", file=sys.stderr)
        return 2
    dt = time.time() - t0
    print(json.dumps({
        "sample_every": opts.sample_every, "seed": opts.seed,
        "index_start": start, "index_end": start + rep.labels_in_range,
        "labels_in_range": rep.labels_in_range,
        "labels_sampled": rep.labels_sampled,
        "labels_checked": rep.labels_checked,
        "labels_missing": rep.labels_missing,
        "labels_bad": rep.labels_bad,
        "bad": [{"index": i, "on_disk": d.hex(), "expected": x.hex()}
                for i, d, x in rep.bad],
        "seconds": round(dt, 2),
        "labels_per_sec": round(rep.labels_checked / dt, 1) if dt > 0
        else None,
    }))
    return 0 if rep.clean else 1


def build_parser():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("providers").set_defaults(fn=cmd_providers)
    b = sub.add_parser("benchmark")
    b.add_argument("--provider", type=int, default=0)
    b.add_argument("--scrypt-n", type=int, default=8192)
    b.set_defaults(fn=cmd_benchmark)
    i = sub.add_parser("init")
    i.add_argument("--datadir", required=True)
    i.add_argument("--node-id", required=True)
    i.add_argument("--atx-id", required=True)
    i.add_argument("--num-units", type=int, default=None)
    i.add_argument("--preset", default=None,
                   help="mainnet|testnet|fastnet parameter preset")
    i.add_argument("--labels-per-unit", type=int, default=4294967296)
    i.add_argument("--scrypt-n", type=int, default=8192)
    i.add_argument("--max-file-size", type=int, default=4294967296)
    i.add_argument("--provider", type=int, default=0)
    i.add_argument("--shard", default=None, help="R/W index-range shard")
    i.add_argument("--pow-difficulty", default=None)
    i.add_argument("--seal", action="store_true",
                   help="write postdata_seal.bin from the device during init")
    i.add_argument("--initial-proof", action="store_true",
                   help="scan for the zero-challenge proof during init")
    i.add_argument("--k1", type=int, default=None)
    i.add_argument("--k2", type=int, default=None)
    i.add_argument("--nonces", type=int, default=None)
    i.set_defaults(fn=cmd_init)
    ip = sub.add_parser("initial-proof")
    ip.add_argument("--datadir", required=True)
    ip.set_defaults(fn=cmd_initial_proof)
    p = sub.add_parser("prove")
    p.add_argument("--datadir", required=True)
    p.add_argument("--challenge", required=True)
    p.add_argument("--nonces", type=int, default=288)
    p.add_argument("--pow-difficulty", default=None)
    p.add_argument("--check-seal", action="store_true",
                   help="check postdata_seal.bin in the same pass")
    p.add_argument("--max-report", type=int, default=64)
    p.add_argument("--heal", action="store_true",
                   help="with --check-seal: recompute the bad pages and "
                        "prove over the recomputed labels")
    p.add_argument("--write-back", action="store_true",
                   help="with --heal: write confirmed pages to the files")
    p.add_argument("--max-heal-pages", type=int, default=0,
                   help="with --heal: heal at most N pages (default 4096)")
    p.set_defaults(fn=cmd_prove)
    s = sub.add_parser("seal")
    s.add_argument("--datadir", required=True)
    s.add_argument("--provider", type=int, default=0)
    s.add_argument("--assemble", action="store_true",
                   help="no pass: put the part files of init --seal together")
    s.set_defaults(fn=cmd_seal)
    c = sub.add_parser("check-seal")
    c.add_argument("--datadir", required=True)
    c.add_argument("--provider", type=int, default=0)
    c.add_argument("--max-report", type=int, default=64)
    c.set_defaults(fn=cmd_check_seal)
    r = sub.add_parser("repair")
    r.add_argument("--datadir", required=True)
    r.add_argument("--provider", type=int, default=0)
    r.add_argument("--max-heal-pages", type=int, default=0)
    r.add_argument("--max-report", type=int, default=64)
    r.set_defaults(fn=cmd_repair)
    v = sub.add_parser("verify")
    v.add_argument("--datadir", required=True)
    v.add_argument("--proof", required=True)
    v.add_argument("--k3", type=int, default=37)
    v.add_argument("--seed", default=None)
    v.add_argument("--pow-difficulty", default=None)
    v.add_argument("--vrf-nonce", nargs="?", type=int, const=True,
                   default=None, metavar="INDEX",
                   help="also check the VRF nonce (default: the Nonce of "
                        "postdata_metadata.json) in the same engine call")
    v.set_defaults(fn=cmd_verify)
    a = sub.add_parser("verify-data")
    a.add_argument("--datadir", required=True)
    how = a.add_mutually_exclusive_group()
    how.add_argument("--every", type=int, default=None,
                     help="check one label per K (1 = every label)")
    how.add_argument("--fraction", type=float, default=None,
                     help="percent of labels to check (default 1)")
    a.add_argument("--seed", type=lambda x: int(x, 0), default=0)
    a.add_argument("--shard", default=None, help="R/W index-range shard")
    a.add_argument("--from", dest="index_from", type=int, default=None)
    a.add_argument("--to", dest="index_to", type=int, default=None)
    a.add_argument("--provider", type=int, default=0)
    a.add_argument("--max-report", type=int, default=64)
    a.set_defaults(fn=cmd_verify_data)
    return ap


def main():
    args = build_parser().parse_args()
    sys.exit(args.fn(args))


if __name__ == "__main__":
    main()
