"""CPU-side engine checks: the C-ABI library loads, exports every symbol the
header declares, host crypto agrees with the oracle and the golden vectors,
and compute entries fail loudly without a GPU (no silent fallback)."""
import ctypes
import json
import os
import random
import re

import pytest

import gsm_amd

HEADER = os.path.join(os.path.dirname(__file__), "..", "include",
                      "spacemesh_post.h")
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                     "golden.json")))


def test_library_loads_and_version():
    eng = gsm_amd.Engine()
    assert "gfx950" in eng.version()


def test_all_header_symbols_exported():
    lib = gsm_amd.load_engine()
    src = open(HEADER).read()
    # function declarations: "<ret> post_xxx(" at top level
    names = re.findall(r"^\s*(?:const char \*|int|void|uint64_t)\s+"
                       r"(post_\w+)\s*\(", src, re.M)
    assert len(names) >= 18, names
    assert "post_selftest_verify_pred" in names
    for n in names:
        assert hasattr(lib, n), f"symbol {n} missing from libpost_hip.so"


def test_engine_blake3_matches_oracle(oracle):
    eng = gsm_amd.Engine()
    rng = random.Random(11)
    for n in [0, 1, 31, 32, 44, 49, 63, 64, 65, 128, 1000]:
        msg = bytes(rng.randrange(256) for _ in range(n))
        assert eng.selftest_blake3(msg) == o_blake3(oracle, msg)
    for v in GOLDEN["blake3_official"]:
        assert eng.selftest_blake3(
            bytes.fromhex(v["input_hex"])).hex() == v["out"]


def o_blake3(oracle, msg):
    return oracle.blake3(msg)


def test_engine_aes_matches_oracle_and_fips(oracle):
    eng = gsm_amd.Engine()
    for v in GOLDEN["aes128_fips197"]:
        assert eng.selftest_aes128(bytes.fromhex(v["key"]),
                                   bytes.fromhex(v["pt"])).hex() == v["ct"]
    rng = random.Random(12)
    for _ in range(50):
        k = bytes(rng.randrange(256) for _ in range(16))
        x = bytes(rng.randrange(256) for _ in range(16))
        assert eng.selftest_aes128(k, x) == oracle.aes128(k, x)


def test_engine_host_label_matches_openssl_golden():
    eng = gsm_amd.Engine()
    lv = GOLDEN["labels_openssl"]
    nid = bytes.fromhex(lv["node_id"])
    atx = bytes.fromhex(lv["atx_id"])
    for v in lv["labels"]:
        if v["N"] > 128:
            continue
        assert eng.selftest_label(nid, atx, v["index"],
                                  v["N"]).hex() == v["full"]


def test_no_gpu_is_loud():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    eng = gsm_amd.Engine()
    assert eng.providers() == []
    mgr = gsm_amd.PostSetupManager(bytes(32), bytes(32), gsm_amd.PostConfig(),
                                   gsm_amd.PostSetupOpts(num_units=4,
                                                         scrypt_n=2))
    with pytest.raises(gsm_amd.EngineError) as ei:
        mgr.prepare_initializer()
    assert ei.value.code == gsm_amd.api.Status.NO_GPU
    ver = gsm_amd.PostVerifier(gsm_amd.PostConfig(), scrypt_n=2)
    meta = gsm_amd.PostProofMetadata(bytes(32), bytes(32), bytes(32), 2, 64)
    with pytest.raises(gsm_amd.EngineError) as ei:
        ver.verify(gsm_amd.PostProof(0, b"\0" * 22, 0), meta)
    assert ei.value.code == gsm_amd.api.Status.NO_GPU


def test_randomx_mode_unsupported_is_explicit():
    """The reference's RandomX pow (post_types.go:84-114) is parity-unpinned:
    the engine must refuse it explicitly rather than silently substitute."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("covered by GPU tests")
    cfg = gsm_amd.PostConfig(pow_mode=gsm_amd.api.POW_MODE_RANDOMX)
    ver = gsm_amd.PostVerifier(cfg, scrypt_n=2)
    meta = gsm_amd.PostProofMetadata(bytes(32), bytes(32), bytes(32), 2, 64)
    with pytest.raises(gsm_amd.EngineError) as ei:
        ver.verify(gsm_amd.PostProof(0, b"\0" * 22, 0), meta)
    # pow-mode check precedes the GPU check in verify? either is acceptable,
    # but the error must be one of the two explicit codes
    assert ei.value.code in (gsm_amd.api.Status.UNSUPPORTED,
                             gsm_amd.api.Status.NO_GPU)


def test_zero_labels_metadata_rejected(oracle):
    """num_units*labels_per_unit == 0 must be rejected, not divide by zero
    (SIGFPE) in the difficulty computation."""
    from oracle import Proof, make_meta
    assert oracle.lib.oracle_proving_difficulty(26, 0) == 0
    meta = make_meta(bytes(32), bytes(32), bytes(32), 0, 64)
    p = Proof()
    p.num_indices = 8
    rc, _ = oracle.verify(p, meta, 2, 12, 8, 8, None, -1, bytes(32))
    assert rc == 3  # malformed


def test_num_units_bounds_enforced():
    """PostConfig.Min/MaxNumUnits validation (Validator.NumUnits,
    validation.go:239-249) happens before any GPU work."""
    cfg = gsm_amd.PostConfig(min_num_units=4, max_num_units=8)
    for bad in (2, 9):
        mgr = gsm_amd.PostSetupManager(
            bytes(32), bytes(32), cfg,
            gsm_amd.PostSetupOpts(num_units=bad, scrypt_n=2))
        with pytest.raises(gsm_amd.EngineError) as ei:
            mgr.prepare_initializer()
        assert ei.value.code == gsm_amd.api.Status.INVALID_ARGS


def test_roofline_traffic_record_contract():
    """bench.py's roofline.traffic rides from the committed PMC record
    (profiles/roofline_traffic.json); guard the fields it reads so a
    kernel change that forgets to re-measure fails fast here."""
    import json
    import os
    rec = json.load(open(os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "profiles", "roofline_traffic.json")))
    assert rec["kernel"] == "post_label_romix_kernel"
    assert rec["labels_per_launch"] > 0
    assert rec["traffic_bytes_per_launch"] == (
        rec["write_bytes_per_launch"] + rec["fetch_bytes_per_launch"])
    # counter-measured traffic must stay within ~5% of algorithmic bytes
    # (128*N*2 + 512 + 16 per label at N=8192) — "no wasted re-reads"
    algo = (128 * 8192 * 2 + 512 + 16) * rec["labels_per_launch"]
    assert abs(rec["traffic_bytes_per_launch"] - algo) / algo < 0.05
    assert "source" in rec and rec["source"].startswith("profiles/")
