"""ctypes bindings for libpost_hip.so + host-side mirrors of the reference's
Go interfaces.

Interface parity map (file:line under /root/reference/):
  PostSetupManager.{PrepareInitializer,StartSession,Status,Reset}
      -> activation/post.go:245,271,341,438
  PostConfig / PostSetupOpts fields -> activation/post.go:27-61
  PostVerifier.Verify(proof, metadata, opts) -> activation/interface.go:26-29,
      activation/post_verifier.go:150-160
  verify options Subset(k3, seed) / SelectedIndex
      -> activation/validation.go:206-209, activation/malfeasance.go:165
  proof shape {nonce, indices, pow} -> api/grpcserver/post_client.go:124-141
"""
from __future__ import annotations

import ctypes
import dataclasses
import enum
import os
import threading
from ctypes import (POINTER, byref, c_char_p, c_int, c_int32, c_size_t,
                    c_uint8, c_uint16, c_uint32, c_uint64, c_void_p)
from typing import Optional

from . import events as _ev
from . import metrics as _metrics

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("POST_ENGINE_LIB",
                           os.path.join(_DIR, "libpost_hip.so"))

LABEL_SIZE = 16
FULL_LABEL_SIZE = 32

POW_MODE_RANDOMX = 0
POW_MODE_BLAKE3 = 1


class Status(enum.IntEnum):
    OK = 0
    ERR = 1
    INVALID_ARGS = 2
    NO_GPU = 3
    OOM = 4
    IO = 5
    CANCELLED = 6
    POW = 7
    INVALID_INDEX = 8
    UNSUPPORTED = 9
    NO_NONCE = 10


class EngineError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = Status(code)
        super().__init__(f"{self.code.name}: {detail}")


class _CProvider(ctypes.Structure):
    _fields_ = [("id", c_uint32), ("model", ctypes.c_char * 256),
                ("device_type", c_uint32), ("memory_bytes", c_uint64),
                ("performance", c_uint64)]


class _CInitConfig(ctypes.Structure):
    _fields_ = [("node_id", c_uint8 * 32), ("commitment_atx_id", c_uint8 * 32),
                ("num_units", c_uint32), ("labels_per_unit", c_uint64),
                ("max_file_size", c_uint64), ("scrypt_n", c_uint32),
                ("provider_id", c_uint32), ("index_start", c_uint64),
                ("index_end", c_uint64), ("data_dir", c_char_p),
                ("scratch_bytes", c_uint64)]


class CProof(ctypes.Structure):
    _fields_ = [("nonce", c_uint32), ("pow", c_uint64),
                ("indices", c_uint8 * 800), ("indices_len", c_uint32),
                ("num_indices", c_uint16)]


class CProofMetadata(ctypes.Structure):
    _fields_ = [("node_id", c_uint8 * 32), ("commitment_atx_id", c_uint8 * 32),
                ("challenge", c_uint8 * 32), ("num_units", c_uint32),
                ("labels_per_unit", c_uint64)]


class _CProveConfig(ctypes.Structure):
    _fields_ = [("challenge", c_uint8 * 32), ("k1", c_uint32),
                ("k2", c_uint32), ("nonces", c_uint32),
                ("pow_difficulty", c_uint8 * 32), ("pow_mode", c_uint32),
                ("pow_threads", c_uint32), ("provider_id", c_uint32)]


class _CVerifyConfig(ctypes.Structure):
    _fields_ = [("k1", c_uint32), ("k2", c_uint32), ("k3", c_uint32),
                ("subset_seed", c_void_p), ("subset_seed_len", c_size_t),
                ("selected_index", c_int32),
                ("pow_difficulty", c_uint8 * 32), ("pow_mode", c_uint32),
                ("scrypt_n", c_uint32), ("provider_id", c_uint32)]


class _CAuditConfig(ctypes.Structure):
    _fields_ = [("provider_id", c_uint32), ("sample_every", c_uint64),
                ("seed", c_uint64), ("index_start", c_uint64),
                ("index_end", c_uint64), ("scratch_bytes", c_uint64),
                ("progress", c_void_p), ("user", c_void_p)]


class _CBadLabel(ctypes.Structure):
    _fields_ = [("index", c_uint64), ("on_disk", c_uint8 * 16),
                ("expected", c_uint8 * 16)]


class _CAuditReport(ctypes.Structure):
    _fields_ = [("labels_in_range", c_uint64), ("labels_sampled", c_uint64),
                ("labels_checked", c_uint64), ("labels_missing", c_uint64),
                ("labels_bad", c_uint64)]


class _CSealReport(ctypes.Structure):
    _fields_ = [("total_labels", c_uint64), ("pages", c_uint64),
                ("pages_bad", c_uint64),
                ("proof_touches_bad_page", c_uint32)]


class _CHealConfig(ctypes.Structure):
    _fields_ = [("max_pages", c_uint32), ("write_back", c_uint32),
                ("scratch_bytes", c_uint64)]


class _CHealReport(ctypes.Structure):
    _fields_ = [("total_labels", c_uint64), ("pages", c_uint64),
                ("pages_bad", c_uint64),
                ("proof_touches_bad_page", c_uint32),
                ("heal_skipped", c_uint32), ("pages_healed", c_uint64),
                ("pages_unconfirmed", c_uint64),
                ("labels_repaired", c_uint64), ("hits_dropped", c_uint64),
                ("hits_added", c_uint64), ("pages_written", c_uint64),
                ("proof_touches_unconfirmed_page", c_uint32),
                ("reserved", c_uint32)]


class _CInitProofReport(ctypes.Structure):
    _fields_ = [("total_labels", c_uint64), ("labels_covered", c_uint64),
                ("hits", c_uint64), ("parts", c_uint32),
                ("reserved", c_uint32)]


_AUDIT_PROGRESS = ctypes.CFUNCTYPE(c_int, c_void_p, c_uint64, c_uint64)

_lib_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None


def load_engine() -> ctypes.CDLL:
    """Load libpost_hip.so.  Raises loudly when the extension is missing —
    a GPU box must never silently run without the HIP engine."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise EngineError(
                Status.ERR,
                f"HIP engine not built: {_LIB_PATH} missing. "
                "Run `make` (or __graft_entry__.build()).")
        lib = ctypes.CDLL(_LIB_PATH)
        sigs = {
            "post_last_error": (c_char_p, []),
            "post_engine_version": (c_char_p, []),
            "post_providers": (c_int, [POINTER(_CProvider), c_uint32,
                                       POINTER(c_uint32)]),
            "post_benchmark": (c_int, [c_uint32, c_uint32,
                                       POINTER(c_uint64)]),
            "post_init_new": (c_int, [POINTER(_CInitConfig),
                                      POINTER(c_void_p)]),
            "post_init_run": (c_int, [c_void_p]),
            "post_init_step": (c_int, [c_void_p, c_uint64,
                                       POINTER(c_uint64)]),
            "post_init_last_kernel_ms": (ctypes.c_double, [c_void_p]),
            "post_init_num_labels_written": (c_uint64, [c_void_p]),
            "post_init_cancel": (None, [c_void_p]),
            "post_init_nonce": (c_int, [c_void_p, POINTER(c_uint64),
                                        ctypes.c_char_p]),
            "post_init_copy_labels": (c_int, [c_void_p, c_uint64, c_uint64,
                                              ctypes.c_char_p]),
            "post_init_free": (None, [c_void_p]),
            "post_prove": (c_int, [c_char_p, POINTER(_CProveConfig),
                                   POINTER(CProof)]),
            "post_prove_buffer": (c_int, [ctypes.c_char_p, c_uint64,
                                          ctypes.c_char_p, ctypes.c_char_p,
                                          POINTER(_CProveConfig),
                                          POINTER(CProof)]),
            "post_verify": (c_int, [POINTER(CProof), POINTER(CProofMetadata),
                                    POINTER(_CVerifyConfig),
                                    POINTER(c_uint32)]),
            "post_verify_batch": (c_int, [POINTER(CProof),
                                          POINTER(CProofMetadata), c_uint32,
                                          POINTER(_CVerifyConfig),
                                          POINTER(c_int), POINTER(c_uint32)]),
            "post_verify_batch_seeded": (c_int, [
                POINTER(CProof), POINTER(CProofMetadata), c_uint32,
                POINTER(_CVerifyConfig), ctypes.c_char_p, c_size_t,
                POINTER(c_int), POINTER(c_uint32)]),
            "post_verify_vrf_nonce": (c_int, [POINTER(CProofMetadata),
                                              c_uint64, c_uint32, c_uint32]),
            "post_verify_batch_vrf": (c_int, [
                POINTER(CProof), POINTER(CProofMetadata), c_uint32,
                POINTER(_CVerifyConfig), ctypes.c_char_p, c_size_t,
                POINTER(CProofMetadata), POINTER(c_uint64), c_uint32,
                POINTER(c_int), POINTER(c_uint32), POINTER(c_int)]),
            "post_verify_vrf_nonce_batch": (c_int, [
                POINTER(CProofMetadata), POINTER(c_uint64), c_uint32,
                c_uint32, c_uint32, POINTER(c_int)]),
            "post_verify_data_sample": (c_int, [
                c_uint64, c_uint64, c_uint64, c_uint64, c_uint64,
                POINTER(c_uint64), c_uint32, POINTER(c_uint32)]),
            "post_verify_data": (c_int, [c_char_p, POINTER(_CAuditConfig),
                                         POINTER(_CBadLabel), c_uint32,
                                         POINTER(_CAuditReport)]),
            "post_verify_data_buffer": (c_int, [
                ctypes.c_char_p, c_uint64, c_uint64, ctypes.c_char_p,
                ctypes.c_char_p, c_uint32, POINTER(_CAuditConfig),
                POINTER(_CBadLabel), c_uint32, POINTER(_CAuditReport)]),
            "post_seal_digest_buffer": (c_int, [
                ctypes.c_char_p, c_uint64, c_uint32, ctypes.c_char_p,
                c_uint64, POINTER(c_uint64)]),
            "post_seal_data": (c_int, [c_char_p, c_uint32,
                                       POINTER(_CSealReport)]),
            "post_init_enable_seal": (c_int, [c_void_p]),
            "post_seal_assemble": (c_int, [c_char_p, POINTER(c_uint64)]),
            "post_init_enable_proof": (c_int, [c_void_p,
                                               POINTER(_CProveConfig)]),
            "post_init_proof_assemble": (c_int, [
                c_char_p, POINTER(CProof), POINTER(_CInitProofReport)]),
            "post_seal_digest_stream": (c_int, [
                ctypes.c_char_p, c_uint64, c_uint64, POINTER(c_uint64),
                c_uint32, c_uint32, c_uint32, ctypes.c_char_p, c_uint64,
                POINTER(c_uint64)]),
            "post_check_seal": (c_int, [c_char_p, c_uint32,
                                        POINTER(c_uint64), c_uint32,
                                        POINTER(_CSealReport)]),
            "post_prove_checked": (c_int, [
                c_char_p, POINTER(_CProveConfig), POINTER(CProof),
                POINTER(c_uint64), c_uint32, POINTER(_CSealReport)]),
            "post_prove_healed": (c_int, [
                c_char_p, POINTER(_CProveConfig), POINTER(_CHealConfig),
                POINTER(CProof), POINTER(c_uint64), c_uint32,
                POINTER(_CHealReport)]),
            "post_repair_data": (c_int, [
                c_char_p, c_uint32, POINTER(_CHealConfig),
                POINTER(c_uint64), c_uint32, POINTER(_CHealReport)]),
            "post_selftest_blake3": (None, [ctypes.c_char_p, c_size_t,
                                            ctypes.c_char_p]),
            "post_selftest_aes128": (None, [ctypes.c_char_p, ctypes.c_char_p,
                                            ctypes.c_char_p]),
            "post_selftest_label": (c_int, [ctypes.c_char_p, ctypes.c_char_p,
                                            c_uint64, c_uint32,
                                            ctypes.c_char_p]),
            "post_selftest_verify_pred": (c_int, [
                ctypes.c_char_p, c_uint64, ctypes.c_char_p, ctypes.c_char_p,
                POINTER(c_uint64), c_uint32, POINTER(c_uint32), c_uint32,
                c_uint32, ctypes.c_char_p]),
            "post_selftest_vrf_pred": (c_int, [
                ctypes.c_char_p, c_uint64, ctypes.c_char_p, c_uint32,
                POINTER(c_uint32), c_uint32, c_uint32, ctypes.c_char_p]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


# ------------------------- config dataclasses -------------------------

@dataclasses.dataclass
class PostConfig:
    """Mirror of activation/post.go:27-49 PostConfig (protocol params)."""
    min_num_units: int = 4
    max_num_units: int = 2**32 - 1
    labels_per_unit: int = 4294967296   # config/mainnet.go:186
    k1: int = 26                        # config/mainnet.go:187
    k2: int = 37
    k3: int = 1
    pow_difficulty: bytes = bytes.fromhex(
        "000dfb23b0979b4b000000000000000000000000000000000000000000000000")
    pow_mode: int = POW_MODE_BLAKE3


@dataclasses.dataclass
class InitialProofOpts:
    """The initial proof found during init: the proving
    parameters of ProveOpts together with those of PostConfig that a proof
    needs, since they must be known when the session is created.  The
    challenge is shared.ZeroChallenge unless a caller knows better."""
    k1: int = 26
    k2: int = 37
    pow_difficulty: bytes = PostConfig.pow_difficulty
    pow_mode: int = POW_MODE_BLAKE3
    nonces: int = 288
    threads: int = 0
    challenge: bytes = bytes(32)

    @classmethod
    def of(cls, cfg: "PostConfig", opts: "Optional[ProveOpts]" = None,
           challenge: bytes = bytes(32)) -> "InitialProofOpts":
        opts = opts or ProveOpts()
        return cls(k1=cfg.k1, k2=cfg.k2, pow_difficulty=cfg.pow_difficulty,
                   pow_mode=cfg.pow_mode, nonces=opts.nonces,
                   threads=opts.threads, challenge=challenge)

    def to_c(self) -> _CProveConfig:
        pc = _CProveConfig()
        ctypes.memmove(pc.challenge, self.challenge, 32)
        pc.k1, pc.k2, pc.nonces = self.k1, self.k2, self.nonces
        ctypes.memmove(pc.pow_difficulty, self.pow_difficulty, 32)
        pc.pow_mode = self.pow_mode
        pc.pow_threads = self.threads
        return pc


@dataclasses.dataclass
class PostSetupOpts:
    """Mirror of activation/post.go:52-61 PostSetupOpts."""
    data_dir: Optional[str] = None
    num_units: int = 4
    max_file_size: int = 4294967296
    provider_id: int = 0
    scrypt_n: int = 8192                # activation/post.go:155 dep default
    index_start: int = 0                # shard range
    index_end: int = 0
    scratch_bytes: int = 0
    # scan for the initial proof during init
    initial_proof: Optional[InitialProofOpts] = None
    seal: bool = False                  # seal during init


@dataclasses.dataclass
class ProveOpts:
    """Mirror of PostProvingOpts (activation/post.go:64-74)."""
    nonces: int = 288                   # config/mainnet.go:61
    threads: int = 0
    provider_id: int = 0


@dataclasses.dataclass
class VerifyOpts:
    """verifying options (validation.go:206-209, malfeasance.go:165)."""
    subset_seed: Optional[bytes] = None
    selected_index: int = -1
    provider_id: int = 0


@dataclasses.dataclass
class AuditOpts:
    """Postdata audit (verify-data): one label per window of `sample_every`
    labels is recomputed and compared with the bytes on disk."""
    sample_every: int = 100             # 1 % of the labels
    seed: int = 0
    index_start: int = 0                # 0,0 = the whole space / buffer
    index_end: int = 0
    provider_id: int = 0
    scratch_bytes: int = 0
    max_report: int = 64                # mismatches returned in detail


@dataclasses.dataclass
class AuditReport:
    labels_in_range: int
    labels_sampled: int
    labels_checked: int
    labels_missing: int
    labels_bad: int                     # the full count, whatever max_report
    # (index, on_disk, expected) of the max_report smallest bad indices
    bad: list = dataclasses.field(default_factory=list)

    @property
    def clean(self) -> bool:
        return self.labels_bad == 0 and self.labels_missing == 0


@dataclasses.dataclass
class PostProof:
    nonce: int
    indices: bytes
    pow: int

    def to_c(self) -> CProof:
        c = CProof()
        c.nonce = self.nonce
        c.pow = self.pow
        c.indices_len = len(self.indices)
        c.num_indices = 0  # set by callers that know k2
        ctypes.memmove(c.indices, self.indices, len(self.indices))
        return c


@dataclasses.dataclass
class PostProofMetadata:
    """shared.ProofMetadata (validation.go:193-199)."""
    node_id: bytes
    commitment_atx_id: bytes
    challenge: bytes
    num_units: int
    labels_per_unit: int

    def to_c(self) -> CProofMetadata:
        return CProofMetadata(
            (c_uint8 * 32)(*self.node_id),
            (c_uint8 * 32)(*self.commitment_atx_id),
            (c_uint8 * 32)(*self.challenge),
            self.num_units, self.labels_per_unit)


class Engine:
    """Thin OO wrapper over the C-ABI."""

    def __init__(self) -> None:
        self.lib = load_engine()

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise EngineError(rc, self.lib.post_last_error().decode())

    def version(self) -> str:
        return self.lib.post_engine_version().decode()

    def providers(self):
        arr = (_CProvider * 16)()
        count = c_uint32(0)
        self._check(self.lib.post_providers(arr, 16, byref(count)))
        return [{"id": arr[i].id, "model": arr[i].model.decode(),
                 "device_type": arr[i].device_type,
                 "memory_bytes": arr[i].memory_bytes}
                for i in range(min(count.value, 16))]

    def benchmark(self, provider_id: int = 0, scrypt_n: int = 8192) -> int:
        out = c_uint64(0)
        self._check(self.lib.post_benchmark(provider_id, scrypt_n,
                                            byref(out)))
        return out.value

    # self-test hooks (used by tests to cross-check vs the oracle)
    def selftest_blake3(self, msg: bytes) -> bytes:
        out = ctypes.create_string_buffer(32)
        self.lib.post_selftest_blake3(msg, len(msg), out)
        return out.raw

    def selftest_aes128(self, key: bytes, block: bytes) -> bytes:
        out = ctypes.create_string_buffer(16)
        self.lib.post_selftest_aes128(key, block, out)
        return out.raw

    def selftest_label(self, node_id: bytes, atx_id: bytes, index: int,
                       scrypt_n: int) -> bytes:
        out = ctypes.create_string_buffer(32)
        rc = self.lib.post_selftest_label(node_id, atx_id, index, scrypt_n,
                                          out)
        self._check(rc)
        return out.raw

    def selftest_verify_pred(self, labels: bytes, keys, halves, difficulties,
                             task_proof, max_blocks: int = 0,
                             provider_id: int = 0) -> bytes:
        """Verification's device predicate over caller-made full labels:
        one pass byte per task.  keys/halves/difficulties are per proof,
        task_proof maps each 32-byte label to its proof."""
        count, n = len(labels) // FULL_LABEL_SIZE, len(keys)
        assert len(labels) == count * FULL_LABEL_SIZE
        assert len(halves) == n and len(difficulties) == n
        assert len(task_proof) == count
        out = ctypes.create_string_buffer(max(count, 1))
        rc = self.lib.post_selftest_verify_pred(
            labels, count, b"".join(keys), bytes(halves),
            (c_uint64 * n)(*difficulties), n,
            (c_uint32 * count)(*task_proof), max_blocks, provider_id, out)
        self._check(rc)
        return out.raw[:count]

    def selftest_vrf_pred(self, labels: bytes, thresholds, task_thr,
                          max_blocks: int = 0, provider_id: int = 0) -> bytes:
        """The VRF-nonce device predicate over caller-made full labels: one
        pass byte per task.  thresholds are 32-byte big-endian values,
        task_thr maps each 32-byte label to its threshold."""
        count, n = len(labels) // FULL_LABEL_SIZE, len(thresholds)
        assert len(labels) == count * FULL_LABEL_SIZE
        assert all(len(t) == FULL_LABEL_SIZE for t in thresholds)
        assert len(task_thr) == count
        out = ctypes.create_string_buffer(max(count, 1))
        rc = self.lib.post_selftest_vrf_pred(
            labels, count, b"".join(thresholds), n,
            (c_uint32 * count)(*task_thr), max_blocks, provider_id, out)
        self._check(rc)
        return out.raw[:count]


class PostSetupManager:
    """Mirror of activation/post.go PostSetupManager: PrepareInitializer /
    StartSession (blocking; resumable) / Status / Reset."""

    NOT_STARTED, PREPARED, IN_PROGRESS, STOPPED, COMPLETE, ERROR = range(1, 7)

    def __init__(self, node_id: bytes, commitment_atx_id: bytes,
                 cfg: PostConfig, opts: PostSetupOpts) -> None:
        self.engine = Engine()
        self.node_id = node_id
        self.commitment_atx_id = commitment_atx_id
        self.cfg = cfg
        self.opts = opts
        self.state = self.NOT_STARTED
        self._session: Optional[c_void_p] = None

    def prepare_initializer(self) -> None:
        if self.state == self.PREPARED:
            raise EngineError(Status.ERR, "already prepared")
        if self.opts.num_units < self.cfg.min_num_units or \
                self.opts.num_units > self.cfg.max_num_units:
            raise EngineError(Status.INVALID_ARGS, "numUnits out of range")
        c = _CInitConfig()
        ctypes.memmove(c.node_id, self.node_id, 32)
        ctypes.memmove(c.commitment_atx_id, self.commitment_atx_id, 32)
        c.num_units = self.opts.num_units
        c.labels_per_unit = self.cfg.labels_per_unit
        c.max_file_size = self.opts.max_file_size
        c.scrypt_n = self.opts.scrypt_n
        c.provider_id = self.opts.provider_id
        c.index_start = self.opts.index_start
        c.index_end = self.opts.index_end
        c.data_dir = self.opts.data_dir.encode() if self.opts.data_dir \
            else None
        c.scratch_bytes = self.opts.scratch_bytes
        handle = c_void_p()
        self.engine._check(self.engine.lib.post_init_new(byref(c),
                                                         byref(handle)))
        self._session = handle
        if self.opts.seal:
            rc = self.engine.lib.post_init_enable_seal(handle)
            if rc != 0:
                err = self.engine.lib.post_last_error().decode()
                self.reset()
                raise EngineError(rc, err)
        if self.opts.initial_proof is not None:
            pc = self.opts.initial_proof.to_c()
            rc = self.engine.lib.post_init_enable_proof(handle, byref(pc))
            if rc != 0:
                err = self.engine.lib.post_last_error().decode()
                self.reset()
                raise EngineError(rc, err)
        self.state = self.PREPARED

    def start_session(self) -> None:
        if self.state != self.PREPARED:
            raise EngineError(Status.ERR, "post session not prepared")
        self.state = self.IN_PROGRESS
        _ev.bus().emit(_ev.InitStart(self.node_id, self.commitment_atx_id))
        _metrics.init_size.labels(step="start").set(self.opts.num_units)
        rc = self.engine.lib.post_init_run(self._session)
        if rc == Status.CANCELLED:
            self.state = self.STOPPED
            raise EngineError(rc, "stopped")
        if rc != 0:
            self.state = self.ERROR
            err = self.engine.lib.post_last_error().decode()
            _ev.bus().emit(_ev.InitFailure(self.node_id, err))
            raise EngineError(rc, err)
        self.state = self.COMPLETE
        _metrics.init_size.labels(step="complete").set(self.opts.num_units)
        _ev.bus().emit(_ev.InitComplete(self.node_id))

    def step(self, max_labels: int) -> tuple:
        """Process up to max_labels labels; returns (labels_done,
        kernel_ms).  One bench step of the init hot path."""
        done = c_uint64(0)
        rc = self.engine.lib.post_init_step(self._session, max_labels,
                                            byref(done))
        self.engine._check(rc)
        kms = self.engine.lib.post_init_last_kernel_ms(self._session)
        return done.value, kms

    def status(self):
        written = 0
        if self._session:
            written = self.engine.lib.post_init_num_labels_written(
                self._session)
        return {"state": self.state, "num_labels_written": written}

    def stop(self) -> None:
        if self._session:
            self.engine.lib.post_init_cancel(self._session)

    def vrf_nonce(self):
        idx = c_uint64(0)
        label = ctypes.create_string_buffer(32)
        rc = self.engine.lib.post_init_nonce(self._session, byref(idx), label)
        if rc != 0:
            return None
        return idx.value, label.raw

    def copy_labels(self, first: int, count: int) -> bytes:
        buf = ctypes.create_string_buffer(count * LABEL_SIZE)
        self.engine._check(self.engine.lib.post_init_copy_labels(
            self._session, first, count, buf))
        return buf.raw

    def reset(self) -> None:
        if self._session:
            self.engine.lib.post_init_free(self._session)
            self._session = None
        self.state = self.NOT_STARTED

    def __del__(self):
        try:
            self.reset()
        except Exception:
            pass


def prove_buffer(labels: bytes, num_labels: int, node_id: bytes,
                 atx_id: bytes, challenge: bytes, cfg: PostConfig,
                 opts: ProveOpts) -> PostProof:
    import time as _time
    _ev.bus().emit(_ev.PostStart(node_id, challenge))
    t0 = _time.monotonic()
    try:
        return _prove_buffer(labels, num_labels, node_id, atx_id, challenge,
                             cfg, opts)
    finally:
        dt = _time.monotonic() - t0
        _metrics.post_seconds.set(dt)          # smh_post_seconds
        _metrics.post_duration.set(dt * 1e9)   # activation_post_duration
        _ev.bus().emit(_ev.PostComplete(node_id))


def _prove_buffer(labels: bytes, num_labels: int, node_id: bytes,
                  atx_id: bytes, challenge: bytes, cfg: PostConfig,
                  opts: ProveOpts) -> PostProof:
    eng = Engine()
    pc = _CProveConfig()
    ctypes.memmove(pc.challenge, challenge, 32)
    pc.k1, pc.k2 = cfg.k1, cfg.k2
    pc.nonces = opts.nonces
    ctypes.memmove(pc.pow_difficulty, cfg.pow_difficulty, 32)
    pc.pow_mode = cfg.pow_mode
    pc.pow_threads = opts.threads
    pc.provider_id = opts.provider_id
    out = CProof()
    eng._check(eng.lib.post_prove_buffer(labels, num_labels, node_id, atx_id,
                                         byref(pc), byref(out)))
    return PostProof(nonce=out.nonce,
                     indices=bytes(out.indices[:out.indices_len]),
                     pow=out.pow)


def prove_dir(data_dir: str, challenge: bytes, cfg: PostConfig,
              opts: ProveOpts) -> PostProof:
    eng = Engine()
    pc = _CProveConfig()
    ctypes.memmove(pc.challenge, challenge, 32)
    pc.k1, pc.k2 = cfg.k1, cfg.k2
    pc.nonces = opts.nonces
    ctypes.memmove(pc.pow_difficulty, cfg.pow_difficulty, 32)
    pc.pow_mode = cfg.pow_mode
    pc.pow_threads = opts.threads
    pc.provider_id = opts.provider_id
    out = CProof()
    eng._check(eng.lib.post_prove(data_dir.encode(), byref(pc), byref(out)))
    return PostProof(nonce=out.nonce,
                     indices=bytes(out.indices[:out.indices_len]),
                     pow=out.pow)


# ------------------------- postdata seal -------------------------

@dataclasses.dataclass
class SealReport:
    """Result of seal_data / check_seal / prove_checked."""
    total_labels: int
    pages: int
    pages_bad: int                      # the full count, whatever max_report
    proof_touches_bad_page: bool = False    # prove_checked only
    # the max_report smallest bad page numbers, ascending
    bad_pages: list = dataclasses.field(default_factory=list)

    @property
    def clean(self) -> bool:
        return self.pages_bad == 0

    def bad_label_ranges(self) -> list:
        """[from, to) label ranges of bad_pages, as verify-data takes them."""
        return [(p * 1024, min((p + 1) * 1024, self.total_labels))
                for p in self.bad_pages]


def _seal_report(rep: _CSealReport, bad, cap: int) -> SealReport:
    return SealReport(rep.total_labels, rep.pages, rep.pages_bad,
                      bool(rep.proof_touches_bad_page),
                      [bad[i] for i in range(min(cap, rep.pages_bad))])


def seal_digest_buffer(labels: bytes, provider_id: int = 0) -> bytes:
    """GPU page digests of a buffer of 16-byte labels, back to back."""
    eng = Engine()
    count = len(labels) // LABEL_SIZE
    cap = -(-count // 1024)
    out = ctypes.create_string_buffer(max(1, cap * 16))
    n = c_uint64(0)
    eng._check(eng.lib.post_seal_digest_buffer(labels, count, provider_id,
                                               out, cap, byref(n)))
    return out.raw[:n.value * 16]


def seal_digest_stream(labels: bytes, first_index: int = 0, cuts=(),
                       stream_end: bool = True,
                       provider_id: int = 0) -> bytes:
    """Page digests of a label stream that starts at first_index (a
    multiple of 1024) and reaches the GPU cut into segments at `cuts`
    (positions within the buffer), as init batches do.  With
    stream_end the buffer's end closes a ragged last page."""
    eng = Engine()
    count = len(labels) // LABEL_SIZE
    pages = -(-count // 1024)
    out = ctypes.create_string_buffer(max(1, pages) * 16)
    n = c_uint64(0)
    cuts = list(cuts)
    arr = (c_uint64 * max(1, len(cuts)))(*cuts)
    eng._check(eng.lib.post_seal_digest_stream(
        labels, count, first_index, arr, len(cuts), 1 if stream_end else 0,
        provider_id, out, pages, byref(n)))
    return out.raw[:n.value * 16]


def seal_assemble(data_dir: str) -> int:
    """Put the part files of a sealed init together into postdata_seal.bin
    (host only); returns the page count.  EngineError(IO) names the first
    missing page range while a shard is unfinished."""
    eng = Engine()
    pages = c_uint64(0)
    eng._check(eng.lib.post_seal_assemble(data_dir.encode(), byref(pages)))
    return pages.value


@dataclasses.dataclass
class InitProofReport:
    """What init_proof_assemble merged."""
    total_labels: int
    labels_covered: int
    hits: int
    parts: int


def init_proof_assemble(data_dir: str) -> tuple:
    """The initial proof of a dir whose init ran with the scan on, from its
    postdata_hits.part-* files: (proof, report).  Host only, reads only.
    EngineError(IO) names the first missing index range while a shard is
    unfinished; EngineError(NO_NONCE) when no nonce reaches K2."""
    eng = Engine()
    out = CProof()
    rep = _CInitProofReport()
    eng._check(eng.lib.post_init_proof_assemble(data_dir.encode(), byref(out),
                                                byref(rep)))
    proof = PostProof(nonce=out.nonce,
                      indices=bytes(out.indices[:out.indices_len]),
                      pow=out.pow)
    return proof, InitProofReport(rep.total_labels, rep.labels_covered,
                                  rep.hits, rep.parts)


def seal_data(data_dir: str, provider_id: int = 0) -> SealReport:
    """Write postdata_seal.bin for the dir's current labels."""
    eng = Engine()
    rep = _CSealReport()
    eng._check(eng.lib.post_seal_data(data_dir.encode(), provider_id,
                                      byref(rep)))
    return _seal_report(rep, None, 0)


def check_seal(data_dir: str, provider_id: int = 0,
               max_report: int = 64) -> SealReport:
    """Compare the dir's labels with its seal.  Corruption is reported
    through the SealReport, not raised."""
    eng = Engine()
    cap = max(0, max_report)
    bad = (c_uint64 * cap)() if cap else None
    rep = _CSealReport()
    eng._check(eng.lib.post_check_seal(data_dir.encode(), provider_id, bad,
                                       cap, byref(rep)))
    return _seal_report(rep, bad, cap)


def prove_checked(data_dir: str, challenge: bytes, cfg: PostConfig,
                  opts: ProveOpts, max_report: int = 64) -> tuple:
    """prove_dir with the seal checked in the same pass: (proof, report).
    A proof whose report has proof_touches_bad_page set must not be
    published."""
    eng = Engine()
    pc = _CProveConfig()
    ctypes.memmove(pc.challenge, challenge, 32)
    pc.k1, pc.k2 = cfg.k1, cfg.k2
    pc.nonces = opts.nonces
    ctypes.memmove(pc.pow_difficulty, cfg.pow_difficulty, 32)
    pc.pow_mode = cfg.pow_mode
    pc.pow_threads = opts.threads
    pc.provider_id = opts.provider_id
    out = CProof()
    cap = max(0, max_report)
    bad = (c_uint64 * cap)() if cap else None
    rep = _CSealReport()
    eng._check(eng.lib.post_prove_checked(data_dir.encode(), byref(pc),
                                          byref(out), bad, cap, byref(rep)))
    proof = PostProof(nonce=out.nonce,
                      indices=bytes(out.indices[:out.indices_len]),
                      pow=out.pow)
    return proof, _seal_report(rep, bad, cap)


# ------------------------- self-healing prove -------------------------

@dataclasses.dataclass
class HealOpts:
    """Healing of the pages the seal pass finds bad."""
    max_pages: int = 0                  # 0 = the engine's default, 4096
    write_back: bool = False            # write confirmed pages to the files
    scratch_bytes: int = 0


@dataclasses.dataclass
class HealReport(SealReport):
    """Result of prove_healed / repair_data.  pages_bad and bad_pages are
    what the pass found on disk."""
    heal_skipped: bool = False          # more bad pages than max_pages
    pages_healed: int = 0               # recomputed: confirmed or not
    pages_unconfirmed: int = 0          # recomputation and seal disagree
    labels_repaired: int = 0            # disk bytes != recomputation
    hits_dropped: int = 0
    hits_added: int = 0
    pages_written: int = 0
    proof_touches_unconfirmed_page: bool = False

    @property
    def publishable(self) -> bool:
        """The proof stands on labels that are sealed-and-intact or
        recomputed-and-confirmed."""
        return not self.heal_skipped \
            and not self.proof_touches_bad_page \
            and not self.proof_touches_unconfirmed_page

    @property
    def repaired(self) -> bool:
        """A following check_seal would be clean."""
        return self.pages_written == self.pages_bad


def _heal_config(heal: Optional[HealOpts]) -> _CHealConfig:
    heal = heal or HealOpts()
    return _CHealConfig(heal.max_pages, 1 if heal.write_back else 0,
                        heal.scratch_bytes)


def _heal_report(rep: _CHealReport, bad, cap: int) -> HealReport:
    return HealReport(
        rep.total_labels, rep.pages, rep.pages_bad,
        bool(rep.proof_touches_bad_page),
        [bad[i] for i in range(min(cap, rep.pages_bad))],
        bool(rep.heal_skipped), rep.pages_healed, rep.pages_unconfirmed,
        rep.labels_repaired, rep.hits_dropped, rep.hits_added,
        rep.pages_written, bool(rep.proof_touches_unconfirmed_page))


def prove_healed(data_dir: str, challenge: bytes, cfg: PostConfig,
                 opts: ProveOpts, heal: Optional[HealOpts] = None,
                 max_report: int = 64) -> tuple:
    """prove_checked that puts right what it finds: bad pages are recomputed
    on the GPU, their hits replaced, and (heal.write_back) confirmed pages
    written over the file bytes: (proof, HealReport).  Publish the proof
    only when report.publishable."""
    eng = Engine()
    pc = _CProveConfig()
    ctypes.memmove(pc.challenge, challenge, 32)
    pc.k1, pc.k2 = cfg.k1, cfg.k2
    pc.nonces = opts.nonces
    ctypes.memmove(pc.pow_difficulty, cfg.pow_difficulty, 32)
    pc.pow_mode = cfg.pow_mode
    pc.pow_threads = opts.threads
    pc.provider_id = opts.provider_id
    hc = _heal_config(heal)
    out = CProof()
    cap = max(0, max_report)
    bad = (c_uint64 * cap)() if cap else None
    rep = _CHealReport()
    eng._check(eng.lib.post_prove_healed(data_dir.encode(), byref(pc),
                                         byref(hc), byref(out), bad, cap,
                                         byref(rep)))
    proof = PostProof(nonce=out.nonce,
                      indices=bytes(out.indices[:out.indices_len]),
                      pow=out.pow)
    return proof, _heal_report(rep, bad, cap)


def repair_data(data_dir: str, heal: Optional[HealOpts] = None,
                provider_id: int = 0, max_report: int = 64) -> HealReport:
    """The check-seal pass that recomputes the bad pages and writes the
    confirmed ones back; no proof.  report.repaired says whether a
    following check_seal would be clean."""
    eng = Engine()
    hc = _heal_config(heal)
    cap = max(0, max_report)
    bad = (c_uint64 * cap)() if cap else None
    rep = _CHealReport()
    eng._check(eng.lib.post_repair_data(data_dir.encode(), provider_id,
                                        byref(hc), bad, cap, byref(rep)))
    return _heal_report(rep, bad, cap)


class PostVerifier:
    """Mirror of the reference PostVerifier (interface.go:26-29): the inner
    verifier the Go worker pool wraps (post_verifier.go:150-160).  Safe for
    concurrent use."""

    def __init__(self, cfg: PostConfig, scrypt_n: int = 8192) -> None:
        self.engine = Engine()
        self.cfg = cfg
        self.scrypt_n = scrypt_n

    def _vc(self, opts: VerifyOpts) -> tuple:
        vc = _CVerifyConfig()
        vc.k1, vc.k2, vc.k3 = self.cfg.k1, self.cfg.k2, self.cfg.k3
        seed_buf = None
        if opts.subset_seed is not None:
            seed_buf = ctypes.create_string_buffer(opts.subset_seed,
                                                   len(opts.subset_seed))
            vc.subset_seed = ctypes.cast(seed_buf, c_void_p)
            vc.subset_seed_len = len(opts.subset_seed)
        vc.selected_index = opts.selected_index
        ctypes.memmove(vc.pow_difficulty, self.cfg.pow_difficulty, 32)
        vc.pow_mode = self.cfg.pow_mode
        vc.scrypt_n = self.scrypt_n
        vc.provider_id = opts.provider_id
        return vc, seed_buf

    def verify(self, proof: PostProof, meta: PostProofMetadata,
               opts: VerifyOpts = VerifyOpts()) -> None:
        """Raises EngineError(INVALID_INDEX/POW/...) on invalid proofs."""
        vc, _seed = self._vc(opts)
        cp = proof.to_c()
        cp.num_indices = self.cfg.k2
        inv = c_uint32(0)
        rc = self.engine.lib.post_verify(byref(cp), byref(meta.to_c()),
                                         byref(vc), byref(inv))
        if rc == Status.INVALID_INDEX:
            raise EngineError(rc, f"invalid POST index at position "
                                  f"{inv.value}")
        self.engine._check(rc)

    def marshal_batch(self, proofs, metas):
        """Pre-build the C argument arrays for verify_batch.  A cgo shim
        holds these layouts natively; the ctypes conversion is a
        Python-mirror cost only, so callers that re-verify (or benchmark
        the ABI boundary) can marshal once and pass the result to
        verify_batch as `marshalled=`."""
        n = len(proofs)
        cps = (CProof * n)()
        cms = (CProofMetadata * n)()
        for i, (p, m) in enumerate(zip(proofs, metas)):
            cps[i] = p.to_c()
            cps[i].num_indices = self.cfg.k2
            cms[i] = m.to_c()
        return cps, cms, n

    @staticmethod
    def marshal_vrf(metas, indices):
        """The C argument arrays of the VRF items of verify_batch(vrf=) and
        verify_vrf_nonce_batch; pass the result in place of (metas,
        indices) to marshal once."""
        n = len(metas)
        assert len(indices) == n
        cms = (CProofMetadata * n)()
        for i, m in enumerate(metas):
            cms[i] = m.to_c()
        return cms, (c_uint64 * n)(*indices), n

    @staticmethod
    def _vrf_args(vrf):
        if len(vrf) == 3:
            return vrf
        return PostVerifier.marshal_vrf(*vrf)

    def verify_batch(self, proofs, metas, opts: VerifyOpts = VerifyOpts(),
                     seeds=None, marshalled=None, vrf=None):
        # seeds (optional): equal-length per-proof subset seeds — each
        # gossip verify samples with its own peer seed
        # (validation.go:206-209).
        # vrf (optional): (metas, indices) of VRF-nonce checks that share
        # the label launch of the proofs; the return value is then
        # (proof results, [Status per VRF item]).  proofs may be empty.
        vc, _seed = self._vc(opts)
        cps, cms, n = (marshalled if marshalled is not None
                       else self.marshal_batch(proofs, metas))
        statuses = (c_int * n)()
        invs = (c_uint32 * n)()
        if vrf is not None:
            vms, vidx, nv = self._vrf_args(vrf)
            blob, slen = None, 0
            if seeds is not None:
                assert len(seeds) == n
                slen = len(seeds[0]) if n else 0
                assert all(len(x) == slen for x in seeds)
                blob = b"".join(seeds) if n else None
            vst = (c_int * nv)()
            self.engine._check(self.engine.lib.post_verify_batch_vrf(
                cps, cms, n, byref(vc), blob, slen, vms, vidx, nv,
                statuses, invs, vst))
            return ([(Status(statuses[i]), invs[i]) for i in range(n)],
                    [Status(vst[j]) for j in range(nv)])
        if seeds is not None:
            assert len(seeds) == n and n > 0
            slen = len(seeds[0])
            assert all(len(x) == slen for x in seeds)
            blob = b"".join(seeds)
            self.engine._check(self.engine.lib.post_verify_batch_seeded(
                cps, cms, n, byref(vc), blob, slen, statuses, invs))
        else:
            self.engine._check(self.engine.lib.post_verify_batch(
                cps, cms, n, byref(vc), statuses, invs))
        return [(Status(statuses[i]), invs[i]) for i in range(n)]

    def verify_vrf_nonce(self, meta: PostProofMetadata, index: int,
                         provider_id: int = 0) -> None:
        rc = self.engine.lib.post_verify_vrf_nonce(byref(meta.to_c()), index,
                                                   self.scrypt_n, provider_id)
        self.engine._check(rc)

    def verify_vrf_nonce_batch(self, metas, indices,
                               provider_id: int = 0) -> list:
        """One Status per (meta, index): OK, INVALID_INDEX (the label is
        not below the threshold) or INVALID_ARGS (num_labels == 0), from one
        label launch.  Nothing is raised for a failing item."""
        vms, vidx, nv = self.marshal_vrf(metas, indices)
        return self.verify_vrf_nonce_batch_marshalled((vms, vidx, nv),
                                                      provider_id)

    def verify_vrf_nonce_batch_marshalled(self, marshalled,
                                          provider_id: int = 0) -> list:
        vms, vidx, nv = marshalled
        vst = (c_int * nv)()
        self.engine._check(self.engine.lib.post_verify_vrf_nonce_batch(
            vms, vidx, nv, self.scrypt_n, provider_id, vst))
        return [Status(vst[j]) for j in range(nv)]


# ------------------------- postdata audit -------------------------

def sample_indices(seed: int, sample_every: int, index_start: int,
                   index_end: int, first_window: int = 0,
                   max_count: Optional[int] = None) -> list:
    """The audit's sampled indices (host-only, needs no GPU): one per window
    of `sample_every` labels of [index_start, index_end), starting at window
    `first_window`, at most `max_count` of them (default: to the end)."""
    eng = Engine()
    mask = (1 << 64) - 1
    out = []
    left = max_count
    while left is None or left > 0:
        page = 1 << 16 if left is None else min(left, 1 << 16)
        buf = (c_uint64 * page)()
        n = c_uint32(0)
        eng._check(eng.lib.post_verify_data_sample(
            seed & mask, sample_every, index_start, index_end,
            first_window + len(out), buf, page, byref(n)))
        out.extend(buf[:n.value])
        if n.value < page:
            break
        if left is not None:
            left -= n.value
    return out


def _audit_call(opts: Optional[AuditOpts], progress, call) -> AuditReport:
    eng = Engine()
    if opts is None:
        opts = AuditOpts()
    ac = _CAuditConfig()
    ac.provider_id = opts.provider_id
    ac.sample_every = opts.sample_every
    ac.seed = opts.seed & ((1 << 64) - 1)
    ac.index_start = opts.index_start
    ac.index_end = opts.index_end
    ac.scratch_bytes = opts.scratch_bytes
    cb = None
    raised = []
    if progress is not None:
        # a truthy return from progress(checked, to_check) stops the audit;
        # so does an exception, which is re-raised once the engine returns
        def trampoline(_user, checked, to_check):
            try:
                return 1 if progress(checked, to_check) else 0
            except BaseException as e:  # noqa: BLE001
                raised.append(e)
                return 1
        cb = _AUDIT_PROGRESS(trampoline)
        ac.progress = ctypes.cast(cb, c_void_p)
    cap = max(0, opts.max_report)
    bad = (_CBadLabel * cap)() if cap else None
    rep = _CAuditReport()
    rc = call(eng.lib, byref(ac), bad, cap, byref(rep))
    if raised:
        raise raised[0]
    eng._check(rc)
    found = [(bad[i].index, bytes(bad[i].on_disk), bytes(bad[i].expected))
             for i in range(min(cap, rep.labels_bad))]
    return AuditReport(rep.labels_in_range, rep.labels_sampled,
                       rep.labels_checked, rep.labels_missing,
                       rep.labels_bad, found)


def verify_data(data_dir: str, opts: Optional[AuditOpts] = None,
                progress=None) -> AuditReport:
    """Audit the labels of a postdata directory against its own metadata.
    Corruption is reported through the AuditReport, not raised."""
    return _audit_call(
        opts, progress,
        lambda lib, ac, bad, cap, rep: lib.post_verify_data(
            data_dir.encode(), ac, bad, cap, rep))


def verify_data_buffer(labels: bytes, index_base: int, node_id: bytes,
                       atx_id: bytes, scrypt_n: int,
                       opts: Optional[AuditOpts] = None,
                       progress=None) -> AuditReport:
    """Audit a host buffer holding labels [index_base, index_base + n)."""
    return _audit_call(
        opts, progress,
        lambda lib, ac, bad, cap, rep: lib.post_verify_data_buffer(
            labels, len(labels) // LABEL_SIZE, index_base, node_id, atx_id,
            scrypt_n, ac, bad, cap, rep))
