/* kernel_args.h — argument blocks shared between engine.cpp (host) and
 * kernels.hip (device).  Kept POD; pointers are device pointers. */
#ifndef POST_KERNEL_ARGS_H
#define POST_KERNEL_ARGS_H

#include <hip/hip_runtime.h>

#include "post_common.h"

struct LabelKernelArgs {
  uint32_t commitment_le[8];
  uint64_t start;
  uint64_t count;
  uint32_t scrypt_n;
  uint32_t gap_shift; /* lookup-gap = 1<<gap_shift: store every gap-th ROMix
                         block, recompute the rest on read (SURVEY §7 step 3
                         HBM-traffic/VALU trade; scratch = N>>gap_shift
                         blocks per lane) */
  uint32_t out_full;
  uint32_t *scratch;
  uint64_t scratch_lanes;
  uint8_t *out;
  const uint64_t *indices;
  const uint32_t *commit_ids;
  const uint32_t *commitments;
  uint32_t *xbuf; /* staging for the per-label working block X between the
                     prologue/romix/tail kernels: 8 uint4 per task, quad-z
                     chunk layout (task*8 + sub, task*8 + sub + 4) */
  uint32_t has_difficulty;
  uint32_t difficulty_be[8];
  PostVrfCandidate *cand;
  unsigned int *cand_count;
  uint32_t cand_cap;
};

/* One phase of the split lean gap-1 ROMix: fill (phase 1, V_j = X, BlockMix)
 * or mix (phase 2, X ^= V_Integerify(X), BlockMix).  A launch owns the
 * scratch columns [slot_base, slot_base + slot_count) of a scratch that is
 * scratch_lanes columns wide; task t < count <= slot_count works in column
 * slot_base + t and keeps its block in xbuf[t] between the two phases. */
struct RomixPhaseArgs {
  uint32_t *scratch;
  uint32_t *xbuf; /* 8 uint4 per task, quad-z chunk layout */
  uint64_t scratch_lanes;
  uint64_t slot_base;
  uint64_t slot_count;
  uint64_t count;
  uint32_t scrypt_n;
};

/* Postdata audit: the prologue and ROMix kernels run on `label` unchanged
 * (index-list mode, one commitment); the audit tail compares instead of
 * storing.  `mismatch` holds label.count entries, so it cannot overflow;
 * *count is zeroed per batch on the stream. */
struct AuditKernelArgs {
  LabelKernelArgs label;
  const uint4 *expected; /* one 16-B on-disk label per task */
  PostAuditMismatch *mismatch;
  unsigned int *count;
};

struct ScanKernelArgs {
  const uint4 *labels;
  uint64_t count;
  uint64_t index_base;
  const uint32_t *te;
  const uint8_t *sbox;
  const uint32_t *rk;
  uint32_t n_ciphers;
  uint64_t difficulty;
  PostScanHit *hits;
  unsigned int *hit_count;
  uint32_t hit_cap;
};

/* Which scan kernel runs and with what geometry; made by poste_scan_plan,
 * the one place that knows a variant's figures, and read by everyone else. */
enum ScanVariant {
  POSTE_SCAN_SHARED,       /* shared T-tables + S-box */
  POSTE_SCAN_BANKREP,      /* bank-replicated Te0 */
  POSTE_SCAN_BANKREP_BG,   /*   with batched gathers */
  POSTE_SCAN_BANKREP512,   /*   at 512 threads */
  POSTE_SCAN_BANKREP512_BG,/*   at 512 threads, batched gathers */
  POSTE_SCAN_TT4,          /* 4 interleaved bank-replicated tables */
};
struct ScanPlan {
  int variant;         /* ScanVariant */
  uint32_t threads;    /* per block */
  uint32_t lds_bytes;  /* dynamic LDS per block */
  uint32_t max_blocks; /* grid cap, >= 1 */
};

/* Postdata seal: page p is labels [1024 p, min(1024 (p + 1), count)) of
 * `labels`; digests[p] receives the first 16 bytes of SHA-256 over the
 * page's bytes.  digests holds ceil(count / 1024) entries. */
#define POSTE_SEAL_PAGE_LABELS 1024
struct SealKernelArgs {
  const uint4 *labels;
  uint64_t count;
  uint4 *digests;
};

/* Seal of a label stream that arrives in segments (init batches, DESIGN
 * 3.7).  What a page that is still open at the end of a segment hands to
 * the next one: the SHA-256 chaining value, the labels of the page absorbed
 * so far (compressed or buffered), and the count % 4 labels not yet
 * compressed, as they lie in memory. */
struct SealCarry {
  uint32_t h[8];
  uint32_t count;
  uint32_t pad[3];
  uint4 buf[3];
};

/* Segment [g0, g0 + count) of the global label stream, count >= 1, lying at
 * `labels`; g0 + count <= stream_end (the stream's label count; UINT64_MAX
 * while the end is not known to lie in this segment).  Lane l works on page
 * g0 / 1024 + l over [max(1024 p, g0), min(1024 (p + 1), g0 + count)).  The
 * page open at g0 (g0 % 1024 != 0) starts from *carry_in, every other from
 * the initial value.  A page that ends inside the segment or at stream_end
 * gets digests[l]; the last page, when it is still open, leaves *carry_out
 * and no digest.  digests holds one entry per page the segment touches;
 * carry_in != carry_out. */
struct SealStreamArgs {
  const uint4 *labels;
  uint64_t g0;
  uint64_t count;
  uint64_t stream_end;
  const SealCarry *carry_in;
  SealCarry *carry_out;
  uint4 *digests;
};

struct VerifyPredArgs {
  const uint4 *labels2;      /* 2 x uint4 per task (full 32-B labels) */
  uint64_t count;
  const uint32_t *te;        /* 1024 words */
  const uint8_t *sbox;       /* 256 bytes */
  const uint32_t *rk;        /* 44 BE words per PROOF */
  const uint32_t *task_proof;/* proof index per task */
  const uint8_t *half;       /* per-proof nonce half (0/1) */
  const uint64_t *difficulty;/* per-proof u64 threshold */
  uint8_t *pass;             /* per-task verdict out */
};

/* VRF-nonce predicate over full labels as the label kernel stores them with
 * out_full: task t passes when its 32 label bytes, read as one big-endian
 * number, are strictly below the 32 bytes of threshold slot task_thr[t]. */
struct VrfPredArgs {
  const uint4 *labels2;      /* 2 x uint4 per task (full 32-B labels) */
  uint64_t count;
  const uint4 *thresholds;   /* 2 x uint4 per slot, big-endian bytes */
  const uint32_t *task_thr;  /* threshold slot per task */
  uint8_t *pass;             /* per-task verdict out */
};

extern "C" {
hipError_t poste_launch_label_kernel(const LabelKernelArgs *args,
                                     uint32_t blocks, hipStream_t stream);
/* the label pipeline one kernel at a time (phase-mixed init path): the
 * prologue and tail as in poste_launch_label_kernel, the lean gap-1 ROMix
 * as its two phases.  The caller checks poste_label_romix_lean_ok. */
hipError_t poste_launch_label_prologue(const LabelKernelArgs *args,
                                       uint32_t blocks, hipStream_t stream);
hipError_t poste_launch_label_tail(const LabelKernelArgs *args,
                                   uint32_t blocks, hipStream_t stream);
hipError_t poste_launch_romix_fill(const RomixPhaseArgs *args,
                                   hipStream_t stream);
hipError_t poste_launch_romix_mix(const RomixPhaseArgs *args,
                                  hipStream_t stream);
hipError_t poste_launch_label_audit(const AuditKernelArgs *args,
                                    uint32_t blocks, hipStream_t stream);
hipError_t poste_launch_verify_pred_kernel(const VerifyPredArgs *args,
                                           uint32_t blocks,
                                           hipStream_t stream);
/* grid-stride, POSTE_THREADS per block; hipErrorInvalidValue for an unset
 * pointer, an empty task list or no block */
hipError_t poste_launch_vrf_pred_kernel(const VrfPredArgs *args,
                                        uint32_t blocks, hipStream_t stream);
/* The scan kernel a plan names.  mode is the exact name; NULL means tt4 and
 * any other string bankrep.  max_blocks, when it parses to a value from 1 up
 * to the variant's own cap, lowers the cap (NULL: the variant's own).  tt4
 * needs a 128 KiB dynamic-LDS opt-in, made here, outside any stream: where it
 * is refused the plan is bankrep's with allow_fallback, the error without.
 * The environment is the caller's business, read once per C-ABI call. */
hipError_t poste_scan_plan(const char *mode, const char *max_blocks,
                           int allow_fallback, ScanPlan *out);
/* the name poste_scan_plan parses for the variant */
const char *poste_scan_variant_name(int variant);
/* on the caller's stream, grid min(ceil(count / threads), max_blocks);
 * hipErrorInvalidValue for an unset pointer, an empty batch or no block */
hipError_t poste_launch_scan(const ScanKernelArgs *args, const ScanPlan *plan,
                             hipStream_t stream);
/* one lane per page; hipErrorInvalidValue for an empty or unset buffer */
hipError_t poste_launch_seal_kernel(const SealKernelArgs *args,
                                    hipStream_t stream);
/* one lane per page the segment touches; hipErrorInvalidValue for an unset
 * pointer, an empty segment, carry_in == carry_out, or a segment that
 * wraps or runs past stream_end */
hipError_t poste_launch_seal_stream_kernel(const SealStreamArgs *args,
                                           hipStream_t stream);
uint64_t poste_label_resident_slots(uint32_t gap_shift);
/* host-only: does the launcher run the lean gap-1 ROMix kernel here? */
int poste_label_romix_lean_ok(uint32_t scrypt_n, uint32_t gap_shift,
                              uint64_t scratch_lanes);
}

#endif
