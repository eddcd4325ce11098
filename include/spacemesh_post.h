/* spacemesh_post.h — C-ABI of the MI355X-native POST engine (libpost_hip.so).
 *
 * This is the drop-in boundary of the rebuild: it plays the
 * role of post-rs's post.h (fetched prebuilt by the reference,
 * Makefile-libs.Inc:49,60-68, consumed via cgo by spacemeshos/post v0.12.9),
 * exporting exactly the entry points the reference's Go side needs:
 *
 *   - provider enumeration/benchmark  -> initialization.OpenCLProviders /
 *     CPUProviderID / Benchmark (activation/post_supervisor.go:105-127,
 *     api/grpcserver/smesher_service.go:248-275)
 *   - incremental init with cancel, progress and resume ->
 *     initialization.NewInitializer(...).Initialize(ctx) /
 *     NumLabelsWritten (activation/post.go:261,267-271,295,355-361)
 *   - prove(challenge) -> {nonce u32, indices bytes, pow u64} ->
 *     the post-service GenProof protocol (api/grpcserver/post_client.go:69-143)
 *   - verify(proof, metadata, opts) -> verifying.ProofVerifier.Verify
 *     (activation/post_verifier.go:150-160, validation.go:182-222), incl.
 *     K3 subset (validation.go:206-209) and selected-index
 *     (activation/malfeasance.go:161-169)
 *   - verify_vrf_nonce -> verifying.VerifyVRFNonce (validation.go:277)
 *   - verify_data -> sampled audit of the labels on disk (upstream postcli
 *     -verify -fraction)
 *
 * The Go binding a maintainer would write against this header (cgo shim
 * satisfying PostSetupProvider / PostVerifier / PostClient) is shown in
 * INTEGRATION.md.  No GPU/torch types cross this boundary: plain pointers,
 * sizes and status codes only.
 *
 * Threading contract: post_verify / post_verify_vrf_nonce are safe to call
 * concurrently from N workers (the reference's pool, post_verifier.go:227).
 * An init session is single-threaded per session object (post.go:276-281);
 * progress/cancel accessors may be called from other threads.
 */
#ifndef SPACEMESH_POST_H
#define SPACEMESH_POST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------- status codes ---------- */
#define POST_OK 0
#define POST_ERR 1              /* generic failure (see post_last_error) */
#define POST_ERR_INVALID_ARGS 2
#define POST_ERR_NO_GPU 3       /* no HIP device / kernels unavailable */
#define POST_ERR_OOM 4
#define POST_ERR_IO 5
#define POST_ERR_CANCELLED 6    /* maps to context.Canceled (post.go:297) */
#define POST_ERR_POW 7          /* invalid proof-of-work */
#define POST_ERR_INVALID_INDEX 8 /* maps to verifying.ErrInvalidIndex */
#define POST_ERR_UNSUPPORTED 9  /* e.g. RandomX pow mode (unpinned) */
#define POST_ERR_NO_NONCE 10    /* prove: no nonce reached K2 */

/* thread-local description of the last error in this thread */
const char *post_last_error(void);

/* ---------- constants ---------- */
#define POST_LABEL_SIZE 16       /* bytes per label in postdata_*.bin */
#define POST_FULL_LABEL_SIZE 32  /* bytes compared for the VRF nonce */
#define POST_MAX_INDICES_BYTES 800 /* wire cap, activation/wire/wire_v1.go:43 */

/* k2pow modes (PostRandomXMode / PowFlags, activation/post_types.go:84-144).
 * RandomX is the reference's mode; it is parity-unpinned in this build
 * (SURVEY.md §7 hard part 1) and returns POST_ERR_UNSUPPORTED. */
#define POST_POW_MODE_RANDOMX 0
#define POST_POW_MODE_BLAKE3 1

/* ---------- provider enumeration ---------- */
typedef struct {
  uint32_t id;
  char model[256];       /* device name, surfaced verbatim over gRPC
                            (api/grpcserver/smesher_service.go:270-275) */
  uint32_t device_type;  /* 0 = GPU (HIP); no CPU provider in this engine */
  uint64_t memory_bytes; /* HBM capacity */
  uint64_t performance;  /* labels/sec estimate; filled by post_benchmark */
} PostProvider;

/* Fills providers[0..cap) and sets *count. POST_OK even when count==0. */
int post_providers(PostProvider *providers, uint32_t cap, uint32_t *count);

/* Measures labels/sec for a provider at the given scrypt N
 * (initialization.Benchmark, activation/post_supervisor.go:120-127). */
int post_benchmark(uint32_t provider_id, uint32_t scrypt_n,
                   uint64_t *labels_per_sec);

/* ---------- configuration ---------- */
typedef struct {
  uint8_t node_id[32];
  uint8_t commitment_atx_id[32];
  uint32_t num_units;
  uint64_t labels_per_unit;   /* mainnet 2^32, config/mainnet.go:186 */
  uint64_t max_file_size;     /* postdata file split, activation/post.go:56 */
  uint32_t scrypt_n;          /* r=1, p=1 fixed (dep default, post.go:155) */
  uint32_t provider_id;
  /* Index-range shard of this session: [index_start, index_end) of the
   * global label space; 0,0 means the whole space.  This is the reference's
   * file/range parallelism (activation/post.go:56-60,166-182) and the
   * 8-GPU sharding axis. */
  uint64_t index_start;
  uint64_t index_end;
  /* Directory for postdata_*.bin + postdata_metadata.json; NULL for
   * in-memory sink mode (benchmark, BASELINE config 2). */
  const char *data_dir;
  /* scratch budget for the ROMix tables, in bytes; 0 = auto (most of free) */
  uint64_t scratch_bytes;
} PostInitConfig;

typedef struct PostInitSession PostInitSession;

/* Create a session. Scans data_dir for existing postdata_*.bin and resumes
 * after the last complete label; the persisted metadata Nonce/NonceValue
 * (re-written whenever the running VRF minimum improves) seeds the
 * session's minimum, so sharded sessions keep their shard-local minimum
 * across kill+resume (StartSession resume semantics,
 * activation/post.go:267-271). */
int post_init_new(const PostInitConfig *cfg, PostInitSession **out);

/* Run initialization to completion (or cancel). Blocking; call from the
 * session's own thread exactly like init.Initialize(ctx) (post.go:295).
 * Returns POST_OK, POST_ERR_CANCELLED, or an error. */
int post_init_run(PostInitSession *s);

/* Process up to max_labels further labels of the session's range (one or
 * more kernel launches), blocking until they are complete.  *done receives
 * the number processed (0 at end of range).  post_init_run is a loop over
 * this.  Exposed for benchmarking (a bench "step"). */
int post_init_step(PostInitSession *s, uint64_t max_labels, uint64_t *done);

/* Kernel-only time of the last post_init_step in milliseconds, measured
 * with HIP events on the session stream (for roofline accounting). */
double post_init_last_kernel_ms(const PostInitSession *s);

/* Progress counter: labels written so far within this session's range
 * (init.NumLabelsWritten, activation/post.go:261). Thread-safe. */
uint64_t post_init_num_labels_written(const PostInitSession *s);

/* Request cancellation; post_init_run returns POST_ERR_CANCELLED.
 * Thread-safe. */
void post_init_cancel(PostInitSession *s);

/* Best VRF nonce found so far: smallest full 32-byte label (big-endian
 * lexicographic) and its index (common/types/activation.go:311-313).
 * Returns POST_OK when one exists, POST_ERR otherwise. */
int post_init_nonce(const PostInitSession *s, uint64_t *index,
                    uint8_t label[32]);

/* In sink mode: borrow the device-resident labels of the last batch /
 * the whole range when kept (for the prove path and parity tests).
 * out_host must hold 16*(count) bytes; copies labels [first,first+count)
 * of the session range to host. */
int post_init_copy_labels(const PostInitSession *s, uint64_t first,
                          uint64_t count, uint8_t *out_host);

void post_init_free(PostInitSession *s);

/* ---------- proving ---------- */
typedef struct {
  uint32_t nonce;
  uint64_t pow;
  uint8_t indices[POST_MAX_INDICES_BYTES];
  uint32_t indices_len;
  uint16_t num_indices;
} PostProof;

typedef struct {
  uint8_t challenge[32];
  uint32_t k1;
  uint32_t k2;
  uint32_t nonces;           /* mainnet 288, config/mainnet.go:61 */
  uint8_t pow_difficulty[32];/* config/mainnet.go:41 */
  uint32_t pow_mode;         /* POST_POW_MODE_* */
  uint32_t pow_threads;      /* host threads for k2pow; 0 = all */
  uint32_t provider_id;
} PostProveConfig;

/* Generate a proof over labels in data_dir (postdata_*.bin +
 * postdata_metadata.json), the post-service GenProof role
 * (api/grpcserver/post_client.go:69-143). */
int post_prove(const char *data_dir, const PostProveConfig *cfg,
               PostProof *out);

/* Same, over a host buffer of 16-byte labels for index range
 * [0, num_labels) (bench/tests). */
int post_prove_buffer(const uint8_t *labels, uint64_t num_labels,
                      const uint8_t node_id[32],
                      const uint8_t commitment_atx_id[32],
                      const PostProveConfig *cfg, PostProof *out);

/* Multi-GPU proving shard: scan labels [index_base,
 * index_base + count) of a space of total_labels labels and return the
 * raw passing (index, nonce) pairs; a coordinator merges shards and packs
 * the winning nonce's indices (go-spacemesh_amd/proving.py).  group_pows
 * must hold nonces/16 k2pow values for the challenge (computed once,
 * shared by all shards). */
typedef struct {
  uint64_t index;
  uint32_t nonce;
  uint32_t pad;
} PostScanHitOut;
int post_prove_scan(const uint8_t *labels, uint64_t count,
                    uint64_t index_base, uint64_t total_labels,
                    const PostProveConfig *cfg, const uint64_t *group_pows,
                    PostScanHitOut *hits, uint32_t cap, uint32_t *n_hits);

/* k2pow helpers so a coordinator can compute/verify group pows once */
int post_k2pow_search(const uint8_t challenge[32], uint32_t nonce_group,
                      const uint8_t pow_difficulty[32], uint32_t pow_mode,
                      uint32_t threads, uint64_t *out);

/* ---------- verification ---------- */
typedef struct {
  /* shared.ProofMetadata as assembled at activation/validation.go:193-199 */
  uint8_t node_id[32];
  uint8_t commitment_atx_id[32];
  uint8_t challenge[32];
  uint32_t num_units;
  uint64_t labels_per_unit;
} PostProofMetadata;

typedef struct {
  uint32_t k1;
  uint32_t k2;
  uint32_t k3;              /* k3 >= k2 -> full verify (validation.go:176) */
  const uint8_t *subset_seed; /* NULL -> full; verifying.Subset seed */
  size_t subset_seed_len;
  int32_t selected_index;   /* >=0 -> verifying.SelectedIndex
                               (malfeasance.go:165); else -1 */
  uint8_t pow_difficulty[32];
  uint32_t pow_mode;
  uint32_t scrypt_n;
  uint32_t provider_id;
} PostVerifyConfig;

/* Verify one proof. POST_OK; POST_ERR_INVALID_INDEX (+ *invalid_index =
 * failing position, for the InvalidPostIndex malfeasance proof,
 * handler_v1.go:228-247); POST_ERR_POW; POST_ERR_INVALID_ARGS.
 * Safe for concurrent callers. */
int post_verify(const PostProof *proof, const PostProofMetadata *meta,
                const PostVerifyConfig *cfg, uint32_t *invalid_index);

/* Batched verification (the verifier-pool steady state, BASELINE config 5):
 * n proofs with per-proof metadata; statuses[i] and invalid_indices[i]
 * receive per-proof results.  One kernel launch recomputes all sampled
 * labels and one applies the AES threshold predicate.  invalid_indices[i]
 * is the first position, in the order the positions are checked (0..k2-1,
 * or the subset's sampling order), that fails either way: its index is out
 * of range, or its label is not below the difficulty. */
int post_verify_batch(const PostProof *proofs, const PostProofMetadata *metas,
                      uint32_t n, const PostVerifyConfig *cfg,
                      int *statuses, uint32_t *invalid_indices);

/* Same with PER-PROOF subset seeds (each gossip verification samples with
 * its own peer-derived seed, validation.go:206-209): subset_seeds holds n
 * fixed-length seeds back to back (NULL -> cfg->subset_seed for all). */
int post_verify_batch_seeded(const PostProof *proofs,
                             const PostProofMetadata *metas, uint32_t n,
                             const PostVerifyConfig *cfg,
                             const uint8_t *subset_seeds, size_t seed_len,
                             int *statuses, uint32_t *invalid_indices);

/* verifying.VerifyVRFNonce (validation.go:261-286): POST_OK when the full
 * 32-byte label at `index` is strictly below the VRF threshold of
 * num_units * labels_per_unit labels as a big-endian number, else
 * POST_ERR_INVALID_INDEX; POST_ERR_INVALID_ARGS for a NULL meta or
 * num_units * labels_per_unit == 0.  The index is not range-checked.  It is
 * the n = 1 case of post_verify_vrf_nonce_batch: the cached per-device
 * workspace, no allocation per call. */
int post_verify_vrf_nonce(const PostProofMetadata *meta, uint64_t index,
                          uint32_t scrypt_n, uint32_t provider_id);

/* Proofs and VRF items verified together (an ATX brings both for the same
 * identity, handler_v1.go:133-149 and :300-324): ONE label-kernel launch
 * recomputes the sampled labels of all proofs and the label of every VRF
 * item; the AES predicate runs over the first, the VRF predicate over the
 * second.  n or n_vrf may be 0 (the arrays of that kind are then not
 * needed).  statuses / invalid_indices are exactly those of
 * post_verify_batch_seeded over the proofs alone; vrf_statuses[j] is what
 * post_verify_vrf_nonce(&vrf_metas[j], vrf_indices[j], cfg->scrypt_n,
 * cfg->provider_id) returns: POST_OK, POST_ERR_INVALID_INDEX, or
 * POST_ERR_INVALID_ARGS for num_units * labels_per_unit == 0 (such an item
 * is not sent to the device and disturbs no other).  The two kinds of
 * verdict do not depend on each other.
 * Validated in this order: POST_ERR_INVALID_ARGS for a NULL cfg, for NULL
 * proofs, metas or statuses with n > 0, for NULL vrf_metas, vrf_indices or
 * vrf_statuses with n_vrf > 0; POST_ERR_UNSUPPORTED for a non-blake3
 * pow_mode when n > 0; POST_OK with nothing touched for n == 0 and
 * n_vrf == 0; then POST_ERR_NO_GPU. */
int post_verify_batch_vrf(const PostProof *proofs, const PostProofMetadata *metas,
                          uint32_t n, const PostVerifyConfig *cfg,
                          const uint8_t *subset_seeds, size_t seed_len,
                          const PostProofMetadata *vrf_metas,
                          const uint64_t *vrf_indices, uint32_t n_vrf,
                          int *statuses, uint32_t *invalid_indices,
                          int *vrf_statuses);

/* The n == 0 form of post_verify_batch_vrf, for callers with no
 * PostVerifyConfig at hand: n VRF items in one label launch and one
 * predicate launch.  POST_ERR_INVALID_ARGS for a NULL array with n > 0,
 * POST_OK for n == 0, then POST_ERR_NO_GPU. */
int post_verify_vrf_nonce_batch(const PostProofMetadata *metas,
                                const uint64_t *indices, uint32_t n,
                                uint32_t scrypt_n, uint32_t provider_id,
                                int *statuses);

/* ---------- postdata audit ---------- */
/* GPU spot-check of on-disk labels: is what is in postdata_*.bin still what
 * init wrote?  (The role of upstream postcli's -verify -fraction.)  The
 * index range [index_start, index_end) is cut into consecutive windows of
 * sample_every labels (the last may be shorter) and exactly one label per
 * window, picked by a seeded hash, is recomputed on the GPU and compared
 * with the 16 bytes on disk.  sample_every = 1 checks every label.  The rule
 * is integer-exact and restated in DESIGN.md 3.4. */

/* Called once per completed batch on the calling thread; a non-zero return
 * stops the audit with POST_ERR_CANCELLED. */
typedef int (*PostAuditProgress)(void *user, uint64_t checked,
                                 uint64_t to_check);

typedef struct {
  uint32_t provider_id;
  uint64_t sample_every;   /* window length K >= 1 */
  uint64_t seed;
  /* [index_start, index_end) of the global label space; 0,0 means the whole
   * space (post_verify_data: NumUnits*LabelsPerUnit from metadata;
   * post_verify_data_buffer: the buffer's span).  A sharded dir is audited
   * with its shard's range. */
  uint64_t index_start;
  uint64_t index_end;
  /* scratch budget for the ROMix tables, in bytes; 0 = auto, as in
   * PostInitConfig */
  uint64_t scratch_bytes;
  PostAuditProgress progress; /* optional */
  void *user;                 /* passed back to progress */
} PostAuditConfig;

typedef struct {
  uint64_t index;
  uint8_t on_disk[POST_LABEL_SIZE];
  uint8_t expected[POST_LABEL_SIZE]; /* recomputed on the GPU */
} PostBadLabel;

typedef struct {
  uint64_t labels_in_range; /* index_end - index_start */
  uint64_t labels_sampled;  /* one per window */
  uint64_t labels_checked;  /* recomputed and compared */
  uint64_t labels_missing;  /* sampled, but file absent or too short */
  uint64_t labels_bad;      /* checked and different; always the full count */
} PostAuditReport;

/* The sampling rule, host-only (needs no GPU): fills out[0..*n) with the
 * sampled indices of windows first_window .. first_window + cap - 1 (fewer
 * at the end of the range) in ascending order. */
int post_verify_data_sample(uint64_t seed, uint64_t sample_every,
                            uint64_t index_start, uint64_t index_end,
                            uint64_t first_window, uint64_t *out,
                            uint32_t cap, uint32_t *n);

/* Audit a postdata directory.  Identity, LabelsPerUnit, NumUnits,
 * MaxFileSize and scrypt N come from postdata_metadata.json; label g lives
 * in postdata_{g / per_file}.bin at byte (g % per_file) * 16 with per_file =
 * MaxFileSize / 16.  A sampled label whose file is absent or ends before its
 * 16th byte counts as missing and is not recomputed.
 *
 * POST_OK means the audit ran to the end: corruption is reported through
 * *report, not as an error.  bad[0..min(cap, labels_bad)) receives the
 * mismatches with the smallest indices, ascending; bad may be NULL when cap
 * is 0.  Arguments and metadata are validated before a GPU is required:
 * POST_ERR_INVALID_ARGS (sample_every == 0, empty/inverted range, range
 * beyond the space), POST_ERR_IO (metadata unreadable or lacking a field),
 * then POST_ERR_NO_GPU.  POST_ERR_CANCELLED when progress asked to stop.
 * Audits on different providers may run concurrently in one process. */
int post_verify_data(const char *data_dir, const PostAuditConfig *cfg,
                     PostBadLabel *bad, uint32_t cap,
                     PostAuditReport *report);

/* Same over a host buffer holding labels [index_base, index_base + count)
 * (bench/tests); 0,0 means that whole span. */
int post_verify_data_buffer(const uint8_t *labels, uint64_t count,
                            uint64_t index_base, const uint8_t node_id[32],
                            const uint8_t commitment_atx_id[32],
                            uint32_t scrypt_n, const PostAuditConfig *cfg,
                            PostBadLabel *bad, uint32_t cap,
                            PostAuditReport *report);

/* ---------- postdata seal ---------- */
/* Page digests checked during the proving pass: every byte the proving scan
 * reads is hashed while it is on the device and compared with a digest
 * written once (the seal), so each epoch's pass covers 100 % of the dir at
 * no extra IO.  The format is fixed in DESIGN.md 3.5:
 *
 *   sealed stream  the labels as post_prove reads the dir: postdata_0.bin,
 *                  postdata_1.bin, ... up to the first absent file,
 *                  floor(size / 16) labels of each, concatenated
 *   page p         labels [1024 p, min(1024 (p + 1), total)) of that stream
 *                  (16 KiB; the last page may be shorter, a page may span
 *                  two files)
 *   digest         the first 16 bytes of SHA-256 over the page's bytes
 *   sidecar        postdata_seal.bin in the data dir: a 32-byte
 *                  little-endian header {magic "PSTSEAL1", u32 page_labels =
 *                  1024, u32 digest_bytes = 16, u64 total_labels, u64 0},
 *                  then ceil(total / 1024) digests
 *
 * A bad page number p is what verify-data confirms by recomputation over
 * labels [1024 p, 1024 (p + 1)).  Sharded dirs are sealed in their own
 * stream's terms, not in global-index terms. */
typedef struct {
  uint64_t total_labels; /* label count of the sealed stream */
  uint64_t pages;        /* ceil(total_labels / 1024) */
  uint64_t pages_bad;    /* always the full count */
  uint32_t proof_touches_bad_page; /* post_prove_checked only */
} PostSealReport;

/* GPU page digests of a host buffer of count >= 1 labels (tests, building
 * block): digests[0 .. 16 * *n_pages).  POST_ERR_INVALID_ARGS when
 * cap_pages is below ceil(count / 1024). */
int post_seal_digest_buffer(const uint8_t *labels, uint64_t count,
                            uint32_t provider_id, uint8_t *digests,
                            uint64_t cap_pages, uint64_t *n_pages);

/* One pass over the dir that writes the sidecar, under a temporary name in
 * the same dir (postdata_seal.bin.tmp) renamed into place. */
int post_seal_data(const char *data_dir, uint32_t provider_id,
                   PostSealReport *r);

/* One pass over the dir, no proof: recompute the digests and compare them
 * with the sidecar.  POST_OK means the pass ran to the end: corruption is
 * reported through *r, not as an error.  bad_pages[0..min(cap, pages_bad))
 * receives the smallest bad page numbers, ascending; bad_pages may be NULL
 * when cap is 0.  *r is filled on POST_OK only.
 *
 * Validated in this order before a GPU is required: POST_ERR_INVALID_ARGS
 * (NULL pointer, or cap > 0 with bad_pages NULL); then POST_ERR_IO for a
 * sidecar that is absent, shorter than its header plus the digests its
 * header announces, of a wrong magic, of a page_labels other than 1024 or
 * a digest_bytes other than 16, or whose total_labels differs from the
 * dir's current label count ("postdata length changed since seal":
 * truncated, removed or grown files); then POST_ERR_NO_GPU. */
int post_check_seal(const char *data_dir, uint32_t provider_id,
                    uint64_t *bad_pages, uint32_t cap, PostSealReport *r);

/* post_prove with the seal checked in the same pass: the proof is the one
 * post_prove returns; *r and bad_pages as for post_check_seal, validated the
 * same way before cfg is looked at.  r->proof_touches_bad_page is 1 when
 * any of the proof's K2 indices lies in a bad page: such a proof may fail on
 * the verifier's side (an invalid index is grounds for a malfeasance proof,
 * handler_v1.go:228-247) and must not be published. */
int post_prove_checked(const char *data_dir, const PostProveConfig *cfg,
                       PostProof *out, uint64_t *bad_pages, uint32_t cap,
                       PostSealReport *r);

/* ---------- seal during init ---------- */
/* The sidecar of post_seal_data, produced by the init session itself from
 * the labels as they lie in device memory behind the label kernels (DESIGN.md
 * 3.7): no second pass over the dir, and the digests witness what the GPU
 * computed, not what came back from the disk.  Off by default.
 *
 * While a session runs, its digests are appended to
 * postdata_seal.part-<index_start>: a 32-byte little-endian header {magic
 * "PSTSEALP", u32 page_labels = 1024, u32 digest_bytes = 16, u64 first_page,
 * u64 end_page (exclusive)}, then one digest per closed page in page order,
 * each appended after the labels of its page were written.  A new session
 * over the same range resumes at min(labels on disk rounded down to a page,
 * 1024 * digests in the part), truncates the part to that and recomputes
 * from there.  When the session's range is complete the parts are assembled
 * (post_seal_assemble); with other shards still running that is left to the
 * last of them.
 *
 * Call after post_init_new and before the first post_init_step.  Validated
 * in this order: POST_ERR_INVALID_ARGS for a NULL session or one without a
 * data dir; POST_ERR_INVALID_ARGS after the first step; POST_ERR_UNSUPPORTED
 * for an index_start that is no multiple of 1024 or an index_end that is
 * neither one nor the end of the label space; POST_ERR_UNSUPPORTED for a
 * max_file_size that is no multiple of 16; POST_ERR_UNSUPPORTED for a range
 * that already has labels on disk but neither a part file nor a finished
 * sidecar; POST_ERR_IO for a part file whose header disagrees with the
 * session. */
int post_init_enable_seal(PostInitSession *s);

/* Host-only, no GPU: collect the part files of data_dir, require them to
 * tile pages [0, ceil(NumUnits * LabelsPerUnit / 1024)) of
 * postdata_metadata.json with no gap or overlap and every part full, write
 * postdata_seal.bin (byte for byte what post_seal_data writes for the same
 * labels) under a temporary name unique to the process, rename it into place
 * and remove the parts.  *pages (may be NULL) receives the page count.
 * POST_ERR_IO, with the first missing page range in the message, when the
 * tiling is incomplete; POST_OK when there is no part and the sidecar is
 * already there. */
int post_seal_assemble(const char *data_dir, uint64_t *pages);

/* Test entry beside post_seal_digest_buffer: the labels are the stream
 * [first_index, first_index + count), first_index a multiple of 1024, cut
 * into segments at cuts[0 .. n_cuts) (ascending positions within the
 * buffer; an empty segment is skipped); the stream kernel runs once per
 * segment with the carry handed on.  With stream_end != 0 the buffer's end
 * is the end of the stream and a ragged last page is closed: ceil(count /
 * 1024) digests, otherwise floor.  POST_ERR_INVALID_ARGS when cap_pages is
 * below that. */
int post_seal_digest_stream(const uint8_t *labels, uint64_t count,
                            uint64_t first_index, const uint64_t *cuts,
                            uint32_t n_cuts, uint32_t stream_end,
                            uint32_t provider_id, uint8_t *digests,
                            uint64_t cap_pages, uint64_t *n_pages);

/* ---------- initial proof during init ---------- */
/* A node proves over the zero challenge as soon as init ends
 * (activation/activation.go:350-402, BuildInitialPost); done with post_prove
 * that is a second read of every byte just written.  A session that opts in
 * runs the proving scan over every batch while it lies in device memory
 * behind the label kernels, so a finished init has the hits
 * of its range on disk and the proof is a host-only merge.  Off by default;
 * a session that does not opt in queues exactly what it queued before.
 *
 * While a session runs, the hits of its range are appended to
 * postdata_hits.part-<index_start>, little-endian: a 128-byte header {magic
 * "PSTHITSP", u32 record_bytes = 16, u32 nonces, u32 k1, u32 k2,
 * challenge[32], pow_difficulty[32], u64 index_start, u64 index_end,
 * u64 total_labels, zeros}, then 16-byte records {u64 index, u32 nonce,
 * u32 tag}.  A hit has tag 0; a marker has nonce 0xFFFFFFFF, tag 0x4B52414D
 * and index = the global index up to which the part is complete.  After the
 * labels of a batch are in the files its hits are appended, sorted by
 * (index, nonce), then one marker; only then does
 * post_init_num_labels_written advance.  The file is ascending, hits are on
 * disk only behind their labels, and every hit is kept (nonces * k1 in
 * expectation over the whole space).
 *
 * A new session over the same range drops what follows the last well-formed
 * marker, resumes at min(labels on disk, last marker, the seal's resume point
 * when the seal is on as well), cuts the part at the first record at or past
 * that point and writes a marker there.  A step that follows a failed step
 * does the same.
 *
 * The difficulty is that of the whole space (NumUnits * LabelsPerUnit), the
 * indices are global, and the k2pow is the smallest one, so shards need no
 * coordination.  The device hit buffer of a batch holds
 * clamp(16 * ceil(batch * nonces * k1 / total_labels), 4096, 65536) records
 * (batch = labels per launch); a batch with more hits fails its step with
 * POST_ERR: nothing of it is appended and post_init_num_labels_written does
 * not advance.
 *
 * The host gets the count of a batch and its first 1024 records with the
 * batch's other results; a batch with more hits is fetched a second time,
 * which waits for everything queued on the device.
 *
 * Environment, read once by post_init_enable_proof and never per launch:
 * POST_INIT_PROOF_SCAN = bankrep (default) or tt4 picks the scan kernel, both
 * leave identical parts (anything else: POST_ERR_INVALID_ARGS, judged before
 * the dir is touched; a tt4 whose 128 KiB of LDS the device refuses is an
 * error too, there is no fallback here); POST_SCAN_MAX_BLOCKS lowers the
 * scan's grid cap as it does for post_prove; the session keeps the resulting
 * scan plan; POST_INIT_PROOF_DEBUG times the scan of every batch
 * with device events and prints the figures on stderr when the range is
 * complete.
 *
 * Not covered: sessions without a data dir, RandomX, a challenge that is not
 * known when init starts, a dir started without the scan.
 *
 * Call after post_init_new (and post_init_enable_seal) and before the first
 * post_init_step; cfg->provider_id is ignored, the session's is used.
 * Validated in this order, all of it before a GPU is required:
 * POST_ERR_INVALID_ARGS for a NULL session, a NULL cfg or a session without a
 * data dir; POST_ERR_INVALID_ARGS after the first step;
 * POST_ERR_INVALID_ARGS for nonces zero or no multiple of 16;
 * POST_ERR_UNSUPPORTED for a pow_mode other than blake3;
 * POST_ERR_UNSUPPORTED for a range that has labels on disk and no part file;
 * POST_ERR_IO for a part file whose header disagrees with the session or
 * with cfg.  A call that fails leaves no part file behind that it created.
 * A second call with the config in force is POST_OK, with another one
 * POST_ERR_INVALID_ARGS. */
int post_init_enable_proof(PostInitSession *s, const PostProveConfig *cfg);

typedef struct {
  uint64_t total_labels;   /* NumUnits * LabelsPerUnit */
  uint64_t labels_covered; /* by the parts found */
  uint64_t hits;           /* records in the merged list */
  uint32_t parts;
  uint32_t reserved;
} PostInitProofReport;

/* Host only, no GPU, reads only: merge the part files of data_dir and choose
 * the winner by the rule of post_prove; the proof is the one post_prove
 * returns on the finished dir.  The parts must agree in everything but
 * their range, tile [0, NumUnits * LabelsPerUnit) of postdata_metadata.json
 * with no gap or overlap, and each must be complete (its last marker at its
 * index_end): otherwise POST_ERR_IO, the message naming the first missing
 * index range.  POST_ERR_NO_NONCE when no nonce reaches K2 (post_prove fails
 * the same way).  It writes nothing and removes nothing, so it may be called
 * at any time and any number of times; r may be NULL and is filled whenever
 * the tiling was complete. */
int post_init_proof_assemble(const char *data_dir, PostProof *out,
                             PostInitProofReport *r);

/* ---------- self-healing prove ---------- */
/* What the seal pass finds bad is put right in the same call (DESIGN.md
 * 3.6): the bad pages are recomputed on the GPU from the identity in
 * postdata_metadata.json, the proving scan is run again over the recomputed
 * labels alone, the first pass's hits in bad pages are replaced by the new
 * ones, and the winner is chosen by the unchanged rule.  The proof is the
 * one post_prove returns on the undamaged dir.
 *
 * A recomputed page whose digest equals the sidecar's is confirmed:
 * recomputation and seal agree.  One whose digest differs is unconfirmed:
 * the sidecar entry is wrong, or the seal was taken over data that was
 * already bad.  The recomputed labels are used either way (they are what a
 * verifier recomputes); only confirmed pages are ever written back. */
typedef struct {
  /* heal at most this many pages; 0 = 4096: 2^22 labels, measured at 2.0 s
   * of recompute at mainnet N on one MI355X, plus up to a few seconds for
   * the ROMix scratch (profiles/heal.md).  With more bad pages nothing is
   * healed and the call is post_prove_checked. */
  uint32_t max_pages;
  /* non-zero: pwrite every confirmed page over the file bytes, then fsync
   * each touched file once (post_repair_data always writes) */
  uint32_t write_back;
  /* scratch budget for the ROMix tables, as in PostAuditConfig */
  uint64_t scratch_bytes;
} PostHealConfig;

typedef struct {
  uint64_t total_labels;
  uint64_t pages;
  uint64_t pages_bad;              /* as found on disk by the pass */
  /* only after a skipped heal, then as post_prove_checked sets it: a healed
   * proof has no index in a page that is still bad */
  uint32_t proof_touches_bad_page;
  uint32_t heal_skipped;           /* 1: pages_bad > the limit */
  uint64_t pages_healed;           /* recomputed and used: confirmed or not */
  uint64_t pages_unconfirmed;
  uint64_t labels_repaired;        /* disk bytes != recomputation */
  uint64_t hits_dropped;           /* first-pass hits in bad pages */
  uint64_t hits_added;             /* hits of the recomputed labels */
  uint64_t pages_written;          /* confirmed pages written back */
  /* any of the proof's K2 indices lies in an unconfirmed page: the proof
   * stands on labels the seal could not vouch for; do not publish */
  uint32_t proof_touches_unconfirmed_page;
  uint32_t reserved;
} PostHealReport;

/* post_prove_checked that heals.  bad_pages / cap as for post_check_seal
 * (what the pass found on disk).  POST_OK means the call ran to the end;
 * *r is filled on POST_OK only.  Pages are written back before the winner
 * is chosen, so POST_ERR_NO_NONCE can leave a repaired dir behind.
 *
 * Validated in this order before a GPU is required: the rungs of
 * post_check_seal; POST_ERR_IO for a postdata_metadata.json that cannot be
 * read or lacks a field (as post_verify_data); POST_ERR_UNSUPPORTED for a
 * stream that is not in global-index terms — a file other than the last
 * that does not hold MaxFileSize / 16 labels, or more labels than
 * NumUnits * LabelsPerUnit (sharded dirs); then cfg as post_prove looks at
 * it, POST_ERR_NO_GPU included. */
int post_prove_healed(const char *data_dir, const PostProveConfig *cfg,
                      const PostHealConfig *heal, PostProof *out,
                      uint64_t *bad_pages, uint32_t cap, PostHealReport *r);

/* The same pass with no proof: check the seal, recompute the bad pages,
 * write the confirmed ones back.  A following post_check_seal is clean
 * exactly when pages_written == pages_bad.  hits_* and the proof flags stay
 * zero.  Validated as post_prove_healed, then POST_ERR_NO_GPU. */
int post_repair_data(const char *data_dir, uint32_t provider_id,
                     const PostHealConfig *heal, uint64_t *bad_pages,
                     uint32_t cap, PostHealReport *r);

/* ---------- introspection / self-test ---------- */
/* Engine's independent blake3 (for cross-checking vs the oracle's in
 * tests; not a product entry point). */
void post_selftest_blake3(const uint8_t *msg, size_t len, uint8_t out[32]);
/* Engine's host AES-128 single block (same purpose). */
void post_selftest_aes128(const uint8_t key[16], const uint8_t in[16],
                          uint8_t out[16]);
/* Engine's host reference label (used only by tests to cross-check the
 * device path; computed with the engine's own host scrypt). */
int post_selftest_label(const uint8_t node_id[32],
                        const uint8_t commitment_atx_id[32], uint64_t index,
                        uint32_t scrypt_n, uint8_t out[32]);
/* Verification's device predicate on labels the caller supplies (used only
 * by tests): `count` full 32-byte labels, `n_proofs` 16-byte AES keys, half
 * bytes (0/1) and u64 difficulties, and `count` task->proof indices, each
 * below n_proofs (POST_ERR_INVALID_ARGS otherwise).  The keys are expanded
 * by the engine's host AES and the production kernel is launched by the
 * production launcher over the device tables verification uses, with
 * min(ceil(count / 256), max_blocks) blocks; max_blocks == 0 is the
 * production cap (8192).  pass[i] is 1 where task i's selected little-endian
 * u64 of AES(key, label[0..16)) is below its proof's difficulty, else 0. */
int post_selftest_verify_pred(const uint8_t *labels, uint64_t count,
                              const uint8_t *keys, const uint8_t *halves,
                              const uint64_t *difficulties, uint32_t n_proofs,
                              const uint32_t *task_proof, uint32_t max_blocks,
                              uint32_t provider_id, uint8_t *pass);

/* The VRF-nonce device predicate on labels the caller supplies (used only by
 * tests): `count` full 32-byte labels, `n_thr` 32-byte big-endian
 * thresholds and `count` task->threshold indices, each below n_thr.  The
 * production kernel is launched by the production launcher with
 * min(ceil(count / 256), max_blocks) blocks; max_blocks == 0 is the
 * production cap (8192).  pass[i] is 1 where label i is strictly below its
 * threshold as a 32-byte big-endian number, else 0.  An index that is not
 * below n_thr, a NULL pointer, count == 0 or n_thr == 0 gives
 * POST_ERR_INVALID_ARGS before a GPU is required. */
int post_selftest_vrf_pred(const uint8_t *labels, uint64_t count,
                           const uint8_t *thresholds, uint32_t n_thr,
                           const uint32_t *task_thr, uint32_t max_blocks,
                           uint32_t provider_id, uint8_t *pass);

/* version / build info string */
const char *post_engine_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SPACEMESH_POST_H */
