/* engine.cpp — C-ABI implementation of the MI355X POST engine
 * (include/spacemesh_post.h).  Host orchestration around the HIP kernels:
 * sessions, streams, file IO, resume, nonce tracking, proving pipeline,
 * batched verification.  No CPU compute fallback: every compute entry
 * requires a HIP device and fails loudly without one (POST_ERR_NO_GPU).
 *
 * Reference lifecycle being mirrored (file:line under /root/reference/):
 *   activation/post.go:261,267-331   init progress/resume/cancel/state
 *   activation/post.go:299-312       reference-label self-check
 *   api/grpcserver/post_client.go:69-143  prove protocol results
 *   activation/post_verifier.go:150-160 + validation.go:182-222  verify
 */
#include "../../include/spacemesh_post.h"

#include <hip/hip_runtime.h>

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <thread>
#include <chrono>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "crypto_host.h"
#include "hip_owned.h"
#include "init_proof_host.h"
#include "kernel_args.h"
#include "post_common.h"

namespace {

using hip_owned::DevBuf;
using hip_owned::Event;
using hip_owned::PinnedBuf;
using hip_owned::Stream;

thread_local std::string g_last_error;

void set_error(const std::string &e) { g_last_error = e; }

int hip_fail(const char *what, hipError_t err) {
  set_error(std::string(what) + ": " + hipGetErrorString(err));
  return err == hipErrorOutOfMemory ? POST_ERR_OOM : POST_ERR;
}

#define HIP_TRY(expr)                                                          \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) return hip_fail(#expr, _e);                          \
  } while (0)

int require_gpu(uint32_t provider_id) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    set_error("no HIP device available (the HIP engine has no CPU fallback)");
    return POST_ERR_NO_GPU;
  }
  if (provider_id >= (uint32_t)count) {
    set_error("provider id out of range");
    return POST_ERR_INVALID_ARGS;
  }
  e = hipSetDevice((int)provider_id);
  if (e != hipSuccess) return hip_fail("hipSetDevice", e);
  return POST_OK;
}

void load_commitment_words(const uint8_t c[32], uint32_t w[8]) {
  std::memcpy(w, c, 32); /* little-endian host/device byte stream words */
}

void difficulty_to_be_words(const uint8_t d[32], uint32_t w[8]) {
  for (int i = 0; i < 8; i++)
    w[i] = ((uint32_t)d[4 * i] << 24) | ((uint32_t)d[4 * i + 1] << 16) |
           ((uint32_t)d[4 * i + 2] << 8) | d[4 * i + 3];
}

constexpr uint32_t THREADS = 256;
/* grid cap of the verification predicate; its loop strides over the rest */
constexpr uint32_t VERIFY_PRED_MAX_BLOCKS = 8192;
constexpr uint32_t CAND_CAP = 1 << 16;

/* lookup-gap (kernel_args.h).  Measured on MI355X (gpurun summary3-5
 * logs): with the quad-cooperative kernels the scratch fits at gap 1 and
 * extra recompute only costs, so the default is gap 1 (shift 0).
 * POST_GAP_SHIFT overrides for scratch-constrained configs. */
uint32_t pick_gap_shift(uint32_t scrypt_n) {
  const char *env = getenv("POST_GAP_SHIFT");
  if (env) {
    uint32_t g = (uint32_t)atoi(env);
    while ((scrypt_n >> g) == 0) g--;
    return g;
  }
  return 0;
}

/* Labels per chunk of the proving scan: 2^24 (256 MiB).
 * POST_PROVE_CHUNK_LABELS lowers it (floor 256; unset, zero, unparsable or
 * not lower = 2^24), so a small buffer crosses several chunk boundaries and
 * reuses both pipeline buffers.  Read per call, as POST_SCAN_MODE is. */
uint64_t prove_chunk_labels() {
  const uint64_t dflt = 1ull << 24;
  const char *env = getenv("POST_PROVE_CHUNK_LABELS");
  if (!env) return dflt;
  const long long v = strtoll(env, nullptr, 10);
  if (v <= 0 || (uint64_t)v >= dflt) return dflt;
  return v < 256 ? 256 : (uint64_t)v;
}

/* The prove path's scan plan: POST_SCAN_MODE and POST_SCAN_MAX_BLOCKS, read
 * once per call (tests switch them between calls inside one process); tt4
 * falls back to bankrep where its LDS opt-in is refused.  The device is
 * current (require_gpu). */
hipError_t prove_scan_plan(ScanPlan *plan) {
  return poste_scan_plan(getenv("POST_SCAN_MODE"),
                         getenv("POST_SCAN_MAX_BLOCKS"), 1, plan);
}

/* Cached per-device verification workspace: the worker-pool call pattern
 * (one proof per post_verify call, post_verifier.go:150-160) would
 * otherwise pay scratch/staging allocation on every call.  Calls remain
 * safe for concurrent workers; they serialize on the device section. */
struct VerifyWorkspace {
  std::mutex mu;
  DevBuf<uint32_t> d_scratch;
  size_t scratch_cap = 0; /* bytes */
  DevBuf<uint64_t> d_idx;
  DevBuf<uint32_t> d_cid;
  DevBuf<uint8_t> d_out;
  DevBuf<uint32_t> d_xbuf;
  size_t tasks_cap = 0;
  DevBuf<uint32_t> d_cm;
  size_t cm_cap = 0; /* words */
  DevBuf<uint32_t> d_vrk; /* 44 words per proof */
  DevBuf<uint8_t> d_half;
  DevBuf<uint64_t> d_vdiff;
  size_t proofs_cap = 0;
  DevBuf<uint8_t> d_pass; /* per task, with tasks_cap */
  DevBuf<uint8_t> d_vthr; /* 32-B VRF threshold per VRF item */
  DevBuf<uint32_t> d_vmap; /* VRF task -> threshold slot */
  size_t vrf_cap = 0;
};
std::mutex g_vws_mu;
std::map<int, VerifyWorkspace *> g_vws;

VerifyWorkspace *get_verify_ws(int dev) {
  std::lock_guard<std::mutex> lk(g_vws_mu);
  auto it = g_vws.find(dev);
  if (it != g_vws.end()) return it->second;
  auto *w = new VerifyWorkspace();
  g_vws[dev] = w;
  return w;
}

/* growing a group releases all of it first, then allocates */
int ws_reserve_proofs(VerifyWorkspace *w, size_t proofs, size_t vrf_items) {
  if (vrf_items > w->vrf_cap) {
    size_t cap = std::max<size_t>(vrf_items, 1024);
    w->d_vthr.reset(); w->d_vmap.reset();
    w->vrf_cap = 0;
    HIP_TRY(w->d_vthr.alloc(cap * 32));
    HIP_TRY(w->d_vmap.alloc(cap * 4));
    w->vrf_cap = cap;
  }
  if (proofs > w->proofs_cap) {
    size_t cap = std::max<size_t>(proofs, 1024);
    w->d_vrk.reset(); w->d_half.reset(); w->d_vdiff.reset();
    w->proofs_cap = 0;
    HIP_TRY(w->d_vrk.alloc(cap * 44 * 4));
    HIP_TRY(w->d_half.alloc(cap));
    HIP_TRY(w->d_vdiff.alloc(cap * 8));
    w->proofs_cap = cap;
  }
  return POST_OK;
}

int ws_reserve(VerifyWorkspace *w, size_t scratch_bytes, size_t tasks,
               size_t cm_words) {
  if (scratch_bytes > w->scratch_cap) {
    w->scratch_cap = 0;
    HIP_TRY(w->d_scratch.alloc(scratch_bytes));
    w->scratch_cap = scratch_bytes;
  }
  if (tasks > w->tasks_cap) {
    size_t cap = std::max<size_t>(tasks, 4096);
    w->d_idx.reset(); w->d_cid.reset(); w->d_out.reset();
    w->d_xbuf.reset(); w->d_pass.reset();
    w->tasks_cap = 0;
    HIP_TRY(w->d_idx.alloc(cap * 8));
    HIP_TRY(w->d_cid.alloc(cap * 4));
    HIP_TRY(w->d_out.alloc(cap * 32));
    HIP_TRY(w->d_xbuf.alloc(cap * 128));
    HIP_TRY(w->d_pass.alloc(cap));
    w->tasks_cap = cap;
  }
  if (cm_words > w->cm_cap) {
    size_t cap = std::max<size_t>(cm_words, 1024);
    w->cm_cap = 0;
    HIP_TRY(w->d_cm.alloc(cap * 4));
    w->cm_cap = cap;
  }
  return POST_OK;
}

struct DeviceTables { /* AES tables, resident per device for good */
  uint32_t *d_te = nullptr;
  uint8_t *d_sbox = nullptr;
};
std::mutex g_tables_mu;
std::map<int, DeviceTables> g_tables;

int get_aes_tables(int dev, DeviceTables &out) {
  std::lock_guard<std::mutex> lk(g_tables_mu);
  auto it = g_tables.find(dev);
  if (it != g_tables.end()) {
    out = it->second;
    return POST_OK;
  }
  static uint32_t te[1024];
  static uint8_t sbox[256];
  poste::aes128_tables(te, sbox);
  DevBuf<uint32_t> d_te;
  DevBuf<uint8_t> d_sbox;
  HIP_TRY(d_te.alloc(sizeof(te)));
  HIP_TRY(d_sbox.alloc(sizeof(sbox)));
  HIP_TRY(hipMemcpy(d_te.get(), te, sizeof(te), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_sbox.get(), sbox, sizeof(sbox), hipMemcpyHostToDevice));
  DeviceTables t;
  t.d_te = d_te.get();
  t.d_sbox = d_sbox.get();
  (void)d_te.release();
  (void)d_sbox.release();
  g_tables[dev] = t;
  out = t;
  return POST_OK;
}

} // namespace

extern "C" {

const char *post_last_error(void) { return g_last_error.c_str(); }

const char *post_engine_version(void) {
  return "spacemesh-post-hip 0.2 (gfx950)";
}

/* ------------------------- providers ------------------------- */

int post_providers(PostProvider *providers, uint32_t cap, uint32_t *count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = (uint32_t)n;
  for (uint32_t i = 0; i < (uint32_t)n && i < cap; i++) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, (int)i) != hipSuccess) continue;
    providers[i].id = i;
    std::snprintf(providers[i].model, sizeof(providers[i].model), "%s",
                  prop.name);
    providers[i].device_type = 0;
    providers[i].memory_bytes = prop.totalGlobalMem;
    providers[i].performance = 0;
  }
  return POST_OK;
}

/* ------------------------- init session ------------------------- */

/* What one batch leaves for the host.  The monolithic path uses set 0 alone
 * (and fetches its candidates through pageable memory); the split path
 * alternates between the two, so batch i is processed while batch i+1 runs.
 * Set 1 exists only on the split path, and its d_out only when the labels
 * are not kept on the device. */
struct OutputSet {
  DevBuf<uint8_t> d_out;     /* batch output (16 B per label) */
  PinnedBuf<uint8_t> h_batch;
  DevBuf<PostVrfCandidate> d_cand;
  DevBuf<unsigned int> d_cand_count;
  /* split path only */
  PinnedBuf<PostVrfCandidate> h_cand;
  PinnedBuf<unsigned int> h_cand_count;
  Event ev_tail[3], ev_end, ev_done;
  Event ev_reset;            /* the set's count zeroed */
  /* seal during init */
  DevBuf<uint4> d_seal_dig;
  PinnedBuf<uint8_t> h_seal_dig;
  /* POST_SEAL_DEBUG: the stream kernel timed per batch, printed at the end */
  Event ev_seal[2];
  /* initial proof during init: the batch's hits, its count, and what the
   * host gets of both in front of ev_done */
  DevBuf<PostScanHit> d_hits;
  DevBuf<unsigned int> d_hit_count;
  PinnedBuf<PostScanHit> h_hits; /* PROOF_HIT_WINDOW records */
  PinnedBuf<unsigned int> h_hit_count;
  Event ev_scan[2];              /* POST_INIT_PROOF_DEBUG */
};

struct PostInitSession {
  PostInitConfig cfg;
  std::string data_dir;
  uint64_t range_start = 0, range_end = 0;
  std::atomic<uint64_t> written{0};
  std::atomic<bool> cancel{false};
  uint8_t commitment[32];

  std::mutex nonce_mu;
  bool nonce_found = false;
  uint64_t nonce_idx = 0;
  uint8_t nonce_label[32];

  uint64_t lanes = 0;       /* concurrent labels (scratch slots); one slot
                               = one quad of 4 threads in the kernel */
  uint64_t batch_seq = 0;   /* batches processed (self-check period) */
  uint32_t gap_shift = 0;
  uint64_t batch = 0;       /* labels per launch */
  DevBuf<uint32_t> d_scratch;
  DevBuf<uint8_t> d_all;    /* whole-range output kept on device (small) */
  bool keep_all = false;
  DevBuf<uint32_t> d_xbuf;  /* 128 B per batch task (3-kernel staging) */
  uint32_t cand_cap = 0;
  OutputSet set[2];
  Event ev0, ev1;
  double last_kernel_ms = 0; /* accumulated over the last post_init_step */

  /* split-kernel init path (init_step_split): 0 = monolithic ROMix on
   * `stream`; 2 or 3 = phase-mixed, the slots divided among `stream`,
   * `stream_b` (and `stream_c`); 1 = the split kernels on `stream` alone
   * (measurement).  `split_chain` holds the fill of a unit behind the fill
   * of the unit before it (two streams only, the earlier schedule, A/B).
   * Output set 1 and `copy_stream` double-buffer what the host reads. */
  int split_streams = 0;
  bool split_chain = false;
  uint64_t unit_cursor = 0; /* units issued so far: unit u runs on stream
                               u % split_streams, across batches and calls */
  uint64_t split_batch_no = 0; /* batches issued so far: output set = & 1 */
  Event ev_fill[4];            /* chain */

  /* seal during init (post_init_enable_seal); all unused and
   * nothing of it queued while seal_on is false */
  bool stepped = false;      /* a post_init_step has begun */
  bool seal_on = false;
  int seal_fd = -1;          /* the part file */
  uint64_t seal_first_page = 0;
  uint64_t seal_pos = 0;     /* relative position the device carry stands at */
  uint64_t seal_launches = 0; /* carry in = launches & 1, out = the other */
  DevBuf<SealCarry> d_seal_carry; /* two */
  double seal_ms = 0, seal_ms_max = 0;
  uint64_t seal_timed = 0;

  /* initial proof during init (post_init_enable_proof); all
   * unused and nothing of it queued while proof_on is false */
  bool proof_on = false;
  int proof_fd = -1;          /* the part file */
  initproof::Header proof_hdr;
  uint64_t proof_pos = 0;     /* relative position of the part's last marker;
                                 UINT64_MAX while an append is under way */
  uint64_t proof_bytes = 0;   /* size of the part file */
  ScanPlan proof_plan{};      /* variant, geometry, grid cap */
  uint32_t proof_hit_cap = 0; /* records per output set */
  ScanKernelArgs proof_scan;  /* tables, round keys, difficulty */
  DevBuf<uint32_t> d_proof_rk;
  double proof_ms = 0, proof_ms_max = 0;
  uint64_t proof_timed = 0, proof_hits = 0, proof_refetch = 0;

  /* declared last, so destroyed first (hip_owned.h) */
  Stream stream, stream_b, stream_c, copy_stream;

  /* every stream on its own: nothing relies on one stream's end implying
   * another's */
  void sync_streams() {
    for (Stream *st : {&stream, &stream_b, &stream_c, &copy_stream})
      if (st->get()) (void)hipStreamSynchronize(st->get());
  }
  ~PostInitSession() {
    sync_streams(); /* they wait on each other's events: all, then release */
    if (seal_fd >= 0) (void)::close(seal_fd);
    if (proof_fd >= 0) (void)::close(proof_fd);
  }
};

static uint64_t existing_labels(const std::string &dir, uint64_t per_file,
                                uint64_t range_start, uint64_t range_total) {
  /* resume point = number of contiguous complete labels already on disk
   * (StartSession resume, activation/post.go:267-271) */
  uint64_t done = 0;
  for (uint64_t pos = range_start; pos < range_start + range_total;) {
    uint64_t file_i = pos / per_file;
    uint64_t in_file = pos % per_file;
    uint64_t file_cap = std::min(per_file - in_file,
                                 range_start + range_total - pos);
    char path[4096];
    std::snprintf(path, sizeof path, "%s/postdata_%llu.bin", dir.c_str(),
                  (unsigned long long)file_i);
    FILE *f = std::fopen(path, "rb");
    if (!f) break;
    std::fseek(f, 0, SEEK_END);
    long sz = std::ftell(f);
    std::fclose(f);
    uint64_t labels_here = (uint64_t)(sz < 0 ? 0 : sz) / POST_LABEL_SIZE;
    if (in_file > labels_here) break;
    uint64_t usable = std::min(labels_here - in_file, file_cap);
    done += usable;
    pos += usable;
    if (usable < file_cap) break;
  }
  return done;
}

static int check_existing_metadata(PostInitSession *s);
static int write_metadata(PostInitSession *s);

int post_init_new(const PostInitConfig *cfg, PostInitSession **out) {
  if (!cfg || !out) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  if (cfg->scrypt_n < 2 || (cfg->scrypt_n & (cfg->scrypt_n - 1))) {
    set_error("scrypt N must be a power of two >= 2");
    return POST_ERR_INVALID_ARGS;
  }
  int rc = require_gpu(cfg->provider_id);
  if (rc != POST_OK) return rc;

  /* everything below must free the session on failure */
  struct Guard {
    PostInitSession *p;
    ~Guard() { delete p; }
  };
  auto *s = new PostInitSession();
  Guard guard{s};
  s->cfg = *cfg;
  if (cfg->data_dir) {
    s->data_dir = cfg->data_dir;
    /* create the data directory like the reference initializer does */
    std::string path;
    for (size_t i = 0; i <= s->data_dir.size(); i++) {
      if (i == s->data_dir.size() || s->data_dir[i] == '/') {
        path = s->data_dir.substr(0, i);
        if (!path.empty()) (void)::mkdir(path.c_str(), 0755);
      }
    }
    struct stat st;
    if (stat(s->data_dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) {
      set_error("cannot create data dir " + s->data_dir);
      return POST_ERR_IO;
    }
  }
  uint64_t total = (uint64_t)cfg->num_units * cfg->labels_per_unit;
  s->range_start = cfg->index_start;
  s->range_end = cfg->index_end ? cfg->index_end : total;
  if (s->range_end > total || s->range_start >= s->range_end) {
    set_error("bad index range");
    return POST_ERR_INVALID_ARGS;
  }
  poste::commitment(cfg->node_id, cfg->commitment_atx_id, s->commitment);

  /* scratch sizing: lanes * 128 * (N >> gap_shift) bytes */
  s->gap_shift = pick_gap_shift(cfg->scrypt_n);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  uint64_t budget = cfg->scratch_bytes
                        ? cfg->scratch_bytes
                        : (uint64_t)((double)free_b * 0.80);
  uint64_t per_lane = ((uint64_t)cfg->scrypt_n >> s->gap_shift) * 128;
  uint64_t lanes = budget / per_lane;
  uint64_t range = s->range_end - s->range_start;
  lanes = std::min<uint64_t>(lanes, std::max<uint64_t>(range, 64));
  /* scratch beyond the kernel's resident capacity is wasted: extra
   * workgroups only queue (grid-stride covers the batch regardless) */
  lanes = std::min<uint64_t>(lanes,
                             poste_label_resident_slots(s->gap_shift));
  /* keep the dual-stream grid block-aligned; the three-stream schedule
   * rounds its thirds to whole workgroups itself and needs whole
   * workgroups only */
  const char *const mx = getenv("POST_ROMIX_MIX");
  const bool want3 = !mx || !*mx || std::strcmp(mx, "free3") == 0;
  const uint64_t lane_round = want3 ? 64 : 128;
  lanes = (lanes / lane_round) * lane_round;
  if (lanes < 128) lanes = 128;
  if (lanes == 0) {
    set_error("not enough device memory for one scratch lane block");
    return POST_ERR_OOM;
  }
  s->lanes = lanes;
  s->batch = std::min<uint64_t>(range, lanes * 4);

  HIP_TRY(s->d_scratch.alloc((size_t)lanes * per_lane));
  uint64_t keep_bytes = range * POST_LABEL_SIZE;
  s->keep_all = s->data_dir.empty() && keep_bytes <= (8ull << 30);
  if (s->keep_all) {
    HIP_TRY(s->d_all.alloc((size_t)keep_bytes));
  }
  const size_t batch_bytes = (size_t)s->batch * POST_LABEL_SIZE;
  HIP_TRY(s->set[0].d_out.alloc(batch_bytes));
  /* The tail appends one candidate per workgroup per launch, whatever the
   * threshold.  The split path launches one tail per unit; units are whole
   * workgroups but for the last of a batch, so a batch appends at most
   * batch/64 plus one ragged workgroup — also when the threshold it was
   * given lags the host's by the batches in flight. */
  s->cand_cap =
      (uint32_t)std::max<uint64_t>(CAND_CAP, s->batch / 64 + 16);
  const size_t cand_bytes = sizeof(PostVrfCandidate) * s->cand_cap;
  HIP_TRY(s->set[0].d_cand.alloc(cand_bytes));
  /* at least one unit per stream of the split path: lanes tasks */
  HIP_TRY(s->d_xbuf.alloc((size_t)std::max<uint64_t>(s->batch, lanes) * 128));
  HIP_TRY(s->set[0].d_cand_count.alloc(sizeof(unsigned int)));
  HIP_TRY(s->set[0].h_batch.alloc(batch_bytes));
  HIP_TRY(s->stream.create());

  /* POST_ROMIX_MIX: unset or free3 = phase-mixed wherever the lean gap-1
   * kernel applies, three free-running streams over thirds of the slots
   * (two over halves below 192 slots); free2 = two free-running streams;
   * chain = two streams with the fill-behind-fill wait of the earlier
   * schedule (both A/B: profiles/r05_freerun.md); 0 = the monolithic
   * kernel on one stream (A/B, fallback); seq = the split kernels back to
   * back on one stream (measures the phases apart:
   * profiles/r04_romix_phases.md) */
  {
    const bool lean = poste_label_romix_lean_ok(cfg->scrypt_n, s->gap_shift,
                                                lanes) != 0;
    if (!lean || (mx && std::strcmp(mx, "0") == 0))
      s->split_streams = 0;
    else if (mx && std::strcmp(mx, "seq") == 0)
      s->split_streams = 1;
    else if (want3 && lanes >= 192)
      s->split_streams = 3;
    else
      s->split_streams = lanes >= 128 ? 2 : 0;
    s->split_chain =
        s->split_streams == 2 && mx && std::strcmp(mx, "chain") == 0;
  }
  if (s->split_streams) {
    if (!s->keep_all) HIP_TRY(s->set[1].d_out.alloc(batch_bytes));
    HIP_TRY(s->set[1].d_cand.alloc(cand_bytes));
    HIP_TRY(s->set[1].d_cand_count.alloc(sizeof(unsigned int)));
    HIP_TRY(s->set[1].h_batch.alloc(batch_bytes));
    for (OutputSet &o : s->set) {
      HIP_TRY(o.h_cand_count.alloc(sizeof(unsigned int)));
      HIP_TRY(o.h_cand.alloc(cand_bytes));
      HIP_TRY(o.ev_end.create());
      HIP_TRY(o.ev_done.create(hipEventDisableTiming));
      HIP_TRY(o.ev_reset.create(hipEventDisableTiming));
      for (int k = 0; k < s->split_streams; k++)
        HIP_TRY(o.ev_tail[k].create(hipEventDisableTiming));
    }
    if (s->split_chain)
      for (Event &e : s->ev_fill) HIP_TRY(e.create(hipEventDisableTiming));
    /* with the copy stream at most four streams: the hardware queues a
     * process gets by default */
    if (s->split_streams >= 2) HIP_TRY(s->stream_b.create());
    if (s->split_streams >= 3) HIP_TRY(s->stream_c.create());
    HIP_TRY(s->copy_stream.create());
  }

  if (!s->data_dir.empty()) {
    /* the dir is bound to one identity/config (verifyMetadata role) */
    rc = check_existing_metadata(s);
    if (rc != POST_OK) return rc;
    rc = write_metadata(s); /* persisted at session creation, like
                               initialization.SaveMetadata; rewritten with
                               the nonce at completion */
    if (rc != POST_OK) return rc;
    uint64_t per_file = std::max<uint64_t>(
        1, s->cfg.max_file_size / POST_LABEL_SIZE);
    s->written = existing_labels(s->data_dir, per_file, s->range_start, range);
  }
  guard.p = nullptr; /* ownership passes to the caller */
  *out = s;
  return POST_OK;
}

uint64_t post_init_num_labels_written(const PostInitSession *s) {
  return s ? s->written.load() : 0;
}

void post_init_cancel(PostInitSession *s) {
  if (s) s->cancel = true;
}

int post_init_nonce(const PostInitSession *s, uint64_t *index,
                    uint8_t label[32]) {
  auto *m = const_cast<PostInitSession *>(s);
  std::lock_guard<std::mutex> lk(m->nonce_mu);
  if (!s->nonce_found) return POST_ERR;
  *index = s->nonce_idx;
  std::memcpy(label, s->nonce_label, 32);
  return POST_OK;
}

static int write_batch_files(PostInitSession *s, uint64_t pos, uint64_t count,
                             const uint8_t *host_labels) {
  uint64_t per_file =
      std::max<uint64_t>(1, s->cfg.max_file_size / POST_LABEL_SIZE);
  uint64_t off = 0;
  while (off < count) {
    uint64_t gpos = pos + off;
    uint64_t file_i = gpos / per_file;
    uint64_t in_file = gpos % per_file;
    uint64_t take = std::min(per_file - in_file, count - off);
    char path[4096];
    std::snprintf(path, sizeof path, "%s/postdata_%llu.bin",
                  s->data_dir.c_str(), (unsigned long long)file_i);
    FILE *f = std::fopen(path, "r+b");
    if (!f) f = std::fopen(path, "w+b");
    if (!f) {
      set_error(std::string("cannot open ") + path);
      return POST_ERR_IO;
    }
    std::fseek(f, (long)(in_file * POST_LABEL_SIZE), SEEK_SET);
    size_t wr = std::fwrite(host_labels + off * POST_LABEL_SIZE,
                            POST_LABEL_SIZE, take, f);
    std::fclose(f);
    if (wr != take) {
      set_error("short write");
      return POST_ERR_IO;
    }
    off += take;
  }
  return POST_OK;
}

static void b64(const uint8_t *in, size_t n, std::string &out) {
  static const char t[] =
      "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  for (size_t i = 0; i < n; i += 3) {
    uint32_t v = (uint32_t)in[i] << 16;
    if (i + 1 < n) v |= (uint32_t)in[i + 1] << 8;
    if (i + 2 < n) v |= in[i + 2];
    out += t[(v >> 18) & 63];
    out += t[(v >> 12) & 63];
    out += i + 1 < n ? t[(v >> 6) & 63] : '=';
    out += i + 2 < n ? t[v & 63] : '=';
  }
}

static bool b64_decode(const std::string &in, uint8_t *out, size_t want) {
  static int8_t rev[256];
  static bool init = false;
  if (!init) {
    static const char t[] =
        "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    for (int i = 0; i < 256; i++) rev[i] = -1;
    for (int i = 0; i < 64; i++) rev[(uint8_t)t[i]] = (int8_t)i;
    init = true;
  }
  size_t n = 0;
  uint32_t acc = 0;
  int bits = 0;
  for (char c : in) {
    if (c == '=') break;
    int8_t v = rev[(uint8_t)c];
    if (v < 0) return false;
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      if (n >= want) return false;
      out[n++] = (uint8_t)(acc >> bits);
    }
  }
  return n == want;
}

/* Minimal reader for the fields write_metadata emits: enough to implement
 * the reference's metadata guard (initialization.LoadMetadata +
 * verifyMetadata semantics: a data dir is bound to one identity/config —
 * activation/post.go:373-435 reads the persisted commitment). */
static bool md_find_string(const std::string &j, const char *key,
                           std::string &out) {
  std::string pat = std::string("\"") + key + "\": \"";
  size_t p = j.find(pat);
  if (p == std::string::npos) return false;
  p += pat.size();
  size_t e = j.find('"', p);
  if (e == std::string::npos) return false;
  out = j.substr(p, e - p);
  return true;
}

static bool md_find_u64(const std::string &j, const char *key,
                        uint64_t &out) {
  std::string pat = std::string("\"") + key + "\": ";
  size_t p = j.find(pat);
  if (p == std::string::npos) return false;
  out = strtoull(j.c_str() + p + pat.size(), nullptr, 10);
  return true;
}

static int check_existing_metadata(PostInitSession *s) {
  char path[4096];
  std::snprintf(path, sizeof path, "%s/postdata_metadata.json",
                s->data_dir.c_str());
  FILE *f = std::fopen(path, "rb");
  if (!f) return POST_OK; /* fresh dir */
  std::string j;
  char buf[4096];
  size_t rd;
  while ((rd = std::fread(buf, 1, sizeof buf, f)) > 0) j.append(buf, rd);
  std::fclose(f);
  std::string nid_b64, atx_b64, want_nid, want_atx;
  b64(s->cfg.node_id, 32, want_nid);
  b64(s->cfg.commitment_atx_id, 32, want_atx);
  uint64_t lpu = 0, n = 0;
  if (md_find_string(j, "NodeId", nid_b64) && nid_b64 != want_nid) {
    set_error("data dir belongs to a different node id (postdata_metadata"
              ".json mismatch)");
    return POST_ERR_INVALID_ARGS;
  }
  if (md_find_string(j, "CommitmentAtxId", atx_b64) &&
      atx_b64 != want_atx) {
    set_error("data dir was initialized for a different commitment ATX");
    return POST_ERR_INVALID_ARGS;
  }
  if (md_find_u64(j, "LabelsPerUnit", lpu) &&
      lpu != s->cfg.labels_per_unit) {
    set_error("data dir was initialized with a different LabelsPerUnit");
    return POST_ERR_INVALID_ARGS;
  }
  if (md_find_u64(j, "N", n) && n != s->cfg.scrypt_n) {
    set_error("data dir was initialized with different scrypt params");
    return POST_ERR_INVALID_ARGS;
  }
  /* Resume must carry the persisted VRF nonce forward: the reference
   * initializer keeps metadata's Nonce/NonceValue across sessions, and a
   * sharded (index_start/end) session that loses its shard-local minimum
   * would corrupt the cross-GPU min-reduce after kill+resume.  Seed the
   * session's running minimum from the file before write_metadata (called
   * right after us) rewrites it. */
  uint64_t nonce_idx = 0;
  std::string nv_b64;
  if (md_find_u64(j, "Nonce", nonce_idx) &&
      md_find_string(j, "NonceValue", nv_b64)) {
    uint8_t label[32];
    if (!b64_decode(nv_b64, label, 32)) {
      set_error("postdata_metadata.json NonceValue is not 32 base64 bytes");
      return POST_ERR_INVALID_ARGS;
    }
    std::lock_guard<std::mutex> lk(s->nonce_mu);
    s->nonce_found = true;
    s->nonce_idx = nonce_idx;
    std::memcpy(s->nonce_label, label, 32);
  }
  return POST_OK;
}

static int write_metadata(PostInitSession *s) {
  /* postdata_metadata.json, field set per shared.PostMetadata usage
   * (activation/post_test.go:305-309; Go json base64 for byte slices) */
  std::string nid, atx, nv;
  b64(s->cfg.node_id, 32, nid);
  b64(s->cfg.commitment_atx_id, 32, atx);
  char path[4096];
  std::snprintf(path, sizeof path, "%s/postdata_metadata.json",
                s->data_dir.c_str());
  FILE *f = std::fopen(path, "w");
  if (!f) {
    set_error("cannot write metadata");
    return POST_ERR_IO;
  }
  std::fprintf(f,
               "{\n  \"NodeId\": \"%s\",\n  \"CommitmentAtxId\": \"%s\",\n"
               "  \"LabelsPerUnit\": %llu,\n  \"NumUnits\": %u,\n"
               "  \"MaxFileSize\": %llu,\n  \"Scrypt\": {\"N\": %u, \"R\": 1,"
               " \"P\": 1}",
               nid.c_str(), atx.c_str(),
               (unsigned long long)s->cfg.labels_per_unit, s->cfg.num_units,
               (unsigned long long)s->cfg.max_file_size, s->cfg.scrypt_n);
  std::lock_guard<std::mutex> lk(s->nonce_mu);
  if (s->nonce_found) {
    b64(s->nonce_label, 32, nv);
    std::fprintf(f, ",\n  \"Nonce\": %llu,\n  \"NonceValue\": \"%s\"",
                 (unsigned long long)s->nonce_idx, nv.c_str());
  }
  std::fprintf(f, "\n}\n");
  std::fclose(f);
  return POST_OK;
}

/* ------------------------- seal during init -------------------------
 *
 * DESIGN 3.7.  The session hashes every batch where the tail kernel left
 * it, with post_seal_stream_kernel, and appends the digests of the pages
 * that closed to postdata_seal.part-<index_start> once the batch's labels
 * are in the files.  All of it hangs off seal_on: a session that never
 * called post_init_enable_seal queues and waits for exactly what it did
 * before. */
static const char SEALP_MAGIC[8] = {'P', 'S', 'T', 'S', 'E', 'A', 'L', 'P'};
constexpr uint64_t SEALP_HEADER = 32;
constexpr uint64_t SEALP_PAGE = POSTE_SEAL_PAGE_LABELS;
constexpr uint64_t SEALP_DIGEST = 16;

static void put_le(uint8_t *p, uint64_t v, int bytes);
static uint64_t get_le(const uint8_t *p, int bytes);
static int seal_assemble(const char *data_dir, uint64_t *pages, bool quiet);

static std::string seal_part_path(const std::string &dir, uint64_t start) {
  return dir + "/postdata_seal.part-" + std::to_string(start);
}

/* pages of the session's range */
static uint64_t seal_range_pages(const PostInitSession *s) {
  return (s->range_end + SEALP_PAGE - 1) / SEALP_PAGE - s->seal_first_page;
}

/* Queue the stream kernel over the batch at relative position pos that lies
 * at d_labels, and the copy of its digests to the pinned buffer of `o`. */
static int seal_launch(PostInitSession *s, hipStream_t stream, OutputSet &o,
                       uint64_t pos, uint64_t count, const uint8_t *d_labels) {
  SealStreamArgs a;
  a.labels = (const uint4 *)d_labels;
  a.g0 = s->range_start + pos;
  a.count = count;
  a.stream_end = (uint64_t)s->cfg.num_units * s->cfg.labels_per_unit;
  a.carry_in = s->d_seal_carry.get() + (s->seal_launches & 1);
  a.carry_out = s->d_seal_carry.get() + ((s->seal_launches + 1) & 1);
  a.digests = o.d_seal_dig.get();
  if (o.ev_seal[0].get()) HIP_TRY(hipEventRecord(o.ev_seal[0].get(), stream));
  HIP_TRY(poste_launch_seal_stream_kernel(&a, stream));
  if (o.ev_seal[1].get()) HIP_TRY(hipEventRecord(o.ev_seal[1].get(), stream));
  s->seal_launches++;
  s->seal_pos = pos + count;
  const uint64_t lanes =
      (a.g0 + count - 1) / SEALP_PAGE - a.g0 / SEALP_PAGE + 1;
  HIP_TRY(hipMemcpyAsync(o.h_seal_dig.get(), o.d_seal_dig.get(),
                         lanes * SEALP_DIGEST, hipMemcpyDeviceToHost, stream));
  return POST_OK;
}

/* The batch's labels are in the files: append the digests of the pages that
 * closed in it.  The caller advances `written` only after this. */
static int seal_commit(PostInitSession *s, OutputSet &o, uint64_t pos,
                       uint64_t count) {
  const uint64_t g0 = s->range_start + pos, end = g0 + count;
  const uint64_t total = (uint64_t)s->cfg.num_units * s->cfg.labels_per_unit;
  const uint64_t p0 = g0 / SEALP_PAGE;
  const uint64_t lanes = (end - 1) / SEALP_PAGE - p0 + 1;
  const uint64_t closed =
      (end % SEALP_PAGE == 0 || end == total) ? lanes : lanes - 1;
  const size_t want = (size_t)(closed * SEALP_DIGEST);
  float ms = 0;
  if (o.ev_seal[0].get() &&
      hipEventElapsedTime(&ms, o.ev_seal[0].get(), o.ev_seal[1].get()) ==
          hipSuccess) {
    s->seal_ms += ms;
    s->seal_ms_max = std::max<double>(s->seal_ms_max, ms);
    s->seal_timed++;
  }
  const off_t at =
      (off_t)(SEALP_HEADER + (p0 - s->seal_first_page) * SEALP_DIGEST);
  size_t put = 0;
  while (put < want) {
    const ssize_t w =
        ::pwrite(s->seal_fd, o.h_seal_dig.get() + put, want - put, at + put);
    if (w <= 0) {
      if (w < 0 && errno == EINTR) continue;
      set_error("short write to " +
                seal_part_path(s->data_dir, s->range_start));
      return POST_ERR_IO;
    }
    put += (size_t)w;
  }
  /* the range is complete: assemble, unless other shards are still open */
  if (end == s->range_end) {
    (void)::close(s->seal_fd);
    s->seal_fd = -1;
    if (s->seal_timed)
      std::fprintf(stderr,
                   "seal: %llu batches of up to %llu labels, stream kernel "
                   "%.3f ms per batch (max %.3f ms, %.1f ms in all)\n",
                   (unsigned long long)s->seal_timed,
                   (unsigned long long)s->batch, s->seal_ms / s->seal_timed,
                   s->seal_ms_max, s->seal_ms);
    return seal_assemble(s->data_dir.c_str(), nullptr, true);
  }
  return POST_OK;
}

/* A call that failed may have left the device carry ahead of `written`
 * (the batch behind the failing one was already queued) or the part file
 * ahead of it.  Fall back to the page boundary, as a new session would. */
static int seal_resync(PostInitSession *s) {
  const uint64_t w = s->written.load();
  if (s->seal_pos == w || s->seal_fd < 0) return POST_OK;
  const uint64_t pos = w / SEALP_PAGE * SEALP_PAGE;
  if (::ftruncate(s->seal_fd,
                  (off_t)(SEALP_HEADER + pos / SEALP_PAGE * SEALP_DIGEST)) !=
      0) {
    set_error("cannot truncate " +
              seal_part_path(s->data_dir, s->range_start));
    return POST_ERR_IO;
  }
  s->written.store(pos);
  s->seal_pos = pos;
  return POST_OK;
}

int post_init_enable_seal(PostInitSession *s) {
  if (!s || s->data_dir.empty()) {
    set_error("seal during init needs a session with a data dir");
    return POST_ERR_INVALID_ARGS;
  }
  if (s->stepped) {
    set_error("post_init_enable_seal must be called before the first step");
    return POST_ERR_INVALID_ARGS;
  }
  if (s->seal_on) return POST_OK;
  const uint64_t total = (uint64_t)s->cfg.num_units * s->cfg.labels_per_unit;
  const uint64_t range = s->range_end - s->range_start;
  if (s->range_start % SEALP_PAGE != 0 ||
      (s->range_end % SEALP_PAGE != 0 && s->range_end != total)) {
    set_error("seal during init needs a range of whole 1024-label pages: "
              "index_start a multiple of 1024, index_end a multiple of 1024 "
              "or the end of the label space");
    return POST_ERR_UNSUPPORTED;
  }
  if (s->cfg.max_file_size % POST_LABEL_SIZE != 0) {
    set_error("seal during init needs a MaxFileSize that is a multiple of "
              "16: pages are in terms of the label stream");
    return POST_ERR_UNSUPPORTED;
  }
  const std::string part = seal_part_path(s->data_dir, s->range_start);
  const std::string sidecar = s->data_dir + "/postdata_seal.bin";
  struct stat st;
  const bool have_part = ::stat(part.c_str(), &st) == 0;
  const uint64_t part_size = have_part ? (uint64_t)st.st_size : 0;
  const bool have_sidecar = ::stat(sidecar.c_str(), &st) == 0;
  const uint64_t on_disk = s->written.load();
  if (!have_part && on_disk > 0) {
    if (have_sidecar && on_disk == range) return POST_OK; /* all done */
    set_error(have_sidecar
                  ? "postdata_seal.bin is finished but the labels of this "
                    "range are not; finish init without a seal and run `seal`"
                  : "dir was started without a seal; finish init and run "
                    "`seal`");
    return POST_ERR_UNSUPPORTED;
  }

  s->seal_first_page = s->range_start / SEALP_PAGE;
  const uint64_t end_page = (s->range_end + SEALP_PAGE - 1) / SEALP_PAGE;
  uint8_t hdr[SEALP_HEADER] = {0};
  std::memcpy(hdr, SEALP_MAGIC, 8);
  put_le(hdr + 8, SEALP_PAGE, 4);
  put_le(hdr + 12, SEALP_DIGEST, 4);
  put_le(hdr + 16, s->seal_first_page, 8);
  put_le(hdr + 24, end_page, 8);
  uint64_t resume = 0;
  if (s->seal_fd >= 0) (void)::close(s->seal_fd); /* an earlier failed call */
  s->seal_fd = ::open(part.c_str(), O_RDWR | O_CREAT, 0644);
  if (s->seal_fd < 0) {
    set_error("cannot open " + part);
    return POST_ERR_IO;
  }
  if (have_part) {
    uint8_t got[SEALP_HEADER];
    if (part_size < SEALP_HEADER ||
        ::pread(s->seal_fd, got, SEALP_HEADER, 0) != (ssize_t)SEALP_HEADER ||
        std::memcmp(got, hdr, SEALP_HEADER) != 0) {
      set_error(part + " has a header that disagrees with the session");
      (void)::close(s->seal_fd);
      s->seal_fd = -1;
      return POST_ERR_IO;
    }
    const uint64_t pages_done = (part_size - SEALP_HEADER) / SEALP_DIGEST;
    if (on_disk == range && pages_done >= seal_range_pages(s))
      resume = range; /* complete; only the assembly may be missing */
    else
      resume = std::min(on_disk / SEALP_PAGE * SEALP_PAGE,
                        std::min(pages_done, seal_range_pages(s)) * SEALP_PAGE);
  } else if (::pwrite(s->seal_fd, hdr, SEALP_HEADER, 0) !=
             (ssize_t)SEALP_HEADER) {
    set_error("cannot write " + part);
    return POST_ERR_IO;
  }
  const uint64_t keep = resume == range ? seal_range_pages(s)
                                        : resume / SEALP_PAGE;
  if (::ftruncate(s->seal_fd, (off_t)(SEALP_HEADER + keep * SEALP_DIGEST)) !=
      0) {
    set_error("cannot truncate " + part);
    return POST_ERR_IO;
  }
  s->written.store(resume);
  s->seal_pos = resume;
  if (resume == range) {
    (void)::close(s->seal_fd);
    s->seal_fd = -1;
    return seal_assemble(s->data_dir.c_str(), nullptr, true);
  }

  int rc = require_gpu(s->cfg.provider_id);
  if (rc != POST_OK) return rc;
  /* a batch touches at most batch / 1024 + 2 pages */
  const size_t dig_bytes = (size_t)((s->batch / SEALP_PAGE + 2) * SEALP_DIGEST);
  HIP_TRY(s->d_seal_carry.alloc(2 * sizeof(SealCarry)));
  HIP_TRY(hipMemset(s->d_seal_carry.get(), 0, 2 * sizeof(SealCarry)));
  for (int i = 0; i < (s->split_streams ? 2 : 1); i++) {
    OutputSet &o = s->set[i];
    HIP_TRY(o.d_seal_dig.alloc(dig_bytes));
    HIP_TRY(o.h_seal_dig.alloc(dig_bytes));
    if (getenv("POST_SEAL_DEBUG"))
      for (Event &e : o.ev_seal) HIP_TRY(e.create());
  }
  s->seal_on = true;
  return POST_OK;
}

/* ------------------- initial proof during init -------------------
 *
 * DESIGN 3.8.  The session runs the proving scan over every batch where the
 * tail kernel left it and appends the hits to postdata_hits.part-<index_start>
 * (format, parser and resume: init_proof_host.h) once the batch's labels are
 * in the files.  All of it hangs off proof_on: a session that never called
 * post_init_enable_proof queues and waits for exactly what it did before. */

/* records of a batch the host gets with the count, in front of ev_done (16
 * KiB): a mainnet batch expects about 0.2 hits, so more is fetched next to
 * never.  Fetching more is a blocking copy behind everything queued, the next
 * batch included, so it empties the pipeline once: at 64 records a 2^24-label
 * space with 288 nonces (234 hits a batch) paid that on every batch, 4 % of
 * the run (profiles/init_proof.md). */
constexpr uint32_t PROOF_HIT_WINDOW = 1024;
constexpr uint64_t PROOF_HIT_CAP_MIN = 4096, PROOF_HIT_CAP_MAX = 1u << 16;

/* device records per batch: 16 times the expectation, within the bounds */
static uint32_t proof_hit_capacity(uint64_t batch, uint32_t nonces,
                                   uint32_t k1, uint64_t total) {
  const unsigned __int128 num = (unsigned __int128)batch * nonces * k1;
  const unsigned __int128 expect = (num + total - 1) / total;
  const unsigned __int128 want = expect * 16;
  if (want < PROOF_HIT_CAP_MIN) return (uint32_t)PROOF_HIT_CAP_MIN;
  if (want > PROOF_HIT_CAP_MAX) return (uint32_t)PROOF_HIT_CAP_MAX;
  return (uint32_t)want;
}

/* Queue, on `stream`, the scan of the batch at relative position pos that
 * lies at d_labels: the set's count zeroed in front of it. */
static int proof_launch(PostInitSession *s, hipStream_t stream, OutputSet &o,
                        uint64_t pos, uint64_t count,
                        const uint8_t *d_labels) {
  ScanKernelArgs a = s->proof_scan;
  a.labels = (const uint4 *)d_labels;
  a.count = count;
  a.index_base = s->range_start + pos; /* global: the parts merge as they are */
  a.hits = o.d_hits.get();
  a.hit_count = o.d_hit_count.get();
  a.hit_cap = s->proof_hit_cap;
  HIP_TRY(hipMemsetAsync(o.d_hit_count.get(), 0, sizeof(unsigned int), stream));
  if (o.ev_scan[0].get()) HIP_TRY(hipEventRecord(o.ev_scan[0].get(), stream));
  HIP_TRY(poste_launch_scan(&a, &s->proof_plan, stream));
  if (o.ev_scan[1].get()) HIP_TRY(hipEventRecord(o.ev_scan[1].get(), stream));
  return POST_OK;
}

/* the count and the first records, with the batch's other small copies */
static int proof_queue_fetch(PostInitSession *s, hipStream_t stream,
                             OutputSet &o) {
  HIP_TRY(hipMemcpyAsync(o.h_hit_count.get(), o.d_hit_count.get(),
                         sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(
      o.h_hits.get(), o.d_hits.get(),
      sizeof(PostScanHit) * std::min(PROOF_HIT_WINDOW, s->proof_hit_cap),
      hipMemcpyDeviceToHost, stream));
  return POST_OK;
}

/* The batch has arrived: its hits, sorted by (index, nonce).  More than the
 * window is fetched here, the one case in which the host goes to the device
 * a second time for a batch.  A count above the capacity fails the step
 * before anything of the batch is persisted. */
static int proof_collect(PostInitSession *s, OutputSet &o, uint64_t pos,
                         uint64_t count, std::vector<PostScanHit> &hits) {
  const unsigned int n = *o.h_hit_count.get();
  float ms = 0;
  if (o.ev_scan[0].get() &&
      hipEventElapsedTime(&ms, o.ev_scan[0].get(), o.ev_scan[1].get()) ==
          hipSuccess) {
    s->proof_ms += ms;
    s->proof_ms_max = std::max<double>(s->proof_ms_max, ms);
    s->proof_timed++;
  }
  if (n > s->proof_hit_cap) {
    set_error("scan hit buffer overflow in the init batch [" +
              std::to_string(s->range_start + pos) + ", " +
              std::to_string(s->range_start + pos + count) + "): " +
              std::to_string(n) + " hits, room for " +
              std::to_string(s->proof_hit_cap) +
              " (pathological K1/num_labels configuration); nothing of the "
              "batch was appended and labels written stays at " +
              std::to_string(s->written.load()));
    return POST_ERR;
  }
  hits.resize(n);
  const unsigned int head = std::min(n, PROOF_HIT_WINDOW);
  if (head) std::memcpy(hits.data(), o.h_hits.get(), sizeof(PostScanHit) * head);
  if (n > head) {
    HIP_TRY(hipMemcpy(hits.data() + head, o.d_hits.get() + head,
                      sizeof(PostScanHit) * (n - head),
                      hipMemcpyDeviceToHost));
    s->proof_refetch++;
  }
  std::sort(hits.begin(), hits.end(),
            [](const PostScanHit &a, const PostScanHit &b) {
              return a.index != b.index ? a.index < b.index
                                        : a.nonce < b.nonce;
            });
  return POST_OK;
}

/* The batch's labels are in the files: append its hits and one marker.  The
 * caller advances `written` only after this. */
static int proof_commit(PostInitSession *s, uint64_t pos, uint64_t count,
                        const std::vector<PostScanHit> &hits) {
  std::vector<uint8_t> rec((hits.size() + 1) * initproof::RECORD_BYTES);
  for (size_t i = 0; i < hits.size(); i++)
    initproof::pack_record(hits[i].index, hits[i].nonce, 0,
                           rec.data() + i * initproof::RECORD_BYTES);
  initproof::pack_record(s->range_start + pos + count, initproof::MARK_NONCE,
                         initproof::MARK_TAG,
                         rec.data() + hits.size() * initproof::RECORD_BYTES);
  s->proof_pos = UINT64_MAX; /* a failure below leaves the part to a resync */
  if (!initproof::write_at(s->proof_fd, rec.data(), rec.size(),
                           s->proof_bytes)) {
    set_error("short write to " +
              initproof::part_path(s->data_dir, s->range_start));
    return POST_ERR_IO;
  }
  s->proof_bytes += rec.size();
  s->proof_pos = pos + count;
  s->proof_hits += hits.size();
  if (s->range_start + pos + count == s->range_end) {
    (void)::close(s->proof_fd);
    s->proof_fd = -1;
    if (s->proof_timed)
      std::fprintf(stderr,
                   "init proof: %llu batches of up to %llu labels, scan (%s) "
                   "%.3f ms per batch (max %.3f ms, %.1f ms in all), %llu "
                   "hits, %llu batches fetched past the window\n",
                   (unsigned long long)s->proof_timed,
                   (unsigned long long)s->batch,
                   poste_scan_variant_name(s->proof_plan.variant),
                   s->proof_ms / s->proof_timed, s->proof_ms_max, s->proof_ms,
                   (unsigned long long)s->proof_hits,
                   (unsigned long long)s->proof_refetch);
  }
  return POST_OK;
}

/* Part and `written` brought to one point, as a new session would: the
 * lower of `written` and the part's last well-formed marker, the part cut
 * there.  Nothing to do while they agree. */
static int proof_resync(PostInitSession *s) {
  const uint64_t w = s->written.load();
  if (s->proof_pos == w || s->proof_fd < 0) return POST_OK;
  uint64_t point = s->range_start + w;
  std::string err;
  const int rc = initproof::sync_part(s->proof_fd, s->proof_hdr, &point,
                                      &s->proof_bytes, err);
  if (rc != POST_OK) {
    set_error(err + ": " + initproof::part_path(s->data_dir, s->range_start));
    return rc;
  }
  s->proof_pos = point - s->range_start;
  s->written.store(s->proof_pos);
  return POST_OK;
}

int post_init_enable_proof(PostInitSession *s, const PostProveConfig *cfg) {
  if (!s || !cfg || s->data_dir.empty()) {
    set_error("initial proof during init needs a session with a data dir and "
              "a proving config");
    return POST_ERR_INVALID_ARGS;
  }
  if (s->stepped) {
    set_error("post_init_enable_proof must be called before the first step");
    return POST_ERR_INVALID_ARGS;
  }
  if (cfg->nonces == 0 || cfg->nonces % POSTE_NONCE_GROUP != 0) {
    set_error("nonces must be a positive multiple of 16");
    return POST_ERR_INVALID_ARGS;
  }
  if (cfg->pow_mode != POST_POW_MODE_BLAKE3) {
    set_error("initial proof during init: RandomX k2pow is not supported by "
              "this engine (use POST_POW_MODE_BLAKE3)");
    return POST_ERR_UNSUPPORTED;
  }
  const uint64_t total = (uint64_t)s->cfg.num_units * s->cfg.labels_per_unit;
  const uint64_t range = s->range_end - s->range_start;
  initproof::Header h;
  h.nonces = cfg->nonces;
  h.k1 = cfg->k1;
  h.k2 = cfg->k2;
  std::memcpy(h.challenge, cfg->challenge, 32);
  std::memcpy(h.pow_difficulty, cfg->pow_difficulty, 32);
  h.index_start = s->range_start;
  h.index_end = s->range_end;
  h.total_labels = total;
  uint8_t hdr[initproof::HEADER_BYTES];
  initproof::pack_header(h, hdr);
  if (s->proof_on) {
    /* a second call: fine with the config in force, refused with another */
    uint8_t have[initproof::HEADER_BYTES];
    initproof::pack_header(s->proof_hdr, have);
    if (std::memcmp(have, hdr, sizeof hdr) == 0) return POST_OK;
    set_error("the initial proof is already enabled with another proving "
              "config");
    return POST_ERR_INVALID_ARGS;
  }
  const std::string part = initproof::part_path(s->data_dir, s->range_start);
  struct stat st;
  const bool have_part = ::stat(part.c_str(), &st) == 0;
  if (!have_part && s->written.load() > 0) {
    set_error("dir was started without the proof scan; finish init and run "
              "prove");
    return POST_ERR_UNSUPPORTED;
  }
  /* POST_INIT_PROOF_SCAN picks the variant, once: bankrep (default) or tt4.
   * Judged before the dir is touched. */
  const char *mode = getenv("POST_INIT_PROOF_SCAN");
  if (!mode || !*mode) mode = "bankrep";
  if (std::strcmp(mode, "tt4") != 0 && std::strcmp(mode, "bankrep") != 0) {
    set_error("POST_INIT_PROOF_SCAN must be bankrep or tt4");
    return POST_ERR_INVALID_ARGS;
  }
  s->proof_hdr = h;
  if (s->proof_fd >= 0) (void)::close(s->proof_fd); /* an earlier failed call */
  s->proof_fd = ::open(part.c_str(), O_RDWR | O_CREAT, 0644);
  if (s->proof_fd < 0) {
    set_error("cannot open " + part);
    return POST_ERR_IO;
  }
  /* a call that fails leaves the dir as it found it: a part it created
   * would otherwise make a later session take a dir that went on without the
   * scan for one that had it */
  auto drop = [s, have_part, &part](int rc) {
    (void)::close(s->proof_fd);
    s->proof_fd = -1;
    if (!have_part) (void)::unlink(part.c_str());
    return rc;
  };
  if (have_part) {
    uint8_t got[initproof::HEADER_BYTES];
    if ((uint64_t)st.st_size < initproof::HEADER_BYTES ||
        ::pread(s->proof_fd, got, sizeof got, 0) != (ssize_t)sizeof got ||
        std::memcmp(got, hdr, sizeof got) != 0) {
      set_error(part + " has a header that disagrees with the session or "
                       "with the proving config");
      return drop(POST_ERR_IO);
    }
  } else if (!initproof::write_at(s->proof_fd, hdr, sizeof hdr, 0)) {
    set_error("cannot write " + part);
    return drop(POST_ERR_IO);
  }
  /* the resume point: labels on disk (and the seal's, which `written`
   * already holds) against the part's last marker */
  s->proof_pos = UINT64_MAX;
  int rc = proof_resync(s);
  if (rc != POST_OK) return drop(rc);
  if (s->seal_on) {
    /* the seal continues from a page boundary only */
    rc = seal_resync(s);
    if (rc == POST_OK) rc = proof_resync(s);
    if (rc != POST_OK) return drop(rc);
  }
  if (s->written.load() == range) {
    /* complete; nothing left to scan */
    (void)::close(s->proof_fd);
    s->proof_fd = -1;
    return POST_OK;
  }

  rc = require_gpu(s->cfg.provider_id);
  if (rc != POST_OK) return drop(rc);
  DeviceTables tbl;
  rc = get_aes_tables((int)s->cfg.provider_id, tbl);
  if (rc != POST_OK) return drop(rc);
  /* POST_SCAN_MAX_BLOCKS lowers the grid cap as on the prove path; no
   * fallback: a tt4 that cannot run here is an error */
  {
    const hipError_t e = poste_scan_plan(mode, getenv("POST_SCAN_MAX_BLOCKS"),
                                         0, &s->proof_plan);
    if (e != hipSuccess) return drop(hip_fail("poste_scan_plan", e));
  }
  s->proof_hit_cap =
      proof_hit_capacity(s->batch, cfg->nonces, cfg->k1, total);

  const uint32_t n_ciphers = cfg->nonces / POSTE_NONCES_PER_AES;
  std::vector<uint32_t> rk((size_t)n_ciphers * 44);
  {
    std::vector<uint64_t> group_pow(cfg->nonces / POSTE_NONCE_GROUP);
    for (uint32_t g = 0; g < group_pow.size(); g++)
      group_pow[g] = poste::k2pow_search_blake3(
          cfg->challenge, g, cfg->pow_difficulty, cfg->pow_threads);
    for (uint32_t c = 0; c < n_ciphers; c++) {
      uint8_t key[16];
      const uint32_t grp = (c * POSTE_NONCES_PER_AES) / POSTE_NONCE_GROUP;
      poste::prove_cipher_key(cfg->challenge, c, group_pow[grp], key);
      poste::aes128_expand(key, rk.data() + (size_t)c * 44);
    }
  }
  auto hip_drop = [&drop](const char *what, hipError_t e) {
    return drop(hip_fail(what, e));
  };
  hipError_t e = s->d_proof_rk.alloc(rk.size() * 4);
  if (e == hipSuccess)
    e = hipMemcpy(s->d_proof_rk.get(), rk.data(), rk.size() * 4,
                  hipMemcpyHostToDevice);
  const bool debug = getenv("POST_INIT_PROOF_DEBUG") != nullptr;
  for (int i = 0; i < (s->split_streams ? 2 : 1) && e == hipSuccess; i++) {
    OutputSet &o = s->set[i];
    e = o.d_hits.alloc(sizeof(PostScanHit) * s->proof_hit_cap);
    if (e == hipSuccess) e = o.d_hit_count.alloc(sizeof(unsigned int));
    if (e == hipSuccess)
      e = o.h_hits.alloc(sizeof(PostScanHit) * PROOF_HIT_WINDOW);
    if (e == hipSuccess) e = o.h_hit_count.alloc(sizeof(unsigned int));
    for (Event &ev : o.ev_scan)
      if (debug && e == hipSuccess) e = ev.create();
  }
  if (e != hipSuccess) return hip_drop("initial proof buffers", e);
  std::memset(&s->proof_scan, 0, sizeof(s->proof_scan));
  s->proof_scan.te = tbl.d_te;
  s->proof_scan.sbox = tbl.d_sbox;
  s->proof_scan.rk = s->d_proof_rk.get();
  s->proof_scan.n_ciphers = n_ciphers;
  s->proof_scan.difficulty = poste::proving_difficulty(cfg->k1, total);
  s->proof_on = true;
  return POST_OK;
}

/* ------------------- host half of an init batch -------------------
 *
 * Shared by the monolithic step, the split step and the nonce search past
 * the end (nonce_only_batch), so the three cannot drift apart. */

/* the LabelKernelArgs fields common to every launch of a session */
static LabelKernelArgs init_label_args(const PostInitSession *s) {
  LabelKernelArgs args;
  std::memset(&args, 0, sizeof(args));
  load_commitment_words(s->commitment, args.commitment_le);
  args.scrypt_n = s->cfg.scrypt_n;
  args.gap_shift = s->gap_shift;
  args.scratch = s->d_scratch.get();
  args.scratch_lanes = s->lanes;
  args.has_difficulty = 1;
  args.cand_cap = s->cand_cap;
  return args;
}

/* the threshold a call starts from: the session's minimum, or all ones */
static void load_running_minimum(PostInitSession *s, uint8_t cur[32]) {
  std::memset(cur, 0xff, 32); /* track the global minimum */
  std::lock_guard<std::mutex> lk(s->nonce_mu);
  if (s->nonce_found) std::memcpy(cur, s->nonce_label, 32);
}

/* Merge n device candidates into the session's running minimum, of which
 * cur_difficulty is the caller's copy: lower label wins, a tie goes to the
 * lower index.  Returns whether the minimum improved. */
static bool merge_candidates(PostInitSession *s, const PostVrfCandidate *cands,
                             unsigned int n, uint8_t cur_difficulty[32]) {
  bool improved = false;
  std::lock_guard<std::mutex> lk(s->nonce_mu);
  for (unsigned int i = 0; i < n; i++) {
    uint8_t lab[32];
    for (int k = 0; k < 8; k++) {
      uint32_t w = cands[i].label_be[k];
      lab[4 * k] = (uint8_t)(w >> 24);
      lab[4 * k + 1] = (uint8_t)(w >> 16);
      lab[4 * k + 2] = (uint8_t)(w >> 8);
      lab[4 * k + 3] = (uint8_t)w;
    }
    int c = std::memcmp(lab, cur_difficulty, 32);
    if (!s->nonce_found || c < 0 ||
        (c == 0 && cands[i].index < s->nonce_idx)) {
      s->nonce_found = true;
      s->nonce_idx = cands[i].index;
      std::memcpy(s->nonce_label, lab, 32);
      std::memcpy(cur_difficulty, lab, 32);
      improved = true;
    }
  }
  return improved;
}

/* Reference-label self-check (ErrReferenceLabelMismatch semantics,
 * activation/post.go:299-312), one object per post_init_step call.  begin()
 * is called once a batch is queued and before the host waits for it: the
 * reference label computes on the host WHILE the kernel runs (a ~5 ms scrypt
 * that would otherwise sit on the critical path between launches).
 * POST_SELFCHECK_PERIOD=k checks every k-th batch instead — with 8 ranks per
 * node the per-rank host scrypt otherwise contends for the same host cores
 * (SCALE readiness); detection latency rises k batches,
 * coverage semantics are unchanged.  finish_batch compares. */
struct SelfCheck {
  uint64_t period = 1;
  bool on = false;    /* this batch is checked */
  uint64_t probe = 0; /* label of the batch that is compared */
  int ref_rc = 0;
  uint8_t ref[32];

  SelfCheck() {
    const char *env = getenv("POST_SELFCHECK_PERIOD");
    const long v = env ? strtol(env, nullptr, 10) : 1;
    if (v > 1) period = (uint64_t)v;
  }
  void begin(PostInitSession *s, uint64_t pos, uint64_t count) {
    on = (s->batch_seq++ % period) == 0;
    probe = count / 2;
    ref_rc = on ? poste::host_label(s->commitment,
                                    s->range_start + pos + probe,
                                    s->cfg.scrypt_n, ref)
                : 0;
  }
};

/* The batch at relative position pos has arrived in `o` and its candidates
 * are merged: check it, persist it, count it. */
static int finish_batch(PostInitSession *s, OutputSet &o, const SelfCheck &sc,
                        uint64_t pos, uint64_t count, bool nonce_improved,
                        const std::vector<PostScanHit> &hits, uint64_t *done) {
  int rc;
  /* persist an improved running minimum immediately: metadata is the
   * only carrier of the shard-local minimum across kill+resume (the
   * creation-time write has no nonce yet, and a completed-at-exit-only
   * write loses it on any interrupt — the cfg4 soak caught exactly
   * that).  Improvements are rare (~log of batches), so this is a few
   * small rewrites per session. */
  if (nonce_improved && !s->data_dir.empty()) {
    rc = write_metadata(s);
    if (rc != POST_OK) return rc;
  }
  if (sc.ref_rc != 0) {
    set_error("host reference label failed");
    return POST_ERR;
  }
  if (sc.on && std::memcmp(sc.ref, o.h_batch.get() + sc.probe * POST_LABEL_SIZE,
                           POST_LABEL_SIZE) != 0) {
    set_error("reference label mismatch: device labels diverge from the "
              "host reference (ErrReferenceLabelMismatch)");
    return POST_ERR;
  }
  if (!s->data_dir.empty()) {
    rc = write_batch_files(s, s->range_start + pos, count, o.h_batch.get());
    if (rc != POST_OK) return rc;
  }
  /* digests only behind their labels (a seal needs a data dir) */
  if (s->seal_on) {
    rc = seal_commit(s, o, pos, count);
    if (rc != POST_OK) return rc;
  }
  /* hits only behind their labels, the marker behind the hits */
  if (s->proof_on) {
    rc = proof_commit(s, pos, count, hits);
    if (rc != POST_OK) return rc;
  }
  s->written.store(pos + count);
  *done += count;
  return POST_OK;
}

/* Init step on the split ROMix kernels (lean gap-1 geometry only).
 *
 * The slots are divided among split_streams streams (two halves when
 * phase-mixed, thirds rounded down to whole workgroups with free3), and
 * `xbuf` alike.  Work is issued in units of at most one such share:
 * prologue -> fill -> mix -> tail, units going round the streams.  Each
 * stream runs its own chain over its own slots and no ROMix kernel waits
 * for another stream: a stream's next fill starts when its previous tail
 * ends, beside whatever the others run (any mixture of fills and mixes),
 * so the chip stays full for the whole call.  Stream order alone protects a
 * slot column (a mix follows its own fill, the next fill its own mix).
 * What streams share is ordered by events, each stated where it is
 * enforced: the batch's candidate count (ev_reset), the outputs the copy
 * stream reads (ev_tail), and the output sets the host hands back
 * (ev_done).  POST_ROMIX_MIX=chain keeps the earlier schedule for A/B: the
 * fill of unit u waits for the fill of unit u-1 on the other stream, which
 * held the streams one phase apart and left the chip half empty while the
 * longer fill finished (profiles/r05_freerun.md).
 *
 * Batches (s->batch labels, as on the monolithic path) only group what the
 * host reads.  Their outputs are double-buffered and copied by
 * copy_stream, so the host merges candidates, self-checks and writes batch
 * i while batch i+1 runs; units are issued across batch boundaries without
 * a drain.  The pipeline drains at the end of the call, on cancel and on
 * error.  The threshold a tail is given lags the host's by the batch in
 * flight; the host merge compares exactly, so the nonce is the same. */
static int init_step_split(PostInitSession *s, SelfCheck &sc,
                           uint64_t max_labels, uint64_t *done) {
  const int ns = s->split_streams;
  /* slots per unit: one stream's share, whole 64-quad workgroups */
  const uint64_t unit = s->lanes / (uint64_t)ns / 64 * 64;
  hipStream_t st[3] = {s->stream.get(), s->stream_b.get(), s->stream_c.get()};
  const hipStream_t copy_stream = s->copy_stream.get();

  LabelKernelArgs args = init_label_args(s);
  RomixPhaseArgs ph;
  std::memset(&ph, 0, sizeof(ph));
  ph.scratch = s->d_scratch.get();
  ph.scratch_lanes = s->lanes;
  ph.slot_count = unit;
  ph.scrypt_n = s->cfg.scrypt_n;

  uint8_t cur_difficulty[32];
  load_running_minimum(s, cur_difficulty);

  if (!s->ev0.get()) HIP_TRY(s->ev0.create());
  const hipEvent_t ev0 = s->ev0.get();
  s->last_kernel_ms = 0;

  struct Batch {
    uint64_t pos = 0, count = 0;
    uint32_t max_cand = 0; /* workgroups of this batch's tails */
    int set = 0;
    bool live = false;
  };
  uint64_t issued = 0; /* units issued in this call */
  int last_set = -1;

  /* queue one batch: its units on the compute streams, its copies on
   * copy_stream behind the last tail of each stream */
  auto issue = [&](Batch &b) -> int {
    /* Output set b.set was last used by the batch two before this one.
     * The host has passed hipEventSynchronize(ev_done) of that batch
     * (process() runs before the next issue()), and ev_done follows every
     * tail and every copy of it, so its buffers, its count and its events
     * (ev_tail, ev_reset, ev_end, ev_done) are free to use again on any
     * stream.  Sets and the stream cursor carry on across calls; a call
     * ends drained, so the first batch of a call may start on any stream. */
    b.set = (int)(s->split_batch_no++ & 1);
    b.max_cand = 0;
    OutputSet &o = s->set[b.set];
    uint8_t *out = s->keep_all ? s->d_all.get() + b.pos * POST_LABEL_SIZE
                               : o.d_out.get();
    args.cand = o.d_cand.get();
    args.cand_count = o.d_cand_count.get();
    difficulty_to_be_words(cur_difficulty, args.difficulty_be);
    /* The batch's candidate count is zeroed on the stream of its first
     * unit, whose tails follow in stream order.  Every other stream's
     * tails append to the same count and nothing else orders them behind
     * the reset (this stream may still be busy with the batch before), so
     * each of them waits for ev_reset before its first tail of the batch. */
    const int k0 = (int)(s->unit_cursor % (uint64_t)ns);
    HIP_TRY(hipMemsetAsync(o.d_cand_count.get(), 0, sizeof(unsigned int),
                           st[k0]));
    if (ns > 1) HIP_TRY(hipEventRecord(o.ev_reset.get(), st[k0]));
    /* units of equal size, whole workgroups: a ragged batch costs every
     * unit a few labels, not one more round for a handful of them */
    const uint64_t nunits = (b.count + unit - 1) / unit;
    const uint64_t per = ((b.count + nunits - 1) / nunits + 63) / 64 * 64;
    bool used[3] = {false, false, false};
    for (uint64_t off = 0; off < b.count; off += per) {
      const int k = (int)(s->unit_cursor % (uint64_t)ns);
      const uint64_t c = std::min(per, b.count - off);
      const uint32_t blocks = (uint32_t)((c + 63) / 64);
      args.start = s->range_start + b.pos + off;
      args.count = c;
      /* stream k owns slots and xbuf tasks [k * unit, (k + 1) * unit) */
      args.xbuf = s->d_xbuf.get() + (uint64_t)k * unit * 32; /* 128 B a task */
      args.out = out + off * POST_LABEL_SIZE;
      ph.xbuf = args.xbuf;
      ph.slot_base = (uint64_t)k * unit;
      ph.count = c;
      /* the streams are idle when a call begins and this unit is queued
       * first, so ev0 marks the start of the call's first kernel */
      if (issued == 0) HIP_TRY(hipEventRecord(ev0, st[k]));
      HIP_TRY(poste_launch_label_prologue(&args, blocks, st[k]));
      if (s->split_chain && issued > 0)
        HIP_TRY(hipStreamWaitEvent(
            st[k], s->ev_fill[(s->unit_cursor - 1) & 3].get(), 0));
      HIP_TRY(poste_launch_romix_fill(&ph, st[k]));
      if (s->split_chain)
        HIP_TRY(hipEventRecord(s->ev_fill[s->unit_cursor & 3].get(), st[k]));
      HIP_TRY(poste_launch_romix_mix(&ph, st[k]));
      if (k != k0 && !used[k])
        HIP_TRY(hipStreamWaitEvent(st[k], o.ev_reset.get(), 0));
      HIP_TRY(poste_launch_label_tail(&args, blocks, st[k]));
      b.max_cand += blocks;
      used[k] = true;
      s->unit_cursor++;
      issued++;
    }
    /* The copy stream reads the batch behind the last tail of every stream
     * that had a unit of it.  It is in order, so ev_end, recorded once
     * those waits are queued, also follows the tails of every earlier
     * batch: with ev0 it brackets the call whichever streams ran the first
     * and the last unit. */
    for (int k = 0; k < ns; k++) {
      if (!used[k]) continue;
      HIP_TRY(hipEventRecord(o.ev_tail[k].get(), st[k]));
      HIP_TRY(hipStreamWaitEvent(copy_stream, o.ev_tail[k].get(), 0));
    }
    HIP_TRY(hipEventRecord(o.ev_end.get(), copy_stream));
    /* the seal of the batch: behind every tail of it like the copies, and
     * behind the seal of the batch before, which left the carry */
    if (s->seal_on) {
      const int rc = seal_launch(s, copy_stream, o, b.pos, b.count, out);
      if (rc != POST_OK) return rc;
    }
    /* the proving scan of the batch, at the same point: it reads what the
     * tails wrote and nothing else of the batch */
    if (s->proof_on) {
      const int rc = proof_launch(s, copy_stream, o, b.pos, b.count, out);
      if (rc != POST_OK) return rc;
    }
    HIP_TRY(hipMemcpyAsync(o.h_batch.get(), out, b.count * POST_LABEL_SIZE,
                           hipMemcpyDeviceToHost, copy_stream));
    HIP_TRY(hipMemcpyAsync(o.h_cand_count.get(), o.d_cand_count.get(),
                           sizeof(unsigned int), hipMemcpyDeviceToHost,
                           copy_stream));
    /* every candidate the batch can have appended, so nothing is fetched
     * later behind the next batch's copies */
    b.max_cand = std::min(b.max_cand, s->cand_cap);
    HIP_TRY(hipMemcpyAsync(o.h_cand.get(), o.d_cand.get(),
                           sizeof(PostVrfCandidate) * b.max_cand,
                           hipMemcpyDeviceToHost, copy_stream));
    if (s->proof_on) {
      const int rc = proof_queue_fetch(s, copy_stream, o);
      if (rc != POST_OK) return rc;
    }
    HIP_TRY(hipEventRecord(o.ev_done.get(), copy_stream));
    last_set = b.set;
    b.live = true;
    return POST_OK;
  };

  /* host side of one batch, as on the monolithic path */
  auto process = [&](Batch &b) -> int {
    b.live = false;
    OutputSet &o = s->set[b.set];
    sc.begin(s, b.pos, b.count);
    HIP_TRY(hipEventSynchronize(o.ev_done.get()));
    std::vector<PostScanHit> hits;
    if (s->proof_on) {
      const int rc = proof_collect(s, o, b.pos, b.count, hits);
      if (rc != POST_OK) return rc;
    }
    const unsigned int take = std::min(*o.h_cand_count.get(), b.max_cand);
    const bool improved =
        merge_candidates(s, o.h_cand.get(), take, cur_difficulty);
    return finish_batch(s, o, sc, b.pos, b.count, improved, hits, done);
  };

  auto run = [&]() -> int {
    const uint64_t range = s->range_end - s->range_start;
    uint64_t pos = s->written.load(); /* relative position (resume) */
    const uint64_t target = std::min(range, pos + max_labels);
    Batch inflight[2];
    int cur = 0;
    bool cancelled = false;
    while (pos < target) {
      /* cancel is seen between batches only: a batch is either issued
       * whole, with all its events, or not at all */
      if (s->cancel.load()) {
        cancelled = true;
        break;
      }
      Batch &b = inflight[cur];
      b.pos = pos;
      b.count = std::min(s->batch, target - pos);
      int rc = issue(b);
      if (rc != POST_OK) return rc;
      pos += b.count;
      if (inflight[cur ^ 1].live) {
        rc = process(inflight[cur ^ 1]);
        if (rc != POST_OK) return rc;
      }
      cur ^= 1;
    }
    /* the batch still in flight is complete work: hand it over, cancelled
     * or not, so `written` covers exactly what reached the sink or the
     * files */
    if (inflight[cur ^ 1].live) {
      int rc = process(inflight[cur ^ 1]);
      if (rc != POST_OK) return rc;
    }
    return cancelled ? POST_ERR_CANCELLED : POST_OK;
  };

  /* End of call, cancel and error all drain here.  Every event a stream
   * waits for is recorded before the wait is queued, so a call that fails
   * half-way through issue() leaves no stream waiting for a record that
   * never comes. */
  const int rc = run();
  s->sync_streams();
  if ((rc == POST_OK || rc == POST_ERR_CANCELLED) && last_set >= 0) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ev0, s->set[last_set].ev_end.get());
    s->last_kernel_ms = ms;
  }
  return rc;
}

int post_init_step(PostInitSession *s, uint64_t max_labels, uint64_t *done) {
  if (!s || !done) return POST_ERR_INVALID_ARGS;
  *done = 0;
  int rc = require_gpu(s->cfg.provider_id);
  if (rc != POST_OK) return rc;
  s->stepped = true;
  /* after a failed step: the part back to its marker, the seal back to its
   * page boundary, and the part once more when that moved `written` */
  if (s->proof_on) {
    rc = proof_resync(s);
    if (rc != POST_OK) return rc;
  }
  if (s->seal_on) {
    rc = seal_resync(s);
    if (rc != POST_OK) return rc;
  }
  if (s->proof_on) {
    rc = proof_resync(s);
    if (rc != POST_OK) return rc;
  }
  SelfCheck sc;
  if (s->split_streams) return init_step_split(s, sc, max_labels, done);

  OutputSet &o = s->set[0];
  const hipStream_t stream = s->stream.get();
  LabelKernelArgs args = init_label_args(s);
  args.xbuf = s->d_xbuf.get();
  args.cand = o.d_cand.get();
  args.cand_count = o.d_cand_count.get();

  uint8_t cur_difficulty[32];
  load_running_minimum(s, cur_difficulty);

  const uint32_t blocks = (uint32_t)(s->lanes / 64); /* 64 quads/block */
  std::vector<PostVrfCandidate> cands(s->cand_cap);

  if (!s->ev0.get()) HIP_TRY(s->ev0.create());
  if (!s->ev1.get()) HIP_TRY(s->ev1.create());
  s->last_kernel_ms = 0;

  uint64_t range = s->range_end - s->range_start;
  uint64_t pos = s->written.load(); /* relative position (resume) */
  uint64_t target = std::min(range, pos + max_labels);
  while (pos < target) {
    if (s->cancel.load()) return POST_ERR_CANCELLED;
    uint64_t count = std::min(s->batch, target - pos);
    args.start = s->range_start + pos;
    args.count = count;
    args.out = s->keep_all ? s->d_all.get() + pos * POST_LABEL_SIZE
                           : o.d_out.get();
    difficulty_to_be_words(cur_difficulty, args.difficulty_be);
    unsigned int zero = 0;
    HIP_TRY(hipMemcpyAsync(o.d_cand_count.get(), &zero, sizeof(zero),
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->ev0.get(), stream));
    HIP_TRY(poste_launch_label_kernel(&args, blocks, stream));
    HIP_TRY(hipEventRecord(s->ev1.get(), stream));
    if (s->seal_on) {
      rc = seal_launch(s, stream, o, pos, count, args.out);
      if (rc != POST_OK) return rc;
    }
    if (s->proof_on) {
      rc = proof_launch(s, stream, o, pos, count, args.out);
      if (rc != POST_OK) return rc;
    }
    HIP_TRY(hipMemcpyAsync(o.h_batch.get(), args.out, count * POST_LABEL_SIZE,
                           hipMemcpyDeviceToHost, stream));
    unsigned int n_cand = 0;
    HIP_TRY(hipMemcpyAsync(&n_cand, o.d_cand_count.get(), sizeof(n_cand),
                           hipMemcpyDeviceToHost, stream));
    if (s->proof_on) {
      rc = proof_queue_fetch(s, stream, o);
      if (rc != POST_OK) return rc;
    }
    sc.begin(s, pos, count);
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<PostScanHit> hits;
    if (s->proof_on) {
      rc = proof_collect(s, o, pos, count, hits);
      if (rc != POST_OK) return rc;
    }
    bool nonce_improved = false;
    if (n_cand > 0) {
      unsigned int take = std::min(n_cand, s->cand_cap);
      HIP_TRY(hipMemcpy(cands.data(), o.d_cand.get(),
                        sizeof(PostVrfCandidate) * take,
                        hipMemcpyDeviceToHost));
      nonce_improved = merge_candidates(s, cands.data(), take, cur_difficulty);
    }
    rc = finish_batch(s, o, sc, pos, count, nonce_improved, hits, done);
    if (rc != POST_OK) return rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s->ev0.get(), s->ev1.get());
    s->last_kernel_ms += ms;
    pos += count;
  }
  return POST_OK;
}

double post_init_last_kernel_ms(const PostInitSession *s) {
  return s ? s->last_kernel_ms : 0.0;
}

/* nonce-only batch beyond the configured range (no label output) */
static int nonce_only_batch(PostInitSession *s, uint64_t gstart,
                            uint64_t count) {
  OutputSet &o = s->set[0];
  LabelKernelArgs args = init_label_args(s);
  args.xbuf = s->d_xbuf.get();
  args.start = gstart;
  args.count = count;
  args.out = nullptr;
  args.cand = o.d_cand.get();
  args.cand_count = o.d_cand_count.get();
  uint8_t cur[32];
  load_running_minimum(s, cur);
  difficulty_to_be_words(cur, args.difficulty_be);
  unsigned int zero = 0;
  HIP_TRY(hipMemcpy(o.d_cand_count.get(), &zero, sizeof(zero),
                    hipMemcpyHostToDevice));
  HIP_TRY(poste_launch_label_kernel(&args, (uint32_t)(s->lanes / 64),
                                    s->stream.get()));
  HIP_TRY(hipStreamSynchronize(s->stream.get()));
  unsigned int n_cand = 0;
  HIP_TRY(hipMemcpy(&n_cand, o.d_cand_count.get(), sizeof(n_cand),
                    hipMemcpyDeviceToHost));
  if (n_cand > 0) {
    unsigned int take = std::min(n_cand, s->cand_cap);
    std::vector<PostVrfCandidate> cands(take);
    HIP_TRY(hipMemcpy(cands.data(), o.d_cand.get(),
                      sizeof(PostVrfCandidate) * take,
                      hipMemcpyDeviceToHost));
    if (merge_candidates(s, cands.data(), take, cur) && !s->data_dir.empty())
      return write_metadata(s);
  }
  return POST_OK;
}

int post_init_run(PostInitSession *s) {
  if (!s) return POST_ERR_INVALID_ARGS;
  uint64_t range = s->range_end - s->range_start;
  while (s->written.load() < range) {
    uint64_t done = 0;
    int rc = post_init_step(s, s->batch * 8, &done);
    if (rc != POST_OK) return rc;
    if (done == 0) break;
  }

  /* When this session covers the whole label space and the tracked minimum
   * does not meet the VRF threshold (p ~ e^-16 with the x16 margin), keep
   * searching past the end — the reference initializer's follow-up nonce
   * search (init completes with Nonce optional; VerifyVRFNonce needs one
   * below threshold, validation.go:261-286). */
  uint64_t total = (uint64_t)s->cfg.num_units * s->cfg.labels_per_unit;
  if (s->range_start == 0 && s->range_end == total) {
    uint8_t diff[32];
    poste::vrf_difficulty(total, diff);
    for (uint64_t ext = total; ext < 2 * total; ext += s->batch) {
      {
        std::lock_guard<std::mutex> lk(s->nonce_mu);
        if (s->nonce_found &&
            std::memcmp(s->nonce_label, diff, 32) < 0)
          break;
      }
      if (s->cancel.load()) return POST_ERR_CANCELLED;
      int rc = nonce_only_batch(s, ext, std::min(s->batch, 2 * total - ext));
      if (rc != POST_OK) return rc;
    }
  }

  if (!s->data_dir.empty()) return write_metadata(s);
  return POST_OK;
}

int post_init_copy_labels(const PostInitSession *s, uint64_t first,
                          uint64_t count, uint8_t *out_host) {
  if (!s || !out_host) return POST_ERR_INVALID_ARGS;
  if (!s->keep_all) {
    set_error("labels were not kept on device (file mode or large range)");
    return POST_ERR_INVALID_ARGS;
  }
  if (first + count > s->range_end - s->range_start) {
    set_error("range out of bounds");
    return POST_ERR_INVALID_ARGS;
  }
  HIP_TRY(hipMemcpy(out_host, s->d_all.get() + first * POST_LABEL_SIZE,
                    count * POST_LABEL_SIZE, hipMemcpyDeviceToHost));
  return POST_OK;
}

void post_init_free(PostInitSession *s) { delete s; }

/* ------------------------- benchmark ------------------------- */

int post_benchmark(uint32_t provider_id, uint32_t scrypt_n,
                   uint64_t *labels_per_sec) {
  int rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;
  PostInitConfig cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  std::memset(cfg.node_id, 0xA5, 32);
  std::memset(cfg.commitment_atx_id, 0x5A, 32);
  cfg.num_units = 1;
  cfg.labels_per_unit = 1ull << 18;
  cfg.max_file_size = 1ull << 40;
  cfg.scrypt_n = scrypt_n;
  cfg.provider_id = provider_id;
  cfg.scratch_bytes = 8ull << 30;
  Event t0, t1;
  HIP_TRY(t0.create());
  HIP_TRY(t1.create());
  PostInitSession *s = nullptr;
  rc = post_init_new(&cfg, &s);
  if (rc != POST_OK) return rc;
  (void)hipEventRecord(t0.get(), nullptr);
  rc = post_init_run(s);
  (void)hipEventRecord(t1.get(), nullptr);
  (void)hipEventSynchronize(t1.get());
  float ms = 0;
  (void)hipEventElapsedTime(&ms, t0.get(), t1.get());
  if (rc == POST_OK && ms > 0)
    *labels_per_sec = (uint64_t)((double)cfg.labels_per_unit / (ms / 1e3));
  post_init_free(s);
  return rc;
}

/* ------------------------- proving ------------------------- */

/* label source: fill dst with labels [base, base+cnt) (16 B each) */
using LabelReader =
    std::function<int(uint64_t base, uint64_t cnt, uint8_t *dst)>;

/* Optional seal step of the pipeline: per chunk, post_seal_kernel hashes the
 * chunk's pages while it is on the device and `sink` receives the digests of
 * pages [first_page, first_page + n_pages) on the host, chunk after chunk in
 * page order.  A non-zero return from sink ends the pass with that status. */
using SealSink = std::function<int(uint64_t first_page, uint64_t n_pages,
                                   const uint8_t *digests)>;

constexpr uint64_t SEAL_PAGE = POSTE_SEAL_PAGE_LABELS;
constexpr uint64_t SEAL_DIGEST = 16;

/* POST_SEAL_STREAM=0 launches the seal step on the scan's own stream instead
 * of a second one (A/B, profiles/seal.md).  Read per call. */
static bool seal_on_second_stream() {
  const char *e = getenv("POST_SEAL_STREAM");
  return !(e && std::strcmp(e, "0") == 0);
}

/* The double-buffered read -> pinned -> H2D pipeline of the proving pass:
 * the disk/host read of chunk i+1 overlaps the device work on chunk i (the
 * 256-GiB config-4 pass never needs the whole label set in host memory).
 * Per chunk it launches the scan (`scan` set: te/sbox/rk/difficulty/hits
 * filled by the caller, labels/count/index_base per chunk here, `plan` the
 * call's scan plan) and/or the
 * seal step (`seal` set).  With no seal step the queue is what it always
 * was: H2D, scan, done[parity].
 *
 * Seal step: the kernel and the copy of its digests (256 KiB per 2^24-label
 * chunk) to pinned memory run on a second stream gated by the chunk's H2D
 * event, beside the scan; the main stream waits for them before it records
 * done[parity], so the event still means "buffers of this parity are free".
 * The host hands a chunk's digests to the sink when it comes back to that
 * parity, and the last two after the drain: always in page order.  Chunks
 * are a multiple of the page, so no page crosses a chunk. */
static int label_pipeline(const LabelReader &read_labels, uint64_t num_labels,
                          ScanKernelArgs *scan, const ScanPlan *plan,
                          const SealSink *seal) {
  uint64_t CHUNK = prove_chunk_labels();
  if (seal) CHUNK = (CHUNK + SEAL_PAGE - 1) / SEAL_PAGE * SEAL_PAGE;
  const uint64_t chunk_lab = std::min(CHUNK, num_labels);
  const uint64_t chunk_pages = (chunk_lab + SEAL_PAGE - 1) / SEAL_PAGE;
  DevBuf<uint8_t> d_labels[2], d_dig[2];
  PinnedBuf<uint8_t> h_labels[2], h_dig[2];
  Event done[2], staged[2], sealed[2];
  Stream main_stream, second_stream; /* last: synchronised, then the rest */
  for (int p = 0; p < 2; p++) {
    HIP_TRY(d_labels[p].alloc(chunk_lab * 16));
    HIP_TRY(h_labels[p].alloc(chunk_lab * 16));
    HIP_TRY(done[p].create());
    if (seal) {
      HIP_TRY(d_dig[p].alloc(chunk_pages * SEAL_DIGEST));
      HIP_TRY(h_dig[p].alloc(chunk_pages * SEAL_DIGEST));
    }
  }
  HIP_TRY(main_stream.create());
  if (seal && seal_on_second_stream()) {
    HIP_TRY(second_stream.create());
    for (int p = 0; p < 2; p++) {
      HIP_TRY(staged[p].create(hipEventDisableTiming));
      HIP_TRY(sealed[p].create(hipEventDisableTiming));
    }
  }
  const hipStream_t stream = main_stream.get();
  const hipStream_t seal_stream = second_stream.get();

  /* digests of the chunk in flight on each parity, not yet handed over */
  uint64_t pend_first[2] = {0, 0}, pend_pages[2] = {0, 0};
  auto hand_over = [&](int p) -> int {
    if (!pend_pages[p]) return POST_OK;
    const uint64_t n = pend_pages[p];
    pend_pages[p] = 0;
    return (*seal)(pend_first[p], n, h_dig[p].get());
  };

  int parity = 0;
  bool inflight[2] = {false, false};
  for (uint64_t base = 0; base < num_labels; base += CHUNK, parity ^= 1) {
    uint64_t cnt = std::min(CHUNK, num_labels - base);
    /* wait until this parity's buffers are free, then stage the chunk */
    if (inflight[parity]) HIP_TRY(hipEventSynchronize(done[parity].get()));
    int rrc = seal ? hand_over(parity) : POST_OK;
    if (rrc == POST_OK) rrc = read_labels(base, cnt, h_labels[parity].get());
    if (rrc != POST_OK) return rrc;
    HIP_TRY(hipMemcpyAsync(d_labels[parity].get(), h_labels[parity].get(),
                           cnt * 16, hipMemcpyHostToDevice, stream));
    if (seal_stream) HIP_TRY(hipEventRecord(staged[parity].get(), stream));
    if (scan) {
      scan->labels = (const uint4 *)d_labels[parity].get();
      scan->count = cnt;
      scan->index_base = base;
      HIP_TRY(poste_launch_scan(scan, plan, stream));
    }
    if (seal) {
      const uint64_t n_pages = (cnt + SEAL_PAGE - 1) / SEAL_PAGE;
      hipStream_t ss = seal_stream ? seal_stream : stream;
      SealKernelArgs ka;
      ka.labels = (const uint4 *)d_labels[parity].get();
      ka.count = cnt;
      ka.digests = (uint4 *)d_dig[parity].get();
      if (seal_stream)
        HIP_TRY(hipStreamWaitEvent(ss, staged[parity].get(), 0));
      HIP_TRY(poste_launch_seal_kernel(&ka, ss));
      HIP_TRY(hipMemcpyAsync(h_dig[parity].get(), d_dig[parity].get(),
                             n_pages * SEAL_DIGEST, hipMemcpyDeviceToHost,
                             ss));
      if (seal_stream) {
        HIP_TRY(hipEventRecord(sealed[parity].get(), ss));
        HIP_TRY(hipStreamWaitEvent(stream, sealed[parity].get(), 0));
      }
      pend_first[parity] = base / SEAL_PAGE;
      pend_pages[parity] = n_pages;
    }
    HIP_TRY(hipEventRecord(done[parity].get(), stream));
    inflight[parity] = true;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  int rc = POST_OK;
  if (seal) {
    /* `parity` now names the older of the two chunks still pending */
    rc = hand_over(parity);
    if (rc == POST_OK) rc = hand_over(parity ^ 1);
  }
  return rc;
}

/* Optional step of prove_core between "hits copied back" and "winner
 * chosen" (post_prove_healed): it may rewrite the hit list, and may launch
 * further scans with the pass's own arguments and plan — tables, round
 * keys, difficulty and hit buffers are still allocated, the hit buffers free
 * for reuse. */
using HitHook =
    std::function<int(const ScanKernelArgs &scan, const ScanPlan &plan,
                      std::vector<PostScanHit> &hits)>;

static int prove_core(const LabelReader &read_labels, uint64_t num_labels,
                      const PostProveConfig *cfg, PostProof *out,
                      const SealSink *seal = nullptr,
                      std::vector<uint64_t> *winner = nullptr,
                      const HitHook *hook = nullptr) {
  if (cfg->nonces == 0 || cfg->nonces % POSTE_NONCE_GROUP != 0) {
    set_error("nonces must be a positive multiple of 16");
    return POST_ERR_INVALID_ARGS;
  }
  if (cfg->pow_mode != POST_POW_MODE_BLAKE3) {
    set_error("RandomX k2pow is not supported by this engine (parity-"
              "unpinned; use POST_POW_MODE_BLAKE3)");
    return POST_ERR_UNSUPPORTED;
  }
  int rc = require_gpu(cfg->provider_id);
  if (rc != POST_OK) return rc;
  int dev = (int)cfg->provider_id;
  DeviceTables tbl;
  rc = get_aes_tables(dev, tbl);
  if (rc != POST_OK) return rc;
  ScanPlan plan;
  HIP_TRY(prove_scan_plan(&plan));

  const uint32_t n_ciphers = cfg->nonces / POSTE_NONCES_PER_AES;
  const uint32_t n_groups = cfg->nonces / POSTE_NONCE_GROUP;
  std::vector<uint64_t> group_pow(n_groups);
  for (uint32_t g = 0; g < n_groups; g++)
    group_pow[g] = poste::k2pow_search_blake3(cfg->challenge, g,
                                              cfg->pow_difficulty,
                                              cfg->pow_threads);
  std::vector<uint32_t> rk((size_t)n_ciphers * 44);
  for (uint32_t c = 0; c < n_ciphers; c++) {
    uint8_t key[16];
    uint32_t grp = (c * POSTE_NONCES_PER_AES) / POSTE_NONCE_GROUP;
    poste::prove_cipher_key(cfg->challenge, c, group_pow[grp], key);
    poste::aes128_expand(key, rk.data() + (size_t)c * 44);
  }
  DevBuf<uint32_t> d_rk;
  HIP_TRY(d_rk.alloc(rk.size() * 4));
  HIP_TRY(hipMemcpy(d_rk.get(), rk.data(), rk.size() * 4,
                    hipMemcpyHostToDevice));

  /* Expected total hits = nonces*k1 (a few thousand) regardless of label
   * count, so hits accumulate in one device buffer drained once at the
   * end of the pipeline. */
  const uint32_t HIT_CAP = 1u << 22;
  DevBuf<PostScanHit> d_hits;
  DevBuf<unsigned int> d_hit_count;
  HIP_TRY(d_hits.alloc(sizeof(PostScanHit) * HIT_CAP));
  HIP_TRY(d_hit_count.alloc(4));
  unsigned int zero = 0;
  HIP_TRY(hipMemcpy(d_hit_count.get(), &zero, 4, hipMemcpyHostToDevice));

  ScanKernelArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.te = tbl.d_te;
  sa.sbox = tbl.d_sbox;
  sa.rk = d_rk.get();
  sa.n_ciphers = n_ciphers;
  sa.difficulty = poste::proving_difficulty(cfg->k1, num_labels);
  sa.hits = d_hits.get();
  sa.hit_count = d_hit_count.get();
  sa.hit_cap = HIT_CAP;

  rc = label_pipeline(read_labels, num_labels, &sa, &plan, seal);
  if (rc != POST_OK) return rc;
  unsigned int n_hits = 0;
  HIP_TRY(hipMemcpy(&n_hits, d_hit_count.get(), 4, hipMemcpyDeviceToHost));
  if (n_hits > HIT_CAP) {
    set_error("scan hit buffer overflow (pathological K1/num_labels "
              "configuration)");
    return POST_ERR;
  }
  std::vector<PostScanHit> all_hits(n_hits);
  if (n_hits)
    HIP_TRY(hipMemcpy(all_hits.data(), d_hits.get(),
                      sizeof(PostScanHit) * n_hits, hipMemcpyDeviceToHost));
  if (hook) {
    rc = (*hook)(sa, plan, all_hits);
    if (rc != POST_OK) return rc;
  }

  /* the winner rule, shared with the assembly of an init's hit parts */
  std::string err;
  rc = initproof::choose_winner(all_hits, cfg->nonces, cfg->k2, num_labels,
                                group_pow, out, winner, err);
  if (rc != POST_OK) set_error(err);
  return rc;
}

int post_prove_buffer(const uint8_t *labels, uint64_t num_labels,
                      const uint8_t node_id[32],
                      const uint8_t commitment_atx_id[32],
                      const PostProveConfig *cfg, PostProof *out) {
  (void)node_id;
  (void)commitment_atx_id; /* scan operates on labels only */
  if (!labels || !cfg || !out) return POST_ERR_INVALID_ARGS;
  LabelReader reader = [labels](uint64_t base, uint64_t cnt, uint8_t *dst) {
    std::memcpy(dst, labels + base * 16, cnt * 16);
    return POST_OK;
  };
  return prove_core(reader, num_labels, cfg, out);
}

int post_k2pow_search(const uint8_t challenge[32], uint32_t nonce_group,
                      const uint8_t pow_difficulty[32], uint32_t pow_mode,
                      uint32_t threads, uint64_t *out) {
  if (pow_mode != POST_POW_MODE_BLAKE3) {
    set_error("RandomX k2pow is not supported (use POST_POW_MODE_BLAKE3)");
    return POST_ERR_UNSUPPORTED;
  }
  *out = poste::k2pow_search_blake3(challenge, nonce_group, pow_difficulty,
                                    threads);
  return POST_OK;
}

int post_prove_scan(const uint8_t *labels, uint64_t count,
                    uint64_t index_base, uint64_t total_labels,
                    const PostProveConfig *cfg, const uint64_t *group_pows,
                    PostScanHitOut *hits, uint32_t cap, uint32_t *n_hits) {
  if (!labels || !cfg || !group_pows || !hits || !n_hits)
    return POST_ERR_INVALID_ARGS;
  if (cfg->nonces == 0 || cfg->nonces % POSTE_NONCE_GROUP != 0) {
    set_error("nonces must be a positive multiple of 16");
    return POST_ERR_INVALID_ARGS;
  }
  int rc = require_gpu(cfg->provider_id);
  if (rc != POST_OK) return rc;
  DeviceTables tbl;
  rc = get_aes_tables((int)cfg->provider_id, tbl);
  if (rc != POST_OK) return rc;
  ScanPlan plan;
  HIP_TRY(prove_scan_plan(&plan));

  const uint32_t n_ciphers = cfg->nonces / POSTE_NONCES_PER_AES;
  std::vector<uint32_t> rk((size_t)n_ciphers * 44);
  for (uint32_t c = 0; c < n_ciphers; c++) {
    uint8_t key[16];
    uint32_t grp = (c * POSTE_NONCES_PER_AES) / POSTE_NONCE_GROUP;
    poste::prove_cipher_key(cfg->challenge, c, group_pows[grp], key);
    poste::aes128_expand(key, rk.data() + (size_t)c * 44);
  }
  DevBuf<uint32_t> d_rk;
  DevBuf<uint8_t> d_labels;
  DevBuf<PostScanHit> d_hits;
  DevBuf<unsigned int> d_hit_count;
  HIP_TRY(d_rk.alloc(rk.size() * 4));
  HIP_TRY(hipMemcpy(d_rk.get(), rk.data(), rk.size() * 4,
                    hipMemcpyHostToDevice));
  const uint64_t CHUNK = prove_chunk_labels();
  HIP_TRY(d_labels.alloc(std::min(CHUNK, count) * 16));
  HIP_TRY(d_hits.alloc(sizeof(PostScanHit) * cap));
  HIP_TRY(d_hit_count.alloc(4));
  unsigned int zero = 0;
  HIP_TRY(hipMemcpy(d_hit_count.get(), &zero, 4, hipMemcpyHostToDevice));

  ScanKernelArgs sa;
  std::memset(&sa, 0, sizeof(sa));
  sa.te = tbl.d_te;
  sa.sbox = tbl.d_sbox;
  sa.rk = d_rk.get();
  sa.n_ciphers = n_ciphers;
  sa.difficulty = poste::proving_difficulty(cfg->k1, total_labels);
  sa.hits = d_hits.get();
  sa.hit_count = d_hit_count.get();
  sa.hit_cap = cap;
  for (uint64_t base = 0; base < count; base += CHUNK) {
    uint64_t cnt = std::min(CHUNK, count - base);
    HIP_TRY(hipMemcpy(d_labels.get(), labels + base * 16, cnt * 16,
                      hipMemcpyHostToDevice));
    sa.labels = (const uint4 *)d_labels.get();
    sa.count = cnt;
    sa.index_base = index_base + base;
    HIP_TRY(poste_launch_scan(&sa, &plan, nullptr));
    HIP_TRY(hipDeviceSynchronize());
  }
  unsigned int got = 0;
  HIP_TRY(hipMemcpy(&got, d_hit_count.get(), 4, hipMemcpyDeviceToHost));
  if (got > cap) {
    set_error("scan hit buffer overflow (raise cap)");
    return POST_ERR;
  }
  std::vector<PostScanHit> tmp(got);
  if (got)
    HIP_TRY(hipMemcpy(tmp.data(), d_hits.get(), sizeof(PostScanHit) * got,
                      hipMemcpyDeviceToHost));
  for (unsigned int i = 0; i < got; i++) {
    hits[i].index = tmp[i].index;
    hits[i].nonce = tmp[i].nonce;
    hits[i].pad = 0;
  }
  *n_hits = got;
  return POST_OK;
}

/* The label stream of a data dir as the proving pass reads it (and as the
 * seal protects it): postdata_0.bin, postdata_1.bin, ... up to the first
 * absent file, floor(size / 16) labels of each, concatenated. */
struct FileSpan {
  std::string path;
  uint64_t first_label;
  uint64_t labels;
};

/* map postdata_*.bin in index order; returns the stream's label count */
static uint64_t map_postdata(const char *data_dir,
                             std::vector<FileSpan> &files) {
  uint64_t total = 0;
  for (uint64_t i = 0;; i++) {
    char path[4096];
    std::snprintf(path, sizeof path, "%s/postdata_%llu.bin", data_dir,
                  (unsigned long long)i);
    FILE *f = std::fopen(path, "rb");
    if (!f) break;
    std::fseek(f, 0, SEEK_END);
    long sz = std::ftell(f);
    std::fclose(f);
    uint64_t nlab = (uint64_t)(sz < 0 ? 0 : sz) / 16;
    files.push_back({path, total, nlab});
    total += nlab;
  }
  return total;
}

/* stream chunks from the mapped files (never the whole set in host memory —
 * config 4 is 256 GiB); `files` must outlive the reader */
static LabelReader dir_reader(const std::vector<FileSpan> &files) {
  return [&files](uint64_t base, uint64_t cnt, uint8_t *dst) -> int {
    uint64_t done = 0;
    for (const auto &fs : files) {
      if (done == cnt) break;
      uint64_t want = base + done;
      if (want < fs.first_label || want >= fs.first_label + fs.labels)
        continue;
      uint64_t in_file = want - fs.first_label;
      uint64_t take = std::min(fs.labels - in_file, cnt - done);
      FILE *f = std::fopen(fs.path.c_str(), "rb");
      if (!f) {
        set_error("cannot reopen " + fs.path);
        return POST_ERR_IO;
      }
      if (std::fseek(f, (long)(in_file * 16), SEEK_SET) != 0 ||
          std::fread(dst + done * 16, 16, take, f) != take) {
        std::fclose(f);
        set_error("short read from " + fs.path);
        return POST_ERR_IO;
      }
      std::fclose(f);
      done += take;
    }
    if (done != cnt) {
      set_error("label range not covered by postdata files");
      return POST_ERR_IO;
    }
    return POST_OK;
  };
}

int post_prove(const char *data_dir, const PostProveConfig *cfg,
               PostProof *out) {
  if (!data_dir || !cfg || !out) return POST_ERR_INVALID_ARGS;
  std::vector<FileSpan> files;
  const uint64_t total = map_postdata(data_dir, files);
  if (total == 0) {
    set_error("no postdata_*.bin in data_dir");
    return POST_ERR_IO;
  }
  return prove_core(dir_reader(files), total, cfg, out);
}

/* ------------------------- postdata seal ------------------------- */

/* postdata_seal.bin: 32-byte little-endian header, then one
 * 16-byte digest per page of the sealed stream. */
static const char SEAL_MAGIC[8] = {'P', 'S', 'T', 'S', 'E', 'A', 'L', '1'};
constexpr uint64_t SEAL_HEADER = 32;

static inline uint64_t seal_pages(uint64_t labels) {
  return labels / SEAL_PAGE + (labels % SEAL_PAGE ? 1 : 0);
}

static void put_le(uint8_t *p, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * i));
}

static uint64_t get_le(const uint8_t *p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

/* A sidecar opened for checking against the dir it lies in: every rung of
 * the validation order of post_check_seal has passed, `f` stands at the
 * first digest.  Compares what the pipeline hands over page by page. */
struct SealChecker {
  FILE *f = nullptr;
  uint64_t total = 0, pages_bad = 0;
  uint64_t *bad_pages = nullptr;
  uint32_t cap = 0;
  std::vector<bool> *bad_map = nullptr; /* set by prove_checked */
  /* set by the healing entries: the first keep_cap bad pages, whatever cap
   * is, each with the digest the sidecar holds for it */
  std::vector<uint64_t> *keep = nullptr;
  std::vector<uint8_t> *keep_want = nullptr;
  uint64_t keep_cap = 0;
  std::vector<uint8_t> want;

  ~SealChecker() {
    if (f) std::fclose(f);
  }

  int open(const char *data_dir, uint64_t dir_total) {
    const std::string path = std::string(data_dir) + "/postdata_seal.bin";
    f = std::fopen(path.c_str(), "rb");
    if (!f) {
      set_error("cannot open " + path + " (run seal first)");
      return POST_ERR_IO;
    }
    struct stat st;
    uint8_t hdr[SEAL_HEADER];
    const bool have_hdr = fstat(fileno(f), &st) == 0 &&
                          (uint64_t)st.st_size >= SEAL_HEADER &&
                          std::fread(hdr, 1, SEAL_HEADER, f) == SEAL_HEADER;
    const uint64_t hdr_total = have_hdr ? get_le(hdr + 16, 8) : 0;
    if (!have_hdr || ((uint64_t)st.st_size - SEAL_HEADER) / SEAL_DIGEST <
                         seal_pages(hdr_total)) {
      set_error("postdata_seal.bin is shorter than its header and digests");
      return POST_ERR_IO;
    }
    if (std::memcmp(hdr, SEAL_MAGIC, 8) != 0) {
      set_error("postdata_seal.bin has a wrong magic");
      return POST_ERR_IO;
    }
    if (get_le(hdr + 8, 4) != SEAL_PAGE || get_le(hdr + 12, 4) != SEAL_DIGEST) {
      set_error("postdata_seal.bin has an unsupported page_labels or "
                "digest_bytes");
      return POST_ERR_IO;
    }
    if (hdr_total != dir_total) {
      set_error("postdata length changed since seal");
      return POST_ERR_IO;
    }
    total = hdr_total;
    return POST_OK;
  }

  int compare(uint64_t first_page, uint64_t n_pages, const uint8_t *got) {
    want.resize(n_pages * SEAL_DIGEST);
    if (std::fread(want.data(), SEAL_DIGEST, n_pages, f) != n_pages) {
      set_error("short read from postdata_seal.bin");
      return POST_ERR_IO;
    }
    for (uint64_t i = 0; i < n_pages; i++) {
      if (std::memcmp(want.data() + i * SEAL_DIGEST, got + i * SEAL_DIGEST,
                      SEAL_DIGEST) == 0)
        continue;
      /* pages arrive in ascending order: the first cap are the smallest */
      if (pages_bad < cap) bad_pages[pages_bad] = first_page + i;
      if (bad_map) (*bad_map)[first_page + i] = true;
      if (keep && keep->size() < keep_cap) {
        keep->push_back(first_page + i);
        keep_want->insert(keep_want->end(), want.data() + i * SEAL_DIGEST,
                          want.data() + (i + 1) * SEAL_DIGEST);
      }
      pages_bad++;
    }
    return POST_OK;
  }

  void report(PostSealReport *r) const {
    r->total_labels = total;
    r->pages = seal_pages(total);
    r->pages_bad = pages_bad;
    r->proof_touches_bad_page = 0;
  }
};

int post_seal_digest_buffer(const uint8_t *labels, uint64_t count,
                            uint32_t provider_id, uint8_t *digests,
                            uint64_t cap_pages, uint64_t *n_pages) {
  if (!labels || !digests || !n_pages || count == 0) {
    set_error("null or empty buffer");
    return POST_ERR_INVALID_ARGS;
  }
  if (cap_pages < seal_pages(count)) {
    set_error("digest buffer holds fewer pages than the labels make");
    return POST_ERR_INVALID_ARGS;
  }
  int rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;
  LabelReader reader = [labels](uint64_t base, uint64_t cnt, uint8_t *dst) {
    std::memcpy(dst, labels + base * 16, cnt * 16);
    return POST_OK;
  };
  SealSink sink = [digests](uint64_t first, uint64_t n, const uint8_t *d) {
    std::memcpy(digests + first * SEAL_DIGEST, d, n * SEAL_DIGEST);
    return POST_OK;
  };
  rc = label_pipeline(reader, count, nullptr, nullptr, &sink);
  if (rc == POST_OK) *n_pages = seal_pages(count);
  return rc;
}

int post_seal_data(const char *data_dir, uint32_t provider_id,
                   PostSealReport *r) {
  if (!data_dir || !r) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  std::vector<FileSpan> files;
  const uint64_t total = map_postdata(data_dir, files);
  if (total == 0) {
    set_error("no postdata_*.bin in data_dir");
    return POST_ERR_IO;
  }
  int rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;

  /* written under a temporary name in the same dir and renamed into place:
   * a reader sees the old sidecar or the new one, never a part of one */
  const std::string path = std::string(data_dir) + "/postdata_seal.bin";
  const std::string tmp = path + ".tmp";
  FILE *f = std::fopen(tmp.c_str(), "wb");
  if (!f) {
    set_error("cannot write " + tmp);
    return POST_ERR_IO;
  }
  uint8_t hdr[SEAL_HEADER] = {0};
  std::memcpy(hdr, SEAL_MAGIC, 8);
  put_le(hdr + 8, SEAL_PAGE, 4);
  put_le(hdr + 12, SEAL_DIGEST, 4);
  put_le(hdr + 16, total, 8);
  bool ok = std::fwrite(hdr, 1, SEAL_HEADER, f) == SEAL_HEADER;
  SealSink sink = [f](uint64_t, uint64_t n, const uint8_t *d) {
    if (std::fwrite(d, SEAL_DIGEST, n, f) == n) return POST_OK;
    set_error("short write to postdata_seal.bin.tmp");
    return POST_ERR_IO;
  };
  if (!ok) {
    set_error("short write to postdata_seal.bin.tmp");
    rc = POST_ERR_IO;
  } else {
    rc = label_pipeline(dir_reader(files), total, nullptr, nullptr, &sink);
  }
  if (rc == POST_OK && (std::fflush(f) != 0 || fsync(fileno(f)) != 0)) {
    set_error("cannot flush postdata_seal.bin.tmp");
    rc = POST_ERR_IO;
  }
  std::fclose(f);
  if (rc == POST_OK && std::rename(tmp.c_str(), path.c_str()) != 0) {
    set_error("cannot rename " + tmp);
    rc = POST_ERR_IO;
  }
  if (rc != POST_OK) {
    (void)::unlink(tmp.c_str());
    return rc;
  }
  r->total_labels = total;
  r->pages = seal_pages(total);
  r->pages_bad = 0;
  r->proof_touches_bad_page = 0;
  return POST_OK;
}

int post_check_seal(const char *data_dir, uint32_t provider_id,
                    uint64_t *bad_pages, uint32_t cap, PostSealReport *r) {
  if (!data_dir || !r || (cap > 0 && !bad_pages)) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  std::vector<FileSpan> files;
  const uint64_t total = map_postdata(data_dir, files);
  SealChecker chk;
  int rc = chk.open(data_dir, total);
  if (rc != POST_OK) return rc;
  if (total == 0) {
    set_error("no postdata_*.bin in data_dir");
    return POST_ERR_IO;
  }
  rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;
  chk.bad_pages = bad_pages;
  chk.cap = cap;
  SealSink sink = [&chk](uint64_t first, uint64_t n, const uint8_t *d) {
    return chk.compare(first, n, d);
  };
  rc = label_pipeline(dir_reader(files), total, nullptr, nullptr, &sink);
  if (rc != POST_OK) return rc;
  chk.report(r);
  return POST_OK;
}

int post_prove_checked(const char *data_dir, const PostProveConfig *cfg,
                       PostProof *out, uint64_t *bad_pages, uint32_t cap,
                       PostSealReport *r) {
  if (!data_dir || !cfg || !out || !r || (cap > 0 && !bad_pages)) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  std::vector<FileSpan> files;
  const uint64_t total = map_postdata(data_dir, files);
  SealChecker chk;
  int rc = chk.open(data_dir, total);
  if (rc != POST_OK) return rc;
  if (total == 0) {
    set_error("no postdata_*.bin in data_dir");
    return POST_ERR_IO;
  }
  std::vector<bool> bad_map(seal_pages(total), false);
  chk.bad_pages = bad_pages;
  chk.cap = cap;
  chk.bad_map = &bad_map;
  SealSink sink = [&chk](uint64_t first, uint64_t n, const uint8_t *d) {
    return chk.compare(first, n, d);
  };
  std::vector<uint64_t> winner;
  rc = prove_core(dir_reader(files), total, cfg, out, &sink, &winner);
  if (rc != POST_OK) return rc;
  chk.report(r);
  for (uint64_t idx : winner)
    if (bad_map[idx / SEAL_PAGE]) r->proof_touches_bad_page = 1;
  return POST_OK;
}

/* ------------------------- postdata audit ------------------------- */

static inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static inline uint64_t audit_windows(uint64_t range, uint64_t k) {
  return range / k + (range % k ? 1 : 0);
}

/* The sampling rule: window w of [index_start, index_end)
 * contributes first + h % len with first = index_start + w*K,
 * len = min(K, index_end - first), h = splitmix64(splitmix64(seed) + w).
 * h % len favours some offsets by at most len / 2^64, below 2^-20 even for
 * a window of 2^44 labels: modulo bias is irrelevant at these sizes. */
int post_verify_data_sample(uint64_t seed, uint64_t sample_every,
                            uint64_t index_start, uint64_t index_end,
                            uint64_t first_window, uint64_t *out,
                            uint32_t cap, uint32_t *n) {
  if (!n || (cap && !out)) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  *n = 0;
  if (sample_every == 0 || index_start >= index_end) {
    set_error("sample_every must be >= 1 and the range non-empty");
    return POST_ERR_INVALID_ARGS;
  }
  const uint64_t windows =
      audit_windows(index_end - index_start, sample_every);
  const uint64_t s = splitmix64(seed);
  uint32_t got = 0;
  for (uint64_t w = first_window; w < windows && got < cap; w++, got++) {
    const uint64_t first = index_start + w * sample_every;
    const uint64_t len = std::min(sample_every, index_end - first);
    out[got] = first + splitmix64(s + w) % len;
  }
  *n = got;
  return POST_OK;
}

/* label source of an audit batch: for the n ascending sampled indices idx,
 * append the labels that exist to (out_idx, out_lab) and set *n_out; the
 * rest are missing */
using AuditGather =
    std::function<int(const uint64_t *idx, uint32_t n, uint64_t *out_idx,
                      uint8_t *out_lab, uint32_t *n_out)>;

/* Up to this period the audit reads the covering span sequentially and
 * picks the sampled labels from it (every 4-KiB page of 256 labels is
 * touched anyway); above it, one pread per sample. */
constexpr uint64_t AUDIT_SEQ_MAX_K = 256;
constexpr size_t AUDIT_SEQ_CHUNK = 4u << 20;

/* postdata_*.bin reader of an audit: one descriptor stays open while the
 * (ascending) samples are inside a file; chunk is the read-ahead. */
struct AuditDirReader {
  std::string dir;
  uint64_t per_file = 1;
  size_t chunk = POST_LABEL_SIZE;
  int fd = -1;
  uint64_t file_i = UINT64_MAX;
  uint64_t file_bytes = 0;
  std::vector<uint8_t> buf;
  uint64_t buf_off = 0;
  size_t buf_len = 0;

  ~AuditDirReader() {
    if (fd >= 0) ::close(fd);
  }

  /* 1 = label copied, 0 = missing (file absent or ends before the label's
   * 16th byte), -1 = IO error (set_error called) */
  int fetch(uint64_t g, uint8_t *dst) {
    const uint64_t fi = g / per_file;
    const uint64_t off = (g % per_file) * POST_LABEL_SIZE;
    if (fi != file_i) {
      if (fd >= 0) ::close(fd);
      fd = -1;
      file_i = fi;
      file_bytes = 0;
      buf_len = 0;
      /* a std::string: a long data dir must not be cut short and then
       * read as "file absent" */
      const std::string path = dir + "/postdata_" +
                               std::to_string((unsigned long long)fi) + ".bin";
      fd = ::open(path.c_str(), O_RDONLY);
      if (fd < 0 && errno != ENOENT) {
        set_error("cannot open " + path);
        return -1;
      }
      if (fd >= 0) {
        struct stat st;
        if (::fstat(fd, &st) != 0) {
          set_error("cannot stat " + path);
          return -1;
        }
        file_bytes = (uint64_t)st.st_size;
      }
    }
    if (fd < 0 || off + POST_LABEL_SIZE > file_bytes) return 0;
    if (off < buf_off || off + POST_LABEL_SIZE > buf_off + buf_len) {
      const size_t want =
          (size_t)std::min<uint64_t>(chunk, file_bytes - off);
      if (buf.size() < want) buf.resize(want);
      size_t got = 0;
      while (got < want) {
        ssize_t r = ::pread(fd, buf.data() + got, want - got,
                            (off_t)(off + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) break;
        got += (size_t)r;
      }
      if (got < POST_LABEL_SIZE) {
        set_error("short read from postdata file " +
                  std::to_string((unsigned long long)fi));
        return -1;
      }
      buf_off = off;
      buf_len = got;
    }
    std::memcpy(dst, buf.data() + (off - buf_off), POST_LABEL_SIZE);
    return 1;
  }
};

/* Shared by post_verify_data and post_verify_data_buffer, which validate
 * their arguments first: [start, end) is non-empty and sample_every >= 1.
 * Batches go in ascending index order; the host gathers batch i+1 while the
 * GPU runs batch i (the prove_core pattern).  Nothing here is global: every
 * buffer and stream belongs to the call. */
static int audit_core(const AuditGather &gather, const uint8_t commitment[32],
                      uint32_t scrypt_n, uint64_t start, uint64_t end,
                      const PostAuditConfig *cfg, PostBadLabel *bad,
                      uint32_t cap, PostAuditReport *report) {
  int rc = require_gpu(cfg->provider_id);
  if (rc != POST_OK) return rc;

  /* POST_AUDIT_DEBUG: where a call's wall time went (stderr) */
  const bool dbg = getenv("POST_AUDIT_DEBUG") != nullptr;
  auto tick = [] {
    return std::chrono::duration<double>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
  };
  const double t_start = tick();
  double t_gather = 0, t_drain = 0;

  const uint64_t windows = audit_windows(end - start, cfg->sample_every);
  std::memset(report, 0, sizeof(*report));
  report->labels_in_range = end - start;
  report->labels_sampled = windows;

  /* lanes and batch exactly as post_init_new sizes them */
  const uint32_t gap_shift = pick_gap_shift(scrypt_n);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  uint64_t budget = cfg->scratch_bytes ? cfg->scratch_bytes
                                       : (uint64_t)((double)free_b * 0.80);
  const uint64_t per_lane = ((uint64_t)scrypt_n >> gap_shift) * 128;
  uint64_t lanes = budget / per_lane;
  lanes = std::min<uint64_t>(lanes, std::max<uint64_t>(windows, 64));
  lanes = std::min<uint64_t>(lanes, poste_label_resident_slots(gap_shift));
  lanes = (lanes / 128) * 128;
  if (lanes == 0) lanes = 128;
  const uint64_t batch = std::min<uint64_t>(windows, lanes * 4);
  const uint32_t blocks = (uint32_t)(lanes / 64); /* 64 quads/block */

  /* everything of the call, released before the "free" time is taken */
  struct Res {
    DevBuf<uint32_t> d_scratch, d_xbuf;
    DevBuf<uint64_t> d_idx[2];
    PinnedBuf<uint64_t> h_idx[2];
    DevBuf<uint8_t> d_exp[2];
    PinnedBuf<uint8_t> h_exp[2];
    DevBuf<PostAuditMismatch> d_mis[2];
    DevBuf<unsigned int> d_count[2];
    PinnedBuf<unsigned int> h_count; /* one per parity */
    Event done[2];
    Stream stream, copy_stream; /* last: synchronised, then the rest */
  };
  std::optional<Res> res(std::in_place);
  Res &r = *res;
  HIP_TRY(r.stream.create());
  HIP_TRY(r.copy_stream.create());
  const hipStream_t stream = r.stream.get();
  const hipStream_t copy_stream = r.copy_stream.get();
  HIP_TRY(r.d_scratch.alloc((size_t)lanes * per_lane));
  HIP_TRY(r.d_xbuf.alloc((size_t)batch * 128));
  HIP_TRY(r.h_count.alloc(2 * sizeof(unsigned int)));
  for (int p = 0; p < 2; p++) {
    HIP_TRY(r.d_idx[p].alloc((size_t)batch * 8));
    HIP_TRY(r.h_idx[p].alloc((size_t)batch * 8));
    HIP_TRY(r.d_exp[p].alloc((size_t)batch * POST_LABEL_SIZE));
    HIP_TRY(r.h_exp[p].alloc((size_t)batch * POST_LABEL_SIZE));
    HIP_TRY(r.d_mis[p].alloc((size_t)batch * sizeof(PostAuditMismatch)));
    HIP_TRY(r.d_count[p].alloc(sizeof(unsigned int)));
    HIP_TRY(r.done[p].create());
  }

  const double t_alloc = tick() - t_start;

  AuditKernelArgs aa;
  std::memset(&aa, 0, sizeof(aa));
  load_commitment_words(commitment, aa.label.commitment_le);
  aa.label.scrypt_n = scrypt_n;
  aa.label.gap_shift = gap_shift;
  aa.label.scratch = r.d_scratch.get();
  aa.label.scratch_lanes = lanes;
  aa.label.xbuf = r.d_xbuf.get();

  std::vector<uint64_t> sample((size_t)batch);
  std::vector<PostAuditMismatch> mis;
  uint32_t in_batch[2] = {0, 0}; /* labels sent to the GPU per parity */
  uint32_t kept = 0;

  /* collect a launched batch: mismatches ascending, then progress */
  auto drain = [&](int p) -> int {
    const uint32_t n = in_batch[p];
    if (n) {
      hipError_t e = hipEventSynchronize(r.done[p].get());
      if (e != hipSuccess) return hip_fail("hipEventSynchronize", e);
      const unsigned int n_bad = r.h_count.get()[p];
      if (n_bad > n) {
        set_error("audit mismatch count exceeds the batch");
        return POST_ERR;
      }
      if (n_bad) {
        mis.resize(n_bad);
        /* its own stream: the next batch is already queued on `stream` */
        e = hipMemcpyAsync(mis.data(), r.d_mis[p].get(),
                           sizeof(PostAuditMismatch) * n_bad,
                           hipMemcpyDeviceToHost, copy_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(copy_stream);
        if (e != hipSuccess) return hip_fail("audit mismatch copy", e);
        std::sort(mis.begin(), mis.end(),
                  [](const PostAuditMismatch &x, const PostAuditMismatch &y) {
                    return x.index < y.index;
                  });
        for (unsigned int i = 0; i < n_bad && kept < cap; i++, kept++) {
          const uint64_t *const idx = r.h_idx[p].get();
          const uint64_t *at =
              std::lower_bound(idx, idx + n, (uint64_t)mis[i].index);
          if (at == idx + n || *at != mis[i].index) {
            set_error("audit mismatch names an index outside its batch");
            return POST_ERR;
          }
          PostBadLabel &b = bad[kept];
          b.index = mis[i].index;
          std::memcpy(b.on_disk,
                      r.h_exp[p].get() + (size_t)(at - idx) * POST_LABEL_SIZE,
                      POST_LABEL_SIZE);
          std::memcpy(b.expected, mis[i].label, POST_LABEL_SIZE);
        }
        report->labels_bad += n_bad;
      }
      report->labels_checked += n;
    }
    if (cfg->progress &&
        cfg->progress(cfg->user, report->labels_checked, windows) != 0) {
      set_error("audit cancelled by the progress callback");
      return POST_ERR_CANCELLED;
    }
    return POST_OK;
  };

  int parity = 0;
  bool have_prev = false;
  for (uint64_t w = 0; w < windows; parity ^= 1) {
    /* this parity's buffers are free: their batch was drained last turn */
    const uint32_t nw = (uint32_t)std::min<uint64_t>(batch, windows - w);
    uint32_t drawn = 0, present = 0;
    double t0 = tick();
    rc = post_verify_data_sample(cfg->seed, cfg->sample_every, start, end, w,
                                 sample.data(), nw, &drawn);
    if (rc == POST_OK)
      rc = gather(sample.data(), drawn, r.h_idx[parity].get(),
                  r.h_exp[parity].get(), &present);
    t_gather += tick() - t0;
    if (rc != POST_OK) return rc;
    report->labels_missing += drawn - present;
    in_batch[parity] = present;
    if (present) {
      HIP_TRY(hipMemcpyAsync(r.d_idx[parity].get(), r.h_idx[parity].get(),
                             (size_t)present * 8, hipMemcpyHostToDevice,
                             stream));
      HIP_TRY(hipMemcpyAsync(r.d_exp[parity].get(), r.h_exp[parity].get(),
                             (size_t)present * POST_LABEL_SIZE,
                             hipMemcpyHostToDevice, stream));
      HIP_TRY(hipMemsetAsync(r.d_count[parity].get(), 0,
                             sizeof(unsigned int), stream));
      aa.label.count = present;
      aa.label.indices = r.d_idx[parity].get();
      aa.expected = (const uint4 *)r.d_exp[parity].get();
      aa.mismatch = r.d_mis[parity].get();
      aa.count = r.d_count[parity].get();
      HIP_TRY(poste_launch_label_audit(&aa, blocks, stream));
      HIP_TRY(hipMemcpyAsync(r.h_count.get() + parity,
                             r.d_count[parity].get(), sizeof(unsigned int),
                             hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipEventRecord(r.done[parity].get(), stream));
    }
    if (have_prev) {
      t0 = tick();
      rc = drain(parity ^ 1);
      t_drain += tick() - t0;
      if (rc != POST_OK) return rc;
    }
    have_prev = true;
    w += nw;
  }
  {
    const double t0 = tick();
    rc = drain(parity ^ 1);
    t_drain += tick() - t0;
  }
  const double t_loop_end = tick();
  res.reset();
  if (dbg)
    std::fprintf(stderr,
                 "[audit] lanes=%llu batch=%llu windows=%llu alloc %.3fs "
                 "gather %.3fs wait+collect %.3fs free %.3fs total %.3fs\n",
                 (unsigned long long)lanes, (unsigned long long)batch,
                 (unsigned long long)windows, t_alloc, t_gather, t_drain,
                 tick() - t_loop_end, tick() - t_start);
  return rc;
}

static int audit_check_args(const PostAuditConfig *cfg, PostBadLabel *bad,
                            uint32_t cap, PostAuditReport *report) {
  if (!cfg || !report || (cap && !bad)) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  if (cfg->sample_every == 0) {
    set_error("sample_every must be >= 1");
    return POST_ERR_INVALID_ARGS;
  }
  const bool whole = cfg->index_start == 0 && cfg->index_end == 0;
  if (!whole && cfg->index_start >= cfg->index_end) {
    set_error("empty or inverted index range");
    return POST_ERR_INVALID_ARGS;
  }
  return POST_OK;
}

int post_verify_data_buffer(const uint8_t *labels, uint64_t count,
                            uint64_t index_base, const uint8_t node_id[32],
                            const uint8_t commitment_atx_id[32],
                            uint32_t scrypt_n, const PostAuditConfig *cfg,
                            PostBadLabel *bad, uint32_t cap,
                            PostAuditReport *report) {
  if (!labels || !node_id || !commitment_atx_id || count == 0 ||
      index_base + count < index_base) {
    set_error("null or empty label buffer");
    return POST_ERR_INVALID_ARGS;
  }
  if (scrypt_n < 2 || (scrypt_n & (scrypt_n - 1))) {
    set_error("scrypt N must be a power of two >= 2");
    return POST_ERR_INVALID_ARGS;
  }
  int rc = audit_check_args(cfg, bad, cap, report);
  if (rc != POST_OK) return rc;
  uint64_t start = index_base, end = index_base + count;
  if (cfg->index_start || cfg->index_end) {
    start = cfg->index_start;
    end = cfg->index_end;
  }
  if (start < index_base || end > index_base + count) {
    set_error("index range beyond the label buffer");
    return POST_ERR_INVALID_ARGS;
  }
  uint8_t commitment[32];
  poste::commitment(node_id, commitment_atx_id, commitment);
  AuditGather gather = [labels, index_base](const uint64_t *idx, uint32_t n,
                                            uint64_t *out_idx,
                                            uint8_t *out_lab,
                                            uint32_t *n_out) {
    for (uint32_t i = 0; i < n; i++) {
      out_idx[i] = idx[i];
      std::memcpy(out_lab + (size_t)i * POST_LABEL_SIZE,
                  labels + (idx[i] - index_base) * POST_LABEL_SIZE,
                  POST_LABEL_SIZE);
    }
    *n_out = n;
    return POST_OK;
  };
  return audit_core(gather, commitment, scrypt_n, start, end, cfg, bad, cap,
                    report);
}

/* Identity and geometry of a data dir, from its own postdata_metadata.json
 * (the audit and the healing paths).  POST_ERR_IO for a file that cannot be
 * read or lacks a valid field. */
struct DirMetadata {
  uint8_t node_id[32], atx_id[32];
  uint64_t lpu = 0, units = 0, max_file = 0, n = 0;
  uint64_t total = 0; /* NumUnits * LabelsPerUnit */
};

static int read_dir_metadata(const char *data_dir, DirMetadata &md) {
  std::string j;
  {
    const std::string path = std::string(data_dir) + "/postdata_metadata.json";
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) {
      set_error("cannot read " + path);
      return POST_ERR_IO;
    }
    char buf[4096];
    size_t rd;
    while ((rd = std::fread(buf, 1, sizeof buf, f)) > 0) j.append(buf, rd);
    std::fclose(f);
  }
  auto lacking = [](const char *field) {
    set_error(std::string("postdata_metadata.json lacks a valid ") + field);
    return POST_ERR_IO;
  };
  /* strict number reader: the audit is what runs on a damaged dir, so a
   * key followed by anything but a plain decimal that fits 64 bits counts
   * as lacking (md_find_u64 would read it as 0 or clamp it) */
  auto find_u64 = [&j](const char *key, uint64_t &out) {
    const std::string pat = std::string("\"") + key + "\": ";
    const size_t p = j.find(pat);
    if (p == std::string::npos) return false;
    const char *b = j.c_str() + p + pat.size();
    if (*b < '0' || *b > '9') return false;
    char *e = nullptr;
    errno = 0;
    out = strtoull(b, &e, 10);
    return errno == 0 && e != b;
  };
  std::string nid_b64, atx_b64;
  if (!md_find_string(j, "NodeId", nid_b64) ||
      !b64_decode(nid_b64, md.node_id, 32))
    return lacking("NodeId");
  if (!md_find_string(j, "CommitmentAtxId", atx_b64) ||
      !b64_decode(atx_b64, md.atx_id, 32))
    return lacking("CommitmentAtxId");
  if (!find_u64("LabelsPerUnit", md.lpu) || md.lpu == 0)
    return lacking("LabelsPerUnit");
  if (!find_u64("NumUnits", md.units) || md.units == 0)
    return lacking("NumUnits");
  if (!find_u64("MaxFileSize", md.max_file) || md.max_file == 0)
    return lacking("MaxFileSize");
  if (!find_u64("N", md.n) || md.n < 2 || md.n > (1ull << 31) ||
      (md.n & (md.n - 1)))
    return lacking("N");

  if (md.units > UINT64_MAX / md.lpu) {
    set_error("postdata_metadata.json: NumUnits*LabelsPerUnit overflows");
    return POST_ERR_IO;
  }
  md.total = md.units * md.lpu;
  return POST_OK;
}

int post_verify_data(const char *data_dir, const PostAuditConfig *cfg,
                     PostBadLabel *bad, uint32_t cap,
                     PostAuditReport *report) {
  if (!data_dir) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  int rc = audit_check_args(cfg, bad, cap, report);
  if (rc != POST_OK) return rc;

  /* identity and geometry come from the dir's own metadata */
  DirMetadata md;
  rc = read_dir_metadata(data_dir, md);
  if (rc != POST_OK) return rc;
  const uint8_t *node_id = md.node_id, *atx_id = md.atx_id;
  const uint64_t total = md.total, max_file = md.max_file, n = md.n;
  uint64_t start = 0, end = total;
  if (cfg->index_start || cfg->index_end) {
    start = cfg->index_start;
    end = cfg->index_end;
  }
  if (end > total) {
    set_error("index range beyond NumUnits*LabelsPerUnit");
    return POST_ERR_INVALID_ARGS;
  }

  AuditDirReader reader;
  reader.dir = data_dir;
  reader.per_file = std::max<uint64_t>(1, max_file / POST_LABEL_SIZE);
  reader.chunk = cfg->sample_every <= AUDIT_SEQ_MAX_K ? AUDIT_SEQ_CHUNK
                                                      : POST_LABEL_SIZE;
  uint8_t commitment[32];
  poste::commitment(node_id, atx_id, commitment);
  AuditGather gather = [&reader](const uint64_t *idx, uint32_t cnt,
                                 uint64_t *out_idx, uint8_t *out_lab,
                                 uint32_t *n_out) {
    uint32_t got = 0;
    for (uint32_t i = 0; i < cnt; i++) {
      const int r =
          reader.fetch(idx[i], out_lab + (size_t)got * POST_LABEL_SIZE);
      if (r < 0) return POST_ERR_IO;
      if (r) out_idx[got++] = idx[i];
    }
    *n_out = got;
    return POST_OK;
  };
  return audit_core(gather, commitment, (uint32_t)n, start, end, cfg, bad,
                    cap, report);
}

/* ------------------------- self-healing prove ------------------------- */

/* DESIGN 3.6.  The pages the seal pass found bad are recomputed from the
 * dir's identity, the recomputation is held against the sidecar digest by
 * post_seal_kernel (confirmed / unconfirmed), the proving scan is run again
 * over the recomputed labels alone, and confirmed pages can be written back.
 * post_prove_healed and post_repair_data share everything but the rescan. */

constexpr uint32_t HEAL_DEFAULT_MAX_PAGES = 4096;

struct HealWork {
  /* in */
  const std::vector<FileSpan> *files = nullptr;
  uint64_t total = 0; /* labels of the stream */
  DirMetadata md;
  uint32_t provider_id = 0;
  uint64_t scratch_bytes = 0;
  std::vector<uint64_t> pages; /* bad pages, ascending */
  std::vector<uint8_t> want;   /* their sidecar digests */
  /* out */
  DevBuf<uint8_t> d_labels;    /* compact buffer: page i at label 1024 i */
  uint64_t count = 0;          /* its labels: (P - 1) 1024 + n_last */
  std::vector<uint8_t> labels; /* the same on the host */
  std::vector<bool> confirmed;
  uint64_t pages_unconfirmed = 0, labels_repaired = 0, pages_written = 0;
  uint64_t hits_dropped = 0, hits_added = 0;
  uint64_t lanes = 0;
  double t_alloc = 0, t_regen = 0, t_digest = 0, t_rescan = 0, t_write = 0;

  uint64_t page_labels(size_t i) const {
    return std::min<uint64_t>(SEAL_PAGE, total - pages[i] * SEAL_PAGE);
  }
};

static double heal_tick() {
  return std::chrono::duration<double>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

/* Healing names a label by its place in the stream, so the stream must be in
 * global-index terms: every file but the last full, nothing past the space
 * (a sharded dir, or one with a short middle file, is refused). */
static int heal_check_layout(const std::vector<FileSpan> &files,
                             uint64_t total, const DirMetadata &md) {
  const uint64_t per_file = md.max_file / POST_LABEL_SIZE;
  for (size_t i = 0; i + 1 < files.size(); i++) {
    if (files[i].labels != per_file) {
      set_error("healing needs the label stream in global-index terms: " +
                files[i].path + " does not hold MaxFileSize / 16 labels");
      return POST_ERR_UNSUPPORTED;
    }
  }
  if (!files.empty() && files.back().labels > per_file) {
    set_error("healing needs the label stream in global-index terms: " +
              files.back().path + " holds more than MaxFileSize / 16 labels");
    return POST_ERR_UNSUPPORTED;
  }
  if (total > md.total) {
    set_error("healing needs the label stream in global-index terms: the "
              "dir holds more labels than NumUnits*LabelsPerUnit");
    return POST_ERR_UNSUPPORTED;
  }
  return POST_OK;
}

/* Steps 4 and 5: recompute w.pages into w.d_labels (index-list mode, lanes
 * and batches sized as audit_core sizes them), digest the buffer as it
 * stands, compare with the sidecar, count the labels that differ on disk. */
static int heal_regenerate(HealWork &w) {
  int rc = require_gpu(w.provider_id);
  if (rc != POST_OK) return rc;
  const size_t P = w.pages.size();
  /* ascending and inside the stream: only the last entry can be the short
   * last page, so page i of the compact buffer starts at label 1024 i */
  if (P == 0 || w.pages[P - 1] >= seal_pages(w.total)) {
    set_error("bad page beyond the stream");
    return POST_ERR;
  }
  for (size_t i = 0; i + 1 < P; i++) {
    if (w.pages[i] >= w.pages[i + 1]) {
      set_error("bad page list is not ascending");
      return POST_ERR;
    }
  }
  const uint64_t count = (uint64_t)(P - 1) * SEAL_PAGE + w.page_labels(P - 1);
  std::vector<uint64_t> idx((size_t)count);
  for (uint64_t q = 0; q < count; q++)
    idx[(size_t)q] = w.pages[(size_t)(q / SEAL_PAGE)] * SEAL_PAGE +
                     q % SEAL_PAGE;

  const uint32_t scrypt_n = (uint32_t)w.md.n;
  const uint32_t gap_shift = pick_gap_shift(scrypt_n);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  const uint64_t budget = w.scratch_bytes ? w.scratch_bytes
                                          : (uint64_t)((double)free_b * 0.80);
  const uint64_t per_lane = ((uint64_t)scrypt_n >> gap_shift) * 128;
  uint64_t lanes = budget / per_lane;
  lanes = std::min<uint64_t>(lanes, std::max<uint64_t>(count, 64));
  lanes = std::min<uint64_t>(lanes, poste_label_resident_slots(gap_shift));
  lanes = (lanes / 128) * 128;
  if (lanes == 0) lanes = 128;
  const uint64_t batch = std::min<uint64_t>(count, lanes * 4);
  const uint32_t blocks = (uint32_t)(lanes / 64); /* 64 quads/block */
  w.lanes = lanes;

  DevBuf<uint32_t> d_scratch, d_xbuf;
  DevBuf<uint64_t> d_idx;
  DevBuf<uint8_t> d_dig;
  /* the kernels run on the null stream: the device is idle before the
   * buffers above go, on every way out */
  struct DeviceSync {
    ~DeviceSync() { (void)hipDeviceSynchronize(); }
  } sync_first;
  double t0 = heal_tick();
  HIP_TRY(d_scratch.alloc((size_t)lanes * per_lane));
  HIP_TRY(d_xbuf.alloc((size_t)batch * 128));
  HIP_TRY(d_idx.alloc((size_t)count * 8));
  HIP_TRY(d_dig.alloc(P * SEAL_DIGEST));
  HIP_TRY(w.d_labels.alloc((size_t)count * POST_LABEL_SIZE));
  w.count = count;
  HIP_TRY(hipMemcpy(d_idx.get(), idx.data(), (size_t)count * 8,
                    hipMemcpyHostToDevice));
  w.t_alloc = heal_tick() - t0;

  t0 = heal_tick();
  uint8_t commitment[32];
  poste::commitment(w.md.node_id, w.md.atx_id, commitment);
  LabelKernelArgs la;
  std::memset(&la, 0, sizeof(la));
  load_commitment_words(commitment, la.commitment_le);
  la.scrypt_n = scrypt_n;
  la.gap_shift = gap_shift;
  la.scratch = d_scratch.get();
  la.scratch_lanes = lanes;
  la.xbuf = d_xbuf.get();
  /* the batches share scratch and xbuf: back to back on one stream */
  for (uint64_t off = 0; off < count; off += batch) {
    la.count = std::min(batch, count - off);
    la.indices = d_idx.get() + off;
    la.out = w.d_labels.get() + off * POST_LABEL_SIZE;
    HIP_TRY(poste_launch_label_kernel(&la, blocks, nullptr));
  }
  HIP_TRY(hipDeviceSynchronize());
  w.t_regen = heal_tick() - t0;

  t0 = heal_tick();
  SealKernelArgs ka;
  ka.labels = (const uint4 *)w.d_labels.get();
  ka.count = count;
  ka.digests = (uint4 *)d_dig.get();
  std::vector<uint8_t> got(P * SEAL_DIGEST);
  HIP_TRY(poste_launch_seal_kernel(&ka, nullptr));
  HIP_TRY(hipMemcpy(got.data(), d_dig.get(), got.size(),
                    hipMemcpyDeviceToHost));
  w.t_digest = heal_tick() - t0;
  w.labels.resize((size_t)count * POST_LABEL_SIZE);
  HIP_TRY(hipMemcpy(w.labels.data(), w.d_labels.get(), w.labels.size(),
                    hipMemcpyDeviceToHost));

  w.confirmed.assign(P, false);
  const LabelReader read = dir_reader(*w.files);
  std::vector<uint8_t> disk(SEAL_PAGE * POST_LABEL_SIZE);
  for (size_t i = 0; i < P; i++) {
    w.confirmed[i] = std::memcmp(got.data() + i * SEAL_DIGEST,
                                 w.want.data() + i * SEAL_DIGEST,
                                 SEAL_DIGEST) == 0;
    if (!w.confirmed[i]) w.pages_unconfirmed++;
    const uint64_t n = w.page_labels(i);
    rc = read(w.pages[i] * SEAL_PAGE, n, disk.data());
    if (rc != POST_OK) return rc;
    const uint8_t *fresh = w.labels.data() + i * SEAL_PAGE * POST_LABEL_SIZE;
    for (uint64_t k = 0; k < n; k++)
      if (std::memcmp(disk.data() + k * POST_LABEL_SIZE,
                      fresh + k * POST_LABEL_SIZE, POST_LABEL_SIZE) != 0)
        w.labels_repaired++;
  }
  return POST_OK;
}

/* Step 6: the production scan over the compact buffer at index base 0, with
 * the pass's own scan arguments and plan; first-pass hits of bad pages go,
 * the new ones come in under their global indices. */
static int heal_rescan(HealWork &w, const ScanKernelArgs &pass,
                       const ScanPlan &plan,
                       const std::vector<bool> &bad_map,
                       std::vector<PostScanHit> &hits) {
  const double t0 = heal_tick();
  ScanKernelArgs sa = pass;
  sa.labels = (const uint4 *)w.d_labels.get();
  sa.count = w.count;
  sa.index_base = 0;
  HIP_TRY(hipMemset(sa.hit_count, 0, 4));
  HIP_TRY(poste_launch_scan(&sa, &plan, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  unsigned int got = 0;
  HIP_TRY(hipMemcpy(&got, sa.hit_count, 4, hipMemcpyDeviceToHost));
  if (got > sa.hit_cap) {
    set_error("scan hit buffer overflow (pathological K1/num_labels "
              "configuration)");
    return POST_ERR;
  }
  std::vector<PostScanHit> fresh(got);
  if (got)
    HIP_TRY(hipMemcpy(fresh.data(), sa.hits, sizeof(PostScanHit) * got,
                      hipMemcpyDeviceToHost));
  const size_t before = hits.size();
  hits.erase(std::remove_if(hits.begin(), hits.end(),
                            [&](const PostScanHit &h) {
                              return (bool)bad_map[h.index / SEAL_PAGE];
                            }),
             hits.end());
  w.hits_dropped = before - hits.size();
  for (PostScanHit &h : fresh) {
    const uint64_t q = h.index;
    if (q >= w.count) {
      set_error("rescan hit outside the compact buffer");
      return POST_ERR;
    }
    h.index = w.pages[(size_t)(q / SEAL_PAGE)] * SEAL_PAGE + q % SEAL_PAGE;
    hits.push_back(h);
  }
  w.hits_added = got;
  w.t_rescan = heal_tick() - t0;
  return POST_OK;
}

/* Step 7: confirmed pages over the file bytes; a page may span two files,
 * every touched file is synced once.  Unconfirmed pages are never written. */
static int heal_write_back(HealWork &w) {
  const double t0 = heal_tick();
  std::map<size_t, int> fds; /* file number -> descriptor */
  auto close_all = [&] {
    for (auto &kv : fds) ::close(kv.second);
  };
  for (size_t i = 0; i < w.pages.size(); i++) {
    if (!w.confirmed[i]) continue;
    uint64_t pos = w.pages[i] * SEAL_PAGE; /* stream label */
    uint64_t left = w.page_labels(i);
    const uint8_t *src = w.labels.data() + i * SEAL_PAGE * POST_LABEL_SIZE;
    for (size_t f = 0; f < w.files->size() && left; f++) {
      const FileSpan &fs = (*w.files)[f];
      if (pos < fs.first_label || pos >= fs.first_label + fs.labels) continue;
      const uint64_t in_file = pos - fs.first_label;
      const uint64_t take = std::min(fs.labels - in_file, left);
      auto it = fds.find(f);
      if (it == fds.end()) {
        const int fd = ::open(fs.path.c_str(), O_WRONLY);
        if (fd < 0) {
          close_all();
          set_error("cannot open " + fs.path + " for writing");
          return POST_ERR_IO;
        }
        it = fds.emplace(f, fd).first;
      }
      size_t done = 0;
      const size_t bytes = (size_t)take * POST_LABEL_SIZE;
      while (done < bytes) {
        const ssize_t r =
            ::pwrite(it->second, src + done, bytes - done,
                     (off_t)(in_file * POST_LABEL_SIZE + done));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          close_all();
          set_error("short write to " + fs.path);
          return POST_ERR_IO;
        }
        done += (size_t)r;
      }
      src += bytes;
      pos += take;
      left -= take;
    }
    if (left) {
      close_all();
      set_error("label range not covered by postdata files");
      return POST_ERR_IO;
    }
    w.pages_written++;
  }
  int rc = POST_OK;
  for (auto &kv : fds) {
    if (::fsync(kv.second) != 0 && rc == POST_OK) {
      set_error("cannot sync " + (*w.files)[kv.first].path);
      rc = POST_ERR_IO;
    }
  }
  close_all();
  w.t_write = heal_tick() - t0;
  return rc;
}

static void heal_debug(const HealWork &w) {
  if (!getenv("POST_HEAL_DEBUG")) return; /* where the time went (stderr) */
  std::fprintf(stderr,
               "[heal] pages=%zu labels=%llu lanes=%llu alloc %.4fs "
               "regenerate %.4fs digest %.4fs rescan %.4fs write %.4fs\n",
               w.pages.size(), (unsigned long long)w.count,
               (unsigned long long)w.lanes, w.t_alloc, w.t_regen, w.t_digest,
               w.t_rescan, w.t_write);
}

static void heal_report(const SealChecker &chk, const HealWork &w,
                        bool healed, PostHealReport *r) {
  std::memset(r, 0, sizeof(*r));
  r->total_labels = chk.total;
  r->pages = seal_pages(chk.total);
  r->pages_bad = chk.pages_bad;
  if (!healed) return;
  r->pages_healed = w.pages.size();
  r->pages_unconfirmed = w.pages_unconfirmed;
  r->labels_repaired = w.labels_repaired;
  r->hits_dropped = w.hits_dropped;
  r->hits_added = w.hits_added;
  r->pages_written = w.pages_written;
}

/* the rungs both healing entries share, after their NULL checks and before
 * a GPU is required */
static int heal_open(const char *data_dir, std::vector<FileSpan> &files,
                     SealChecker &chk, HealWork &w) {
  const uint64_t total = map_postdata(data_dir, files);
  int rc = chk.open(data_dir, total);
  if (rc != POST_OK) return rc;
  if (total == 0) {
    set_error("no postdata_*.bin in data_dir");
    return POST_ERR_IO;
  }
  rc = read_dir_metadata(data_dir, w.md);
  if (rc != POST_OK) return rc;
  rc = heal_check_layout(files, total, w.md);
  if (rc != POST_OK) return rc;
  w.files = &files;
  w.total = total;
  return POST_OK;
}

int post_prove_healed(const char *data_dir, const PostProveConfig *cfg,
                      const PostHealConfig *heal, PostProof *out,
                      uint64_t *bad_pages, uint32_t cap, PostHealReport *r) {
  if (!data_dir || !cfg || !heal || !out || !r || (cap > 0 && !bad_pages)) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  std::vector<FileSpan> files;
  SealChecker chk;
  HealWork w;
  int rc = heal_open(data_dir, files, chk, w);
  if (rc != POST_OK) return rc;
  const uint64_t limit =
      heal->max_pages ? heal->max_pages : HEAL_DEFAULT_MAX_PAGES;
  w.provider_id = cfg->provider_id;
  w.scratch_bytes = heal->scratch_bytes;

  std::vector<bool> bad_map(seal_pages(w.total), false);
  chk.bad_pages = bad_pages;
  chk.cap = cap;
  chk.bad_map = &bad_map;
  chk.keep = &w.pages;
  chk.keep_want = &w.want;
  chk.keep_cap = limit;
  SealSink sink = [&chk](uint64_t first, uint64_t n, const uint8_t *d) {
    return chk.compare(first, n, d);
  };
  bool healed = false;
  /* by the time the hook runs the pass is over: chk holds every bad page */
  HitHook hook = [&](const ScanKernelArgs &scan, const ScanPlan &plan,
                     std::vector<PostScanHit> &hits) -> int {
    if (chk.pages_bad == 0 || chk.pages_bad > limit) return POST_OK;
    int hrc = heal_regenerate(w);
    if (hrc == POST_OK) hrc = heal_rescan(w, scan, plan, bad_map, hits);
    if (hrc == POST_OK && heal->write_back) hrc = heal_write_back(w);
    if (hrc == POST_OK) healed = true;
    return hrc;
  };
  std::vector<uint64_t> winner;
  rc = prove_core(dir_reader(files), w.total, cfg, out, &sink, &winner, &hook);
  if (healed) heal_debug(w);
  if (rc != POST_OK) return rc;
  heal_report(chk, w, healed, r);
  if (healed) {
    /* no index of the proof lies in a page that is still bad; what is left
     * to doubt is a page the seal could not confirm */
    for (uint64_t idx : winner) {
      const auto at = std::lower_bound(w.pages.begin(), w.pages.end(),
                                       idx / SEAL_PAGE);
      if (at != w.pages.end() && *at == idx / SEAL_PAGE &&
          !w.confirmed[(size_t)(at - w.pages.begin())])
        r->proof_touches_unconfirmed_page = 1;
    }
  } else if (chk.pages_bad) {
    r->heal_skipped = 1;
    for (uint64_t idx : winner)
      if (bad_map[idx / SEAL_PAGE]) r->proof_touches_bad_page = 1;
  }
  return POST_OK;
}

int post_repair_data(const char *data_dir, uint32_t provider_id,
                     const PostHealConfig *heal, uint64_t *bad_pages,
                     uint32_t cap, PostHealReport *r) {
  if (!data_dir || !heal || !r || (cap > 0 && !bad_pages)) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  std::vector<FileSpan> files;
  SealChecker chk;
  HealWork w;
  int rc = heal_open(data_dir, files, chk, w);
  if (rc != POST_OK) return rc;
  rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;
  const uint64_t limit =
      heal->max_pages ? heal->max_pages : HEAL_DEFAULT_MAX_PAGES;
  w.provider_id = provider_id;
  w.scratch_bytes = heal->scratch_bytes;
  chk.bad_pages = bad_pages;
  chk.cap = cap;
  chk.keep = &w.pages;
  chk.keep_want = &w.want;
  chk.keep_cap = limit;
  SealSink sink = [&chk](uint64_t first, uint64_t n, const uint8_t *d) {
    return chk.compare(first, n, d);
  };
  rc = label_pipeline(dir_reader(files), w.total, nullptr, nullptr, &sink);
  if (rc != POST_OK) return rc;
  const bool heal_it = chk.pages_bad && chk.pages_bad <= limit;
  if (heal_it) {
    rc = heal_regenerate(w);
    if (rc == POST_OK) rc = heal_write_back(w);
    heal_debug(w);
    if (rc != POST_OK) return rc;
  }
  heal_report(chk, w, heal_it, r);
  if (chk.pages_bad && !heal_it) r->heal_skipped = 1;
  return POST_OK;
}

/* ------------------- seal during init: assembly ------------------- */

/* One postdata_seal.part-<index_start> of a dir, header checked. */
struct SealPart {
  std::string path;
  uint64_t first = 0, end = 0; /* pages [first, end) */
  uint64_t have = 0;           /* digests in the file */
};

/* The parts of DESIGN 3.7 put together into the sidecar of 3.5.  `quiet` is
 * the call a session makes when its own range is complete: whatever keeps
 * the parts from being assembled (other shards still running, a damaged
 * part of another shard) is then left for the direct call to report. */
static int seal_assemble(const char *data_dir, uint64_t *pages, bool quiet) {
  if (pages) *pages = 0;
  DirMetadata md;
  int rc = read_dir_metadata(data_dir, md);
  if (rc != POST_OK) return quiet ? POST_OK : rc;
  const uint64_t npages = seal_pages(md.total);
  const std::string dir(data_dir);
  const std::string sidecar = dir + "/postdata_seal.bin";
  auto fail = [quiet](const std::string &msg) -> int {
    if (quiet) return POST_OK;
    set_error(msg);
    return POST_ERR_IO;
  };

  static const char PREFIX[] = "postdata_seal.part-";
  std::vector<SealPart> parts;
  DIR *dh = ::opendir(data_dir);
  if (!dh) return fail("cannot list " + dir);
  std::vector<std::string> names;
  while (struct dirent *de = ::readdir(dh)) {
    if (std::strncmp(de->d_name, PREFIX, sizeof PREFIX - 1) == 0)
      names.push_back(de->d_name);
  }
  ::closedir(dh);
  for (const std::string &name : names) {
    const char *num = name.c_str() + sizeof PREFIX - 1;
    char *e = nullptr;
    errno = 0;
    const uint64_t start = strtoull(num, &e, 10);
    if (*num < '0' || *num > '9' || *e != 0 || errno != 0) continue;
    SealPart p;
    p.path = dir + "/" + name;
    FILE *f = std::fopen(p.path.c_str(), "rb");
    if (!f) {
      if (errno == ENOENT) continue; /* another shard assembled meanwhile */
      return fail("cannot open " + p.path);
    }
    uint8_t hdr[SEALP_HEADER];
    struct stat st;
    const bool ok = fstat(fileno(f), &st) == 0 &&
                    std::fread(hdr, 1, SEALP_HEADER, f) == SEALP_HEADER;
    std::fclose(f);
    if (!ok) return fail(name + " is shorter than its header");
    if (std::memcmp(hdr, SEALP_MAGIC, 8) != 0)
      return fail(name + " has a wrong magic");
    if (get_le(hdr + 8, 4) != SEAL_PAGE || get_le(hdr + 12, 4) != SEAL_DIGEST)
      return fail(name + " has an unsupported page_labels or digest_bytes");
    p.first = get_le(hdr + 16, 8);
    p.end = get_le(hdr + 24, 8);
    p.have = ((uint64_t)st.st_size - SEALP_HEADER) / SEAL_DIGEST;
    if (p.first != start / SEAL_PAGE || start % SEAL_PAGE != 0)
      return fail(name + ": first_page " + std::to_string(p.first) +
                  " disagrees with the file name");
    if (p.end <= p.first || p.end > npages)
      return fail(name + ": pages [" + std::to_string(p.first) + ", " +
                  std::to_string(p.end) + ") lie outside the dir's " +
                  std::to_string(npages) + " pages");
    parts.push_back(p);
  }
  if (parts.empty()) {
    /* nothing to assemble: fine when it has been done already */
    FILE *f = std::fopen(sidecar.c_str(), "rb");
    uint8_t hdr[SEAL_HEADER];
    const bool done = f && std::fread(hdr, 1, SEAL_HEADER, f) == SEAL_HEADER &&
                      std::memcmp(hdr, SEAL_MAGIC, 8) == 0 &&
                      get_le(hdr + 16, 8) == md.total;
    if (f) std::fclose(f);
    if (!done)
      return fail("no postdata_seal.part-* in " + dir +
                  " and no finished postdata_seal.bin: pages [0, " +
                  std::to_string(npages) + ") are missing");
    if (pages) *pages = npages;
    return POST_OK;
  }
  std::sort(parts.begin(), parts.end(),
            [](const SealPart &a, const SealPart &b) {
              return a.first < b.first;
            });
  auto missing = [](uint64_t a, uint64_t b) {
    return "pages [" + std::to_string(a) + ", " + std::to_string(b) +
           ") are missing";
  };
  uint64_t next = 0;
  for (const SealPart &p : parts) {
    if (p.first > next)
      return fail("the parts leave a gap: " + missing(next, p.first));
    if (p.first < next)
      return fail("the parts overlap: pages [" + std::to_string(p.first) +
                  ", " + std::to_string(std::min(next, p.end)) +
                  ") are in more than one");
    if (p.have < p.end - p.first)
      return fail(p.path.substr(dir.size() + 1) + " is short, its shard is "
                  "not finished: " + missing(p.first + p.have, p.end));
    next = p.end;
  }
  if (next < npages)
    return fail("the parts leave a gap: " + missing(next, npages));

  /* as post_seal_data: temporary in the same dir, renamed into place; the
   * name is the process's own, since two shards may finish together */
  const std::string tmp = sidecar + ".tmp." + std::to_string((long)getpid());
  FILE *out = std::fopen(tmp.c_str(), "wb");
  if (!out) {
    set_error("cannot write " + tmp);
    return POST_ERR_IO;
  }
  uint8_t hdr[SEAL_HEADER] = {0};
  std::memcpy(hdr, SEAL_MAGIC, 8);
  put_le(hdr + 8, SEAL_PAGE, 4);
  put_le(hdr + 12, SEAL_DIGEST, 4);
  put_le(hdr + 16, md.total, 8);
  rc = std::fwrite(hdr, 1, SEAL_HEADER, out) == SEAL_HEADER ? POST_OK
                                                            : POST_ERR_IO;
  bool vanished = false;
  std::vector<uint8_t> buf;
  for (size_t i = 0; i < parts.size() && rc == POST_OK; i++) {
    const SealPart &p = parts[i];
    buf.resize((size_t)((p.end - p.first) * SEAL_DIGEST));
    FILE *f = std::fopen(p.path.c_str(), "rb");
    if (!f) {
      vanished = errno == ENOENT;
      rc = POST_ERR_IO;
      break;
    }
    if (std::fseek(f, (long)SEALP_HEADER, SEEK_SET) != 0 ||
        std::fread(buf.data(), 1, buf.size(), f) != buf.size() ||
        std::fwrite(buf.data(), 1, buf.size(), out) != buf.size())
      rc = POST_ERR_IO;
    std::fclose(f);
  }
  if (rc == POST_OK && (std::fflush(out) != 0 || fsync(fileno(out)) != 0))
    rc = POST_ERR_IO;
  std::fclose(out);
  if (rc == POST_OK && std::rename(tmp.c_str(), sidecar.c_str()) != 0)
    rc = POST_ERR_IO;
  if (rc != POST_OK) {
    (void)::unlink(tmp.c_str());
    /* a part that went away under us: the shard that finished beside this
     * one has assembled and is removing them */
    struct stat st;
    if (vanished && ::stat(sidecar.c_str(), &st) == 0) {
      if (pages) *pages = npages;
      return POST_OK;
    }
    set_error("cannot write " + sidecar + " from the part files");
    return rc;
  }
  for (const SealPart &p : parts)
    if (::unlink(p.path.c_str()) != 0 && errno != ENOENT) {
      set_error("cannot remove " + p.path);
      return POST_ERR_IO;
    }
  if (pages) *pages = npages;
  return POST_OK;
}

int post_seal_assemble(const char *data_dir, uint64_t *pages) {
  if (!data_dir) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  return seal_assemble(data_dir, pages, false);
}

/* the hit parts of DESIGN 3.8 merged into the initial proof; reads only */
int post_init_proof_assemble(const char *data_dir, PostProof *out,
                             PostInitProofReport *r) {
  if (!data_dir || !out) {
    set_error("null args");
    return POST_ERR_INVALID_ARGS;
  }
  DirMetadata md;
  int rc = read_dir_metadata(data_dir, md);
  if (rc != POST_OK) return rc;
  std::string err;
  rc = initproof::assemble_dir(data_dir, md.total, out, r, err);
  if (rc != POST_OK) set_error(err);
  return rc;
}

int post_seal_digest_stream(const uint8_t *labels, uint64_t count,
                            uint64_t first_index, const uint64_t *cuts,
                            uint32_t n_cuts, uint32_t stream_end,
                            uint32_t provider_id, uint8_t *digests,
                            uint64_t cap_pages, uint64_t *n_pages) {
  if (!labels || !digests || !n_pages || count == 0 || (n_cuts && !cuts)) {
    set_error("null or empty buffer");
    return POST_ERR_INVALID_ARGS;
  }
  if (first_index % SEAL_PAGE != 0 || first_index + count < first_index) {
    set_error("first_index must be a multiple of 1024 and the stream must "
              "not wrap");
    return POST_ERR_INVALID_ARGS;
  }
  for (uint32_t i = 0; i < n_cuts; i++)
    if (cuts[i] > count || (i && cuts[i] < cuts[i - 1])) {
      set_error("cuts must ascend and lie within the buffer");
      return POST_ERR_INVALID_ARGS;
    }
  const uint64_t out_pages = stream_end ? seal_pages(count) : count / SEAL_PAGE;
  if (cap_pages < out_pages) {
    set_error("digest buffer holds fewer pages than the labels make");
    return POST_ERR_INVALID_ARGS;
  }
  int rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;

  DevBuf<uint4> d_labels, d_dig;
  DevBuf<SealCarry> d_carry;
  const uint64_t all_pages = seal_pages(count);
  HIP_TRY(d_labels.alloc((size_t)count * 16));
  HIP_TRY(d_dig.alloc((size_t)(all_pages * SEAL_DIGEST)));
  HIP_TRY(d_carry.alloc(2 * sizeof(SealCarry)));
  HIP_TRY(hipMemcpy(d_labels.get(), labels, (size_t)count * 16,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_dig.get(), 0, (size_t)(all_pages * SEAL_DIGEST)));
  HIP_TRY(hipMemset(d_carry.get(), 0, 2 * sizeof(SealCarry)));
  uint64_t launches = 0, at = 0;
  for (uint32_t i = 0; i <= n_cuts; i++) {
    const uint64_t to = i < n_cuts ? cuts[i] : count;
    if (to == at) continue;
    SealStreamArgs a;
    a.labels = d_labels.get() + at;
    a.g0 = first_index + at;
    a.count = to - at;
    a.stream_end = stream_end ? first_index + count : UINT64_MAX;
    a.carry_in = d_carry.get() + (launches & 1);
    a.carry_out = d_carry.get() + ((launches + 1) & 1);
    /* lane l of the segment is page at / 1024 + l of the buffer */
    a.digests = d_dig.get() + at / SEAL_PAGE;
    HIP_TRY(poste_launch_seal_stream_kernel(&a, nullptr));
    launches++;
    at = to;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (out_pages)
    HIP_TRY(hipMemcpy(digests, d_dig.get(), (size_t)(out_pages * SEAL_DIGEST),
                      hipMemcpyDeviceToHost));
  *n_pages = out_pages;
  return POST_OK;
}

/* ------------------------- verification ------------------------- */

int post_verify_batch(const PostProof *proofs, const PostProofMetadata *metas,
                      uint32_t n, const PostVerifyConfig *cfg, int *statuses,
                      uint32_t *invalid_indices) {
  return post_verify_batch_seeded(proofs, metas, n, cfg, nullptr, 0,
                                  statuses, invalid_indices);
}

/* The batch behind every verification entry, after validation and
 * require_gpu: n proofs and n_vrf VRF items (either may be 0) in one label
 * launch.  Proof tasks come first, in proof order; the VRF items that reach
 * the device follow, item j under commitment slot n + j and threshold slot
 * j.  A VRF item with num_labels == 0 gets POST_ERR_INVALID_ARGS and no
 * task. */
static int verify_core(const PostProof *proofs, const PostProofMetadata *metas,
                       uint32_t n, const PostVerifyConfig *cfg,
                       const uint8_t *subset_seeds, size_t seed_len,
                       const PostProofMetadata *vrf_metas,
                       const uint64_t *vrf_indices, uint32_t n_vrf,
                       int *statuses, uint32_t *invalid_indices,
                       int *vrf_statuses) {
  int rc = POST_OK;
  struct Task {
    uint64_t label_index;
    uint32_t proof;
    uint32_t position; /* position within the proof's k2 indices */
  };
  std::vector<Task> tasks;
  std::vector<uint32_t> commit_words(((size_t)n + n_vrf) * 8);
  std::vector<std::vector<uint64_t>> proof_indices(n);
  std::vector<std::vector<Task>> per_proof_tasks(n);
  /* position of a proof's first out-of-range index among the positions
   * checked, UINT32_MAX for none.  The verdict walks the positions in
   * order and stops at the first failure of either kind (an index out of
   * range, a label above the difficulty), so this one holds only if no
   * task before it fails on the device. */
  std::vector<uint32_t> oor_position(n, UINT32_MAX);

  /* per-proof host prep (commitment blake3, pow verify, index unpack,
   * subset sampling) is independent across proofs and dominates the
   * K3=1 batch wall time — spread it across host threads; every slot
   * written is per-proof disjoint.  The commitment table is indexed by
   * ABSOLUTE proof number from the kernel tasks, so every proof gets a
   * slot — including ones rejected here. */
  auto prep_one = [&](uint32_t p) {
    statuses[p] = POST_OK;
    const PostProof &pr = proofs[p];
    const PostProofMetadata &me = metas[p];
    {
      uint8_t cm[32];
      poste::commitment(me.node_id, me.commitment_atx_id, cm);
      std::memcpy(commit_words.data() + (size_t)p * 8, cm, 32);
    }
    uint64_t num_labels = (uint64_t)me.num_units * me.labels_per_unit;
    if (num_labels == 0) { /* malformed metadata */
      statuses[p] = POST_ERR_INVALID_ARGS;
      return;
    }
    uint32_t bpi = poste::bits_per_index(num_labels);
    if (pr.num_indices != cfg->k2 ||
        pr.indices_len != ((uint64_t)cfg->k2 * bpi + 7) / 8) {
      statuses[p] = POST_ERR_INVALID_ARGS;
      return;
    }
    uint32_t group = pr.nonce / POSTE_NONCE_GROUP;
    if (poste::k2pow_verify_blake3(me.challenge, group, pr.pow,
                                   cfg->pow_difficulty) != 0) {
      statuses[p] = POST_ERR_POW;
      return;
    }
    proof_indices[p].resize(cfg->k2);
    poste::unpack_indices(pr.indices, cfg->k2, bpi,
                          proof_indices[p].data());

    std::vector<uint32_t> positions;
    const uint8_t *seed = subset_seeds ? subset_seeds + (size_t)p * seed_len
                                       : cfg->subset_seed;
    size_t slen = subset_seeds ? seed_len : cfg->subset_seed_len;
    if (cfg->selected_index >= 0) {
      positions.push_back((uint32_t)cfg->selected_index);
    } else if (seed && cfg->k3 < cfg->k2) {
      positions.resize(cfg->k3);
      poste::subset_positions(cfg->k2, cfg->k3, seed, slen,
                              positions.data());
    } else {
      positions.resize(cfg->k2);
      for (uint32_t i = 0; i < cfg->k2; i++) positions[i] = i;
    }
    for (uint32_t pos : positions) {
      if (pos >= cfg->k2) {
        statuses[p] = POST_ERR_INVALID_ARGS;
        return;
      }
      uint64_t li = proof_indices[p][pos];
      if (li >= num_labels) { /* later positions cannot decide */
        oor_position[p] = pos;
        return;
      }
      per_proof_tasks[p].push_back({li, p, pos});
    }
  };
  /* a VRF item's prep: its commitment into slot n + j */
  auto vrf_prep_one = [&](uint32_t j) {
    const PostProofMetadata &me = vrf_metas[j];
    if ((uint64_t)me.num_units * me.labels_per_unit == 0) {
      vrf_statuses[j] = POST_ERR_INVALID_ARGS;
      return;
    }
    vrf_statuses[j] = POST_OK;
    uint8_t cm[32];
    poste::commitment(me.node_id, me.commitment_atx_id, cm);
    std::memcpy(commit_words.data() + ((size_t)n + j) * 8, cm, 32);
  };
  auto for_each_item = [](uint32_t count, auto &&one) {
    unsigned hw = std::thread::hardware_concurrency();
    unsigned nthreads = std::min<unsigned>(hw ? hw : 1, 32);
    if (count < 64) nthreads = 1; /* not worth spawning for small batches */
    if (nthreads <= 1) {
      for (uint32_t p = 0; p < count; p++) one(p);
    } else {
      std::vector<std::thread> ths;
      std::atomic<uint32_t> next{0};
      for (unsigned t = 0; t < nthreads; t++)
        ths.emplace_back([&] {
          for (;;) {
            uint32_t p = next.fetch_add(64);
            if (p >= count) return;
            uint32_t e = std::min(count, p + 64);
            for (; p < e; p++) one(p);
          }
        });
      for (auto &th : ths) th.join();
    }
  };
  for_each_item(n, prep_one);
  for_each_item(n_vrf, vrf_prep_one);
  /* concatenate in proof order (deterministic task->index mapping) */
  for (uint32_t p = 0; p < n; p++) {
    if (statuses[p] != POST_OK) continue;
    tasks.insert(tasks.end(), per_proof_tasks[p].begin(),
                 per_proof_tasks[p].end());
  }
  auto apply_out_of_range = [&] {
    for (uint32_t p = 0; p < n; p++) {
      if (statuses[p] != POST_OK || oor_position[p] == UINT32_MAX) continue;
      statuses[p] = POST_ERR_INVALID_INDEX;
      if (invalid_indices) invalid_indices[p] = oor_position[p];
    }
  };
  /* VRF items that go to the device, in item order */
  std::vector<uint32_t> vrf_items;
  vrf_items.reserve(n_vrf);
  for (uint32_t j = 0; j < n_vrf; j++)
    if (vrf_statuses[j] == POST_OK) vrf_items.push_back(j);
  const size_t n_ptasks = tasks.size();
  const size_t n_tasks = n_ptasks + vrf_items.size();
  if (n_tasks == 0) {
    apply_out_of_range();
    return POST_OK;
  }

  /* scratch-bounded chunks of label recomputes on the GPU */
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  uint32_t gap_shift = pick_gap_shift(cfg->scrypt_n);
  uint64_t per_lane = ((uint64_t)cfg->scrypt_n >> gap_shift) * 128;
  uint64_t max_lanes = (uint64_t)((double)free_b * 0.75) / per_lane;
  max_lanes = std::min<uint64_t>(max_lanes,
                                 poste_label_resident_slots(gap_shift));
  max_lanes = (max_lanes / 128) * 128;
  if (max_lanes == 0) max_lanes = 128;
  if (max_lanes == 0) {
    set_error("not enough memory for verification scratch");
    return POST_ERR_OOM;
  }

  std::vector<uint64_t> h_idx(n_tasks);
  std::vector<uint32_t> h_cid(n_tasks);
  for (size_t i = 0; i < n_ptasks; i++) {
    h_idx[i] = tasks[i].label_index;
    h_cid[i] = tasks[i].proof;
  }
  for (size_t k = 0; k < vrf_items.size(); k++) {
    h_idx[n_ptasks + k] = vrf_indices[vrf_items[k]];
    h_cid[n_ptasks + k] = n + vrf_items[k];
  }
  uint64_t lanes = std::min<uint64_t>(
      max_lanes, ((n_tasks + 127) / 128) * 128);

  /* per-proof cipher data for the device predicate (absolute indexing:
   * every proof gets a slot, matching task_proof).  Declared here,
   * COMPUTED after the label kernel launches — the ~10k blake3+AES key
   * expansions overlap the label recompute instead of preceding it. */
  std::vector<uint32_t> vrk((size_t)n * 44, 0);
  std::vector<uint8_t> vhalf(n, 0);
  std::vector<uint64_t> vdiff(n, 0);
  auto cipher_prep = [&] {
    for (uint32_t p = 0; p < n; p++) {
      if (statuses[p] != POST_OK) continue;
      const PostProof &pr = proofs[p];
      const PostProofMetadata &me = metas[p];
      uint8_t key[16];
      poste::prove_cipher_key(me.challenge, pr.nonce / POSTE_NONCES_PER_AES,
                              pr.pow, key);
      poste::aes128_expand(key, vrk.data() + (size_t)p * 44);
      vhalf[p] = (uint8_t)(pr.nonce % POSTE_NONCES_PER_AES);
      uint64_t num_labels = (uint64_t)me.num_units * me.labels_per_unit;
      vdiff[p] = poste::proving_difficulty(cfg->k1, num_labels);
    }
  };
  /* per-item VRF thresholds, computed beside cipher_prep */
  std::vector<uint8_t> vthr((size_t)n_vrf * 32, 0);
  auto vrf_threshold_prep = [&] {
    for (uint32_t j : vrf_items) {
      const PostProofMetadata &me = vrf_metas[j];
      poste::vrf_difficulty((uint64_t)me.num_units * me.labels_per_unit,
                            vthr.data() + (size_t)j * 32);
    }
  };
  DeviceTables tbl;
  if (n_ptasks) {
    rc = get_aes_tables((int)cfg->provider_id, tbl);
    if (rc != POST_OK) return rc;
  }

  std::vector<uint8_t> h_pass(n_tasks);
  const bool dbg = getenv("POST_VERIFY_DEBUG") != nullptr;
  auto tick = [] {
    return std::chrono::duration<double>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
  };
  double t0 = tick();
  {
    VerifyWorkspace *ws = get_verify_ws((int)cfg->provider_id);
    std::lock_guard<std::mutex> lk(ws->mu);
    rc = ws_reserve(ws, (size_t)lanes * per_lane, n_tasks,
                    commit_words.size());
    if (rc != POST_OK) return rc;
    if (dbg) {
      std::fprintf(stderr,
                   "[verify] reserve %.3fs (tasks=%zu lanes=%llu vrf=%u)\n",
                   tick() - t0, n_tasks, (unsigned long long)lanes, n_vrf);
      t0 = tick();
    }
    HIP_TRY(hipMemcpy(ws->d_idx.get(), h_idx.data(), h_idx.size() * 8,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ws->d_cid.get(), h_cid.data(), h_cid.size() * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ws->d_cm.get(), commit_words.data(),
                      commit_words.size() * 4, hipMemcpyHostToDevice));

    LabelKernelArgs la;
    std::memset(&la, 0, sizeof(la));
    la.scrypt_n = cfg->scrypt_n;
    la.gap_shift = gap_shift;
    la.xbuf = ws->d_xbuf.get();
    la.out_full = 1;
    la.scratch = ws->d_scratch.get();
    la.scratch_lanes = lanes;
    la.out = ws->d_out.get();
    la.indices = h_idx.size() ? ws->d_idx.get() : nullptr;
    la.commit_ids = ws->d_cid.get();
    la.commitments = ws->d_cm.get();
    la.count = n_tasks;
    if (dbg) {
      std::fprintf(stderr, "[verify] h2d %.3fs\n", tick() - t0);
      t0 = tick();
    }
    HIP_TRY(poste_launch_label_kernel(&la, (uint32_t)(lanes / 64),
                                      nullptr));
    cipher_prep(); /* overlaps the label kernel (launch is async) */
    vrf_threshold_prep();
    if (dbg) {
      (void)hipDeviceSynchronize();
      std::fprintf(stderr, "[verify] label kernel %.3fs\n", tick() - t0);
      t0 = tick();
    }
    rc = ws_reserve_proofs(ws, n_ptasks ? n : 0, vrf_items.empty() ? 0 : n_vrf);
    if (rc != POST_OK) return rc;
    if (n_ptasks) {
      /* device-side AES threshold predicate over the recomputed labels */
      HIP_TRY(hipMemcpy(ws->d_vrk.get(), vrk.data(), vrk.size() * 4,
                        hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(ws->d_half.get(), vhalf.data(), vhalf.size(),
                        hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(ws->d_vdiff.get(), vdiff.data(), vdiff.size() * 8,
                        hipMemcpyHostToDevice));
      VerifyPredArgs pa;
      std::memset(&pa, 0, sizeof(pa));
      pa.labels2 = (const uint4 *)ws->d_out.get();
      pa.count = n_ptasks;
      pa.te = tbl.d_te;
      pa.sbox = tbl.d_sbox;
      pa.rk = ws->d_vrk.get();
      pa.task_proof = ws->d_cid.get(); /* task->proof map doubles as commit id */
      pa.half = ws->d_half.get();
      pa.difficulty = ws->d_vdiff.get();
      pa.pass = ws->d_pass.get();
      uint32_t pblocks = (uint32_t)std::min<uint64_t>(
          (n_ptasks + THREADS - 1) / THREADS, VERIFY_PRED_MAX_BLOCKS);
      HIP_TRY(poste_launch_verify_pred_kernel(&pa, pblocks, nullptr));
    }
    if (!vrf_items.empty()) {
      /* the VRF predicate over the tail of the same label buffer; the
       * threshold table has a slot per ITEM (skipped items leave unused
       * zero slots) and the map carries each task's item number */
      HIP_TRY(hipMemcpy(ws->d_vthr.get(), vthr.data(), vthr.size(),
                        hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(ws->d_vmap.get(), vrf_items.data(),
                        vrf_items.size() * 4, hipMemcpyHostToDevice));
      VrfPredArgs va;
      std::memset(&va, 0, sizeof(va));
      va.labels2 = (const uint4 *)ws->d_out.get() + 2 * n_ptasks;
      va.count = vrf_items.size();
      va.thresholds = (const uint4 *)ws->d_vthr.get();
      va.task_thr = ws->d_vmap.get();
      va.pass = ws->d_pass.get() + n_ptasks;
      uint32_t vblocks = (uint32_t)std::min<uint64_t>(
          (vrf_items.size() + THREADS - 1) / THREADS, VERIFY_PRED_MAX_BLOCKS);
      HIP_TRY(poste_launch_vrf_pred_kernel(&va, vblocks, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    if (dbg) {
      std::fprintf(stderr, "[verify] predicate %.3fs\n", tick() - t0);
      t0 = tick();
    }
    HIP_TRY(hipMemcpy(h_pass.data(), ws->d_pass.get(), h_pass.size(),
                      hipMemcpyDeviceToHost));
  }

  /* collect per-proof verdicts from the device predicate */
  for (size_t i = 0; i < n_ptasks; i++) {
    const Task &t = tasks[i];
    if (statuses[t.proof] != POST_OK) continue;
    if (!h_pass[i]) {
      statuses[t.proof] = POST_ERR_INVALID_INDEX;
      if (invalid_indices) invalid_indices[t.proof] = t.position;
    }
  }
  apply_out_of_range();
  for (size_t k = 0; k < vrf_items.size(); k++)
    if (!h_pass[n_ptasks + k])
      vrf_statuses[vrf_items[k]] = POST_ERR_INVALID_INDEX;
  return POST_OK;
}

int post_verify_batch_seeded(const PostProof *proofs,
                             const PostProofMetadata *metas, uint32_t n,
                             const PostVerifyConfig *cfg,
                             const uint8_t *subset_seeds, size_t seed_len,
                             int *statuses, uint32_t *invalid_indices) {
  if (!proofs || !metas || !cfg || !statuses) return POST_ERR_INVALID_ARGS;
  if (cfg->pow_mode != POST_POW_MODE_BLAKE3) {
    set_error("RandomX k2pow is not supported (use POST_POW_MODE_BLAKE3)");
    return POST_ERR_UNSUPPORTED;
  }
  int rc = require_gpu(cfg->provider_id);
  if (rc != POST_OK) return rc;
  return verify_core(proofs, metas, n, cfg, subset_seeds, seed_len, nullptr,
                     nullptr, 0, statuses, invalid_indices, nullptr);
}

int post_verify_batch_vrf(const PostProof *proofs,
                          const PostProofMetadata *metas, uint32_t n,
                          const PostVerifyConfig *cfg,
                          const uint8_t *subset_seeds, size_t seed_len,
                          const PostProofMetadata *vrf_metas,
                          const uint64_t *vrf_indices, uint32_t n_vrf,
                          int *statuses, uint32_t *invalid_indices,
                          int *vrf_statuses) {
  if (!cfg) return POST_ERR_INVALID_ARGS;
  if (n > 0 && (!proofs || !metas || !statuses)) return POST_ERR_INVALID_ARGS;
  if (n_vrf > 0 && (!vrf_metas || !vrf_indices || !vrf_statuses))
    return POST_ERR_INVALID_ARGS;
  if (n > 0 && cfg->pow_mode != POST_POW_MODE_BLAKE3) {
    set_error("RandomX k2pow is not supported (use POST_POW_MODE_BLAKE3)");
    return POST_ERR_UNSUPPORTED;
  }
  if (n == 0 && n_vrf == 0) return POST_OK;
  int rc = require_gpu(cfg->provider_id);
  if (rc != POST_OK) return rc;
  return verify_core(proofs, metas, n, cfg, subset_seeds, seed_len, vrf_metas,
                     vrf_indices, n_vrf, statuses, invalid_indices,
                     vrf_statuses);
}

int post_verify_vrf_nonce_batch(const PostProofMetadata *metas,
                                const uint64_t *indices, uint32_t n,
                                uint32_t scrypt_n, uint32_t provider_id,
                                int *statuses) {
  PostVerifyConfig cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.selected_index = -1;
  cfg.pow_mode = POST_POW_MODE_BLAKE3;
  cfg.scrypt_n = scrypt_n;
  cfg.provider_id = provider_id;
  return post_verify_batch_vrf(nullptr, nullptr, 0, &cfg, nullptr, 0, metas,
                               indices, n, nullptr, nullptr, statuses);
}

int post_verify(const PostProof *proof, const PostProofMetadata *meta,
                const PostVerifyConfig *cfg, uint32_t *invalid_index) {
  int status = 0;
  uint32_t inv = 0;
  int rc = post_verify_batch(proof, meta, 1, cfg, &status, &inv);
  if (rc != POST_OK) return rc;
  if (invalid_index) *invalid_index = inv;
  return status;
}

int post_verify_vrf_nonce(const PostProofMetadata *meta, uint64_t index,
                          uint32_t scrypt_n, uint32_t provider_id) {
  if (!meta) return POST_ERR_INVALID_ARGS;
  int status = POST_OK;
  int rc = post_verify_vrf_nonce_batch(meta, &index, 1, scrypt_n, provider_id,
                                       &status);
  if (rc != POST_OK) return rc;
  if (status == POST_ERR_INVALID_INDEX)
    set_error("vrf nonce label above threshold");
  else if (status == POST_ERR_INVALID_ARGS)
    set_error("vrf nonce: num_units * labels_per_unit is zero");
  return status;
}

/* ------------------------- self-test exports ------------------------- */

void post_selftest_blake3(const uint8_t *msg, size_t len, uint8_t out[32]) {
  poste::blake3(msg, len, out, 32);
}

void post_selftest_aes128(const uint8_t key[16], const uint8_t in[16],
                          uint8_t out[16]) {
  uint32_t rk[44];
  poste::aes128_expand(key, rk);
  poste::aes128_enc_block(rk, in, out);
}

int post_selftest_label(const uint8_t node_id[32],
                        const uint8_t commitment_atx_id[32], uint64_t index,
                        uint32_t scrypt_n, uint8_t out[32]) {
  uint8_t cm[32];
  poste::commitment(node_id, commitment_atx_id, cm);
  return poste::host_label(cm, index, scrypt_n, out);
}

int post_selftest_verify_pred(const uint8_t *labels, uint64_t count,
                              const uint8_t *keys, const uint8_t *halves,
                              const uint64_t *difficulties, uint32_t n_proofs,
                              const uint32_t *task_proof, uint32_t max_blocks,
                              uint32_t provider_id, uint8_t *pass) {
  if (!labels || !keys || !halves || !difficulties || !task_proof || !pass ||
      count == 0 || n_proofs == 0)
    return POST_ERR_INVALID_ARGS;
  for (uint64_t i = 0; i < count; i++)
    if (task_proof[i] >= n_proofs) {
      set_error("task_proof entry out of range");
      return POST_ERR_INVALID_ARGS;
    }
  int rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;

  std::vector<uint32_t> rk((size_t)n_proofs * 44);
  for (uint32_t p = 0; p < n_proofs; p++)
    poste::aes128_expand(keys + (size_t)p * 16, rk.data() + (size_t)p * 44);
  DeviceTables tbl;
  rc = get_aes_tables((int)provider_id, tbl);
  if (rc != POST_OK) return rc;

  DevBuf<uint8_t> d_labels, d_half, d_pass;
  DevBuf<uint32_t> d_rk, d_task_proof;
  DevBuf<uint64_t> d_diff;
  HIP_TRY(d_labels.alloc((size_t)count * 32));
  HIP_TRY(d_task_proof.alloc((size_t)count * 4));
  HIP_TRY(d_pass.alloc((size_t)count));
  HIP_TRY(d_rk.alloc(rk.size() * 4));
  HIP_TRY(d_half.alloc(n_proofs));
  HIP_TRY(d_diff.alloc((size_t)n_proofs * 8));
  HIP_TRY(hipMemcpy(d_labels.get(), labels, (size_t)count * 32,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_task_proof.get(), task_proof, (size_t)count * 4,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_pass.get(), 0xEE, (size_t)count)); /* neither verdict */
  HIP_TRY(hipMemcpy(d_rk.get(), rk.data(), rk.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_half.get(), halves, n_proofs, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_diff.get(), difficulties, (size_t)n_proofs * 8,
                    hipMemcpyHostToDevice));

  VerifyPredArgs pa;
  std::memset(&pa, 0, sizeof(pa));
  pa.labels2 = (const uint4 *)d_labels.get();
  pa.count = count;
  pa.te = tbl.d_te;
  pa.sbox = tbl.d_sbox;
  pa.rk = d_rk.get();
  pa.task_proof = d_task_proof.get();
  pa.half = d_half.get();
  pa.difficulty = d_diff.get();
  pa.pass = d_pass.get();
  uint32_t pblocks = (uint32_t)std::min<uint64_t>(
      (count + THREADS - 1) / THREADS,
      max_blocks ? max_blocks : VERIFY_PRED_MAX_BLOCKS);
  HIP_TRY(poste_launch_verify_pred_kernel(&pa, pblocks, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(pass, d_pass.get(), (size_t)count, hipMemcpyDeviceToHost));
  return POST_OK;
}

int post_selftest_vrf_pred(const uint8_t *labels, uint64_t count,
                           const uint8_t *thresholds, uint32_t n_thr,
                           const uint32_t *task_thr, uint32_t max_blocks,
                           uint32_t provider_id, uint8_t *pass) {
  if (!labels || !thresholds || !task_thr || !pass || count == 0 ||
      n_thr == 0)
    return POST_ERR_INVALID_ARGS;
  for (uint64_t i = 0; i < count; i++)
    if (task_thr[i] >= n_thr) {
      set_error("task_thr entry out of range");
      return POST_ERR_INVALID_ARGS;
    }
  int rc = require_gpu(provider_id);
  if (rc != POST_OK) return rc;

  DevBuf<uint8_t> d_labels, d_thr, d_pass;
  DevBuf<uint32_t> d_task_thr;
  HIP_TRY(d_labels.alloc((size_t)count * 32));
  HIP_TRY(d_thr.alloc((size_t)n_thr * 32));
  HIP_TRY(d_task_thr.alloc((size_t)count * 4));
  HIP_TRY(d_pass.alloc((size_t)count));
  HIP_TRY(hipMemcpy(d_labels.get(), labels, (size_t)count * 32,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_thr.get(), thresholds, (size_t)n_thr * 32,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_task_thr.get(), task_thr, (size_t)count * 4,
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_pass.get(), 0xEE, (size_t)count)); /* neither verdict */

  VrfPredArgs va;
  std::memset(&va, 0, sizeof(va));
  va.labels2 = (const uint4 *)d_labels.get();
  va.count = count;
  va.thresholds = (const uint4 *)d_thr.get();
  va.task_thr = d_task_thr.get();
  va.pass = d_pass.get();
  uint32_t vblocks = (uint32_t)std::min<uint64_t>(
      (count + THREADS - 1) / THREADS,
      max_blocks ? max_blocks : VERIFY_PRED_MAX_BLOCKS);
  HIP_TRY(poste_launch_vrf_pred_kernel(&va, vblocks, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(pass, d_pass.get(), (size_t)count, hipMemcpyDeviceToHost));
  return POST_OK;
}

} /* extern "C" */
