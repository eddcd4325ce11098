/* kernels.hip — MI355X (gfx950/CDNA4) kernels for the POST hot path.
 *
 * Labeling (the init hot loop the reference reaches at
 *   activation/post.go:295): one label per 4-lane quad, run as a 3-kernel
 *   pipeline (SHA prologue -> register-lean ROMix at 8 waves/SIMD -> SHA
 *   tail + VRF reduce), working block staged through xbuf.  The N-entry
 *   ROMix scratchpad V (128 B * N per in-flight label at gap 1) lives in
 *   HBM; a quad's block accesses are aligned 64-B transactions.  No MFMA:
 *   a u32 add/xor/rotate hash loop (BASELINE.json north_star).  Also used
 *   in index-list mode for verification's label recompute
 *   (validation.go:182-222 -> K3 sampled indices) with per-task commitments.
 *
 * post_scan_*_kernel: the proving index scan (post-service GenProof,
 *   api/grpcserver/post_client.go:69-143): AES-128 over each 16-B label for
 *   n_ciphers ciphers (2 nonces per cipher), T-tables staged in LDS by one
 *   of three table policies, passing (nonce,index) pairs appended with a
 *   global atomic.
 *
 * post_seal_kernel: the postdata seal: 16 bytes of SHA-256 per
 *   1024-label page of a chunk the proving pass has on the device, one lane
 *   per page, 64-thread workgroups.
 *
 * post_seal_stream_kernel: the same digests over a stream that arrives in
 *   segments of any start and length (init batches); the page
 *   open at a segment's end is carried to the next launch.
 *
 * Wave size 64, 256-thread workgroups.  Grid-stride loops size the in-flight
 * label set to the scratch allocation, independent of batch size.
 */
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kernel_args.h"
#include "post_common.h"

#define POSTE_THREADS 256

/* ROMix scratch V is written once and read once ~N iterations later — far
 * beyond any cache. -DPOSTE_NT=1 builds with non-temporal loads/stores on
 * V to keep it out of L2 (A/B via POST_ENGINE_LIB). */
#if defined(POSTE_NT) && POSTE_NT
typedef uint32_t poste_v4u __attribute__((ext_vector_type(4)));
#define VSTORE(p, v)                                                           \
  do {                                                                         \
    uint4 _t = (v);                                                            \
    __builtin_nontemporal_store(*(poste_v4u *)&_t, (poste_v4u *)(p));          \
  } while (0)
#define VLOAD(p)                                                               \
  ({                                                                           \
    poste_v4u _r = __builtin_nontemporal_load((const poste_v4u *)(p));         \
    *(uint4 *)&_r;                                                             \
  })
#else
#define VSTORE(p, v) (*(p) = (v))
#define VLOAD(p) (*(p))
#endif

/* ------------------------- SHA-256 (device) ------------------------- */
__constant__ uint32_t c_sha_k[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1,
    0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
    0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b,
    0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
    0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t ror32(uint32_t x, int n) {
  return __builtin_rotateright32(x, n);
}

/* m holds big-endian message words; h updated in place. */
__device__ void sha_compress(uint32_t h[8], const uint32_t m[16]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = m[i];
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
  uint32_t e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; t++) {
    uint32_t wt;
    if (t < 16) {
      wt = w[t];
    } else {
      uint32_t a15 = w[(t - 15) & 15], a2 = w[(t - 2) & 15];
      wt = w[t & 15] += (ror32(a15, 7) ^ ror32(a15, 18) ^ (a15 >> 3)) +
                        w[(t - 7) & 15] +
                        (ror32(a2, 17) ^ ror32(a2, 19) ^ (a2 >> 10));
    }
    uint32_t t1 = hh + (ror32(e, 6) ^ ror32(e, 11) ^ ror32(e, 25)) +
                  ((e & f) ^ (~e & g)) + c_sha_k[t] + wt;
    uint32_t t2 = (ror32(a, 2) ^ ror32(a, 13) ^ ror32(a, 22)) +
                  ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

__device__ __forceinline__ void sha_init(uint32_t h[8]) {
  h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a;
  h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
}

/* --------------- salsa20/8 + BlockMix, 4-lane cooperative ---------------
 *
 * One label is computed by FOUR adjacent lanes (a quad).  The 16-word salsa
 * state lives as four z-diagonal vectors across the quad — lane l holds
 *   z0[l]=x[5l%16], z1[l]=x[(4+5l)%16], z2[l]=x[(8+5l)%16], z3[l]=x[(12+5l)%16]
 * so the column round is lane-local and the row round needs only quad
 * rotations (ds_swizzle quad-perm).  The payoff is memory shape: a quad's
 * 128-B scratch block is read/written as aligned 64-B transactions
 * (measured 7.7 TB/s random vs 1.2 TB/s for the 1-lane 16-B pattern —
 * profiles/probe2 gather1 vs gather4). */

/* quad permutes via DPP (VALU pipe, ~2-cycle) instead of ds_swizzle
 * (LDS pipe, ~50-cycle latency in the salsa dependency chain) */
#define SWZ(v, pat)                                                            \
  ((uint32_t)__builtin_amdgcn_mov_dpp((int)(v), (pat), 0xf, 0xf, true))
#define QROT1 0x39 /* quad perm (1,2,3,0): lane l reads elem (l+1)&3 */
#define QROT2 0x4E /* (2,3,0,1) */
#define QROT3 0x93 /* (3,0,1,2) */
#define QBCAST0 0x00 /* all lanes read elem 0 */

/* z-vector salsa20/8 on one quad: A..D are this lane's elements of z0..z3 */
__device__ __forceinline__ void salsa8_z(uint32_t &A, uint32_t &B,
                                         uint32_t &C, uint32_t &D) {
  uint32_t a = A, b = B, c = C, d = D;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    /* column round: QR(z0,z1,z2,z3) element-wise */
    b ^= __builtin_rotateleft32(a + d, 7);
    c ^= __builtin_rotateleft32(b + a, 9);
    d ^= __builtin_rotateleft32(c + b, 13);
    a ^= __builtin_rotateleft32(d + c, 18);
    /* row round: QR(z0, rot1(z3), rot2(z2), rot3(z1)).  The compiler
     * fuses these permutes into the consuming xor/add as *_dpp forms; the
     * VALU->DPP hazard s_nops that remain cost nothing at 8 waves/SIMD:
     * other waves issue into them (measured: source order neutral,
     * two interleaved labels per quad slower — profiles/r03_romix_isa.md,
     * profiles/r03_kernel_stats.md). */
    uint32_t y1 = SWZ(d, QROT1);
    uint32_t y2 = SWZ(c, QROT2);
    uint32_t y3 = SWZ(b, QROT3);
    y1 ^= __builtin_rotateleft32(a + y3, 7);
    y2 ^= __builtin_rotateleft32(y1 + a, 9);
    y3 ^= __builtin_rotateleft32(y2 + y1, 13);
    a ^= __builtin_rotateleft32(y3 + y2, 18);
    /* un-rotate for the next column round */
    d = SWZ(y1, QROT3);
    c = SWZ(y2, QROT2);
    b = SWZ(y3, QROT1);
  }
  A += a; B += b; C += c; D += d;
}

/* BlockMix r=1 on a quad: X = (B0,B1) as two z-vectors per lane (8 regs) */
__device__ __forceinline__ void blockmix_z(uint32_t X0[4], uint32_t X1[4]) {
  uint32_t t0 = X0[0] ^ X1[0], t1 = X0[1] ^ X1[1], t2 = X0[2] ^ X1[2],
           t3 = X0[3] ^ X1[3];
  salsa8_z(t0, t1, t2, t3);
  X0[0] = t0; X0[1] = t1; X0[2] = t2; X0[3] = t3;
  t0 ^= X1[0]; t1 ^= X1[1]; t2 ^= X1[2]; t3 ^= X1[3];
  salsa8_z(t0, t1, t2, t3);
  X1[0] = t0; X1[1] = t1; X1[2] = t2; X1[3] = t3;
}

/* ------------------------- label kernel ------------------------- */
/* LabelKernelArgs: see kernel_args.h */

/* PBKDF2 helper: one outer HMAC finalisation of a 32-byte inner digest */
__device__ __forceinline__ void hmac_outer(const uint32_t ho[8],
                                           const uint32_t inner[8],
                                           uint32_t out[8]) {
  uint32_t h[8], m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = ho[i];
#pragma unroll
  for (int i = 0; i < 8; i++) m[i] = inner[i];
  m[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; i++) m[i] = 0;
  m[15] = (64 + 32) * 8;
  sha_compress(h, m);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = h[i];
}

/* The labeling path runs as THREE kernels per batch so the ROMix hot loop
 * stays register-lean (8 waves/SIMD) while the SHA-heavy prologue/tail keep
 * their own (lower) occupancy.  The per-label working block X round-trips
 * through xbuf (128 B per task, quad-z chunk layout) — 256 B of extra
 * traffic against the ~2 MiB/label scratch stream. */

/* shared helper: password = commitment || LE64(index) -> HMAC states */
__device__ __forceinline__ void hmac_states_for(const uint32_t *cw,
                                                unsigned long long index,
                                                uint32_t hi[8],
                                                uint32_t ho[8]) {
  uint32_t pw_be[10], m[16];
#pragma unroll
  for (int i = 0; i < 8; i++) pw_be[i] = __builtin_bswap32(cw[i]);
  pw_be[8] = __builtin_bswap32((uint32_t)index);
  pw_be[9] = __builtin_bswap32((uint32_t)(index >> 32));
  sha_init(hi);
#pragma unroll
  for (int i = 0; i < 10; i++) m[i] = pw_be[i] ^ 0x36363636u;
#pragma unroll
  for (int i = 10; i < 16; i++) m[i] = 0x36363636u;
  sha_compress(hi, m);
  sha_init(ho);
#pragma unroll
  for (int i = 0; i < 10; i++) m[i] = pw_be[i] ^ 0x5c5c5c5cu;
#pragma unroll
  for (int i = 10; i < 16; i++) m[i] = 0x5c5c5c5cu;
  sha_compress(ho, m);
}

/* The SHA kernels (prologue, tail, audit tail) run ONE lane per label, so a
 * compression is computed once; only ROMix works in quads.  xbuf keeps the
 * quad-z layout ROMix reads: of a task's eight uint4, chunk c is what quad
 * lane c holds of block 0, (z0[c], z1[c], z2[c], z3[c]) with
 * z_v[l] = x[(4v + 5l) % 16], and chunk 4 + c the same of block 1.  A lane
 * here reads or writes all eight, the permutation resolved at compile
 * time. */

/* canonical 16 words of one 64-B block -> its four chunks */
__device__ __forceinline__ void canon_to_chunks(const uint32_t x[16],
                                                uint4 *p) {
#pragma unroll
  for (int c = 0; c < 4; c++)
    p[c] = make_uint4(x[(5 * c) & 15], x[(4 + 5 * c) & 15],
                      x[(8 + 5 * c) & 15], x[(12 + 5 * c) & 15]);
}

/* four chunks of one block -> big-endian SHA message words of the canonical
 * 64-B block */
__device__ __forceinline__ void chunks_to_msg_be(const uint4 *p,
                                                 uint32_t m[16]) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const uint4 v = p[c];
    m[(5 * c) & 15] = __builtin_bswap32(v.x);
    m[(4 + 5 * c) & 15] = __builtin_bswap32(v.y);
    m[(8 + 5 * c) & 15] = __builtin_bswap32(v.z);
    m[(12 + 5 * c) & 15] = __builtin_bswap32(v.w);
  }
}

/* prologue: PBKDF2(P, "", 1, 128) -> xbuf in quad-z layout */
__global__ void __launch_bounds__(POSTE_THREADS)
post_label_prologue_kernel(LabelKernelArgs a) {
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long gstride =
      (unsigned long long)gridDim.x * blockDim.x;
  uint4 *X = (uint4 *)a.xbuf;

  for (unsigned long long task = lane; task < a.count; task += gstride) {
    const unsigned long long index = a.indices ? a.indices[task]
                                               : a.start + task;
    const uint32_t *cw = a.commit_ids
                             ? a.commitments + 8ull * a.commit_ids[task]
                             : a.commitment_le;
    uint32_t hi[8], ho[8], m[16];
    hmac_states_for(cw, index, hi, ho);
    uint4 *p = X + task * 8ull;
    for (uint32_t half = 0; half < 2; half++) {
      uint32_t cblk[16];
#pragma unroll
      for (uint32_t q = 0; q < 2; q++) {
        const uint32_t blk = half * 2 + q + 1;
        uint32_t h[8];
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = hi[i];
        m[0] = blk;
        m[1] = 0x80000000u;
#pragma unroll
        for (int i = 2; i < 15; i++) m[i] = 0;
        m[15] = (64 + 4) * 8;
        sha_compress(h, m);
        uint32_t d[8];
        hmac_outer(ho, h, d);
#pragma unroll
        for (int k = 0; k < 8; k++)
          cblk[8 * q + k] = __builtin_bswap32(d[k]);
      }
      canon_to_chunks(cblk, p + 4 * half);
    }
  }
}

/* generic ROMix: any lookup-gap (POST_GAP_SHIFT > 0), and gap 1 when the
 * scratch geometry is outside what the lean kernel below addresses */
__global__ void __launch_bounds__(POSTE_THREADS, 8)
post_label_romix_gap_kernel(LabelKernelArgs a) {
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long group = lane >> 2;
  const uint32_t sub = (uint32_t)(lane & 3);
  const uint32_t n = a.scrypt_n;
  const uint32_t mask = n - 1;
  const uint32_t gmask = (1u << a.gap_shift) - 1u;
  uint4 *V = (uint4 *)a.scratch;
  uint4 *X = (uint4 *)a.xbuf;

  for (unsigned long long task = group; task < a.count;
       task += a.scratch_lanes) {
    uint32_t Z0[4], Z1[4];
    {
      uint4 *p = X + task * 8ull;
      uint4 v0 = p[sub], v1 = p[sub + 4];
      Z0[0] = v0.x; Z0[1] = v0.y; Z0[2] = v0.z; Z0[3] = v0.w;
      Z1[0] = v1.x; Z1[1] = v1.y; Z1[2] = v1.z; Z1[3] = v1.w;
    }
    /* phase 1: V_j = X for j % gap == 0; X = BlockMix(X).  Stored block
     * j/gap of this quad is 8 consecutive uint4 at ((j/gap)*slots+group)*8;
     * lane sub covers chunks sub and sub+4 -> aligned 64-B transactions. */
    {
      unsigned long long base = group * 8ull + sub;
      const unsigned long long stride = a.scratch_lanes * 8ull;
      for (uint32_t j = 0; j < n; j++) {
        if ((j & gmask) == 0) {
          uint4 *p = V + base;
          VSTORE(p, make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]));
          VSTORE(p + 4, make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]));
          base += stride;
        }
        blockmix_z(Z0, Z1);
      }
    }
    /* phase 2: j = Integerify(X) & (n-1); regenerate V_j from the stored
     * block by j%gap BlockMixes; X ^= V_j; BlockMix.  Integerify =
     * canonical word 16 = B1's z0[0] -> quad broadcast. */
    for (uint32_t i = 0; i < n; i++) {
      uint32_t j = SWZ(Z1[0], QBCAST0) & mask;
      const uint32_t r = j & gmask;
      const uint4 *p =
          V + ((unsigned long long)(j >> a.gap_shift) * a.scratch_lanes +
               group) * 8ull + sub;
      uint32_t Y0[4], Y1[4];
      {
        uint4 v0 = VLOAD(p), v1 = VLOAD(p + 4);
        Y0[0] = v0.x; Y0[1] = v0.y; Y0[2] = v0.z; Y0[3] = v0.w;
        Y1[0] = v1.x; Y1[1] = v1.y; Y1[2] = v1.z; Y1[3] = v1.w;
      }
      for (uint32_t t = 0; t < r; t++) blockmix_z(Y0, Y1);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        Z0[k] ^= Y0[k];
        Z1[k] ^= Y1[k];
      }
      blockmix_z(Z0, Z1);
    }
    {
      uint4 *p = X + task * 8ull;
      p[sub] = make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]);
      p[sub + 4] = make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]);
    }
  }
}

/* ---- lean lookup-gap-1 ROMix ----
 * VALU issue is the busiest resource of this kernel
 * (profiles/r03_romix_isa.md), so vector instructions around the two salsa
 * calls of an iteration cost throughput.  The gap-1 kernel carries no gap
 * machinery and addresses the scratch with 24-bit multiplies: stored block
 * j of a quad lies j * (scratch_lanes * 8) uint4 past the quad's own base
 * pointer.  The launcher only picks it when scrypt_n <= 2^24 and
 * scratch_lanes * 8 < 2^24, so both factors fit v_mul_u32_u24 /
 * v_mul_hi_u32_u24 (full rate) and one v_lshl_add_u64 forms the address —
 * no 64-bit multiply or shift.  The `& 0xffffff` below never changes a
 * value; it tells the compiler the range. */
#define POSTE_U24 0xffffffu

__device__ __forceinline__ const uint4 *vblock(const uint4 *qbase, uint32_t j,
                                               uint32_t stride16) {
  return qbase + (unsigned long long)j * stride16;
}

/* a ^ b ^ c as one v_bitop3_b32 (truth table 0x96).  Written `a ^ b ^ c`
 * the compiler reassociates it back into two 2-input xors. */
#define XOR3(a, b, c) ((uint32_t)__builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96))

/* phase-2 step: X ^= V; X = BlockMix(X).  X0 ^ V0 is needed only as part
 * of the first salsa input X0 ^ V0 ^ (X1 ^ V1), a 3-input xor: 8 xors per
 * lane instead of 12. */
__device__ __forceinline__ void blockmix_xor_z(uint32_t X0[4], uint32_t X1[4],
                                               const uint4 v0,
                                               const uint4 v1) {
  X1[0] ^= v1.x; X1[1] ^= v1.y; X1[2] ^= v1.z; X1[3] ^= v1.w;
  uint32_t t0 = XOR3(X0[0], v0.x, X1[0]), t1 = XOR3(X0[1], v0.y, X1[1]),
           t2 = XOR3(X0[2], v0.z, X1[2]), t3 = XOR3(X0[3], v0.w, X1[3]);
  salsa8_z(t0, t1, t2, t3);
  X0[0] = t0; X0[1] = t1; X0[2] = t2; X0[3] = t3;
  t0 ^= X1[0]; t1 ^= X1[1]; t2 ^= X1[2]; t3 ^= X1[3];
  salsa8_z(t0, t1, t2, t3);
  X1[0] = t0; X1[1] = t1; X1[2] = t2; X1[3] = t3;
}

/* the ROMix hot loop at lookup-gap 1: register-lean, 8 waves/SIMD */
__global__ void __launch_bounds__(POSTE_THREADS, 8)
post_label_romix_kernel(LabelKernelArgs a) {
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long group = lane >> 2;
  const uint32_t sub = (uint32_t)(lane & 3);
  const uint32_t n = a.scrypt_n;
  const uint32_t mask = (n - 1) & POSTE_U24;
  const uint32_t stride16 = ((uint32_t)a.scratch_lanes * 8u) & POSTE_U24;
  /* this quad's column of V: lane sub covers chunks sub and sub+4 of each
   * 8-uint4 block -> aligned 64-B transactions */
  uint4 *const qbase = (uint4 *)a.scratch + (group * 8ull + sub);
  uint4 *X = (uint4 *)a.xbuf;

  for (unsigned long long task = group; task < a.count;
       task += a.scratch_lanes) {
    uint32_t Z0[4], Z1[4];
    {
      uint4 *p = X + task * 8ull;
      uint4 v0 = p[sub], v1 = p[sub + 4];
      Z0[0] = v0.x; Z0[1] = v0.y; Z0[2] = v0.z; Z0[3] = v0.w;
      Z1[0] = v1.x; Z1[1] = v1.y; Z1[2] = v1.z; Z1[3] = v1.w;
    }
    /* phase 1: V_j = X; X = BlockMix(X) */
    {
      uint4 *p = qbase;
      for (uint32_t j = 0; j < n; j++) {
        VSTORE(p, make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]));
        VSTORE(p + 4, make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]));
        p += stride16;
        blockmix_z(Z0, Z1);
      }
    }
    /* phase 2: j = Integerify(X) & (n-1); X ^= V_j; BlockMix.  Integerify
     * = canonical word 16 = B1's z0[0] -> quad broadcast. */
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t j = SWZ(Z1[0], QBCAST0) & mask;
      const uint4 *p = vblock(qbase, j, stride16);
      const uint4 v0 = VLOAD(p), v1 = VLOAD(p + 4);
      blockmix_xor_z(Z0, Z1, v0, v1);
    }
    {
      uint4 *p = X + task * 8ull;
      p[sub] = make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]);
      p[sub + 4] = make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]);
    }
  }
}

/* ---- the lean kernel as two launches (RomixPhaseArgs, kernel_args.h) ----
 * Same loop bodies, V layout and 24-bit addressing as the kernel above, one
 * task per quad and no loop over rounds: fill must have ended before mix
 * starts, and the next round's fill may only follow this round's mix, which
 * stream order provides.  X round-trips through xbuf once more, 256 B per
 * label.  Launches on different column ranges can run side by side in any
 * combination, fill beside mix, fill beside fill or mix beside mix: the
 * init path gives each stream its own columns and lets the streams run
 * free, with no wait between the ROMix kernels of different streams
 * (engine.cpp, init_step_split). */
__global__ void __launch_bounds__(POSTE_THREADS, 8)
post_label_romix_fill_kernel(RomixPhaseArgs a) {
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long task = lane >> 2;
  const uint32_t sub = (uint32_t)(lane & 3);
  if (task >= a.count || task >= a.slot_count) return;
  const uint32_t n = a.scrypt_n;
  const uint32_t stride16 = ((uint32_t)a.scratch_lanes * 8u) & POSTE_U24;
  uint4 *p = (uint4 *)a.scratch + ((a.slot_base + task) * 8ull + sub);
  uint4 *x = (uint4 *)a.xbuf + task * 8ull;

  uint32_t Z0[4], Z1[4];
  {
    uint4 v0 = x[sub], v1 = x[sub + 4];
    Z0[0] = v0.x; Z0[1] = v0.y; Z0[2] = v0.z; Z0[3] = v0.w;
    Z1[0] = v1.x; Z1[1] = v1.y; Z1[2] = v1.z; Z1[3] = v1.w;
  }
  /* phase 1: V_j = X; X = BlockMix(X) */
  for (uint32_t j = 0; j < n; j++) {
    VSTORE(p, make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]));
    VSTORE(p + 4, make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]));
    p += stride16;
    blockmix_z(Z0, Z1);
  }
  x[sub] = make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]);
  x[sub + 4] = make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]);
}

__global__ void __launch_bounds__(POSTE_THREADS, 8)
post_label_romix_mix_kernel(RomixPhaseArgs a) {
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long task = lane >> 2;
  const uint32_t sub = (uint32_t)(lane & 3);
  if (task >= a.count || task >= a.slot_count) return;
  const uint32_t n = a.scrypt_n;
  const uint32_t mask = (n - 1) & POSTE_U24;
  const uint32_t stride16 = ((uint32_t)a.scratch_lanes * 8u) & POSTE_U24;
  const uint4 *const qbase =
      (const uint4 *)a.scratch + ((a.slot_base + task) * 8ull + sub);
  uint4 *x = (uint4 *)a.xbuf + task * 8ull;

  uint32_t Z0[4], Z1[4];
  {
    uint4 v0 = x[sub], v1 = x[sub + 4];
    Z0[0] = v0.x; Z0[1] = v0.y; Z0[2] = v0.z; Z0[3] = v0.w;
    Z1[0] = v1.x; Z1[1] = v1.y; Z1[2] = v1.z; Z1[3] = v1.w;
  }
  /* phase 2: j = Integerify(X) & (n-1); X ^= V_j; BlockMix */
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t j = SWZ(Z1[0], QBCAST0) & mask;
    const uint4 *p = vblock(qbase, j, stride16);
    const uint4 v0 = VLOAD(p), v1 = VLOAD(p + 4);
    blockmix_xor_z(Z0, Z1, v0, v1);
  }
  x[sub] = make_uint4(Z0[0], Z0[1], Z0[2], Z0[3]);
  x[sub + 4] = make_uint4(Z1[0], Z1[1], Z1[2], Z1[3]);
}

/* tail: PBKDF2(P, X, 1, 32) -> labels, VRF-minimum tracking + exact
 * per-workgroup candidate reduce */
__global__ void __launch_bounds__(POSTE_THREADS)
post_label_tail_kernel(LabelKernelArgs a) {
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long gstride =
      (unsigned long long)gridDim.x * blockDim.x;
  uint4 *X = (uint4 *)a.xbuf;

  uint32_t min_lab[8];
  unsigned long long min_idx = 0;
  int min_found = 0;

  for (unsigned long long task = lane; task < a.count; task += gstride) {
    const unsigned long long index = a.indices ? a.indices[task]
                                               : a.start + task;
    const uint32_t *cw = a.commit_ids
                             ? a.commitments + 8ull * a.commit_ids[task]
                             : a.commitment_le;
    uint32_t hi[8], ho[8], m[16];
    hmac_states_for(cw, index, hi, ho);
    const uint4 *p = X + task * 8ull;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = hi[i];
    chunks_to_msg_be(p, m);
    sha_compress(h, m);
    chunks_to_msg_be(p + 4, m);
    sha_compress(h, m);
    m[0] = 1;
    m[1] = 0x80000000u;
#pragma unroll
    for (int i = 2; i < 15; i++) m[i] = 0;
    m[15] = (64 + 128 + 4) * 8;
    sha_compress(h, m);
    uint32_t lab_be[8]; /* full label as big-endian words */
    hmac_outer(ho, h, lab_be);

    if (a.out) {
      if (a.out_full) {
        uint4 *o = (uint4 *)(a.out + task * 32ull);
        o[0] = make_uint4(__builtin_bswap32(lab_be[0]),
                          __builtin_bswap32(lab_be[1]),
                          __builtin_bswap32(lab_be[2]),
                          __builtin_bswap32(lab_be[3]));
        o[1] = make_uint4(__builtin_bswap32(lab_be[4]),
                          __builtin_bswap32(lab_be[5]),
                          __builtin_bswap32(lab_be[6]),
                          __builtin_bswap32(lab_be[7]));
      } else {
        *(uint4 *)(a.out + task * 16ull) =
            make_uint4(__builtin_bswap32(lab_be[0]),
                       __builtin_bswap32(lab_be[1]),
                       __builtin_bswap32(lab_be[2]),
                       __builtin_bswap32(lab_be[3]));
      }
    }

    if (a.has_difficulty) {
      /* lexicographic byte compare == numeric compare of BE word sequence */
      bool below_diff = false, below_min = false;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        if (lab_be[k] != a.difficulty_be[k]) {
          below_diff = lab_be[k] < a.difficulty_be[k];
          break;
        }
      }
      if (below_diff) {
        if (!min_found) {
          below_min = true;
        } else {
          below_min = false;
#pragma unroll
          for (int k = 0; k < 8; k++) {
            if (lab_be[k] != min_lab[k]) {
              below_min = lab_be[k] < min_lab[k];
              break;
            }
          }
        }
        if (below_min) {
          min_found = 1;
          min_idx = index;
#pragma unroll
          for (int k = 0; k < 8; k++) min_lab[k] = lab_be[k];
        }
      }
    }
  }

  /* one exact candidate per workgroup: LDS gather + lane-0 scan */
  if (a.has_difficulty) {
    __shared__ uint32_t s_lab[POSTE_THREADS][8];
    __shared__ unsigned long long s_idx[POSTE_THREADS];
    __shared__ uint8_t s_found[POSTE_THREADS];
    s_found[threadIdx.x] = (uint8_t)min_found;
    if (min_found) {
      s_idx[threadIdx.x] = min_idx;
#pragma unroll
      for (int k = 0; k < 8; k++) s_lab[threadIdx.x][k] = min_lab[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int best = -1;
      for (int t = 0; t < POSTE_THREADS; t++) {
        if (!s_found[t]) continue;
        if (best < 0) {
          best = t;
          continue;
        }
        /* order by (label bytes, index) ascending */
        int cmp = 0;
        for (int k = 0; k < 8 && cmp == 0; k++) {
          if (s_lab[t][k] < s_lab[best][k]) cmp = -1;
          else if (s_lab[t][k] > s_lab[best][k]) cmp = 1;
        }
        if (cmp < 0 || (cmp == 0 && s_idx[t] < s_idx[best])) best = t;
      }
      if (best >= 0) {
        unsigned int slot = atomicAdd(a.cand_count, 1u);
        if (slot < a.cand_cap) {
          a.cand[slot].index = s_idx[best];
          for (int k = 0; k < 8; k++)
            a.cand[slot].label_be[k] = s_lab[best][k];
        }
      }
    }
  }
}

/* audit tail (postdata audit, AuditKernelArgs): PBKDF2(P, X, 1, 32) as in
 * the tail above, then compare with the label read from disk instead of
 * storing.  No label output and no VRF tracking; a differing label is
 * appended as {index, recomputed 16 B}.  Each task appends at most once and
 * the list holds label.count entries, so a slot is always in bounds. */
__global__ void __launch_bounds__(POSTE_THREADS)
post_label_audit_tail_kernel(AuditKernelArgs aa) {
  const LabelKernelArgs &a = aa.label;
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long gstride =
      (unsigned long long)gridDim.x * blockDim.x;
  const uint4 *X = (const uint4 *)a.xbuf;

  for (unsigned long long task = lane; task < a.count; task += gstride) {
    const unsigned long long index = a.indices ? a.indices[task]
                                               : a.start + task;
    const uint32_t *cw = a.commit_ids
                             ? a.commitments + 8ull * a.commit_ids[task]
                             : a.commitment_le;
    uint32_t hi[8], ho[8], m[16];
    hmac_states_for(cw, index, hi, ho);
    const uint4 *p = X + task * 8ull;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = hi[i];
    chunks_to_msg_be(p, m);
    sha_compress(h, m);
    chunks_to_msg_be(p + 4, m);
    sha_compress(h, m);
    m[0] = 1;
    m[1] = 0x80000000u;
#pragma unroll
    for (int i = 2; i < 15; i++) m[i] = 0;
    m[15] = (64 + 128 + 4) * 8;
    sha_compress(h, m);
    uint32_t lab_be[8];
    hmac_outer(ho, h, lab_be);

    {
      const uint4 want = aa.expected[task];
      const uint4 got = make_uint4(__builtin_bswap32(lab_be[0]),
                                   __builtin_bswap32(lab_be[1]),
                                   __builtin_bswap32(lab_be[2]),
                                   __builtin_bswap32(lab_be[3]));
      if (got.x != want.x || got.y != want.y || got.z != want.z ||
          got.w != want.w) {
        const unsigned int slot = atomicAdd(aa.count, 1u);
        PostAuditMismatch *o = aa.mismatch + slot;
        o->index = index;
        o->label[0] = got.x;
        o->label[1] = got.y;
        o->label[2] = got.z;
        o->label[3] = got.w;
      }
    }
  }
}

/* ------------------------- proving scan kernels ------------------------- */
/* ScanKernelArgs and ScanPlan: see kernel_args.h.
 *
 * One AES-128 encryption and one scan body.  The kernels differ in where a
 * T-table word comes from, which a table policy says: its LDS layout and
 * fill, te<T>(x) for the word of table T (rot<T> brings it into place where
 * one table serves all four), sb<S>(x) for the S-box byte of x at bit S, and
 * whether the scan body copies a cipher's round keys into registers.  Lookups
 * through the vector L1, all or half of them, measured conclusively worse:
 * profiles/r02_scan_tt_verdict.md. */

/* Independent labels (AES chains) per lane.  A single chain leaves the wave
 * ~76% latency-stalled (profiles: SQ_ACTIVE_INST 10%, LDS 14%); interleaving
 * chains fills the LDS-latency shadows.  2 chains at 8 waves/SIMD measured
 * best at 256 and 512 threads.  tt4 runs max(4, POSTE_SCAN_ILP): 4 measured
 * best there (r2d sweep); at one workgroup per CU there are only 16 waves to
 * hide latency, so deeper chains pay.  -DPOSTE_SCAN_ILP=n: make scan1/scan4. */
#ifndef POSTE_SCAN_ILP
#define POSTE_SCAN_ILP 2
#endif

/* Shared tables: Te0..Te3 and the S-box once per workgroup, random per-lane
 * indices.  LDS-conflict-throughput bound (ILP 1/2/4 all measure ~274 M
 * labels/s; a random 32-lane b32 gather costs 2 x E[max 32-into-32-bank
 * load] ~ 6.4 LDS cycles — see profiles/r01_scan_sweep.md and
 * MI355X_MICROARCH.md §LDS).  Round keys stay in global: the cipher loop is
 * wave-uniform, so they compile to scalar loads through the constant cache
 * instead of ~5.8K extra LDS reads per label. */
struct TeShared {
  static constexpr uint32_t LDS_BYTES = 1024 * 4 + 256;
  static constexpr bool RK_IN_REGS = false;
  const uint32_t *sTe;  /* 1024 words */
  const uint8_t *sSbox; /* 256 bytes */
  __device__ __forceinline__ TeShared(uint32_t *lds, const uint32_t *te,
                                      const uint8_t *sbox) {
    uint8_t *sb = (uint8_t *)(lds + 1024);
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) lds[i] = te[i];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) sb[i] = sbox[i];
    __syncthreads();
    sTe = lds;
    sSbox = sb;
  }
  template <int T>
  __device__ __forceinline__ uint32_t te(uint32_t x) const {
    return sTe[T * 256 + x];
  }
  template <int T>
  static __device__ __forceinline__ uint32_t rot(uint32_t g) { return g; }
  template <int S>
  __device__ __forceinline__ uint32_t sb(uint32_t x) const {
    return (uint32_t)sSbox[x] << S;
  }
};

/* S-box byte of a Te0 word at bit S: te[x] packs [s2,s,s,s3], so s =
 * (te[x]>>8)&0xff and the shift folds into the mask. */
template <int S>
static __device__ __forceinline__ uint32_t te0_sbox(uint32_t g) {
  if constexpr (S >= 8)
    return (g & 0xff00u) << (S - 8);
  else
    return (g >> 8) & 0xffu;
}

/* Bank-replicated: one Te0 table replicated across the 32 LDS banks.
 * Copy c is strided so element x of copy c sits at word x*32 + c; the bank
 * of word w is w%32 = c, and each lane reads only copy (lane%32), so every
 * ds_read_b32 gather in the cipher loop is conflict-free BY CONSTRUCTION
 * (2 LDS cycles per wave-gather, MI355X_MICROARCH §LDS, vs ~6.4 measured
 * for the shared-table random gather — profiles/r01_scan_sweep.md).  The
 * round-2 TT retest (profiles/r02_scan_tt_verdict.md) proved the L1 pipe
 * cannot bypass that wall, so this attacks it inside the LDS instead:
 * 3.2x fewer LDS cycles for 32 KB of LDS per workgroup and a few extra
 * VALU ops — Te1/2/3 derive from Te0 by byte rotation (one v_alignbit
 * each; te[256+x] = ror8(te[x]), crypto_host.cpp:332-334), and the final
 * round's S-box is byte 1 of Te0 — no separate sbox table at all.
 * Round keys go into registers up front: a.rk accesses inside the round
 * loop compile to per-round VECTOR global loads (wave-uniform but the
 * compiler cannot prove it) whose vmcnt waits serialize the cipher loop. */
struct TeBankrep {
  static constexpr uint32_t LDS_BYTES = 8192 * 4; /* 32 copies x 1 KiB */
  static constexpr bool RK_IN_REGS = true;
  const uint32_t *sTe;
  uint32_t lane31;
  __device__ __forceinline__ TeBankrep(uint32_t *lds, const uint32_t *te,
                                       const uint8_t *) {
    for (uint32_t i = threadIdx.x; i < 8192; i += blockDim.x)
      lds[i] = te[i >> 5]; /* consecutive lanes -> consecutive banks */
    __syncthreads();
    sTe = lds;
    lane31 = threadIdx.x & 31;
  }
  template <int T>
  __device__ __forceinline__ uint32_t te(uint32_t x) const {
    return sTe[(x << 5) | lane31];
  }
  template <int T>
  static __device__ __forceinline__ uint32_t rot(uint32_t g) {
    return T == 0 ? g : __builtin_amdgcn_alignbit(g, g, 8 * T);
  }
  template <int S>
  __device__ __forceinline__ uint32_t sb(uint32_t x) const {
    return te0_sbox<S>(te<0>(x));
  }
};

/* 4-table interleaved bank-replicated: all four Te tables, each
 * bank-replicated, interleaved so entry (x, t, lane) sits at word
 * x*128 + t*32 + lane%32 — per-gather addressing is one v_lshl_add with
 * the t*128-byte offset folded into the ds_read immediate, and the
 * alignbit rotations of the 1-table variant disappear (~20% of its
 * VALU).  Costs 128 KiB LDS, so one 1024-thread workgroup per CU
 * (16 waves) instead of 20. */
struct TeTt4 {
  static constexpr uint32_t LDS_BYTES = 32768 * 4; /* 4 tables x 32 copies */
  static constexpr bool RK_IN_REGS = true;
  const uint32_t *t0p;
  __device__ __forceinline__ TeTt4(uint32_t *lds, const uint32_t *te,
                                   const uint8_t *) {
    for (uint32_t i = threadIdx.x; i < 32768; i += blockDim.x)
      lds[i] = te[((i >> 5) & 3) * 256 + (i >> 7)];
    __syncthreads();
    t0p = lds + (threadIdx.x & 31);
  }
  template <int T>
  __device__ __forceinline__ uint32_t te(uint32_t x) const {
    return t0p[(x << 7) + 32 * T];
  }
  template <int T>
  static __device__ __forceinline__ uint32_t rot(uint32_t g) { return g; }
  template <int S>
  __device__ __forceinline__ uint32_t sb(uint32_t x) const {
    return te0_sbox<S>(te<0>(x));
  }
};

/* AES-128 encryption of L blocks p (big-endian words) under the 44 round-key
 * words rk, in two steps so that a caller can leave out the last round of a
 * block it will not look at.  aes128_rounds: the whitening and rounds 1-9,
 * state into w.  BATCHG issues all of a round's gathers before any combine:
 * it widens the read->use distance so partial lgkmcnt waits overlap the
 * whole gather batch with the previous combines. */
template <class Tab, int L, bool BATCHG>
static __device__ __forceinline__ void
aes128_rounds(const Tab &tab, const uint32_t (&p)[L][4], const uint32_t *rk,
              uint32_t (&w)[L][4]) {
#pragma unroll
  for (int u = 0; u < L; u++)
#pragma unroll
    for (int k = 0; k < 4; k++) w[u][k] = p[u][k] ^ rk[k];
#pragma unroll
  for (int r = 1; r < 10; r++) {
    if (BATCHG) {
      uint32_t g[L][16];
#pragma unroll
      for (int u = 0; u < L; u++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          g[u][4 * q + 0] = tab.template te<0>(w[u][q] >> 24);
          g[u][4 * q + 1] =
              tab.template te<1>((w[u][(q + 1) & 3] >> 16) & 0xff);
          g[u][4 * q + 2] =
              tab.template te<2>((w[u][(q + 2) & 3] >> 8) & 0xff);
          g[u][4 * q + 3] = tab.template te<3>(w[u][(q + 3) & 3] & 0xff);
        }
#pragma unroll
      for (int u = 0; u < L; u++)
#pragma unroll
        for (int q = 0; q < 4; q++)
          w[u][q] = Tab::template rot<0>(g[u][4 * q]) ^
                    Tab::template rot<1>(g[u][4 * q + 1]) ^
                    Tab::template rot<2>(g[u][4 * q + 2]) ^
                    Tab::template rot<3>(g[u][4 * q + 3]) ^ rk[4 * r + q];
    } else {
#pragma unroll
      for (int u = 0; u < L; u++) {
        uint32_t n[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
          n[q] = Tab::template rot<0>(tab.template te<0>(w[u][q] >> 24)) ^
                 Tab::template rot<1>(tab.template te<1>(
                     (w[u][(q + 1) & 3] >> 16) & 0xff)) ^
                 Tab::template rot<2>(tab.template te<2>(
                     (w[u][(q + 2) & 3] >> 8) & 0xff)) ^
                 Tab::template rot<3>(
                     tab.template te<3>(w[u][(q + 3) & 3] & 0xff)) ^
                 rk[4 * r + q];
#pragma unroll
        for (int q = 0; q < 4; q++) w[u][q] = n[q];
      }
    }
  }
}

/* round 10 of one block: the S-box, no MixColumns; the ciphertext into f */
template <class Tab>
static __device__ __forceinline__ void
aes128_last_round(const Tab &tab, const uint32_t (&w)[4], const uint32_t *rk,
                  uint32_t (&f)[4]) {
#pragma unroll
  for (int q = 0; q < 4; q++)
    f[q] = (tab.template sb<24>(w[q] >> 24) |
            tab.template sb<16>((w[(q + 1) & 3] >> 16) & 0xff) |
            tab.template sb<8>((w[(q + 2) & 3] >> 8) & 0xff) |
            tab.template sb<0>(w[(q + 3) & 3] & 0xff)) ^
           rk[40 + q];
}

/* the two nonce values of a ciphertext, as the difficulty compares them */
static __device__ __forceinline__ unsigned long long
aes_nonce_value(const uint32_t (&f)[4], int half) {
  return __builtin_bswap64(((unsigned long long)f[2 * half] << 32) |
                           f[2 * half + 1]);
}

static __device__ __forceinline__ void
scan_append(const ScanKernelArgs &a, unsigned long long index,
            uint32_t nonce) {
  unsigned int s = atomicAdd(a.hit_count, 1u);
  if (s < a.hit_cap) {
    a.hits[s].index = index;
    a.hits[s].nonce = nonce;
  }
}

/* Grid-stride scan, L labels per lane and iteration: chain u of the lane at
 * t0 takes label t0 + u*stride.  A chain past the end is clamped to t0 and
 * does duplicate work; hits are recorded for the `live` chains only. */
template <class Tab, int L, bool BATCHG>
static __device__ __forceinline__ void scan_body(const ScanKernelArgs &a) {
  extern __shared__ uint32_t scan_lds[];
  const Tab tab(scan_lds, a.te, a.sbox);
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long span = stride * L;
  for (unsigned long long t0 =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       t0 < a.count; t0 += span) {
    uint32_t p[L][4];
    unsigned long long ts[L];
#pragma unroll
    for (int u = 0; u < L; u++) {
      unsigned long long t = t0 + (unsigned long long)u * stride;
      ts[u] = t < a.count ? t : t0;
      uint4 lraw = a.labels[ts[u]];
      p[u][0] = __builtin_bswap32(lraw.x);
      p[u][1] = __builtin_bswap32(lraw.y);
      p[u][2] = __builtin_bswap32(lraw.z);
      p[u][3] = __builtin_bswap32(lraw.w);
    }
    const int live = (int)((a.count - t0 + stride - 1) / stride) < L
                         ? (int)((a.count - t0 + stride - 1) / stride)
                         : L;
    for (uint32_t c = 0; c < a.n_ciphers; c++) {
      const uint32_t *rk = a.rk + c * 44;
      uint32_t rk_regs[Tab::RK_IN_REGS ? 44 : 1];
      if constexpr (Tab::RK_IN_REGS) {
#pragma unroll
        for (int k = 0; k < 44; k++) rk_regs[k] = rk[k];
        rk = rk_regs;
      }
      uint32_t w[L][4];
      aes128_rounds<Tab, L, BATCHG>(tab, p, rk, w);
#pragma unroll
      for (int u = 0; u < L; u++) {
        if (u >= live) break;
        uint32_t f[4];
        aes128_last_round(tab, w[u], rk, f);
#pragma unroll
        for (int h = 0; h < POSTE_NONCES_PER_AES; h++)
          if (aes_nonce_value(f, h) < a.difficulty)
            scan_append(a, a.index_base + ts[u], c * POSTE_NONCES_PER_AES + h);
      }
    }
  }
}

__global__ void __launch_bounds__(POSTE_THREADS)
post_scan_kernel(ScanKernelArgs a) {
  scan_body<TeShared, POSTE_SCAN_ILP, false>(a);
}

template <int THREADS_, bool BATCHG>
__global__ void __launch_bounds__(THREADS_)
post_scan_bankrep_kernel(ScanKernelArgs a) {
  scan_body<TeBankrep, POSTE_SCAN_ILP, BATCHG>(a);
}

__global__ void __launch_bounds__(1024)
post_scan_tt4_kernel(ScanKernelArgs a) {
  scan_body<TeTt4, (POSTE_SCAN_ILP > 4 ? POSTE_SCAN_ILP : 4), false>(a);
}

/* verification's final predicate: AES-encrypt each recomputed label with
 * its proof's cipher and compare the nonce-half u64 against the proof's
 * difficulty (the last step of verifying.ProofVerifier.Verify,
 * post_verifier.go:159 -> per-index AES threshold check). */
__global__ void __launch_bounds__(POSTE_THREADS)
post_verify_pred_kernel(VerifyPredArgs a) {
  extern __shared__ uint32_t verify_lds[];
  const TeShared tab(verify_lds, a.te, a.sbox);
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long t =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       t < a.count; t += stride) {
    const uint32_t pidx = a.task_proof[t];
    const uint32_t *rk = a.rk + (unsigned long long)pidx * 44;
    uint4 lraw = a.labels2[2 * t]; /* first 16 B of the full label */
    const uint32_t p[1][4] = {
        {__builtin_bswap32(lraw.x), __builtin_bswap32(lraw.y),
         __builtin_bswap32(lraw.z), __builtin_bswap32(lraw.w)}};
    uint32_t w[1][4], f[4];
    aes128_rounds<TeShared, 1, false>(tab, p, rk, w);
    aes128_last_round(tab, w[0], rk, f);
    unsigned long long v = a.half[pidx] == 0 ? aes_nonce_value(f, 0)
                                             : aes_nonce_value(f, 1);
    a.pass[t] = v < a.difficulty[pidx] ? 1 : 0;
  }
}

/* VRF-nonce predicate (verifying.VerifyVRFNonce, validation.go:261-286):
 * the full label against its item's threshold as 32-byte big-endian
 * numbers, strictly below.  The words are walked from the last to the
 * first, so the first word that differs is the one that decides. */
__global__ void __launch_bounds__(POSTE_THREADS)
post_vrf_pred_kernel(VrfPredArgs a) {
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long t =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       t < a.count; t += stride) {
    const uint4 *th = a.thresholds + 2ull * a.task_thr[t];
    const uint4 l0 = a.labels2[2 * t], l1 = a.labels2[2 * t + 1];
    const uint4 d0 = th[0], d1 = th[1];
    const uint32_t lw[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
    const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    uint32_t below = 0;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
      const uint32_t x = __builtin_bswap32(lw[k]);
      const uint32_t y = __builtin_bswap32(dw[k]);
      if (x != y) below = x < y ? 1u : 0u;
    }
    a.pass[t] = (uint8_t)below;
  }
}

/* Postdata seal: one lane hashes one 1024-label page of the chunk the
 * proving pass has already put on the device.  A page of n
 * labels is n / 4 whole 64-byte blocks and one closing block: the n % 4
 * labels left over (at most 48 bytes), the 0x80 byte, zeros and the bit
 * length — 49 bytes at the most before the length, so the padding never
 * needs a block of its own.  The next block's four loads are issued before
 * the current block is compressed.  A lane's loads are 64 bytes at a 16 KiB
 * stride; a whole chunk is only 256 waves, one per CU, which is what lets
 * the kernel run beside the scan instead of after it. */
#define POSTE_SEAL_THREADS 64

__global__ void __launch_bounds__(POSTE_SEAL_THREADS)
post_seal_kernel(SealKernelArgs a) {
  const unsigned long long pages =
      (a.count + POSTE_SEAL_PAGE_LABELS - 1) / POSTE_SEAL_PAGE_LABELS;
  const unsigned long long page =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (page >= pages) return;
  const unsigned long long first = page * POSTE_SEAL_PAGE_LABELS;
  const unsigned long long left = a.count - first;
  const uint32_t n =
      left < POSTE_SEAL_PAGE_LABELS ? (uint32_t)left : POSTE_SEAL_PAGE_LABELS;
  const uint4 *src = a.labels + first;
  const uint32_t full = n / 4, rest = n % 4;

  uint32_t h[8], m[16];
  sha_init(h);
  uint4 q[4];
  if (full) {
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = src[i];
  }
  for (uint32_t b = 0; b < full; b++) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      m[4 * i] = __builtin_bswap32(q[i].x);
      m[4 * i + 1] = __builtin_bswap32(q[i].y);
      m[4 * i + 2] = __builtin_bswap32(q[i].z);
      m[4 * i + 3] = __builtin_bswap32(q[i].w);
    }
    if (b + 1 < full) {
#pragma unroll
      for (int i = 0; i < 4; i++) q[i] = src[4 * (b + 1) + i];
    }
    sha_compress(h, m);
  }
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if ((uint32_t)i < rest) {
      const uint4 l = src[4 * full + i];
      m[4 * i] = __builtin_bswap32(l.x);
      m[4 * i + 1] = __builtin_bswap32(l.y);
      m[4 * i + 2] = __builtin_bswap32(l.z);
      m[4 * i + 3] = __builtin_bswap32(l.w);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    if ((uint32_t)i == rest) m[4 * i] = 0x80000000u;
  m[15] = n * 128; /* bits; at most 2^17 */
  sha_compress(h, m);
  a.digests[page] =
      make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]),
                 __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
}

__device__ __forceinline__ void seal_msg_label(uint32_t *m, const uint4 l) {
  m[0] = __builtin_bswap32(l.x);
  m[1] = __builtin_bswap32(l.y);
  m[2] = __builtin_bswap32(l.z);
  m[3] = __builtin_bswap32(l.w);
}

/* Postdata seal of a stream that arrives in segments: init has
 * every batch of labels on the device behind the tail kernel, but a batch
 * neither starts on a page boundary nor holds whole pages.  One lane per
 * page the segment [g0, g0 + count) touches.  The lane of the page open at
 * g0 resumes from *carry_in: its message is the r = carry.count % 4 labels
 * the carry buffers followed by the segment's labels, so its first block is
 * those r and the first 4 - r labels of the segment; every later block is
 * four consecutive labels, 16-byte aligned like the buffer itself.  A page
 * that ends in the segment (or at stream_end) closes as in post_seal_kernel,
 * with the bit length of the whole page; the last lane, when its page stays
 * open, writes *carry_out instead.  r is a run-time value: every q[] and m[]
 * index is a compile-time constant under a predicate, so nothing is indexed
 * dynamically and nothing goes to scratch. */
__global__ void __launch_bounds__(POSTE_SEAL_THREADS)
post_seal_stream_kernel(SealStreamArgs a) {
  const unsigned long long end = a.g0 + a.count;
  const unsigned long long p0 = a.g0 / POSTE_SEAL_PAGE_LABELS;
  const unsigned long long lanes = (end - 1) / POSTE_SEAL_PAGE_LABELS - p0 + 1;
  const unsigned long long lane =
      (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= lanes) return;
  const unsigned long long page_lo = (p0 + lane) * POSTE_SEAL_PAGE_LABELS;
  const unsigned long long page_hi = page_lo + POSTE_SEAL_PAGE_LABELS;
  const unsigned long long lo = page_lo > a.g0 ? page_lo : a.g0;
  const unsigned long long hi = page_hi < end ? page_hi : end;
  const uint32_t n_seg = (uint32_t)(hi - lo);       /* 1..1024 */
  const uint32_t before = (uint32_t)(lo - page_lo); /* of the page, earlier */
  const bool closes = hi == page_hi || hi == a.stream_end;
  const uint4 *src = a.labels + (lo - a.g0);

  uint32_t h[8], m[16];
  uint4 buf[3];
  uint32_t r = 0;
  if (before) {
    const uint4 *c = (const uint4 *)a.carry_in;
    const uint4 h0 = c[0], h1 = c[1];
    h[0] = h0.x; h[1] = h0.y; h[2] = h0.z; h[3] = h0.w;
    h[4] = h1.x; h[5] = h1.y; h[6] = h1.z; h[7] = h1.w;
    r = before % 4;
#pragma unroll
    for (int i = 0; i < 3; i++) buf[i] = c[3 + i];
  } else {
    sha_init(h);
#pragma unroll
    for (int i = 0; i < 3; i++) buf[i] = make_uint4(0, 0, 0, 0);
  }
  /* label k of the lane's message is buf[k] for k < r, else src[k - r] */
  const uint32_t msg = r + n_seg;
  const uint32_t full = msg / 4, rest = msg % 4;

  uint4 q[4];
  if (full) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if ((uint32_t)i < r) {
        if (i < 3) q[i] = buf[i];
      } else {
        q[i] = src[i - r];
      }
    }
  }
  for (uint32_t b = 0; b < full; b++) {
#pragma unroll
    for (int i = 0; i < 4; i++) seal_msg_label(m + 4 * i, q[i]);
    if (b + 1 < full) {
      const uint4 *nx = src + (4 * (b + 1) - r);
#pragma unroll
      for (int i = 0; i < 4; i++) q[i] = nx[i];
    }
    sha_compress(h, m);
  }
  /* the rest labels behind the last whole block: still in buf when no block
   * was compressed, otherwise in memory */
  uint4 t[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    t[i] = make_uint4(0, 0, 0, 0);
    if ((uint32_t)i < rest)
      t[i] = (full == 0 && (uint32_t)i < r) ? buf[i] : src[4 * full + i - r];
  }
  if (!closes) {
    uint4 *c = (uint4 *)a.carry_out;
    c[0] = make_uint4(h[0], h[1], h[2], h[3]);
    c[1] = make_uint4(h[4], h[5], h[6], h[7]);
    c[2] = make_uint4(before + n_seg, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 3; i++) c[3 + i] = t[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = 0;
#pragma unroll
  for (int i = 0; i < 3; i++)
    if ((uint32_t)i < rest) seal_msg_label(m + 4 * i, t[i]);
#pragma unroll
  for (int i = 0; i < 4; i++)
    if ((uint32_t)i == rest) m[4 * i] = 0x80000000u;
  m[15] = (before + n_seg) * 128; /* bits of the whole page; at most 2^17 */
  sha_compress(h, m);
  a.digests[lane] =
      make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]),
                 __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
}

/* host-visible launchers (called from engine.cpp) */
extern "C" {

hipError_t poste_launch_seal_stream_kernel(const SealStreamArgs *args,
                                           hipStream_t stream) {
  if (!args->labels || !args->digests || !args->carry_in ||
      !args->carry_out || args->carry_in == args->carry_out ||
      args->count == 0 || args->g0 + args->count < args->g0 ||
      args->g0 + args->count > args->stream_end)
    return hipErrorInvalidValue;
  const uint64_t lanes = (args->g0 + args->count - 1) / POSTE_SEAL_PAGE_LABELS -
                         args->g0 / POSTE_SEAL_PAGE_LABELS + 1;
  hipLaunchKernelGGL(
      post_seal_stream_kernel,
      dim3((uint32_t)((lanes + POSTE_SEAL_THREADS - 1) / POSTE_SEAL_THREADS)),
      dim3(POSTE_SEAL_THREADS), 0, stream, *args);
  return hipGetLastError();
}

hipError_t poste_launch_seal_kernel(const SealKernelArgs *args,
                                    hipStream_t stream) {
  if (!args->labels || !args->digests || args->count == 0)
    return hipErrorInvalidValue;
  const uint64_t pages =
      (args->count + POSTE_SEAL_PAGE_LABELS - 1) / POSTE_SEAL_PAGE_LABELS;
  hipLaunchKernelGGL(
      post_seal_kernel,
      dim3((uint32_t)((pages + POSTE_SEAL_THREADS - 1) / POSTE_SEAL_THREADS)),
      dim3(POSTE_SEAL_THREADS), 0, stream, *args);
  return hipGetLastError();
}

/* Whether the lean gap-1 ROMix kernel can address this scratch geometry:
 * its block offset is a 24-bit x 24-bit multiply of j < scrypt_n by the
 * slot stride scratch_lanes * 8 (in uint4), so scratch_lanes must stay
 * below 2^21 and scrypt_n within 2^24; the block index
 * scrypt_n * scratch_lanes is kept inside 32 bits as well.  Both always
 * hold on a 288 GB part: scratch_lanes never exceeds the resident quads
 * (256 CUs x 2048 threads / 4 = 2^17, twice that in slots), and the
 * scratch, 128 B * scrypt_n * scratch_lanes, would pass 512 GiB before the
 * block index passed 2^32.  Anything else runs the generic kernel. */
int poste_label_romix_lean_ok(uint32_t scrypt_n, uint32_t gap_shift,
                              uint64_t scratch_lanes) {
  return gap_shift == 0 && scrypt_n <= (1u << 24) &&
         scratch_lanes < (1ull << 21) &&
         (uint64_t)scrypt_n * scratch_lanes < (1ull << 32);
}

/* Grid of a SHA kernel (prologue, tail, audit tail): one lane per label, so
 * one workgroup per POSTE_THREADS labels, and never more workgroups than
 * the caller's `blocks`, which counts 64-quad ROMix workgroups.  The tail
 * appends at most one candidate per workgroup, so the callers' bounds on
 * candidates per launch, taken from `blocks`, hold as before. */
static uint32_t sha_blocks(const LabelKernelArgs *args, uint32_t blocks) {
  const uint64_t need = (args->count + POSTE_THREADS - 1) / POSTE_THREADS;
  const uint64_t g = need < blocks ? need : blocks;
  return g ? (uint32_t)g : 1u;
}

/* prologue + ROMix, the part every label pipeline shares */
static void launch_label_prologue_romix(const LabelKernelArgs *args,
                                        uint32_t blocks, hipStream_t stream) {
  /* Two labels per quad (a dual-stream form of the lean kernel, spill-free
   * at 58 VGPRs) measured 4% slower than one label per quad and was
   * removed: profiles/r03_kernel_stats.md. */
  hipLaunchKernelGGL(post_label_prologue_kernel,
                     dim3(sha_blocks(args, blocks)), dim3(POSTE_THREADS), 0,
                     stream, *args);
  if (poste_label_romix_lean_ok(args->scrypt_n, args->gap_shift,
                                args->scratch_lanes)) {
    hipLaunchKernelGGL(post_label_romix_kernel, dim3(blocks),
                       dim3(POSTE_THREADS), 0, stream, *args);
  } else {
    hipLaunchKernelGGL(post_label_romix_gap_kernel, dim3(blocks),
                       dim3(POSTE_THREADS), 0, stream, *args);
  }
}

hipError_t poste_launch_label_kernel(const LabelKernelArgs *args,
                                     uint32_t blocks, hipStream_t stream) {
  launch_label_prologue_romix(args, blocks, stream);
  hipLaunchKernelGGL(post_label_tail_kernel, dim3(sha_blocks(args, blocks)),
                     dim3(POSTE_THREADS), 0, stream, *args);
  return hipGetLastError();
}

hipError_t poste_launch_label_prologue(const LabelKernelArgs *args,
                                       uint32_t blocks, hipStream_t stream) {
  hipLaunchKernelGGL(post_label_prologue_kernel,
                     dim3(sha_blocks(args, blocks)), dim3(POSTE_THREADS), 0,
                     stream, *args);
  return hipGetLastError();
}

hipError_t poste_launch_label_tail(const LabelKernelArgs *args,
                                   uint32_t blocks, hipStream_t stream) {
  hipLaunchKernelGGL(post_label_tail_kernel, dim3(sha_blocks(args, blocks)),
                     dim3(POSTE_THREADS), 0, stream, *args);
  return hipGetLastError();
}

/* a phase launch must stay inside its columns and inside what the lean
 * addressing reaches; one workgroup per 64 tasks */
static bool romix_phase_ok(const RomixPhaseArgs *a) {
  return a->count >= 1 && a->count <= a->slot_count &&
         a->slot_base + a->slot_count <= a->scratch_lanes &&
         poste_label_romix_lean_ok(a->scrypt_n, 0, a->scratch_lanes);
}

hipError_t poste_launch_romix_fill(const RomixPhaseArgs *args,
                                   hipStream_t stream) {
  if (!romix_phase_ok(args)) return hipErrorInvalidValue;
  const uint32_t quads = POSTE_THREADS / 4;
  hipLaunchKernelGGL(post_label_romix_fill_kernel,
                     dim3((uint32_t)((args->count + quads - 1) / quads)),
                     dim3(POSTE_THREADS), 0, stream, *args);
  return hipGetLastError();
}

hipError_t poste_launch_romix_mix(const RomixPhaseArgs *args,
                                  hipStream_t stream) {
  if (!romix_phase_ok(args)) return hipErrorInvalidValue;
  const uint32_t quads = POSTE_THREADS / 4;
  hipLaunchKernelGGL(post_label_romix_mix_kernel,
                     dim3((uint32_t)((args->count + quads - 1) / quads)),
                     dim3(POSTE_THREADS), 0, stream, *args);
  return hipGetLastError();
}

/* postdata audit batch: same prologue and ROMix, then the comparing tail */
hipError_t poste_launch_label_audit(const AuditKernelArgs *args,
                                    uint32_t blocks, hipStream_t stream) {
  launch_label_prologue_romix(&args->label, blocks, stream);
  hipLaunchKernelGGL(post_label_audit_tail_kernel,
                     dim3(sha_blocks(&args->label, blocks)),
                     dim3(POSTE_THREADS), 0, stream, *args);
  return hipGetLastError();
}

hipError_t poste_launch_verify_pred_kernel(const VerifyPredArgs *args,
                                           uint32_t blocks,
                                           hipStream_t stream) {
  hipLaunchKernelGGL(post_verify_pred_kernel, dim3(blocks),
                     dim3(POSTE_THREADS), TeShared::LDS_BYTES, stream, *args);
  return hipGetLastError();
}

hipError_t poste_launch_vrf_pred_kernel(const VrfPredArgs *args,
                                        uint32_t blocks,
                                        hipStream_t stream) {
  if (!args->labels2 || !args->thresholds || !args->task_thr ||
      !args->pass || args->count == 0 || blocks == 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(post_vrf_pred_kernel, dim3(blocks),
                     dim3(POSTE_THREADS), 0, stream, *args);
  return hipGetLastError();
}

/* Max simultaneously-resident label SLOTS (in-flight labels) of the ROMix
 * kernel for the given gap config.  Scratch beyond this is wasted memory:
 * extra workgroups just queue. */
uint64_t poste_label_resident_slots(uint32_t gap_shift) {
  const void *kern =
      gap_shift == 0
          ? reinterpret_cast<const void *>(post_label_romix_kernel)
          : reinterpret_cast<const void *>(post_label_romix_gap_kernel);
  int blocks_per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kern,
                                                   POSTE_THREADS, 0) !=
          hipSuccess ||
      blocks_per_cu <= 0)
    blocks_per_cu = 2;
  hipDeviceProp_t prop;
  int dev = 0;
  (void)hipGetDevice(&dev);
  int cus = 256;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess)
    cus = prop.multiProcessorCount;
  return (uint64_t)blocks_per_cu * cus * (POSTE_THREADS / 4);
}

/* The scan variants, indexed by ScanVariant: name, threads per block, LDS
 * bytes, block cap.  The caps keep the grid at 2^21 lanes. */
static const struct {
  const char *name;
  ScanPlan plan;
} SCAN_VARIANTS[] = {
    {"shared",
     {POSTE_SCAN_SHARED, POSTE_THREADS, TeShared::LDS_BYTES, 8192}},
    {"bankrep",
     {POSTE_SCAN_BANKREP, POSTE_THREADS, TeBankrep::LDS_BYTES, 8192}},
    {"bankrepbg",
     {POSTE_SCAN_BANKREP_BG, POSTE_THREADS, TeBankrep::LDS_BYTES, 8192}},
    {"bankrep512", {POSTE_SCAN_BANKREP512, 512, TeBankrep::LDS_BYTES, 4096}},
    {"bankrep512bg",
     {POSTE_SCAN_BANKREP512_BG, 512, TeBankrep::LDS_BYTES, 4096}},
    {"tt4", {POSTE_SCAN_TT4, 1024, TeTt4::LDS_BYTES, 2048}},
};
constexpr int SCAN_VARIANT_COUNT =
    (int)(sizeof SCAN_VARIANTS / sizeof SCAN_VARIANTS[0]);
static_assert(SCAN_VARIANT_COUNT == POSTE_SCAN_TT4 + 1,
              "one SCAN_VARIANTS row per ScanVariant, in enum order");

const char *poste_scan_variant_name(int variant) {
  return variant >= 0 && variant < SCAN_VARIANT_COUNT
             ? SCAN_VARIANTS[variant].name
             : "?";
}

hipError_t poste_scan_plan(const char *mode, const char *max_blocks,
                           int allow_fallback, ScanPlan *out) {
  /* tt4 is the fastest measured (r2d sweep) */
  int v = mode ? POSTE_SCAN_BANKREP : POSTE_SCAN_TT4;
  for (const auto &e : SCAN_VARIANTS)
    if (mode && strcmp(mode, e.name) == 0) v = e.plan.variant;
  if (v == POSTE_SCAN_TT4) {
    const hipError_t e = hipFuncSetAttribute(
        (const void *)post_scan_tt4_kernel,
        hipFuncAttributeMaxDynamicSharedMemorySize, TeTt4::LDS_BYTES);
    if (e != hipSuccess && !allow_fallback) return e;
    if (e != hipSuccess) {
      v = POSTE_SCAN_BANKREP;
      (void)hipGetLastError(); /* the refusal must not meet the launch's */
    }
  }
  *out = SCAN_VARIANTS[v].plan;
  /* POST_SCAN_MAX_BLOCKS: lowers the cap, never raises it, never below 1;
   * zero or unparsable = the variant's own.  With a cap of a few blocks a
   * few thousand labels already make every ILP chain live and the
   * grid-stride loop iterate — what mainnet's 2^24-label chunks do at the
   * full grid — so tests reach those paths at small sizes. */
  if (max_blocks) {
    const long m = strtol(max_blocks, nullptr, 10);
    if (m >= 1 && m < (long)out->max_blocks) out->max_blocks = (uint32_t)m;
  }
  return hipSuccess;
}

hipError_t poste_launch_scan(const ScanKernelArgs *args, const ScanPlan *plan,
                             hipStream_t stream) {
  if (!args->labels || !args->hits || !args->hit_count || args->count == 0 ||
      plan->max_blocks == 0)
    return hipErrorInvalidValue;
  const uint64_t need = (args->count + plan->threads - 1) / plan->threads;
  const dim3 grid(need < plan->max_blocks ? (uint32_t)need : plan->max_blocks);
  const dim3 block(plan->threads);
  const size_t lds = plan->lds_bytes;
  switch (plan->variant) {
  case POSTE_SCAN_SHARED:
    hipLaunchKernelGGL(post_scan_kernel, grid, block, lds, stream, *args);
    break;
  case POSTE_SCAN_BANKREP:
    hipLaunchKernelGGL((post_scan_bankrep_kernel<POSTE_THREADS, false>), grid,
                       block, lds, stream, *args);
    break;
  case POSTE_SCAN_BANKREP_BG:
    hipLaunchKernelGGL((post_scan_bankrep_kernel<POSTE_THREADS, true>), grid,
                       block, lds, stream, *args);
    break;
  case POSTE_SCAN_BANKREP512:
    hipLaunchKernelGGL((post_scan_bankrep_kernel<512, false>), grid, block,
                       lds, stream, *args);
    break;
  case POSTE_SCAN_BANKREP512_BG:
    hipLaunchKernelGGL((post_scan_bankrep_kernel<512, true>), grid, block,
                       lds, stream, *args);
    break;
  case POSTE_SCAN_TT4:
    hipLaunchKernelGGL(post_scan_tt4_kernel, grid, block, lds, stream, *args);
    break;
  default:
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}
