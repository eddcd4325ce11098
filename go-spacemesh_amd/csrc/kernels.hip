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
 * post_scan_kernel: the proving index scan (post-service GenProof,
 *   api/grpcserver/post_client.go:69-143): AES-128 over each 16-B label for
 *   n_ciphers ciphers (2 nonces per cipher), T-tables + round keys staged in
 *   LDS, passing (nonce,index) pairs appended with a global atomic.
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

/* ------------------------- proving scan kernel ------------------------- */
/* ScanKernelArgs: see kernel_args.h */

__global__ void __launch_bounds__(POSTE_THREADS)
post_scan_kernel(ScanKernelArgs a) {
  /* T-tables + sbox in LDS (random per-lane indices); round keys stay in
   * global — the cipher loop is wave-uniform, so they compile to scalar
   * loads through the constant cache instead of ~5.8K extra LDS reads per
   * label.  The kernel is LDS-conflict-throughput bound (ILP 1/2/4 all
   * measure ~274 M labels/s; a random 32-lane b32 gather costs
   * 2 x E[max 32-into-32-bank load] ~ 6.4 LDS cycles — see
   * profiles/r01_scan_sweep.md and MI355X_MICROARCH.md §LDS).  Two
   * gated A/B variants attack that wall (both UNVERIFIED on hardware,
   * round-2 retest):
   *   POSTE_SCAN_GLOBAL_TT — all lookups through the vector L1;
   *   POSTE_SCAN_SPLIT_TT — Te0/Te1 from LDS, Te2/Te3 through the L1,
   *     so the two memory pipes each carry half the gathers. */
#if defined(POSTE_SCAN_GLOBAL_TT)
  const uint32_t *TE_LO = a.te; /* Te0/Te1 (offsets 0, 256) */
  const uint32_t *TE_HI = a.te; /* Te2/Te3 (offsets 512, 768) */
  const uint8_t *sSbox = a.sbox;
#elif defined(POSTE_SCAN_SPLIT_TT)
  extern __shared__ uint32_t lds[];
  uint32_t *TE_LO = lds;                     /* Te0/Te1: 512 words */
  const uint32_t *TE_HI = a.te;              /* Te2/Te3 via L1 */
  uint8_t *sSbox = (uint8_t *)(lds + 512);   /* 256 bytes */
  for (uint32_t i = threadIdx.x; i < 512; i += blockDim.x) TE_LO[i] = a.te[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    sSbox[i] = a.sbox[i];
  __syncthreads();
#else
  extern __shared__ uint32_t lds[];
  uint32_t *sTe = lds;                      /* 1024 words */
  uint8_t *sSbox = (uint8_t *)(sTe + 1024); /* 256 bytes */
  uint32_t *TE_LO = sTe, *TE_HI = sTe;

  for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) sTe[i] = a.te[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    sSbox[i] = a.sbox[i];
  __syncthreads();
#endif

  /* Four independent labels per lane (ILP): a single AES chain leaves the
   * wave ~76% latency-stalled (profiles: SQ_ACTIVE_INST 10%, LDS 14%);
   * interleaving L chains fills the LDS-latency shadows. */
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
#ifndef POSTE_SCAN_ILP
#define POSTE_SCAN_ILP 2 /* 2 chains @ 8 waves/SIMD measured best */
#endif
  constexpr int L = POSTE_SCAN_ILP;
  const unsigned long long span = stride * L;
  for (unsigned long long t0 =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       t0 < a.count; t0 += span) {
    uint32_t p[L][4];
    unsigned long long ts[L];
#pragma unroll
    for (int u = 0; u < L; u++) {
      unsigned long long t = t0 + (unsigned long long)u * stride;
      ts[u] = t < a.count ? t : t0; /* clamp: duplicates are harmless
                                       (hits deduped by nonce list merge
                                       never occur: same index+nonce hits
                                       only appended for u==0's slot) */
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
      uint32_t w[L][4];
#pragma unroll
      for (int u = 0; u < L; u++)
#pragma unroll
        for (int k = 0; k < 4; k++) w[u][k] = p[u][k] ^ rk[k];
#pragma unroll
      for (int r = 1; r < 10; r++) {
#pragma unroll
        for (int u = 0; u < L; u++) {
          uint32_t n0 = TE_LO[w[u][0] >> 24] ^
                        TE_LO[256 + ((w[u][1] >> 16) & 0xff)] ^
                        TE_HI[512 + ((w[u][2] >> 8) & 0xff)] ^
                        TE_HI[768 + (w[u][3] & 0xff)] ^ rk[4 * r];
          uint32_t n1 = TE_LO[w[u][1] >> 24] ^
                        TE_LO[256 + ((w[u][2] >> 16) & 0xff)] ^
                        TE_HI[512 + ((w[u][3] >> 8) & 0xff)] ^
                        TE_HI[768 + (w[u][0] & 0xff)] ^ rk[4 * r + 1];
          uint32_t n2 = TE_LO[w[u][2] >> 24] ^
                        TE_LO[256 + ((w[u][3] >> 16) & 0xff)] ^
                        TE_HI[512 + ((w[u][0] >> 8) & 0xff)] ^
                        TE_HI[768 + (w[u][1] & 0xff)] ^ rk[4 * r + 2];
          uint32_t n3 = TE_LO[w[u][3] >> 24] ^
                        TE_LO[256 + ((w[u][0] >> 16) & 0xff)] ^
                        TE_HI[512 + ((w[u][1] >> 8) & 0xff)] ^
                        TE_HI[768 + (w[u][2] & 0xff)] ^ rk[4 * r + 3];
          w[u][0] = n0; w[u][1] = n1; w[u][2] = n2; w[u][3] = n3;
        }
      }
#pragma unroll
      for (int u = 0; u < L; u++) {
        if (u >= live) break;
        uint32_t f0 = (((uint32_t)sSbox[w[u][0] >> 24] << 24) |
                       ((uint32_t)sSbox[(w[u][1] >> 16) & 0xff] << 16) |
                       ((uint32_t)sSbox[(w[u][2] >> 8) & 0xff] << 8) |
                       sSbox[w[u][3] & 0xff]) ^ rk[40];
        uint32_t f1 = (((uint32_t)sSbox[w[u][1] >> 24] << 24) |
                       ((uint32_t)sSbox[(w[u][2] >> 16) & 0xff] << 16) |
                       ((uint32_t)sSbox[(w[u][3] >> 8) & 0xff] << 8) |
                       sSbox[w[u][0] & 0xff]) ^ rk[41];
        uint32_t f2 = (((uint32_t)sSbox[w[u][2] >> 24] << 24) |
                       ((uint32_t)sSbox[(w[u][3] >> 16) & 0xff] << 16) |
                       ((uint32_t)sSbox[(w[u][0] >> 8) & 0xff] << 8) |
                       sSbox[w[u][1] & 0xff]) ^ rk[42];
        uint32_t f3 = (((uint32_t)sSbox[w[u][3] >> 24] << 24) |
                       ((uint32_t)sSbox[(w[u][0] >> 16) & 0xff] << 16) |
                       ((uint32_t)sSbox[(w[u][1] >> 8) & 0xff] << 8) |
                       sSbox[w[u][2] & 0xff]) ^ rk[43];
        unsigned long long v0 =
            __builtin_bswap64(((unsigned long long)f0 << 32) | f1);
        unsigned long long v1 =
            __builtin_bswap64(((unsigned long long)f2 << 32) | f3);
        if (v0 < a.difficulty) {
          unsigned int s = atomicAdd(a.hit_count, 1u);
          if (s < a.hit_cap) {
            a.hits[s].index = a.index_base + ts[u];
            a.hits[s].nonce = c * POSTE_NONCES_PER_AES;
          }
        }
        if (v1 < a.difficulty) {
          unsigned int s = atomicAdd(a.hit_count, 1u);
          if (s < a.hit_cap) {
            a.hits[s].index = a.index_base + ts[u];
            a.hits[s].nonce = c * POSTE_NONCES_PER_AES + 1;
          }
        }
      }
    }
  }
}

/* Bank-replicated scan: one Te0 table replicated across the 32 LDS banks.
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
 * round's S-box is byte 1 of Te0 (te[x] packs [s2,s,s,s3] so s =
 * (te[x]>>8)&0xff) — no separate sbox table at all. */
#define ROR8(x) __builtin_amdgcn_alignbit((x), (x), 8)
#define ROR16(x) __builtin_amdgcn_alignbit((x), (x), 16)
#define ROR24(x) __builtin_amdgcn_alignbit((x), (x), 24)

template <int THREADS_, bool BATCHG>
__global__ void __launch_bounds__(THREADS_)
post_scan_bankrep_kernel(ScanKernelArgs a) {
  extern __shared__ uint32_t sTe[]; /* 8192 words = 32 copies x 1 KiB */
  for (uint32_t i = threadIdx.x; i < 8192; i += blockDim.x)
    sTe[i] = a.te[i >> 5]; /* consecutive lanes -> consecutive banks */
  __syncthreads();
  const uint32_t lane31 = threadIdx.x & 31;
#define TE0R(idx) sTe[(((uint32_t)(idx)) << 5) | lane31]

  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
#ifndef POSTE_SCAN_ILP
#define POSTE_SCAN_ILP 2
#endif
  constexpr int L = POSTE_SCAN_ILP;
  const unsigned long long span = stride * L;
  for (unsigned long long t0 =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       t0 < a.count; t0 += span) {
    uint32_t p[L][4];
    unsigned long long ts[L];
#pragma unroll
    for (int u = 0; u < L; u++) {
      unsigned long long t = t0 + (unsigned long long)u * stride;
      ts[u] = t < a.count ? t : t0; /* clamp: duplicate work, hits only
                                       recorded for live chains below */
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
      /* expanded key into registers up front: a.rk accesses inside the
       * round loop compile to per-round VECTOR global loads (wave-uniform
       * but the compiler cannot prove it) whose vmcnt waits serialize the
       * cipher loop */
      uint32_t rk[44];
#pragma unroll
      for (int k = 0; k < 44; k++) rk[k] = a.rk[c * 44 + k];
      uint32_t w[L][4];
#pragma unroll
      for (int u = 0; u < L; u++)
#pragma unroll
        for (int k = 0; k < 4; k++) w[u][k] = p[u][k] ^ rk[k];
#pragma unroll
      for (int r = 1; r < 10; r++) {
        if (BATCHG) {
          /* issue all of the round's gathers before any combine: widens
           * the read->use distance so partial lgkmcnt waits overlap the
           * whole gather batch with the previous combines */
          uint32_t g[L][16];
#pragma unroll
          for (int u = 0; u < L; u++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
              g[u][4 * q + 0] = TE0R(w[u][q] >> 24);
              g[u][4 * q + 1] = TE0R((w[u][(q + 1) & 3] >> 16) & 0xff);
              g[u][4 * q + 2] = TE0R((w[u][(q + 2) & 3] >> 8) & 0xff);
              g[u][4 * q + 3] = TE0R(w[u][(q + 3) & 3] & 0xff);
            }
#pragma unroll
          for (int u = 0; u < L; u++)
#pragma unroll
            for (int q = 0; q < 4; q++)
              w[u][q] = g[u][4 * q] ^ ROR8(g[u][4 * q + 1]) ^
                        ROR16(g[u][4 * q + 2]) ^ ROR24(g[u][4 * q + 3]) ^
                        rk[4 * r + q];
        } else {
#pragma unroll
        for (int u = 0; u < L; u++) {
          uint32_t n0 = TE0R(w[u][0] >> 24) ^
                        ROR8(TE0R((w[u][1] >> 16) & 0xff)) ^
                        ROR16(TE0R((w[u][2] >> 8) & 0xff)) ^
                        ROR24(TE0R(w[u][3] & 0xff)) ^ rk[4 * r];
          uint32_t n1 = TE0R(w[u][1] >> 24) ^
                        ROR8(TE0R((w[u][2] >> 16) & 0xff)) ^
                        ROR16(TE0R((w[u][3] >> 8) & 0xff)) ^
                        ROR24(TE0R(w[u][0] & 0xff)) ^ rk[4 * r + 1];
          uint32_t n2 = TE0R(w[u][2] >> 24) ^
                        ROR8(TE0R((w[u][3] >> 16) & 0xff)) ^
                        ROR16(TE0R((w[u][0] >> 8) & 0xff)) ^
                        ROR24(TE0R(w[u][1] & 0xff)) ^ rk[4 * r + 2];
          uint32_t n3 = TE0R(w[u][3] >> 24) ^
                        ROR8(TE0R((w[u][0] >> 16) & 0xff)) ^
                        ROR16(TE0R((w[u][1] >> 8) & 0xff)) ^
                        ROR24(TE0R(w[u][2] & 0xff)) ^ rk[4 * r + 3];
          w[u][0] = n0; w[u][1] = n1; w[u][2] = n2; w[u][3] = n3;
        }
        }
      }
      /* final round: S[x] = (Te0[x]>>8)&0xff; assemble each output word
       * from four replicated-table gathers (still conflict-free) */
#define SB24(idx) ((TE0R(idx) & 0xff00u) << 16)
#define SB16(idx) ((TE0R(idx) & 0xff00u) << 8)
#define SB08(idx) (TE0R(idx) & 0xff00u)
#define SB00(idx) ((TE0R(idx) >> 8) & 0xffu)
#pragma unroll
      for (int u = 0; u < L; u++) {
        if (u >= live) break;
        uint32_t f0 = (SB24(w[u][0] >> 24) | SB16((w[u][1] >> 16) & 0xff) |
                       SB08((w[u][2] >> 8) & 0xff) | SB00(w[u][3] & 0xff)) ^
                      rk[40];
        uint32_t f1 = (SB24(w[u][1] >> 24) | SB16((w[u][2] >> 16) & 0xff) |
                       SB08((w[u][3] >> 8) & 0xff) | SB00(w[u][0] & 0xff)) ^
                      rk[41];
        uint32_t f2 = (SB24(w[u][2] >> 24) | SB16((w[u][3] >> 16) & 0xff) |
                       SB08((w[u][0] >> 8) & 0xff) | SB00(w[u][1] & 0xff)) ^
                      rk[42];
        uint32_t f3 = (SB24(w[u][3] >> 24) | SB16((w[u][0] >> 16) & 0xff) |
                       SB08((w[u][1] >> 8) & 0xff) | SB00(w[u][2] & 0xff)) ^
                      rk[43];
        unsigned long long v0 =
            __builtin_bswap64(((unsigned long long)f0 << 32) | f1);
        unsigned long long v1 =
            __builtin_bswap64(((unsigned long long)f2 << 32) | f3);
        if (v0 < a.difficulty) {
          unsigned int s = atomicAdd(a.hit_count, 1u);
          if (s < a.hit_cap) {
            a.hits[s].index = a.index_base + ts[u];
            a.hits[s].nonce = c * POSTE_NONCES_PER_AES;
          }
        }
        if (v1 < a.difficulty) {
          unsigned int s = atomicAdd(a.hit_count, 1u);
          if (s < a.hit_cap) {
            a.hits[s].index = a.index_base + ts[u];
            a.hits[s].nonce = c * POSTE_NONCES_PER_AES + 1;
          }
        }
      }
    }
  }
#undef TE0R
#undef SB24
#undef SB16
#undef SB08
#undef SB00
}

/* 4-table interleaved bank-replicated scan: all four Te tables, each
 * bank-replicated, interleaved so entry (x, t, lane) sits at word
 * x*128 + t*32 + lane%32 — per-gather addressing is one v_lshl_add with
 * the t*128-byte offset folded into the ds_read immediate, and the
 * alignbit rotations of the 1-table variant disappear (~20% of its
 * VALU).  Costs 128 KiB LDS, so one 1024-thread workgroup per CU
 * (16 waves) instead of 20. */
__global__ void __launch_bounds__(1024)
post_scan_tt4_kernel(ScanKernelArgs a) {
  extern __shared__ uint32_t sTe[]; /* 32768 words = 4 tables x 32 copies */
  for (uint32_t i = threadIdx.x; i < 32768; i += blockDim.x)
    sTe[i] = a.te[((i >> 5) & 3) * 256 + (i >> 7)];
  __syncthreads();
  const uint32_t *t0p = sTe + (threadIdx.x & 31);
#define TT4(t, idx) t0p[(((uint32_t)(idx)) << 7) + 32 * (t)]

  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  /* ILP 4 measured best for this variant (r2d sweep); at one workgroup
   * per CU there are only 16 waves to hide latency, so deeper chains pay */
  constexpr int L = POSTE_SCAN_ILP > 4 ? POSTE_SCAN_ILP : 4;
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
      uint32_t rk[44];
#pragma unroll
      for (int k = 0; k < 44; k++) rk[k] = a.rk[c * 44 + k];
      uint32_t w[L][4];
#pragma unroll
      for (int u = 0; u < L; u++)
#pragma unroll
        for (int k = 0; k < 4; k++) w[u][k] = p[u][k] ^ rk[k];
#pragma unroll
      for (int r = 1; r < 10; r++) {
#pragma unroll
        for (int u = 0; u < L; u++) {
          uint32_t n0 = TT4(0, w[u][0] >> 24) ^
                        TT4(1, (w[u][1] >> 16) & 0xff) ^
                        TT4(2, (w[u][2] >> 8) & 0xff) ^
                        TT4(3, w[u][3] & 0xff) ^ rk[4 * r];
          uint32_t n1 = TT4(0, w[u][1] >> 24) ^
                        TT4(1, (w[u][2] >> 16) & 0xff) ^
                        TT4(2, (w[u][3] >> 8) & 0xff) ^
                        TT4(3, w[u][0] & 0xff) ^ rk[4 * r + 1];
          uint32_t n2 = TT4(0, w[u][2] >> 24) ^
                        TT4(1, (w[u][3] >> 16) & 0xff) ^
                        TT4(2, (w[u][0] >> 8) & 0xff) ^
                        TT4(3, w[u][1] & 0xff) ^ rk[4 * r + 2];
          uint32_t n3 = TT4(0, w[u][3] >> 24) ^
                        TT4(1, (w[u][0] >> 16) & 0xff) ^
                        TT4(2, (w[u][1] >> 8) & 0xff) ^
                        TT4(3, w[u][2] & 0xff) ^ rk[4 * r + 3];
          w[u][0] = n0; w[u][1] = n1; w[u][2] = n2; w[u][3] = n3;
        }
      }
      /* final round: S[x] = (Te0[x]>>8)&0xff, t=0 plane */
#define SB24_4(idx) ((TT4(0, idx) & 0xff00u) << 16)
#define SB16_4(idx) ((TT4(0, idx) & 0xff00u) << 8)
#define SB08_4(idx) (TT4(0, idx) & 0xff00u)
#define SB00_4(idx) ((TT4(0, idx) >> 8) & 0xffu)
#pragma unroll
      for (int u = 0; u < L; u++) {
        if (u >= live) break;
        uint32_t f0 = (SB24_4(w[u][0] >> 24) |
                       SB16_4((w[u][1] >> 16) & 0xff) |
                       SB08_4((w[u][2] >> 8) & 0xff) |
                       SB00_4(w[u][3] & 0xff)) ^ rk[40];
        uint32_t f1 = (SB24_4(w[u][1] >> 24) |
                       SB16_4((w[u][2] >> 16) & 0xff) |
                       SB08_4((w[u][3] >> 8) & 0xff) |
                       SB00_4(w[u][0] & 0xff)) ^ rk[41];
        uint32_t f2 = (SB24_4(w[u][2] >> 24) |
                       SB16_4((w[u][3] >> 16) & 0xff) |
                       SB08_4((w[u][0] >> 8) & 0xff) |
                       SB00_4(w[u][1] & 0xff)) ^ rk[42];
        uint32_t f3 = (SB24_4(w[u][3] >> 24) |
                       SB16_4((w[u][0] >> 16) & 0xff) |
                       SB08_4((w[u][1] >> 8) & 0xff) |
                       SB00_4(w[u][2] & 0xff)) ^ rk[43];
        unsigned long long v0 =
            __builtin_bswap64(((unsigned long long)f0 << 32) | f1);
        unsigned long long v1 =
            __builtin_bswap64(((unsigned long long)f2 << 32) | f3);
        if (v0 < a.difficulty) {
          unsigned int s = atomicAdd(a.hit_count, 1u);
          if (s < a.hit_cap) {
            a.hits[s].index = a.index_base + ts[u];
            a.hits[s].nonce = c * POSTE_NONCES_PER_AES;
          }
        }
        if (v1 < a.difficulty) {
          unsigned int s = atomicAdd(a.hit_count, 1u);
          if (s < a.hit_cap) {
            a.hits[s].index = a.index_base + ts[u];
            a.hits[s].nonce = c * POSTE_NONCES_PER_AES + 1;
          }
        }
      }
    }
  }
#undef TT4
#undef SB24_4
#undef SB16_4
#undef SB08_4
#undef SB00_4
}

/* verification's final predicate: AES-encrypt each recomputed label with
 * its proof's cipher and compare the nonce-half u64 against the proof's
 * difficulty (the last step of verifying.ProofVerifier.Verify,
 * post_verifier.go:159 -> per-index AES threshold check). */
__global__ void __launch_bounds__(POSTE_THREADS)
post_verify_pred_kernel(VerifyPredArgs a) {
  extern __shared__ uint32_t lds[];
  uint32_t *sTe = lds;
  uint8_t *sSbox = (uint8_t *)(sTe + 1024);
  for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) sTe[i] = a.te[i];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
    sSbox[i] = a.sbox[i];
  __syncthreads();
  const unsigned long long stride =
      (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long t =
           (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       t < a.count; t += stride) {
    const uint32_t pidx = a.task_proof[t];
    const uint32_t *rk = a.rk + (unsigned long long)pidx * 44;
    uint4 lraw = a.labels2[2 * t]; /* first 16 B of the full label */
    uint32_t w0 = __builtin_bswap32(lraw.x) ^ rk[0];
    uint32_t w1 = __builtin_bswap32(lraw.y) ^ rk[1];
    uint32_t w2 = __builtin_bswap32(lraw.z) ^ rk[2];
    uint32_t w3 = __builtin_bswap32(lraw.w) ^ rk[3];
#pragma unroll
    for (int r = 1; r < 10; r++) {
      uint32_t n0 = sTe[w0 >> 24] ^ sTe[256 + ((w1 >> 16) & 0xff)] ^
                    sTe[512 + ((w2 >> 8) & 0xff)] ^ sTe[768 + (w3 & 0xff)] ^
                    rk[4 * r];
      uint32_t n1 = sTe[w1 >> 24] ^ sTe[256 + ((w2 >> 16) & 0xff)] ^
                    sTe[512 + ((w3 >> 8) & 0xff)] ^ sTe[768 + (w0 & 0xff)] ^
                    rk[4 * r + 1];
      uint32_t n2 = sTe[w2 >> 24] ^ sTe[256 + ((w3 >> 16) & 0xff)] ^
                    sTe[512 + ((w0 >> 8) & 0xff)] ^ sTe[768 + (w1 & 0xff)] ^
                    rk[4 * r + 2];
      uint32_t n3 = sTe[w3 >> 24] ^ sTe[256 + ((w0 >> 16) & 0xff)] ^
                    sTe[512 + ((w1 >> 8) & 0xff)] ^ sTe[768 + (w2 & 0xff)] ^
                    rk[4 * r + 3];
      w0 = n0; w1 = n1; w2 = n2; w3 = n3;
    }
    uint32_t f0 = (((uint32_t)sSbox[w0 >> 24] << 24) |
                   ((uint32_t)sSbox[(w1 >> 16) & 0xff] << 16) |
                   ((uint32_t)sSbox[(w2 >> 8) & 0xff] << 8) |
                   sSbox[w3 & 0xff]) ^ rk[40];
    uint32_t f1 = (((uint32_t)sSbox[w1 >> 24] << 24) |
                   ((uint32_t)sSbox[(w2 >> 16) & 0xff] << 16) |
                   ((uint32_t)sSbox[(w3 >> 8) & 0xff] << 8) |
                   sSbox[w0 & 0xff]) ^ rk[41];
    uint32_t f2 = (((uint32_t)sSbox[w2 >> 24] << 24) |
                   ((uint32_t)sSbox[(w3 >> 16) & 0xff] << 16) |
                   ((uint32_t)sSbox[(w0 >> 8) & 0xff] << 8) |
                   sSbox[w1 & 0xff]) ^ rk[42];
    uint32_t f3 = (((uint32_t)sSbox[w3 >> 24] << 24) |
                   ((uint32_t)sSbox[(w0 >> 16) & 0xff] << 16) |
                   ((uint32_t)sSbox[(w1 >> 8) & 0xff] << 8) |
                   sSbox[w2 & 0xff]) ^ rk[43];
    unsigned long long v =
        a.half[pidx] == 0
            ? __builtin_bswap64(((unsigned long long)f0 << 32) | f1)
            : __builtin_bswap64(((unsigned long long)f2 << 32) | f3);
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
  size_t lds = 1024 * 4 + 256;
  hipLaunchKernelGGL(post_verify_pred_kernel, dim3(blocks),
                     dim3(POSTE_THREADS), lds, stream, *args);
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

/* POST_SCAN_MAX_BLOCKS lowers a scan variant's block cap (never raises it,
 * never below 1; unset, zero or unparsable = the variant's own cap).  With
 * a cap of a few blocks a few thousand labels already make every ILP chain
 * live and the grid-stride loop iterate — what mainnet's 2^24-label chunks
 * do at the full grid — so tests reach those paths at small sizes. */
static uint32_t scan_block_cap(uint32_t variant_cap) {
  const char *e = getenv("POST_SCAN_MAX_BLOCKS");
  if (!e) return variant_cap;
  long v = strtol(e, nullptr, 10);
  return v >= 1 && v < (long)variant_cap ? (uint32_t)v : variant_cap;
}

hipError_t poste_launch_scan_kernel(const ScanKernelArgs *args,
                                    uint32_t blocks, hipStream_t stream) {
  /* POST_SCAN_MODE: shared = round-1 shared-T-table kernel; tt4 =
   * 4-table/128KiB replicated kernel; bankrep512 / bankrepbg /
   * bankrep512bg = bank-replicated at 512-thread workgroups and/or
   * batched-gather scheduling; default = bank-replicated Te0 at 256.
   * Read per launch (launches are ms-scale) so tests can A/B kernels
   * within one process. */
  const uint32_t cap = scan_block_cap(8192);
  if (blocks > cap) blocks = cap;
  const char *e = getenv("POST_SCAN_MODE");
  const char *m = e ? e : "tt4"; /* fastest measured (r2d sweep); falls
                                    back to bankrep without 128 KiB LDS */
  if (strcmp(m, "shared") == 0) {
    size_t lds = 1024 * 4 + 256;
    hipLaunchKernelGGL(post_scan_kernel, dim3(blocks), dim3(POSTE_THREADS),
                       lds, stream, *args);
    return hipGetLastError();
  }
  if (strcmp(m, "tt4") == 0) {
    static bool attr_ok = [] {
      return hipFuncSetAttribute(
                 (const void *)post_scan_tt4_kernel,
                 hipFuncAttributeMaxDynamicSharedMemorySize,
                 32768 * 4) == hipSuccess;
    }();
    if (attr_ok) {
      uint32_t b4 = (uint32_t)((args->count + 1023) / 1024);
      const uint32_t cap4 = scan_block_cap(2048);
      if (b4 > cap4) b4 = cap4;
      if (b4 == 0) b4 = 1;
      hipLaunchKernelGGL(post_scan_tt4_kernel, dim3(b4), dim3(1024),
                         32768 * 4, stream, *args);
      return hipGetLastError();
    }
    m = "bankrep"; /* 128 KiB dynamic LDS unavailable */
  }
  const bool bg = strstr(m, "bg") != nullptr;
  const bool wide = strstr(m, "512") != nullptr;
  size_t lds = 8192 * 4; /* 32 bank-strided copies of Te0 */
  if (wide) {
    uint32_t b5 = (uint32_t)((args->count + 511) / 512);
    const uint32_t cap5 = scan_block_cap(4096);
    if (b5 > cap5) b5 = cap5;
    if (b5 == 0) b5 = 1;
    if (bg)
      hipLaunchKernelGGL((post_scan_bankrep_kernel<512, true>), dim3(b5),
                         dim3(512), lds, stream, *args);
    else
      hipLaunchKernelGGL((post_scan_bankrep_kernel<512, false>), dim3(b5),
                         dim3(512), lds, stream, *args);
  } else if (bg) {
    hipLaunchKernelGGL((post_scan_bankrep_kernel<POSTE_THREADS, true>),
                       dim3(blocks), dim3(POSTE_THREADS), lds, stream,
                       *args);
  } else {
    hipLaunchKernelGGL((post_scan_bankrep_kernel<POSTE_THREADS, false>),
                       dim3(blocks), dim3(POSTE_THREADS), lds, stream,
                       *args);
  }
  return hipGetLastError();
}

/* The proving scan over a batch that already lies in device memory (an init
 * batch behind its tail kernels), on the caller's stream.  The
 * kernels are those of poste_launch_scan_kernel, unchanged; what differs is
 * that nothing is read from the environment per launch: the session picks
 * the variant once, prepares it once (the 128 KiB dynamic-LDS opt-in of tt4
 * is a function attribute, set outside any stream), and fixes the grid cap. */
hipError_t poste_scan_resident_prepare(int variant) {
  if (variant == POSTE_SCAN_RESIDENT_BANKREP) return hipSuccess;
  if (variant != POSTE_SCAN_RESIDENT_TT4) return hipErrorInvalidValue;
  return hipFuncSetAttribute((const void *)post_scan_tt4_kernel,
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             32768 * 4);
}

uint32_t poste_scan_resident_threads(int variant) {
  return variant == POSTE_SCAN_RESIDENT_TT4 ? 1024 : POSTE_THREADS;
}

hipError_t poste_launch_scan_resident(const ScanKernelArgs *args, int variant,
                                      uint32_t max_blocks,
                                      hipStream_t stream) {
  if (!args->labels || !args->hits || !args->hit_count || args->count == 0 ||
      max_blocks == 0)
    return hipErrorInvalidValue;
  const uint32_t threads = poste_scan_resident_threads(variant);
  const uint64_t need = (args->count + threads - 1) / threads;
  const uint32_t blocks = need < max_blocks ? (uint32_t)need : max_blocks;
  if (variant == POSTE_SCAN_RESIDENT_TT4)
    hipLaunchKernelGGL(post_scan_tt4_kernel, dim3(blocks), dim3(1024),
                       32768 * 4, stream, *args);
  else if (variant == POSTE_SCAN_RESIDENT_BANKREP)
    hipLaunchKernelGGL((post_scan_bankrep_kernel<POSTE_THREADS, false>),
                       dim3(blocks), dim3(POSTE_THREADS), 8192 * 4, stream,
                       *args);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
}
