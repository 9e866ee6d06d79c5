// gemm_rec3.h -- the rec64 GEMM of gemm_bf16s.h at f32 accuracy: both operands as arrays of THREE-part records, for the
// three large GEMMs of the R2D2 learner's LSTM input backward (R2d2BwdPlan::lstm_in_rec3, learner_plan.h):
//   dW_ih = dg^T a3   (2048 x 3136 x rows)      dW_hh = dg^T hprev   (2048 x 512 x rows)      d_a3 = dg W_ih   (rows x 3136 x 2048)
//
//   C[m][n] = sum_k A[m][k] * B[n][k]          ("NT": both operands k-contiguous)
//
// Record ("rec3"): per row, per chunk of 64 k, 384 B = [64 x p0 | 64 x p1 | 64 x p2] bf16 with x = p0 + p1 + p2 EXACTLY
// (p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), round to nearest even).  This is the split3 record of
// gemm_s3.h for C = 64, and the split kernels below call that header's split3_4: same arithmetic, same bits.
// Products: the six part products with i + j <= 2 on v_mfma_f32_16x16x32_bf16; p0 x p0 in an accumulator of its own, the
// five small ones in a second, added once in the epilogue (gemm_s3.h, dgrad_conv_x3.h; merged was measured less accurate).
// An f32 operand is split ONCE per step into records (gemm_bf16x3, PARTS = 3, re-splits every operand in every 64 x 64
// block that touches it).
//
// Kernel.  A k-stage of 32 is 3 x 64 B = 192 B per tile row.  Chosen: the two-part kernel's 256 x 128 block tile with
// UNPADDED 192-byte rows and a swizzle, 2 x 384 x 192 = 147,456 B of LDS, rather than 128 x 128 tiles with padded 224-byte
// rows (114,688 B): the GEMMs are bound by operand traffic (gemm_bf16s.h measured its own 128 x 128 form slower on the
// large GEMMs), a block's bytes per MFMA go with 1 / BM + 1 / BN, and neither form leaves room for a second block on the
// CU, so the padded form would only give up a third of the reuse.  The small GEMM (dW_hh, 32 large tiles) and d_a3 below
// 1,281 rows run the same template at 128 x 128 (98,304 B, eight waves of 64 x 32), as gemm_rec64_nt_s does.
//  * LDS row = [p0: 4 units | p1: 4 units | p2: 4 units] of 16 B, no pad.  Rows are 12 units apart, so rows r and r + 4
//    start on the same bank group: unit g of a part is stored at g ^ sw(r), sw(r) = bit-reversed ((r >> 2) & 3).  The 16
//    lanes of a ds_read_b128 pass then hit the 16 bank groups once each in both groupings the project's kernels allow for
//    (16 rows x 1 k-group: 12 r mod 16 gives four multiples of 4 by r & 3, sw the four units between them by r >> 2;
//    8 rows x 2 k-groups: rows 0-7 have sw in {0, 2}, rows 8-15 in {1, 3}, either XORed onto a pair {0, 1} or {2, 3}
//    gives four different units), and the 16 lanes of a ds_write_b128 pass (4 rows x 4 units) likewise.  Enumerated on
//    the host for every fragment read and staging store of both forms: at most one address per bank and pass; with
//    unswizzled 192-byte rows the same enumeration gives 4 (reads) and 1 (stores).
//  * Eight waves, two per SIMD, 64 x 64 each: 16 tiles x 2 accumulators = 128 registers.  Fragments per stage: B's p0 / p1
//    of the wave's four column tiles stay (32 registers); per row tile A's p0 is kept (16 in all), its p1 and p2 are read,
//    used for their products with B's p0 / p1 and dropped; B's p2 is read last, one column tile at a time, against the kept
//    A p0.  No p2 fragment outlives one group of four MFMAs.
//  * The next stage waits in nine named staging registers (no arrays, no branches around the loads) while this one's 96
//    MFMAs per wave run -- twice the two-part kernel's MFMA time per stage, which is why one register set is enough here
//    (and a second would not fit: 36 more registers); one barrier per stage; the XCD-aware block map of gemm_bf16s.h.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "gemm_bf16s.h"
#include "gemm_s3.h"
#include "prof.h"

namespace rela_amd {
namespace rec3 {
namespace {

using gemm16::bf16x8;
using gemm16::f32x4;

constexpr int kT = 512;              // 8 waves
constexpr int BM = 256, SBM = 128;   // row tile of the large / the small form
constexpr int BN = 128;              // column tile of both
constexpr int ROW = 192;             // LDS bytes per tile row and stage: three parts x 32 k, unpadded
constexpr int REC = 384;             // bytes per record (chunk of 64 k)
constexpr int PART = 128;            // bytes between the parts of a record
constexpr int lds_bytes(int bm) { return 2 * (bm + BN) * ROW; }  // 147,456 / 98,304

// the three parts of 8 consecutive f32 as three uint4 of packed bf16 (s3::split3_4 on either half)
__device__ __forceinline__ void split8_3(const float4 a, const float4 b, uint4& p0, uint4& p1, uint4& p2) {
  uint2 a0, a1, a2, b0, b1, b2;
  s3::split3_4(f32x4{a.x, a.y, a.z, a.w}, a0, a1, a2);
  s3::split3_4(f32x4{b.x, b.y, b.z, b.w}, b0, b1, b2);
  p0 = make_uint4(a0.x, a0.y, b0.x, b0.y), p1 = make_uint4(a1.x, a1.y, b1.x, b1.y), p2 = make_uint4(a2.x, a2.y, b2.x, b2.y);
}

// rows of an f32 matrix src[R][K] (K a multiple of 64, row stride K) -> records dst[R][K / 64]
__global__ void split_rows_rec3(const float* __restrict__ src, int64_t R, int K, uint8_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per 8 elements
  const int per_row = K >> 3;
  if (i >= R * per_row) return;
  const int64_t r = i / per_row;
  const int o = (int)(i - r * per_row);  // octet within the row
  const float* p = src + r * K + (int64_t)o * 8;
  uint4 p0, p1, p2;
  split8_3(*reinterpret_cast<const float4*>(p), *reinterpret_cast<const float4*>(p + 4), p0, p1, p2);
  uint8_t* rec = dst + (r * (K >> 6) + (o >> 3)) * REC + (o & 7) * 16;
  *reinterpret_cast<uint4*>(rec) = p0;
  *reinterpret_cast<uint4*>(rec + PART) = p1;
  *reinterpret_cast<uint4*>(rec + 2 * PART) = p2;
}

// COLUMNS of an f32 matrix src[R][C] (row stride C, C a multiple of 64) -> records dst[C][ceil(R / 64)]: record (c', chunk)
// holds rows 64 chunk .. 64 chunk + 63 of column c (zeros past row R), c' = c or, with a3_order, the state_dict column
// ch * 49 + pos of the channel-last column c = pos * 64 + ch (gemm_bf16s.h: split_cols_rec64).  One block per 64 x 64 tile.
__global__ __launch_bounds__(256) void split_cols_rec3(const float* __restrict__ src, int64_t R, int C, int a3_order,
                                                       uint8_t* __restrict__ dst) {
  __shared__ float tile[64][65];
  const int c0 = blockIdx.x * 64;
  const int64_t r0 = (int64_t)blockIdx.y * 64;
  const int tid = threadIdx.x;
  for (int i = tid; i < 64 * 16; i += 256) {
    const int r = i >> 4, q = i & 15;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < R) v = *reinterpret_cast<const float4*>(src + (r0 + r) * C + c0 + 4 * q);
    tile[r][4 * q] = v.x, tile[r][4 * q + 1] = v.y, tile[r][4 * q + 2] = v.z, tile[r][4 * q + 3] = v.w;
  }
  __syncthreads();
  const int64_t chunks = (R + 63) >> 6;
  for (int i = tid; i < 64 * 8; i += 256) {
    const int c = i >> 3, o = i & 7;  // column of the tile, octet of rows
    float4 a, b;
    a.x = tile[8 * o][c], a.y = tile[8 * o + 1][c], a.z = tile[8 * o + 2][c], a.w = tile[8 * o + 3][c];
    b.x = tile[8 * o + 4][c], b.y = tile[8 * o + 5][c], b.z = tile[8 * o + 6][c], b.w = tile[8 * o + 7][c];
    uint4 p0, p1, p2;
    split8_3(a, b, p0, p1, p2);
    const int cc = c0 + c;
    const int64_t row = a3_order ? (int64_t)(cc & 63) * 49 + (cc >> 6) : cc;
    uint8_t* rec = dst + (row * chunks + blockIdx.y) * REC + o * 16;
    *reinterpret_cast<uint4*>(rec) = p0;
    *reinterpret_cast<uint4*>(rec + PART) = p1;
    *reinterpret_cast<uint4*>(rec + 2 * PART) = p2;
  }
}

// the swizzle of a tile row: which of the four 16-byte units of a part its unit 0 is stored at
__device__ __forceinline__ int row_swizzle(int r) { return ((r >> 1) & 2) | ((r >> 3) & 1); }

// A: records [M][KC], B: records [N][KC] (N a multiple of 4), KC chunks of 64 k.  grid = 8 * NCB * ceil(NRB / 8).
// BM_ = 256: 4 x 2 waves of 64 x 64; BM_ = 128: 2 x 4 waves of 64 x 32.
template <int BM_, class Epi>
__global__ __launch_bounds__(kT) void gemm_rec3_nt(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, int M,
                                                   int N, int KC, Epi epi) {
  static_assert(BM_ == BM || BM_ == SBM, "row tile");
  constexpr bool kLarge = BM_ == BM;
  constexpr int NU = kLarge ? 4 : 2;  // column tiles of a wave
  constexpr int A_BYTES = BM_ * ROW, STAGE = (BM_ + BN) * ROW;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int NRB = (M + BM_ - 1) / BM_, NCB = (N + BN - 1) / BN;
  const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3;
  const int cb = sidx % NCB, rb = (sidx / NCB) * 8 + xcd;
  if (rb >= NRB) return;
  const int m0 = rb * BM_, n0 = cb * BN;
  const int wm = kLarge ? wave >> 1 : wave >> 2, wn = kLarge ? wave & 1 : wave & 3;

  // staging: thread -> unit su of the stage's 64 B of a part, tile rows srow (+ 128 for the large form's second half of A);
  // one named register per (row, part) (clamped rows: a tail block re-reads its last row instead of branching; those
  // accumulators are never stored)
  uint4 a0_0, a0_1, a0_2, a1_0, a1_1, a1_2, b_0, b_1, b_2;
  const int su = tid & 3, srow = tid >> 2;
  const size_t rstride = (size_t)KC * REC;
  const uint8_t* pa0 = A + (size_t)min(m0 + srow, M - 1) * rstride + su * 16;
  const uint8_t* pa1 = A + (size_t)min(m0 + srow + 128, M - 1) * rstride + su * 16;
  const uint8_t* pb = B + (size_t)min(n0 + srow, N - 1) * rstride + su * 16;
  const int sofs = srow * ROW + ((su ^ row_swizzle(srow)) << 4);  // (rows srow and srow + 128 share their swizzle)
#define RELA_R3_LOAD(ST)                                                \
  do {                                                                  \
    const int st__ = min((ST), 2 * KC - 1);                             \
    const int o__ = (st__ >> 1) * REC + (st__ & 1) * 64;                \
    a0_0 = *reinterpret_cast<const uint4*>(pa0 + o__);                  \
    a0_1 = *reinterpret_cast<const uint4*>(pa0 + o__ + PART);           \
    a0_2 = *reinterpret_cast<const uint4*>(pa0 + o__ + 2 * PART);       \
    if constexpr (kLarge) {                                             \
      a1_0 = *reinterpret_cast<const uint4*>(pa1 + o__);                \
      a1_1 = *reinterpret_cast<const uint4*>(pa1 + o__ + PART);         \
      a1_2 = *reinterpret_cast<const uint4*>(pa1 + o__ + 2 * PART);     \
    }                                                                   \
    b_0 = *reinterpret_cast<const uint4*>(pb + o__);                    \
    b_1 = *reinterpret_cast<const uint4*>(pb + o__ + PART);             \
    b_2 = *reinterpret_cast<const uint4*>(pb + o__ + 2 * PART);         \
  } while (0)
#define RELA_R3_STORE(BUF)                                              \
  do {                                                                  \
    uint8_t* ta__ = smem + (BUF) * STAGE + sofs;                        \
    *reinterpret_cast<uint4*>(ta__) = a0_0;                             \
    *reinterpret_cast<uint4*>(ta__ + 64) = a0_1;                        \
    *reinterpret_cast<uint4*>(ta__ + 128) = a0_2;                       \
    if constexpr (kLarge) {                                             \
      *reinterpret_cast<uint4*>(ta__ + 128 * ROW) = a1_0;               \
      *reinterpret_cast<uint4*>(ta__ + 128 * ROW + 64) = a1_1;          \
      *reinterpret_cast<uint4*>(ta__ + 128 * ROW + 128) = a1_2;         \
    }                                                                   \
    *reinterpret_cast<uint4*>(ta__ + A_BYTES) = b_0;                    \
    *reinterpret_cast<uint4*>(ta__ + A_BYTES + 64) = b_1;               \
    *reinterpret_cast<uint4*>(ta__ + A_BYTES + 128) = b_2;              \
  } while (0)

  f32x4 acc[4][NU], sml[4][NU];  // p0 x p0 | the five small products
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[t][u] = sml[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int NS = 2 * KC;
  RELA_R3_LOAD(0);
  RELA_R3_STORE(0);
  RELA_R3_LOAD(1);
  __syncthreads();
  // fragment of (tile row li, k-group g): the rows of a 16-row tile differ in li only, so li gives the swizzle
  const int fofs = li * ROW + ((g ^ row_swizzle(li)) << 4);
  const int aoff = wm * 64 * ROW + fofs, boff = A_BYTES + wn * (16 * NU) * ROW + fofs;
#define RELA_R3_MMA(C, W, X) C = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, W), __builtin_bit_cast(bf16x8, X), C, 0, 0, 0)
  // stage st is in LDS buffer st & 1 when iteration st starts; the staging registers hold stage st + 1
  for (int st = 0; st < NS; ++st) {
    const uint8_t* base = smem + (st & 1) * STAGE;
    uint4 w0[NU], w1[NU], x0[4];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      w0[u] = *reinterpret_cast<const uint4*>(base + boff + u * 16 * ROW);
      w1[u] = *reinterpret_cast<const uint4*>(base + boff + u * 16 * ROW + 64);
    }
    // operands swapped (B as the first operand): a lane ends up with C[m = li][n = 4 g .. 4 g + 3] of every tile
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      x0[t] = *reinterpret_cast<const uint4*>(base + aoff + t * 16 * ROW);
      const uint4 x1 = *reinterpret_cast<const uint4*>(base + aoff + t * 16 * ROW + 64);
      const uint4 x2 = *reinterpret_cast<const uint4*>(base + aoff + t * 16 * ROW + 128);
#pragma unroll
      for (int u = 0; u < NU; ++u) RELA_R3_MMA(sml[t][u], w0[u], x2);
#pragma unroll
      for (int u = 0; u < NU; ++u) RELA_R3_MMA(sml[t][u], w1[u], x1);
#pragma unroll
      for (int u = 0; u < NU; ++u) RELA_R3_MMA(sml[t][u], w0[u], x1);
#pragma unroll
      for (int u = 0; u < NU; ++u) RELA_R3_MMA(sml[t][u], w1[u], x0[t]);
#pragma unroll
      for (int u = 0; u < NU; ++u) RELA_R3_MMA(acc[t][u], w0[u], x0[t]);
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const uint4 w2 = *reinterpret_cast<const uint4*>(base + boff + u * 16 * ROW + 128);
#pragma unroll
      for (int t = 0; t < 4; ++t) RELA_R3_MMA(sml[t][u], w2, x0[t]);
    }
    RELA_R3_STORE((st + 1) & 1);  // (that buffer was last read in stage st - 1: every wave is past that barrier)
    RELA_R3_LOAD(st + 2);
    __syncthreads();
  }
#undef RELA_R3_MMA
#undef RELA_R3_LOAD
#undef RELA_R3_STORE
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int m = m0 + wm * 64 + t * 16 + li;
    if (m >= M) continue;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int n = n0 + wn * (16 * NU) + u * 16 + 4 * g;
      if (n < N) epi(m, n, acc[t][u] + sml[t][u]);
    }
  }
}

template <int BM_, class Epi>
inline int launch_rec3_form(const uint8_t* A, const uint8_t* B, int M, int N, int KC, Epi epi, hipStream_t s, const char* name) {
  // (initialised once, thread-safely: launches may come from several host threads)
  static const hipError_t attr_set = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_rec3_nt<BM_, Epi>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes(BM_));
  RELA_HIP(attr_set);
  const int NRB = ceil_div(M, BM_), NCB = ceil_div(N, BN);
  ProfScope prof(name, s);
  note_launch("gemm_rec3_nt");
  hipLaunchKernelGGL((gemm_rec3_nt<BM_, Epi>), dim3(8 * NCB * ceil_div(NRB, 8)), dim3(kT), lds_bytes(BM_), s, A, B, M, N, KC, epi);
  return RELA_OK;
}

// the small form when the large one would leave most CUs without a block (launch_rec64_nt's rule)
template <class Epi>
inline int launch_rec3_nt(const uint8_t* A, const uint8_t* B, int M, int N, int KC, Epi epi, hipStream_t s, const char* name) {
  if (ceil_div(M, BM) * ceil_div(N, BN) < 128) return launch_rec3_form<SBM>(A, B, M, N, KC, epi, s, name);
  return launch_rec3_form<BM>(A, B, M, N, KC, epi, s, name);
}

}  // namespace
}  // namespace rec3
}  // namespace rela_amd
