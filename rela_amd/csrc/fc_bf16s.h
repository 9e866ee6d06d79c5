// fc_bf16s.h -- the AtariFFNet's fc (3136 -> 512): fc_bf16s on split-bf16 MFMA straight from a3's records, whole or split
// over slices of positions (fc_reduce, gemm_f32.h, sums them).  Included by ffnet.hip only: the kernels live in
// rela_amd::(anonymous).
#pragma once
#include <type_traits>

#include "ffnet_plan.h"
#include "gemm_f32.h"

namespace rela_amd {
namespace {

// fc on split records: out[N][512] = relu(A x W + b), A = a3 records [N][49][hi 64 | lo 64], k = pos*64 + c.
// Block = BM rows x 128 columns (8 waves, one 16-column tile each).  A arrives per position (256 B per row) through
// registers into a THREE-deep LDS ring (row stride 288 B: conflict-free ds_read_b128), loaded from HBM two
// positions before it is stored; the A fragment reads run RT (hi, lo) pairs ahead of their MFMAs in a register
// ring that continues across positions (the next position's tile was published one barrier earlier); weight
// fragments stream from L2 one position ahead.  BM = 112 fills 232 of the 256 CUs at N = 6400 (128: 200).
template <int BM_>
struct FcFastT {
  static constexpr int OC = 512, BM = BM_, RT = BM / 16, NPOS = 49, KS = 98;  // K = 3136 = 98 k-steps of 32
  static constexpr int RS = 288;                                              // LDS row stride in bytes (18 units = 2 mod 16)
  static constexpr int TILE = BM * RS, NBUF = 3;
  static constexpr int LDS_BYTES = NBUF * TILE;
  static constexpr int V16 = BM * 16;  // 16-byte chunks per position
  static constexpr int IT = (V16 + kThreads - 1) / kThreads;
  static constexpr int TOT = 2 * RT, D = RT;  // fragment pairs per position, pairs in flight
};
using FcFast = FcFastT<112>;
static_assert(FcFast::BM == kFcBf16BlockRows && FcFast::NPOS == kFcPositions && kNumCU == kPlanCUs,
              "fc_bf16_slices (ffnet_plan.h) counts with the kernel's own block");

// SPLIT (batches of a few hundred rows, where 4 x ceil(N / BM) blocks would leave most CUs idle): blockIdx.z owns the
// positions [z * per, z * per + per) of the contraction and writes its raw partial sums to out[z][N][512]; fc_reduce adds
// them up in z order with the bias and the ReLU.  Without SPLIT the range is the compile-time [0, 49).
// grid of fc_bf16s for `units` (row block, slice) pairs: the XCD-aware 1-D form (see the block map in the kernel)
inline dim3 fc_grid_xcd(int rb, int slices) { return dim3(32 * ceil_div(rb * slices, 8)); }
// Loads stay ordinary (compiler-tracked) loads.  Tried in r3 and dropped: issuing them through inline asm with
// hand-placed `s_waitcnt vmcnt(N)` (hipcc drains the loads in flight across the loop's back-edge every other position,
// vmcnt(4), i.e. a prefetch distance of one position where the source asks for two).  With the copy-behind-the-wait
// blocks that makes sound (a tied "+v" wait is not: the compiler satisfies the tie with a copy BEFORE the wait, and it
// reuses the registers of a prefetch past the end while that load can still land) the kernel was 4 % SLOWER
// (71.3 vs 68.2 us at N = 6400): the exposed wait is not what bounds a position.
template <class F, bool SPLIT = false, bool STAMPS = false>
__global__ __launch_bounds__(kThreads) void fc_bf16s(const uint8_t* __restrict__ A, const uint4* __restrict__ Bfrag,
                                                     const float* __restrict__ bias, float* __restrict__ out, int N,
                                                     int per, unsigned long long* stamps = nullptr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  // STAMPS (rela_ffnet_debug_fc_stamps only): shader clock at the phase boundaries of positions 8..15, block 0,
  // waves 0 and 7 -> stamps [2][kStampFrames][kStampPoints]
  int stamp_pos = 0;
  auto stamp = [&](int point) {
    if constexpr (STAMPS) {
      if (blockIdx.x == 0 && (threadIdx.x == 0 || threadIdx.x == 448) && stamp_pos >= 8 && stamp_pos < 8 + kStampFrames)
        stamps[((threadIdx.x == 0 ? 0 : 1) * kStampFrames + stamp_pos - 8) * kStampPoints + point] = __builtin_amdgcn_s_memtime();
    }
  };
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  // Block -> (column group, row block, slice).  A 1-D grid (fc_grid_xcd) is XCD-aware: workgroups go to the 8 XCDs
  // round-robin by linear id, so the four column groups that read the SAME rows of A are given ids with the same
  // id % 8 and consecutive id / 8 -- they run on one XCD at the same time and A comes from HBM once instead of four
  // times (the (4, rb) grid put them on four XCDs: 334 MB of HBM reads for 80 MB of records at N = 6400; 126 MB now,
  // the weights included, which no longer fit one XCD's L2).  Ids past the last unit leave at once (block-uniform,
  // before any barrier).
  int cg, rb_, sl;
  if (gridDim.x == 4) {
    cg = blockIdx.x, rb_ = blockIdx.y, sl = blockIdx.z;
  } else {
    const int rb = (N + F::BM - 1) / F::BM;
    const int units = rb * (SPLIT ? (F::NPOS + per - 1) / per : 1);
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int unit = (j >> 2) * 8 + xcd;
    if (unit >= units) return;
    cg = j & 3, rb_ = unit % rb, sl = unit / rb;
  }
  const int ct = cg * kWaves + wave;
  const int row0 = rb_ * F::BM;
  const int p0 = SPLIT ? sl * per : 0;
  const int p1 = SPLIT ? min(F::NPOS, p0 + per) : F::NPOS;
  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;
  // Staging registers: set s holds the tile chunks / weight fragments of the positions of parity s (relative to p0).
  // No predicates on the staging loads and stores (clamped indices repeat a neighbour's chunk, row or position).
  u32x4 st0[F::IT], st1[F::IT], bq0[4], bq1[4];
  const int nrow = min(F::BM, N - row0);
  const uint8_t* arow[F::IT];  // this thread's chunk j of position 0
  int soff[F::IT];
#pragma unroll
  for (int j = 0; j < F::IT; ++j) {
    const int i = min(tid + j * kThreads, F::V16 - 1);
    arow[j] = A + (size_t)(row0 + min(i >> 4, nrow - 1)) * (F::NPOS * 256) + (i & 15) * 16;
    soff[j] = (i >> 4) * F::RS + (i & 15) * 16;
  }
  auto load_chunk = [&](int pos, auto set, int j) {
    const uint8_t* src = arow[j] + min(pos, p1 - 1) * 256;
    if constexpr (decltype(set)::value == 0) st0[j] = *reinterpret_cast<const u32x4*>(src); else st1[j] = *reinterpret_cast<const u32x4*>(src);
  };
  auto store_chunk = [&](int buf, auto set, int j) {
    u32x4* dst = reinterpret_cast<u32x4*>(smem + buf * F::TILE + soff[j]);
    if constexpr (decltype(set)::value == 0) *dst = st0[j]; else *dst = st1[j];
  };
  const uint4* bp = Bfrag + (size_t)ct * F::KS * 2 * 64 + lane;
  auto load_w = [&](int pos, auto set) {  // k-steps 0, 1 of the position x (hi, lo)
    const u32x4* src = reinterpret_cast<const u32x4*>(bp + (size_t)(min(pos, p1 - 1) * 4) * 64);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (decltype(set)::value == 0) bq0[q] = src[q * 64]; else bq1[q] = src[q * 64];
    }
  };
  f32x4 acc[F::RT];
#pragma unroll
  for (int t = 0; t < F::RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Prologue: tiles p0 and p0 + 1 into the ring; then the loads a steady-state position finds in flight, in its
  // order: W(p) | A(p + 2) | W(p + 1) | A(p + 3)
#pragma unroll
  for (int j = 0; j < F::IT; ++j) load_chunk(p0, Set0{}, j);
#pragma unroll
  for (int j = 0; j < F::IT; ++j) load_chunk(p0 + 1, Set1{}, j);
#pragma unroll
  for (int j = 0; j < F::IT; ++j) {
    store_chunk(0, Set0{}, j);
    store_chunk(1, Set1{}, j);
  }
  load_w(p0, Set0{});
#pragma unroll
  for (int j = 0; j < F::IT; ++j) load_chunk(p0 + 2, Set0{}, j);
  load_w(p0 + 1, Set1{});
#pragma unroll
  for (int j = 0; j < F::IT; ++j) load_chunk(p0 + 3, Set1{}, j);
  __syncthreads();

  // A fragment ring: pair i of a position = (sub = i / RT, row tile t = i % RT)
  uint4 ah[F::D], al[F::D];
  const int aoff = li * F::RS + g * 16;
  auto a_issue = [&](const uint8_t* tile, int i, int slot) {
    const int sub = i / F::RT, t = i - sub * F::RT;
    const uint8_t* ap = tile + aoff + t * 16 * F::RS + sub * 64;
    ah[slot] = *reinterpret_cast<const uint4*>(ap);
    al[slot] = *reinterpret_cast<const uint4*>(ap + 128);
  };
#pragma unroll
  for (int i = 0; i < F::D; ++i) a_issue(smem, i, i);

  // One position.  In flight when it starts (issue order): W(pos) | A(pos + 2) x IT | W(pos + 1) | A(pos + 3) x IT.
  // The chunks of the tile of position + 2 go to LDS and the loads of position + 4 are issued INSIDE the MFMA loop,
  // one 16-byte chunk per fragment pair: as a block after the loop, on all eight waves at once, they left the matrix
  // pipe idle for ~640 of a position's ~2980 cycles (tools/fc_phases.py).  The tile stored during position p lives in
  // the buffer that was last read during p - 1, which every wave left at the previous barrier.
  static_assert(2 * F::IT + 1 <= F::TOT, "a store and a load slot per chunk");
  int buf = 0;  // (pos - p0) % 3
  auto body = [&](int pos, auto set) {
    constexpr int SB = decltype(set)::value;
    u32x4 bcur[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (SB == 0) bcur[q] = bq0[q]; else bcur[q] = bq1[q];
    }
    load_w(pos + 2, set);
    const int nbuf = (buf == F::NBUF - 1) ? 0 : buf + 1;
    const int sbuf = (nbuf == F::NBUF - 1) ? 0 : nbuf + 1;
    const uint8_t* tile = smem + buf * F::TILE;
    const uint8_t* ntile = smem + nbuf * F::TILE;  // (after the last position: stale rows, read and dropped)
    __builtin_amdgcn_sched_barrier(0);
    stamp(0);
#pragma unroll
    for (int i = 0; i < F::TOT; ++i) {
      const int sub = i / F::RT, t = i - sub * F::RT;
      const int slot = i % F::D;
      const bf16x8 bh = __builtin_bit_cast(bf16x8, bcur[sub * 2]);
      const bf16x8 bl = __builtin_bit_cast(bf16x8, bcur[sub * 2 + 1]);
      const bf16x8 xh = __builtin_bit_cast(bf16x8, ah[slot]);
      const bf16x8 xl = __builtin_bit_cast(bf16x8, al[slot]);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, bh, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, bl, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, bh, acc[t], 0, 0, 0);
      if (i + F::D < F::TOT)
        a_issue(tile, i + F::D, slot);
      else
        a_issue(ntile, i + F::D - F::TOT, slot);
      // chunk j of the tile of position pos + 2 (past the end: rewrites a tile nobody reads again) goes to LDS after
      // pair 2 j + 1 and its registers take chunk j of position pos + 4 after pair 2 j + 2
      if ((i & 1) == 1 && i / 2 < F::IT) store_chunk(sbuf, set, i / 2);
      if ((i & 1) == 0 && i >= 2 && i / 2 - 1 < F::IT) load_chunk(pos + 4, set, i / 2 - 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    stamp(1);
    __syncthreads();
    stamp(4);
    stamp_pos += 1;
    buf = nbuf;
  };
  for (int pos = p0; pos < p1; pos += 2) {
    body(pos, Set0{});
    if (pos + 1 < p1) body(pos + 1, Set1{});
  }
  const int col = ct * 16 + li;
  if constexpr (SPLIT) {
    float* part = out + (size_t)sl * N * F::OC;
#pragma unroll
    for (int t = 0; t < F::RT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + t * 16 + g * 4 + r;
        if (row < N) part[(size_t)row * F::OC + col] = acc[t][r];
      }
    return;
  }
  const float bv = bias[col];
#pragma unroll
  for (int t = 0; t < F::RT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + t * 16 + g * 4 + r;
      if (row < N) {
        const float o = acc[t][r] + bv;
        out[(size_t)row * F::OC + col] = o > 0.f ? o : 0.f;
      }
    }
}

// h [N][512] = relu(a3's records x Bff + bf)
inline void launch_fc_bf16s(const uint8_t* a3_records, const uint4* Bff, const float* bf, float* h, int N, hipStream_t s) {
  note_launch("fc_bf16s");
  hipLaunchKernelGGL(fc_bf16s<FcFast>, fc_grid_xcd(ceil_div(N, FcFast::BM), 1), dim3(kThreads), FcFast::LDS_BYTES, s,
                     a3_records, Bff, bf, h, N, 0);
}
// ... the contraction split over slices of positions so that ~256 blocks run (fc_bf16_slices, ffnet_plan.h), timed as
// `label`, then fc_reduce; a3 STAYS in records
inline void launch_fc_bf16_splitk(const uint8_t* a3_records, const uint4* Bff, const float* bf, float* part, float* h, int N,
                                  const char* label, hipStream_t s) {
  int per = 0;
  const int slices = fc_bf16_slices(N, &per);
  {
    ProfScope prof(label, s);
    note_launch("fc_bf16s (split-K)");
    hipLaunchKernelGGL((fc_bf16s<FcFast, true>), fc_grid_xcd(ceil_div(N, FcFast::BM), slices), dim3(kThreads),
                       FcFast::LDS_BYTES, s, a3_records, Bff, bf, part, N, per);
  }
  launch_fc_reduce(part, slices, N, bf, h, s);
}
// rela_ffnet_debug_fc_stamps: the diagnostic variant opts in on its first use
inline hipError_t opt_in_fc_bf16s_stamps() {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&fc_bf16s<FcFast, false, true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, FcFast::LDS_BYTES);
  return attr;
}
inline void launch_fc_bf16s_stamps(const uint8_t* a3_records, const uint4* Bff, const float* bf, float* h, int N,
                                   unsigned long long* stamps, hipStream_t s) {
  hipLaunchKernelGGL((fc_bf16s<FcFast, false, true>), fc_grid_xcd(ceil_div(N, FcFast::BM), 1), dim3(kThreads),
                     FcFast::LDS_BYTES, s, a3_records, Bff, bf, h, N, 0, stamps);
}
inline int opt_in_lds_fc_bf16s() {
  const LdsOptIn ks[] = {{reinterpret_cast<const void*>(&fc_bf16s<FcFast, true>), FcFast::LDS_BYTES},
                         {reinterpret_cast<const void*>(&fc_bf16s<FcFast>), FcFast::LDS_BYTES}};
  return opt_in(ks);
}

}  // namespace
}  // namespace rela_amd
