// dgrad_conv_x3.h -- the conv2 / conv3 data gradients of dgrad_conv_bf16.h (same mathematics, same buffers: read its
// head) with THREE-part bf16 operands: f32 accuracy on the bf16 matrix cores, for the f32-accurate learner modes whose
// data gradients otherwise run as f32 GEMMs (gemm_lds.h).  Option `dgrad_x3` of the learners (learner_plan.h).
//
// Arithmetic: every f32 gradient and weight is split exactly into hi + mid + lo bf16 (gemm3::split4x3); of the nine part
// products the six with part indices i + j <= 2 are multiplied on v_mfma_f32_16x16x32_bf16: hi x hi into an accumulator of
// its own, the five small ones (lo x hi, hi x lo, mid x mid, mid x hi, hi x mid, smallest first) into a second one, the two
// added once in the epilogue, as gemm_bf16x3.h does with PARTS = 3.  Nothing is reduced across blocks: the bits do not
// depend on the grid.
//
// Kept from dgrad_conv_bf16.h: one persistent block per CU over min(frames, 256) blocks, the frame's gradient as split
// records in LDS, double buffered (the next frame's loads wait in registers during the MFMAs), one barrier per frame, a
// tap is a record offset, A fragments three steps ahead in a register ring, the ReLU mask rows loaded before the MFMA
// loop, the weights as the first MFMA operand so that a lane's four results are one 16-byte masked store.
//
// New here:
//  * Record = hi | mid | lo (3 x 128 B) + 32 B pad = 416 B.  A fragment read is one ds_read_b128 per part by 16 lanes
//    (records) x 4 groups (16 B apart).  416 mod 256 = 160 = 5 x 32 with 5 odd, so eight consecutive records start at the
//    eight different multiples of 32 B of the 256 B bank row and two lane groups fill the 16 B halves: the rule by which
//    REC = 288 (9 x 32) was chosen there.  Checked by enumerating on the host, for every (pixel tile, tap) of both
//    kernels, the most distinct addresses any of the 64 banks sees within a 16-lane quarter of the read, in both plausible
//    groupings of a quarter ({8 records} x {2 groups}, {16 records} x {1 group}): 416 gives exactly the figures of 288 in
//    the same padded grid (worst 2 / mean 1.7 and worst 3 / mean 2.6 -- the excess over 1 and 2 comes from the two records
//    a pixel row skips at its end, not from the stride), 384 (no pad) gives 4 / 3.7 and 8 / 7.1.
//  * The tile is the gradient ZERO-PADDED to 11 x 11 records (conv2: one ring around 9 x 9, conv3: two around 7 x 7), not
//    81 / 49 records + one zero record: an out-of-range tap lands in the border, so a lane's tap address is ONE base per
//    pixel tile plus a compile-time constant, instead of a table of tiles x taps offsets (28 / 54 registers, which the
//    third part's fragments need).  2 x 121 x 416 B = 100,672 B of LDS for either kernel.
//  * conv2: wave = (parity class, channel tile) as before, its 8 k-steps x 3 parts = 24 weight fragments (96 VGPRs) in
//    registers, two waves per SIMD.
//  * conv3: 54 fragments per channel tile (216 VGPRs).  256-thread blocks, ONE wave per SIMD with the 512-register budget:
//    wave = channel tile, all 54 fragments in registers for the whole launch, all six pixel tiles of the frame per wave.
//    No weight traffic at all inside the frame loop and no LDS for weights.  Weighed on paper and not built: hi + mid in
//    registers with lo in LDS at two waves per SIMD needs 144 fragment + 48 accumulator / mask + 36 ring registers before
//    any address, over 256 (conv2 with 96 fragment registers already needed two passes to fit), and 72 KB of LDS beside
//    100 KB of padded tiles; lo streamed from L2 adds 72 KB of reads per frame and CU to the MFMA loop.
//    profiles/dgrad_x3_ab.md has the figures.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"
#include "gemm_bf16x3.h"
#include "prof.h"

namespace rela_amd {
namespace dgx3 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int REC = 416;                   // LDS bytes per pixel record: hi | mid | lo (128 B each) | 32 pad
constexpr int GW = 11;                     // the padded gradient grid is GW x GW records
constexpr int TILE = GW * GW * REC;        // 50,336 B
constexpr int LDS = 2 * TILE;              // double buffered
constexpr int kBlocks = 256;               // persistent blocks: one per CU
static_assert(REC % 16 == 0 && (REC % 256) % 64 == 32, "record stride: 16-byte aligned, an odd multiple of 32 B mod 256");
static_assert(LDS <= 160 * 1024, "LDS of a CU");

// ---- weight fragments (MFMA 16x16x32 operand order, parts hi / mid / lo): 8 bf16 per lane, k-step and part ----
// the k-steps, lanes and elements are those of pack_dgrad{2,3}_frags (dgrad_conv_bf16.h); [part 3] where that has [hl 2]
__device__ __forceinline__ void store_parts(const float (&v)[8], uint4* dst) {
  uint2 h0, m0, l0, h1, m1, l1;
  gemm3::split4x3(make_float4(v[0], v[1], v[2], v[3]), h0, m0, l0);
  gemm3::split4x3(make_float4(v[4], v[5], v[6], v[7]), h1, m1, l1);
  dst[0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
  dst[64] = make_uint4(m0.x, m0.y, m1.x, m1.y);
  dst[128] = make_uint4(l0.x, l0.y, l1.x, l1.y);
}
// conv2: frag[cls 4][nt 2][ks 8][part 3][lane 64] from w2p[oc][(kh * 4 + kw) * 32 + c]
__global__ void pack_dgrad2_x3_frags(const float* __restrict__ w2p, uint4* __restrict__ frag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (cls, nt, ks, lane)
  if (idx >= 4 * 2 * 8 * 64) return;
  const int lane = idx & 63, ks = (idx >> 6) & 7, nt = (idx >> 9) & 1, cls = idx >> 10;
  const int li = lane & 15, g = lane >> 4;
  const int s = cls >> 1, r = cls & 1, tap = ks >> 1, p = tap >> 1, q = tap & 1;
  const int kh = 2 * p + s, kw = 2 * q + r, c = 16 * nt + li;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = w2p[(size_t)(32 * (ks & 1) + 8 * g + j) * 512 + (kh * 4 + kw) * 32 + c];
  store_parts(v, frag + ((size_t)((cls * 2 + nt) * 8 + ks) * 3) * 64 + lane);
}
// conv3: frag[nt 4][ks 18][part 3][lane 64] from w3p[oc][(kh * 3 + kw) * 64 + c]
__global__ void pack_dgrad3_x3_frags(const float* __restrict__ w3p, uint4* __restrict__ frag) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (nt, ks, lane)
  if (idx >= 4 * 18 * 64) return;
  const int lane = idx & 63, ks = (idx >> 6) % 18, nt = (idx >> 6) / 18;
  const int li = lane & 15, g = lane >> 4;
  const int tap = ks >> 1, c = 16 * nt + li;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = w3p[(size_t)(32 * (ks & 1) + 8 * g + j) * 576 + tap * 64 + c];
  store_parts(v, frag + ((size_t)(nt * 18 + ks) * 3) * 64 + lane);
}

// float4 number i of a frame's gradient ([pixel][64 channels], W pixels per row) -> its three parts in the padded tile,
// whose interior starts PAD records in from the border
template <int W, int PAD>
__device__ __forceinline__ void put(uint8_t* tile, int i, float4 v) {
  uint2 hi, mid, lo;
  gemm3::split4x3(v, hi, mid, lo);
  const int px = i >> 4, oy = px / W, ox = px - oy * W;
  uint8_t* rec = tile + ((oy + PAD) * GW + ox + PAD) * REC + (i & 15) * 8;
  *reinterpret_cast<uint2*>(rec) = hi;
  *reinterpret_cast<uint2*>(rec + 128) = mid;
  *reinterpret_cast<uint2*>(rec + 256) = lo;
}

// the six products of one k-step: w[part] (weights, first operand) x the three parts of one A fragment (gradient)
__device__ __forceinline__ void mfma6(const bf16x8& w0, const bf16x8& w1, const bf16x8& w2, const uint4& p0, const uint4& p1,
                                      const uint4& p2, f32x4& hi, f32x4& small) {
  const bf16x8 a0 = __builtin_bit_cast(bf16x8, p0), a1 = __builtin_bit_cast(bf16x8, p1), a2 = __builtin_bit_cast(bf16x8, p2);
  small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, a0, small, 0, 0, 0);
  small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, a2, small, 0, 0, 0);
  small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, a1, small, 0, 0, 0);
  small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, a0, small, 0, 0, 0);
  small = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, a1, small, 0, 0, 0);
  hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, a0, hi, 0, 0, 0);
}

// ---- conv2: 512 threads, wave = (parity class, channel tile), 7 tiles of 16 output pixels (100 of 112) ----
struct X2 {
  static constexpr int kT = 512, QUADS = 81 * 16, MT = 7, KS = 8;
  static constexpr size_t kFragBytes = (size_t)4 * 2 * KS * 3 * 64 * 16;
};
#define DGX3_KERNEL __global__
DGX3_KERNEL __launch_bounds__(X2::kT) void dgrad_conv2_x3(const float* __restrict__ d_a2, const uint4* __restrict__ frag,
                                                         const float* __restrict__ a1, float* __restrict__ d_a1,
                                                         int frames) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int kT = X2::kT, MT = X2::MT, KS = X2::KS;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int cls = wave >> 1, nt = wave & 1;
  const int s = cls >> 1, r = cls & 1;
  for (int i = tid; i < LDS / 16; i += kT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  bf16x8 w[KS][3];
  {
    const uint4* fp = frag + (size_t)((cls * 2 + nt) * KS) * 3 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int pt = 0; pt < 3; ++pt) w[ks][pt] = __builtin_bit_cast(bf16x8, fp[(size_t)(ks * 3 + pt) * 64]);
  }
  // output pixel m = 16 mt + li = 10 u + v of the class; tap (p, q) reads gradient pixel (u - p, v - q), record
  // (u - p + 1, v - q + 1) of the padded grid = base + ((1 - p) * GW + (1 - q)) records (pixels past 99: those of 99)
  int base[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = min(mt * 16 + li, 99), u = m / 10, v = m - u * 10;
    base[mt] = (u * GW + v) * REC + g * 16;
  }
  float4 x0, x1, x2;
#define DGX2_I(J) min(tid + (J) * kT, X2::QUADS - 1)
#define DGX2_LOAD(F)                                                    \
  do {                                                                  \
    const float* fd__ = d_a2 + (size_t)(F) * (81 * 64);                 \
    x0 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX2_I(0) * 4); \
    x1 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX2_I(1) * 4); \
    x2 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX2_I(2) * 4); \
  } while (0)
#define DGX2_PUT(T) (put<9, 1>(T, DGX2_I(0), x0), put<9, 1>(T, DGX2_I(1), x1), put<9, 1>(T, DGX2_I(2), x2))
  int f = blockIdx.x;
  DGX2_LOAD(f);     // (blocks <= frames)
  __syncthreads();  // zero fill done
  DGX2_PUT(smem);
  {
    const int fn = (f + (int)gridDim.x < frames) ? f + (int)gridDim.x : f;
    DGX2_LOAD(fn);
  }
  __syncthreads();
  int buf = 0;
  for (; f < frames; f += gridDim.x) {
    const uint8_t* tile = smem + buf * TILE;
    // The seven pixel tiles in two passes (tiles 0..3, then 4..6) over the resident weights: two accumulators and a mask
    // row per tile are 12 registers, and with seven tiles live beside the 96 of the weights the kernel does not fit the
    // 256 registers of two waves per SIMD.  A pass: mask rows, MFMAs, masked stores.
    auto pass = [&](auto mt0_, auto nmt_) {
      constexpr int MT0 = decltype(mt0_)::value, NMT = decltype(nmt_)::value;
      f32x4 am[NMT];  // the ReLU mask rows of the pass's outputs, issued before its MFMAs
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt) {
        const int m = min((MT0 + mt) * 16 + li, 99), u = m / 10, v = m - u * 10;
        am[mt] = *reinterpret_cast<const f32x4*>(a1 + ((size_t)f * 400 + (2 * u + s) * 20 + (2 * v + r)) * 32 + 16 * nt + 4 * g);
      }
      __builtin_amdgcn_sched_barrier(0);
      f32x4 acc[NMT], acs[NMT];  // hi x hi | the five small products
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt) acc[mt] = acs[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      {
        constexpr int TOT = KS * NMT, D = 3;  // A fragments D (k-step, tile) pairs ahead of their MFMAs
        uint4 r0[D], r1[D], r2[D];            // the ring: hi, mid, lo of one fragment per slot
        auto a_issue = [&](int idx, int slot) {
          const int ks = idx / NMT, mt = idx - ks * NMT, tap = ks >> 1;
          const uint8_t* ap = tile + base[MT0 + mt] + ((1 - (tap >> 1)) * GW + (1 - (tap & 1))) * REC + (ks & 1) * 64;
          r0[slot] = *reinterpret_cast<const uint4*>(ap);
          r1[slot] = *reinterpret_cast<const uint4*>(ap + 128);
          r2[slot] = *reinterpret_cast<const uint4*>(ap + 256);
        };
#pragma unroll
        for (int i = 0; i < D; ++i) a_issue(i, i);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int idx = 0; idx < TOT; ++idx) {
          const int ks = idx / NMT, mt = idx - ks * NMT, slot = idx % D;
          mfma6(w[ks][0], w[ks][1], w[ks][2], r0[slot], r1[slot], r2[slot], acc[mt], acs[mt]);
          if (idx + D < TOT) a_issue(idx + D, slot);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // lane: channels 16 nt + 4 g .. + 3 of output pixel m = 16 mt + li -> (y, x) = (2 u + s, 2 v + r)
#pragma unroll
      for (int mt = 0; mt < NMT; ++mt) {
        const int m = (MT0 + mt) * 16 + li;
        if (m < 100) {
          const int u = m / 10, v = m - u * 10;
          const size_t o = ((size_t)f * 400 + (2 * u + s) * 20 + (2 * v + r)) * 32 + 16 * nt + 4 * g;
          f32x4 d;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) d[rr] = am[mt][rr] > 0.f ? acc[mt][rr] + acs[mt][rr] : 0.f;
          *reinterpret_cast<f32x4*>(d_a1 + o) = d;
        }
      }
    };
    pass(std::integral_constant<int, 0>(), std::integral_constant<int, 4>());
    __builtin_amdgcn_sched_barrier(0);
    pass(std::integral_constant<int, 4>(), std::integral_constant<int, MT - 4>());
    // the next frame's records go into the other buffer (last read two frames ago: every wave is past that barrier)
    uint8_t* ntile = smem + (buf ^ 1) * TILE;
    DGX2_PUT(ntile);
    {
      const int f2 = f + 2 * (int)gridDim.x;
      DGX2_LOAD(f2 < frames ? f2 : f);
    }
    __syncthreads();
    buf ^= 1;
  }
#undef DGX2_PUT
#undef DGX2_LOAD
#undef DGX2_I
}

// ---- conv3: 256 threads, one wave per SIMD, wave = channel tile, 6 tiles of 16 output pixels (81 of 96) ----
struct X3 {
  static constexpr int kT = 256, QUADS = 49 * 16, MT = 6, KS = 18;
  static constexpr size_t kFragBytes = (size_t)4 * KS * 3 * 64 * 16;
};
DGX3_KERNEL __launch_bounds__(X3::kT) void dgrad_conv3_x3(const float* __restrict__ d_a3, const uint4* __restrict__ frag,
                                                         const float* __restrict__ a2, float* __restrict__ d_a2,
                                                         int frames) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int kT = X3::kT, MT = X3::MT, KS = X3::KS;
  const int tid = threadIdx.x;
  const int nt = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  for (int i = tid; i < LDS / 16; i += kT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  bf16x8 w[KS][3];  // 216 registers: the whole channel tile, for the whole launch
  {
    const uint4* fp = frag + (size_t)(nt * KS) * 3 * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int pt = 0; pt < 3; ++pt) w[ks][pt] = __builtin_bit_cast(bf16x8, fp[(size_t)(ks * 3 + pt) * 64]);
  }
  // output pixel m = 16 mt + li = 9 y + x; tap (kh, kw) reads gradient pixel (y - kh, x - kw), record
  // (y - kh + 2, x - kw + 2) of the padded grid = base + ((2 - kh) * GW + (2 - kw)) records (pixels past 80: those of 80)
  int base[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = min(mt * 16 + li, 80), y = m / 9, x = m - y * 9;
    base[mt] = (y * GW + x) * REC + g * 16;
  }
  float4 x0, x1, x2, x3;
#define DGX3_I(J) min(tid + (J) * kT, X3::QUADS - 1)
#define DGX3_LOAD(F)                                                    \
  do {                                                                  \
    const float* fd__ = d_a3 + (size_t)(F) * (49 * 64);                 \
    x0 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX3_I(0) * 4); \
    x1 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX3_I(1) * 4); \
    x2 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX3_I(2) * 4); \
    x3 = *reinterpret_cast<const float4*>(fd__ + (size_t)DGX3_I(3) * 4); \
  } while (0)
#define DGX3_PUT(T) \
  (put<7, 2>(T, DGX3_I(0), x0), put<7, 2>(T, DGX3_I(1), x1), put<7, 2>(T, DGX3_I(2), x2), put<7, 2>(T, DGX3_I(3), x3))
  int f = blockIdx.x;
  DGX3_LOAD(f);     // (blocks <= frames)
  __syncthreads();  // zero fill done
  DGX3_PUT(smem);
  {
    const int fn = (f + (int)gridDim.x < frames) ? f + (int)gridDim.x : f;
    DGX3_LOAD(fn);
  }
  __syncthreads();
  int buf = 0;
  for (; f < frames; f += gridDim.x) {
    const uint8_t* tile = smem + buf * TILE;
    f32x4 am[MT];  // ReLU mask rows, issued before the MFMAs
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = min(mt * 16 + li, 80);
      am[mt] = *reinterpret_cast<const f32x4*>(a2 + ((size_t)f * 81 + m) * 64 + 16 * nt + 4 * g);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[MT], acs[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = acs[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      constexpr int TOT = KS * MT, D = 3;
      uint4 r0[D], r1[D], r2[D];  // the ring: hi, mid, lo of one fragment per slot
      auto a_issue = [&](int idx, int slot) {
        const int ks = idx / MT, mt = idx - ks * MT, tap = ks >> 1;
        const uint8_t* ap = tile + base[mt] + ((2 - tap / 3) * GW + (2 - tap % 3)) * REC + (ks & 1) * 64;
        r0[slot] = *reinterpret_cast<const uint4*>(ap);
        r1[slot] = *reinterpret_cast<const uint4*>(ap + 128);
        r2[slot] = *reinterpret_cast<const uint4*>(ap + 256);
      };
#pragma unroll
      for (int i = 0; i < D; ++i) a_issue(i, i);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int idx = 0; idx < TOT; ++idx) {
        const int ks = idx / MT, mt = idx - ks * MT, slot = idx % D;
        mfma6(w[ks][0], w[ks][1], w[ks][2], r0[slot], r1[slot], r2[slot], acc[mt], acs[mt]);
        if (idx + D < TOT) a_issue(idx + D, slot);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    uint8_t* ntile = smem + (buf ^ 1) * TILE;
    DGX3_PUT(ntile);
    {
      const int f2 = f + 2 * (int)gridDim.x;
      DGX3_LOAD(f2 < frames ? f2 : f);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mt * 16 + li;
      if (m < 81) {
        const size_t o = ((size_t)f * 81 + m) * 64 + 16 * nt + 4 * g;
        f32x4 d;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) d[rr] = am[mt][rr] > 0.f ? acc[mt][rr] + acs[mt][rr] : 0.f;
        *reinterpret_cast<f32x4*>(d_a2 + o) = d;
      }
    }
    __syncthreads();
    buf ^= 1;
  }
#undef DGX3_PUT
#undef DGX3_LOAD
#undef DGX3_I
}
#undef DGX3_KERNEL

constexpr size_t kFrag2Bytes = X2::kFragBytes, kFrag3Bytes = X3::kFragBytes;

// The weight fragments alone (a caller that keeps them across steps packs them when the weights change and passes them
// as `frags` below)
inline void pack_frags(const float* w2p, const float* w3p, void* frag2, void* frag3, hipStream_t s) {
  hipLaunchKernelGGL(pack_dgrad2_x3_frags, dim3(ceil_div(4 * 2 * 8 * 64, 256)), dim3(256), 0, s, w2p, (uint4*)frag2);
  hipLaunchKernelGGL(pack_dgrad3_x3_frags, dim3(ceil_div(4 * 18 * 64, 256)), dim3(256), 0, s, w3p, (uint4*)frag3);
}

// d_a1 = [a1 > 0] * conv2^T(d_a2); `scratch` (>= kFrag2Bytes) receives the weight fragments unless `frags` has them
inline int launch_conv2(const float* d_a2, const float* w2p, const float* a1, float* d_a1, int frames, void* scratch,
                        hipStream_t s, const void* frags = nullptr) {
  // (initialised once, thread-safely: launches may come from several host threads)
  static const hipError_t attr_set =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&dgrad_conv2_x3), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  RELA_HIP(attr_set);
  if (!frags) hipLaunchKernelGGL(pack_dgrad2_x3_frags, dim3(ceil_div(4 * 2 * 8 * 64, 256)), dim3(256), 0, s, w2p, (uint4*)scratch);
  note_launch("dgrad_conv2_x3");
  hipLaunchKernelGGL(dgrad_conv2_x3, dim3(frames < kBlocks ? frames : kBlocks), dim3(X2::kT), LDS, s, d_a2,
                     (const uint4*)(frags ? frags : scratch), a1, d_a1, frames);
  return RELA_OK;
}
// d_a2 = [a2 > 0] * conv3^T(d_a3); `scratch` (>= kFrag3Bytes) as above
inline int launch_conv3(const float* d_a3, const float* w3p, const float* a2, float* d_a2, int frames, void* scratch,
                        hipStream_t s, const void* frags = nullptr) {
  static const hipError_t attr_set =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&dgrad_conv3_x3), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  RELA_HIP(attr_set);
  if (!frags) hipLaunchKernelGGL(pack_dgrad3_x3_frags, dim3(ceil_div(4 * 18 * 64, 256)), dim3(256), 0, s, w3p, (uint4*)scratch);
  note_launch("dgrad_conv3_x3");
  hipLaunchKernelGGL(dgrad_conv3_x3, dim3(frames < kBlocks ? frames : kBlocks), dim3(X3::kT), LDS, s, d_a3,
                     (const uint4*)(frags ? frags : scratch), a2, d_a2, frames);
  return RELA_OK;
}

}  // namespace
}  // namespace dgx3
}  // namespace rela_amd
