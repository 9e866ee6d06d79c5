// wgrad_conv3_x3.h -- conv3's weight gradient on the bf16 matrix cores with THREE-part operands, f32 accuracy.
// Option `wgrad3_x3` of the learners (learner_plan.h); without it the f32-accurate modes run this contraction through the
// split-K GEMM (gemm_bf16x3.h, PARTS = 3) with an im2col gather and the operand splits inside its k-loop.
//
//   dW3[oc][c][kh][kw] = sum_{b, oy, ox} d_a3[b][oy][ox][oc] * a2[b][oy + kh][ox + kw][c]             (3 x 3, stride 1)
//
// The construction is wgrad_conv3_bf16.h's (read that first): the contraction runs over pixels, k = 16 oy + ox' with
// 7 rows = 112 -> 128 = 4 k-steps, the row tap kh is an address offset of the image operand (rows 32 B apart) and the
// column tap kw one of three copies of the gradient operand, shifted by 0, 1 and 2 pixels.  Every f32 operand is split
// exactly into hi + mid + lo bf16 (gemm3::split4x3) and the six products with i + j <= 2 are taken, hi x hi alone in the main
// accumulator and the five small ones in a second, added once at the store (the rule of gemm_bf16x3.h and
// wgrad_conv_x3.h).  One persistent block of 512 threads per CU, frames strided over the blocks, one partial tile
// part[block][oc][(kh * 3 + kw) * 64 + c] per block for reduce_splits (kRedConv3); the number of blocks is the plan's
// (plan_wgrad3_x3_blocks).  Every output element is owned by one wave and no block waits for another: the same inputs
// and the same block count give the same bits on every run.
//
// Output-channel halves.  Three parts of the two-part kernel's layout would be 230,400 B, so the three shifted copies of
// d^T hold 32 output channels at a time beside the whole three-part image, and a frame runs in two passes H = 0, 1:
//   LDS: image [part 3][c 64][10 rows][16] bf16 (336 B apart) 64,512 B | d^T [kw 3][part 3][oc 32][128 k] bf16 (rows
//        272 B apart: 16 lanes' 16-byte reads fall on different banks) 78,336 B: 142,848 B.  Row 9 and columns 9 .. 15 of the image, row 7 and the columns beside the
//        shifted gradient of d^T are read and never written: the zero fill at the start of the launch.
//   Work: wave w owns the 16 input channels cg = w & 3 and the 16 output channels 32 H + 16 (w >> 2) .. + 15 of either
//        pass with all nine taps: 2 x 9 main + 2 x 9 small accumulator tiles = 144 registers.  Per k-step 9 image
//        fragments (kh x part) stay in registers, 9 gradient fragments pass through three at a time: 54 MFMAs, three
//        independent accumulator chains (one per kh) interleaved; 432 MFMAs per wave and frame.
//   Staging: a thread holds one row of one channel, so that what it stores is contiguous along k.  Image: thread
//        (row y = tid >> 6 of 0 .. 7, channel tid & 63) loads nine f32 and stores, per part, the row's first eight
//        pixels as ONE 16-byte store and the ninth as a 2-byte store; row 8 goes one pixel per thread.  d^T: thread
//        (oy = tid >> 5 of 0 .. 6, oc tid & 31; 224 threads) loads seven f32 and stores, per part and copy, one 16-byte
//        store -- the shift by kw pixels is made in registers on the packed pairs -- and for kw = 2 the ninth position as a
//        4-byte store.  39 stores per thread and frame at most (the two-part kernel: 88 two-byte ones).
//   Loads under the MFMAs: the next frame's image row is loaded before the first pass and stored after the second; the
//        gradient rows of half 1 are loaded before the first pass, those of the next frame's half 0 before the second.
//        Four barriers per frame (each pass: tiles written | fragments read).
// No scratch, no spills, two waves per SIMD (tests/test_wgrad3_x3_plan_host.py asserts the first two;
// profiles/wgrad3_x3_ab.md has the figures and the budget of the design that was not built).
#pragma once
#include "prof.h"
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"
#include "gemm_bf16x3.h"

namespace rela_amd {
namespace wg3x3 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kT = 512;
constexpr int kMaxBlocks = 256;
constexpr int SUB = 336;                         // bytes per channel image: 10 rows x 16 el x 2 B + 16
constexpr int IMG_PART = 64 * SUB;               // one part: 21,504
constexpr int IMG_BYTES = 3 * IMG_PART;          // 64,512
constexpr int DT_PITCH = 272;                    // bytes per (copy, part, oc) row: 128 k x 2 B + 16
constexpr int DT_PART = 32 * DT_PITCH;           // one part of one copy: 8,704
constexpr int DT_BYTES = 9 * DT_PART;            // [kw][part][32 oc] = 78,336
constexpr int LDS_TOTAL = IMG_BYTES + DT_BYTES;  // 142,848
static_assert(LDS_TOTAL == 142848 && LDS_TOTAL <= 160 * 1024, "LDS budget");
constexpr int kDThreads = 7 * 32;  // the threads that stage d^T: (oy, oc of the half)

__device__ __forceinline__ bf16x8 frag(const uint8_t* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p)); }
// the packed pair one bf16 further along k: the upper element of `lo` below the lower element of `hi`
__device__ __forceinline__ uint32_t shift1(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbit(hi, lo, 16); }

__global__ __launch_bounds__(kT) void wgrad_conv3_x3(const float* __restrict__ a2, const float* __restrict__ d_a3, int frames,
                                                     float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* img = smem;
  uint8_t* dt = smem + IMG_BYTES;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int cg = wave & 3, mt = wave >> 2;

  for (int i = tid; i < LDS_TOTAL / 16; i += kT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  f32x4 acc[2][9], accs[2][9];  // [pass H][kh * 3 + kw]: hi x hi | the five small products
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 9; ++n) acc[m][n] = accs[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- staging registers: one image row of one channel (and a pixel or two of row 8), one gradient row of one oc ----
  float av[9], aw0, aw1 = 0.f, dv[7];
  const int ac = tid & 63, ay = tid >> 6;  // (ay is the wave: row 8's ninth pixel is wave 0's)
  const int dc = tid & 31, dy = tid >> 5;
  const bool d_thread = tid < kDThreads;
#pragma unroll
  for (int x = 0; x < 7; ++x) dv[x] = 0.f;
  auto load_a = [&](int f) {
    const float* fa = a2 + (size_t)f * (81 * 64) + ac;
#pragma unroll
    for (int x = 0; x < 9; ++x) av[x] = fa[(ay * 9 + x) * 64];
    aw0 = fa[(72 + ay) * 64];
    if (wave == 0) aw1 = fa[80 * 64];
  };
  auto load_d = [&](int f, int H) {
    if (d_thread) {
      const float* fd = d_a3 + (size_t)f * (49 * 64) + H * 32 + dc;
#pragma unroll
      for (int x = 0; x < 7; ++x) dv[x] = fd[(dy * 7 + x) * 64];
    }
  };
  auto put_a = [&]() {
    uint2 p0[3], p1[3], p2[3];
    gemm3::split4x3(make_float4(av[0], av[1], av[2], av[3]), p0[0], p0[1], p0[2]);
    gemm3::split4x3(make_float4(av[4], av[5], av[6], av[7]), p1[0], p1[1], p1[2]);
    gemm3::split4x3(make_float4(av[8], aw0, aw1, 0.f), p2[0], p2[1], p2[2]);
    uint8_t* ch = img + ac * SUB;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      uint8_t* c = ch + k * IMG_PART;
      *reinterpret_cast<uint4*>(c + ay * 32) = make_uint4(p0[k].x, p0[k].y, p1[k].x, p1[k].y);
      *reinterpret_cast<uint16_t*>(c + ay * 32 + 16) = (uint16_t)(p2[k].x & 0xffffu);
      *reinterpret_cast<uint16_t*>(c + 8 * 32 + ay * 2) = (uint16_t)(p2[k].x >> 16);
      if (wave == 0) *reinterpret_cast<uint16_t*>(c + 8 * 32 + 16) = (uint16_t)(p2[k].y & 0xffffu);
    }
  };
  auto put_d = [&]() {
    if (d_thread) {
      uint2 p0[3], p1[3];
      gemm3::split4x3(make_float4(dv[0], dv[1], dv[2], dv[3]), p0[0], p0[1], p0[2]);
      gemm3::split4x3(make_float4(dv[4], dv[5], dv[6], 0.f), p1[0], p1[1], p1[2]);
      uint8_t* row = dt + dc * DT_PITCH + dy * 32;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t w0 = p0[k].x, w1 = p0[k].y, w2 = p1[k].x, w3 = p1[k].y;  // (w3's upper element is the split of 0: 0)
        uint8_t* r = row + k * DT_PART;
        *reinterpret_cast<uint4*>(r) = make_uint4(w0, w1, w2, w3);                                                    // kw = 0
        *reinterpret_cast<uint4*>(r + 3 * DT_PART) = make_uint4(w0 << 16, shift1(w1, w0), shift1(w2, w1), shift1(w3, w2));  // 1
        *reinterpret_cast<uint4*>(r + 6 * DT_PART) = make_uint4(0u, w0, w1, w2);                                      // kw = 2
        *reinterpret_cast<uint32_t*>(r + 6 * DT_PART + 16) = w3;
      }
    }
  };

  const int b_base = (cg * 16 + li) * SUB;
  const int a_base = (mt * 16 + li) * DT_PITCH;
  // the MFMAs of one pass into accumulator slot H: the image x the staged oc half over the four k-steps
  auto mma = [&](auto slot) {
    constexpr int H = decltype(slot)::value;
    // (d part, image part) with i + j <= 2, smallest first, into accs; hi x hi alone into acc
    constexpr int PA[5] = {2, 0, 1, 1, 0}, PB[5] = {0, 2, 1, 0, 1};
    // (not unrolled: the fragments of two k-steps at once do not fit beside 144 accumulator registers)
#pragma unroll 1
    for (int ks = 0; ks < 4; ++ks) {
      // k-group of 8 G = 4 ks + g: row G >> 1 = 2 ks + (g >> 1), columns 8 (G & 1) ..: both offsets advance by 64 B a step
      const int bo = b_base + (g >> 1) * 32 + (g & 1) * 16 + ks * 64;
      const int ao = a_base + g * 16 + ks * 64;
      bf16x8 bf[3][3];  // [kh][part]
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int k = 0; k < 3; ++k) bf[kh][k] = frag(img + k * IMG_PART + bo + kh * 32);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        bf16x8 af[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) af[k] = frag(dt + (kw * 3 + k) * DT_PART + ao);
#pragma unroll
        for (int t = 0; t < 5; ++t)
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
            accs[H][kh * 3 + kw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[PA[t]], bf[kh][PB[t]], accs[H][kh * 3 + kw], 0, 0, 0);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
          acc[H][kh * 3 + kw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0], bf[kh][0], acc[H][kh * 3 + kw], 0, 0, 0);
      }
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;

  int f = blockIdx.x;  // (blocks <= frames: f is a frame)
  load_a(f), load_d(f, 0);
  __syncthreads();  // zero fill done
  for (; f < frames; f += gridDim.x) {
    const int fn = (f + (int)gridDim.x < frames) ? f + (int)gridDim.x : f;  // (the last round re-reads its own frame)
    put_a(), put_d();
    load_d(f, 1), load_a(fn);
    __syncthreads();
    mma(S0{});
    __syncthreads();  // d^T read: the other half may overwrite it
    put_d();
    load_d(fn, 0);
    __syncthreads();
    mma(S1{});
    __syncthreads();  // tiles read: the next frame may overwrite them
  }
  // every wave owns its elements: straight to this block's partial tile
  float* out = part + (size_t)blockIdx.x * (64 * 576);
#pragma unroll
  for (int H = 0; H < 2; ++H)
#pragma unroll
    for (int n = 0; n < 9; ++n)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        out[(size_t)(H * 32 + mt * 16 + 4 * g + rr) * 576 + n * 64 + cg * 16 + li] = acc[H][n][rr] + accs[H][n][rr];
}

inline int launch(const float* a2, const float* d_a3, int frames, float* part, int blocks, hipStream_t s) {
  // (initialised once, thread-safely: launches may come from several host threads)
  static const hipError_t attr_set =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_conv3_x3), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TOTAL);
  RELA_HIP(attr_set);
  RELA_CHECK(blocks >= 1 && blocks <= kMaxBlocks && blocks <= frames, RELA_EINVAL, "wgrad_conv3_x3: %d blocks for %d frames",
             blocks, frames);
  note_launch("wgrad_conv3_x3");
  hipLaunchKernelGGL(wgrad_conv3_x3, dim3(blocks), dim3(kT), LDS_TOTAL, s, a2, d_a3, frames, part);
  return RELA_OK;
}

}  // namespace
}  // namespace wg3x3
}  // namespace rela_amd
