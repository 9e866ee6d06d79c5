// wgrad_conv_x3.h -- conv1's and conv2's weight gradients on the bf16 matrix cores with THREE-part operands, f32 accuracy.
// Option `wgrad_x3` of the learners (learner_plan.h); without it the f32-accurate modes run these two contractions through
// the split-K GEMM (gemm_bf16x3.h, PARTS = 3) with an im2col gather and the operand splits inside its k-loop.
//
// Both kernels keep the space-to-depth construction of wgrad_conv1_bf16.h / wgrad_conv2_bf16.h (read those first): the
// contraction runs over pixels, the frame is split into stride x stride sub-images so that the row tap p is an address
// offset of the image operand and the column tap q a second copy of the gradient operand shifted by one pixel; one
// persistent block of 512 threads per CU, frames strided over the blocks, the next frame's raw data in registers during the
// MFMAs; part[block][oc][j] partial tiles for reduce_splits (kRedConv1 with its 1/255, kRedConv2).  Every f32 operand is
// split exactly into hi + mid + lo bf16 (gemm3::split4x3) and the products with i + j <= 2 are taken, hi x hi alone in the
// main accumulator and the small ones in a second, added once at the store (the rule of gemm_bf16x3.h).  Every output
// element is owned by one wave, or folded over waves in a fixed order: the same inputs give the same bits on every run.
// The number of blocks (= partial tiles) is the plan's (plan_wgrad1_x3_blocks / plan_wgrad2_x3_blocks, learner_plan.h).
//
// wgrad_conv1_x3: the u8 frame is exact in ONE bf16 part, so a k-step costs three MFMAs per tile (the two-part kernel:
//   two) and every product is exact.
//   LDS: sub-images as in wgrad_conv1_bf16.h, 37,888 B | d^T [q 2][hi, mid, lo][32 oc][256 k] bf16, rows 544 B apart,
//        104,448 B: 142,336 B.  The final fold's 32 KB live in the d^T area.
//   Work: 32 oc x 256 j is 32 tiles; main + small would be 64 tiles = 256 registers for a wave that owned them all as in
//   the two-part kernel, which two waves per SIMD do not have.  So wave = (k pair kg = wave >> 1, column tap q = wave & 1):
//   two of the half frame's eight k-steps and the 2 x 8 tiles of its q (16 main + 16 small = 128 accumulator registers).
//   Per k-step 6 A fragments (3 parts x 2 m) and 8 B fragments feed 48 MFMAs.  The four kg waves of a tile are folded in
//   kg order at the end of the launch.
//
// wgrad_conv2_x3: both operands in three parts, six products.  Three-part sub-images (3 x 47,104 B) and three-part d^T of
//   32 output channels (67,584 B) do not fit a CU together, so a frame runs in four passes over (input-channel half ch,
//   output-channel half H), in the order (0,0) (0,1) (1,1) (1,0): the sub-images of ONE channel half
//   [hi, mid, lo][s r][16 c][11 rows][16] bf16 = 70,656 B and d^T [q][hi, mid, lo][32 oc][160 k] = 67,584 B, 138,240 B.
//   Each half of the sub-images is staged once per frame, d^T three times (half 0 twice: its eight registers per thread
//   stay live until the fourth pass; a second staging of d is 48 two-byte stores per thread, of a sub-image half the same).
//   Work: in a pass wave = (sub-image sr = wave & 3, m tile wave >> 2 of the staged 32 oc) owns the four (p, q) taps of the
//   staged 16 channels: 4 tiles per pass, 16 main + 16 small tiles = 128 accumulator registers over the four passes, every
//   output element in exactly one wave.  Per k-step 6 A + 6 B fragments feed 24 MFMAs (480 per wave and frame).
//   Registers held during the MFMAs: the second channel half (4 float4), d of both oc halves (4 float4), and from the third
//   pass on the next frame's first channel half; the next frame's second half and d are loaded in the fourth pass.
// Neither kernel uses scratch (tests/test_wgrad_x3_plan_host.py asserts it; profiles/wgrad_x3_ab.md has the figures).
#pragma once
#include "prof.h"
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"
#include "gemm_bf16x3.h"

namespace rela_amd {
namespace wgx3 {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kT = 512;
constexpr int kMaxBlocks = 256;

__device__ __forceinline__ bf16x8 frag(const uint8_t* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(p)); }
#define WGX3_MFMA(A, B, C) C = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, C, 0, 0, 0)
// element t (0..3) of four packed bf16
__device__ __forceinline__ uint16_t bf16_of(const uint2& v, int t) {
  const uint32_t w = t < 2 ? v.x : v.y;
  return (uint16_t)((t & 1) ? (w >> 16) : (w & 0xffffu));
}

// ---------------------------------------------------------------------------------------------------------------- conv1
namespace c1 {
constexpr int SUB = 592;                         // bytes per sub-image: 12 rows x 24 el x 2 B + 16
constexpr int IMG_BYTES = 64 * SUB;              // 37,888
constexpr int DT_PITCH = 544;                    // bytes per (copy, part, oc) row: 256 k x 2 B + 32
constexpr int DT_PART = 32 * DT_PITCH;           // one part of one copy
constexpr int DT_BYTES = 2 * 3 * DT_PART;        // 104,448
constexpr int LDS_TOTAL = IMG_BYTES + DT_BYTES;  // 142,336
static_assert(LDS_TOTAL == 142336 && LDS_TOTAL <= 160 * 1024, "LDS budget");
static_assert(DT_BYTES >= 32 * 256 * 4, "the final fold reuses the d^T area");
}  // namespace c1

__global__ __launch_bounds__(kT) void wgrad_conv1_x3(const uint8_t* __restrict__ obs, const float* __restrict__ d_a1, int frames,
                                                     float* __restrict__ part) {
  using namespace c1;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* img = smem;
  uint8_t* dt = smem + IMG_BYTES;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int kg = wave >> 1, q = wave & 1;

  for (int i = tid; i < LDS_TOTAL / 16; i += kT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  f32x4 acc[2][8], accs[2][8];  // [m tile][(c, p)] of this wave's q: hi products | mid and lo products
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = accs[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging registers of the half frame after the one being multiplied: the cells and numbering of wgrad_conv1_bf16.h
  uint32_t im[2][4];
  float4 d[4];
  int cell_g[2], cell_l[2], d_g[4], d_l[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = min(tid + j * kT, 923);
    const int pl = c / 231, rem = c - pl * 231;
    const int yq = rem / 21, xq = rem - yq * 21;
    cell_g[j] = pl * 7056 + 4 * yq * 84 + 4 * xq;
    cell_l[j] = pl * 16 * SUB + (yq * 24 + xq) * 2;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int di = min(tid + j * kT, 1599);
    const int px = di % 200, oc0 = (di / 200) * 4;
    const int oy = px / 20, ox = px - oy * 20;
    d_g[j] = px * 32 + oc0;
    d_l[j] = oc0 * DT_PITCH + (oy * 24 + ox) * 2;
  }
  auto load = [&](int f, int h) {
    const uint8_t* fo = obs + (size_t)f * 28224 + h * (40 * 84);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) im[j][r] = *reinterpret_cast<const uint32_t*>(fo + cell_g[j] + r * 84);
    const float* fd = d_a1 + ((size_t)f * 400 + h * 200) * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = *reinterpret_cast<const float4*>(fd + d_g[j]);
  };
  auto put_img = [&](int j) {
    uint8_t* base = img + cell_l[j];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = (float)((im[j][r] >> (8 * c)) & 0xffu);  // exact in bf16: its bits are the float's upper half
        *reinterpret_cast<uint16_t*>(base + (r * 4 + c) * SUB) = (uint16_t)(__float_as_uint(v) >> 16);
      }
  };
  auto put_d = [&](int j) {
    uint2 pt[3];
    gemm3::split4x3(d[j], pt[0], pt[1], pt[2]);
    uint8_t* r0 = dt + d_l[j];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint16_t v = bf16_of(pt[k], t);
        *reinterpret_cast<uint16_t*>(r0 + t * DT_PITCH + k * DT_PART) = v;                // q = 0
        *reinterpret_cast<uint16_t*>(r0 + t * DT_PITCH + (3 + k) * DT_PART + 2) = v;      // q = 1: shifted by one pixel
      }
  };

  // fragment addresses of this wave's two k-steps ks = 2 kg + t (k = 32 ks + 8 g .. + 7)
  int a_off[2], b_off[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ks = 2 * kg + t, G = ks * 4 + g;
    const int oyr = G / 3, ox0 = (G - oyr * 3) * 8;
    a_off[t] = q * 3 * DT_PART + li * DT_PITCH + (32 * ks + 8 * g) * 2;
    b_off[t] = li * SUB + (oyr * 24 + ox0) * 2;
  }

  int f = blockIdx.x;  // (blocks <= frames: f is a frame)
  load(f, 0);
  __syncthreads();  // zero fill done
  for (; f < frames; f += gridDim.x) {
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      put_img(0), put_img(1);
      put_d(0), put_d(1), put_d(2), put_d(3);
      {  // the half after this one (the last one re-reads itself)
        const bool more = f + (int)gridDim.x < frames;
        load(h == 0 ? f : (more ? f + (int)gridDim.x : f), h == 0 ? 1 : (more ? 0 : 1));
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bf16x8 af[3][2];  // [part][m tile]
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int m = 0; m < 2; ++m) af[k][m] = frag(dt + k * DT_PART + m * 16 * DT_PITCH + a_off[t]);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const bf16x8 bf = frag(img + c * 16 * SUB + p * 48 + b_off[t]);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              WGX3_MFMA(af[2][m], bf, accs[m][c * 2 + p]);
              WGX3_MFMA(af[1][m], bf, accs[m][c * 2 + p]);
              WGX3_MFMA(af[0][m], bf, acc[m][c * 2 + p]);
            }
          }
      }
      __syncthreads();  // fragments read: the tiles may be overwritten
    }
  }
  // ---- fold the four k pairs in kg order (the two q waves of a pair write different columns), one coalesced store ----
  float* red = reinterpret_cast<float*>(dt);
  for (int w = 0; w < 4; ++w) {
    if (kg == w) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 8; ++n) {
          const int c = n >> 1, p = n & 1;
          const int j = c * 64 + (4 * p + (li >> 2)) * 8 + 4 * q + (li & 3);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* dst = red + (m * 16 + 4 * g + r) * 256 + j;
            const float v = acc[m][n][r] + accs[m][n][r];
            *dst = (w == 0) ? v : *dst + v;
          }
        }
    }
    __syncthreads();
  }
  float* out = part + (size_t)blockIdx.x * (32 * 256);
  for (int i = tid; i < 32 * 256 / 4; i += kT) reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(red)[i];
}

// ---------------------------------------------------------------------------------------------------------------- conv2
namespace c2 {
constexpr int SUB = 368;                         // bytes per sub-image (one channel): 11 rows x 16 el x 2 B + 16
constexpr int IMG_PART = 4 * 16 * SUB;           // one part of one channel half: 23,552
constexpr int IMG_BYTES = 3 * IMG_PART;          // 70,656
constexpr int DT_PITCH = 352;                    // bytes per (copy, part, oc) row: 160 k x 2 B + 32
constexpr int DT_PART = 32 * DT_PITCH;           // one part of one copy
constexpr int DT_BYTES = 2 * 3 * DT_PART;        // 67,584
constexpr int LDS_TOTAL = IMG_BYTES + DT_BYTES;  // 138,240
static_assert(LDS_TOTAL == 138240 && LDS_TOTAL <= 160 * 1024, "LDS budget");
constexpr int kAQuads = 400 * 4, kDQuads = 81 * 8;  // float4 per frame and channel half of a1; per frame and oc half of d_a2
}  // namespace c2

__global__ __launch_bounds__(kT) void wgrad_conv2_x3(const float* __restrict__ a1, const float* __restrict__ d_a2, int frames,
                                                     float* __restrict__ part) {
  using namespace c2;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* img = smem;
  uint8_t* dt = smem + IMG_BYTES;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int sr = wave & 3, mt = wave >> 2;

  for (int i = tid; i < LDS_TOTAL / 16; i += kT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);

  f32x4 acc[4][4], accs[4][4];  // [pass slot 2 ch + H][(p, q)]: hi x hi | the five small products
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = accs[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- staging registers.  A channel half of a1 is 1,600 float4 numbered (channel quad, parity class, cell of the 10 x 10
  // sub-image) as in wgrad_conv2_bf16.h, four per thread (the last threads repeat number 1,599); an oc half of d_a2 is 648
  // float4 numbered (channel quad, pixel), two per thread (clamped likewise). ----
  float4 xa[4], xb[4];  // a1: channel half 0 | 1
  float4 e[2][2];       // d_a2: [oc half][j]
  int a_g[4], a_l[4], d_g[2], d_l[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ai = min(tid + j * kT, kAQuads - 1);
    const int cq = ai / 400, rest = ai - cq * 400, cls = rest / 100, cl = rest - cls * 100;
    const int y = cl / 10, x = cl - y * 10;
    a_g[j] = ((2 * y + (cls >> 1)) * 20 + 2 * x + (cls & 1)) * 32 + cq * 4;
    a_l[j] = (cls * 16 + cq * 4) * SUB + (y * 16 + x) * 2;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int di = min(tid + j * kT, kDQuads - 1);
    const int px = di % 81, oc0 = (di / 81) * 4;
    const int oy = px / 9, ox = px - oy * 9;
    d_g[j] = px * 64 + oc0;
    d_l[j] = oc0 * DT_PITCH + (oy * 16 + ox) * 2;
  }
  auto load_a = [&](float4 (&x)[4], int f, int ch) {
    const float* fa = a1 + (size_t)f * (400 * 32) + ch * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const float4*>(fa + a_g[j]);
  };
  auto load_d = [&](int f) {
    const float* fd = d_a2 + (size_t)f * (81 * 64);
#pragma unroll
    for (int H = 0; H < 2; ++H)
#pragma unroll
      for (int j = 0; j < 2; ++j) e[H][j] = *reinterpret_cast<const float4*>(fd + d_g[j] + H * 32);
  };
  auto put_a = [&](const float4 (&x)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint2 pt[3];
      gemm3::split4x3(x[j], pt[0], pt[1], pt[2]);
      uint8_t* cell = img + a_l[j];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<uint16_t*>(cell + t * SUB + k * IMG_PART) = bf16_of(pt[k], t);
    }
  };
  auto put_d = [&](const float4 (&x)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint2 pt[3];
      gemm3::split4x3(x[j], pt[0], pt[1], pt[2]);
      uint8_t* r0 = dt + d_l[j];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const uint16_t v = bf16_of(pt[k], t);
          *reinterpret_cast<uint16_t*>(r0 + t * DT_PITCH + k * DT_PART) = v;            // q = 0
          *reinterpret_cast<uint16_t*>(r0 + t * DT_PITCH + (3 + k) * DT_PART + 2) = v;  // q = 1: shifted by one pixel
        }
    }
  };

  const int b_base = (sr * 16 + li) * SUB;
  const int a_base = (mt * 16 + li) * DT_PITCH;
  // the MFMAs of one pass into accumulator slot SLOT: the staged channel half x the staged oc half over the five k-steps
  auto mma = [&](auto slot) {
    constexpr int SLOT = decltype(slot)::value;
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
      const int G = ks * 4 + g;  // k-group of 8: row G >> 1, columns 8 (G & 1) ..
      const int bo = b_base + ((G >> 1) * 16 + (G & 1) * 8) * 2;
      const int ao = a_base + (32 * ks + 8 * g) * 2;
      bf16x8 af[2][3];  // [q][part]
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) af[q][k] = frag(dt + (q * 3 + k) * DT_PART + ao);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        bf16x8 bf[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) bf[k] = frag(img + k * IMG_PART + bo + p * 32);
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // (d part, image part) with i + j <= 2, smallest first; hi x hi alone in acc
          f32x4& cs = accs[SLOT][p * 2 + q];
          WGX3_MFMA(af[q][2], bf[0], cs);
          WGX3_MFMA(af[q][0], bf[2], cs);
          WGX3_MFMA(af[q][1], bf[1], cs);
          WGX3_MFMA(af[q][1], bf[0], cs);
          WGX3_MFMA(af[q][0], bf[1], cs);
          WGX3_MFMA(af[q][0], bf[0], acc[SLOT][p * 2 + q]);
        }
      }
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  using S3 = std::integral_constant<int, 3>;

  int f = blockIdx.x;  // (blocks <= frames: f is a frame)
  load_a(xa, f, 0), load_a(xb, f, 1), load_d(f);
  __syncthreads();  // zero fill done
  for (; f < frames; f += gridDim.x) {
    const int fn = (f + (int)gridDim.x < frames) ? f + (int)gridDim.x : f;  // (the last round re-reads its own frame)
    put_a(xa), put_d(e[0]);
    __syncthreads();
    mma(S0{});  // ch 0, H 0
    __syncthreads();
    put_d(e[1]);
    __syncthreads();
    mma(S1{});  // ch 0, H 1
    __syncthreads();
    put_a(xb);
    load_a(xa, fn, 0);
    __syncthreads();
    mma(S3{});  // ch 1, H 1
    __syncthreads();
    put_d(e[0]);
    load_a(xb, fn, 1), load_d(fn);
    __syncthreads();
    mma(S2{});  // ch 1, H 0
    __syncthreads();  // tiles read: the next frame may overwrite them
  }
  // every wave owns its elements: straight to this block's partial tile, column (kh * 4 + kw) * 32 + c
  float* out = part + (size_t)blockIdx.x * (64 * 512);
  const int s = sr >> 1, r = sr & 1;
#pragma unroll
  for (int slot = 0; slot < 4; ++slot)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int ch = slot >> 1, H = slot & 1, p = n >> 1, q = n & 1;
      const int col = ((2 * p + s) * 4 + (2 * q + r)) * 32 + ch * 16 + li;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        out[(size_t)(H * 32 + mt * 16 + 4 * g + rr) * 512 + col] = acc[slot][n][rr] + accs[slot][n][rr];
    }
}
#undef WGX3_MFMA

inline int launch_conv1(const uint8_t* obs, const float* d_a1, int frames, float* part, int blocks, hipStream_t s) {
  // (initialised once, thread-safely: launches may come from several host threads)
  static const hipError_t attr_set = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_conv1_x3),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, c1::LDS_TOTAL);
  RELA_HIP(attr_set);
  RELA_CHECK(blocks >= 1 && blocks <= kMaxBlocks && blocks <= frames, RELA_EINVAL, "wgrad_conv1_x3: %d blocks for %d frames",
             blocks, frames);
  note_launch("wgrad_conv1_x3");
  hipLaunchKernelGGL(wgrad_conv1_x3, dim3(blocks), dim3(kT), c1::LDS_TOTAL, s, obs, d_a1, frames, part);
  return RELA_OK;
}

inline int launch_conv2(const float* a1, const float* d_a2, int frames, float* part, int blocks, hipStream_t s) {
  static const hipError_t attr_set = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_conv2_x3),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, c2::LDS_TOTAL);
  RELA_HIP(attr_set);
  RELA_CHECK(blocks >= 1 && blocks <= kMaxBlocks && blocks <= frames, RELA_EINVAL, "wgrad_conv2_x3: %d blocks for %d frames",
             blocks, frames);
  note_launch("wgrad_conv2_x3");
  hipLaunchKernelGGL(wgrad_conv2_x3, dim3(blocks), dim3(kT), c2::LDS_TOTAL, s, a1, d_a2, frames, part);
  return RELA_OK;
}

}  // namespace
}  // namespace wgx3
}  // namespace rela_amd
