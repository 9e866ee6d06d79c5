// learner_common.h -- pieces shared by the two hand-written learner steps (learner.hip: Ape-X /
// AtariFFNet; learner_r2d2.hip: R2D2 / AtariLSTMNet): the tiles of their GEMMs and the one dispatch that obeys the
// backward plan (learner_plan.h), the gemm_lds problem descriptions of the conv trunk's backward pass, split-K reduction, column sums, global-norm clipping and the optimisers, and -- host side, at the
// end -- LearnerCore, the base of rela_apex_learner and rela_r2d2_learner: the flat parameter / gradient /
// optimiser-state store and what the entry points do with it (its device buffers belong to a DevBuffers, common.h).
// Everything sits in an anonymous namespace: each translation unit gets its own copy of the kernels.
#pragma once
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"
#include "ffnet_layout.h"
#include "gemm_lds.h"
#include "gemm_bf16x3.h"
#include "learner_plan.h"
#include "param_layout.h"
#include "prof.h"
#include "value_rescale.h"
#include "weight_pack.h"
#include "dgrad_conv_bf16.h"
#include "wgrad_conv1_bf16.h"
#include "wgrad_conv2_bf16.h"
#include "wgrad_conv3_bf16.h"

namespace rela_amd {
namespace {

using namespace gemm;

// ---- the tiles of the learners' GEMMs, by shape and arithmetic --------------------------------------------------------
// A shape's f32 tile runs on gemm_lds (f32 MFMA).  The two-part tile runs on the bf16 matrix cores (gemm_bf16x3.h: operands
// split into bf16 hi + lo on the way into LDS, three MFMAs per product): the learners' bf16x2 mode.  The three-part tile
// (PARTS = 3, six products) has f32 accuracy on the bf16 MFMA: the f32x3 modes.
using TileDgrad = TileCfg<128, 64, 4, 2, false>;  // M = batch rows, A k-contiguous
using Tile3Dgrad = gemm3::TileCfg<128, 64, 4, 2, false>;
using Tile6Dgrad = gemm3::TileCfg<128, 64, 4, 2, false, 3>;
using TileWfc = TileCfg<128, 64, 4, 2, true>;     // fc weight gradient (M = 512 units)
using Tile3Wfc = gemm3::TileCfg<128, 64, 4, 2, true>;
using Tile6Wfc = gemm3::TileCfg<128, 64, 4, 2, true, 3>;
// conv2 / conv3 weight gradients (M = 64 channels).  The 64 x 64 tiles stay at S = 1 (stages of one chunk per barrier): at
// S = 2 the f32 tile measured 4 us (512 frames) and 3 - 11 us (5,312) BEHIND; the three-part tile then fits one block on a CU
// instead of two and conv2 / conv3 measured 8 / 7 us behind.
using TileW64 = TileCfg<64, 64, 2, 4, true>;
using Tile3W64 = gemm3::TileCfg<64, 64, 2, 4, true>;
using Tile6W64 = gemm3::TileCfg<64, 64, 2, 4, true, 3>;
using TileW32 = TileCfg<32, 64, 2, 4, true>;      // head weight gradients (M = 32)
using Tile3W32 = gemm3::TileCfg<32, 64, 2, 4, true>;
using Tile6W32 = gemm3::TileCfg<32, 64, 2, 4, true, 3>;
// conv1's weight gradient in f32: stages of FOUR chunks per barrier (gemm_lds.h, S; 128 KB of dynamic LDS, one block per CU
// as before: 256 blocks).  Measured alone at 512 / 5,312 frames: S = 1 60 / 627 us, S = 2 53 / 590, S = 4 54 / 553.
using TileW1 = TileCfg<32, 64, 2, 4, true, 4>;
// ... in three parts: the B operand is the u8 frame, exact in ONE bf16 part -- its mid and lo parts would be zeros --
// at a stage of TWO chunks: 45 -> 37 us alone at 512 frames.  S = 4 measured 36 us but takes 112 KB of LDS and 138
// registers: a second block no longer fits the CU (tests/test_trunk_backward_resources_cpu.py); S = 2 keeps 56 KB, 72 registers.
// (The bf16x2 mode runs wgrad_conv1_bf16.h instead.)
using Tile6W32U8 = gemm3::SinglePartB<gemm3::TileCfg<32, 64, 2, 4, true, 3, 2>>;
// conv3's / conv2's data gradients (N = 64 / 32 input channels), f32 in every mode: 64 rows per block measured ahead of 128
// (and of 256 for conv2) at 512 frames -- K is only 576 / 256, so more and smaller blocks hide more of each block's fixed costs
using TileDgrad3 = TileCfg<64, 64, 2, 4, false>;
using TileDgrad2 = TileCfg<64, 32, 4, 2, false>;
// the R2D2 learner's (learner_r2d2.hip)
using TileRows = TileCfg<128, 64, 4, 2, false>;  // M = many rows, A k-contiguous
using TileRec = TileCfg<64, 64, 2, 4, false>;    // M = batch rows of one time step
using TileWg = TileCfg<128, 64, 4, 2, true>;     // weight gradients, M = 2048 gate rows
using TileW32r = TileCfg<32, 64, 2, 4, true>;    // head weight gradients (M = 32)
// The backward GEMMs of its mode 3 (f32x3_bwd).  64 x 64 tiles (100 registers, 60 KB of LDS: two blocks per CU) measured
// ahead of the 128 x 64 tiles of TileRows / TileWg (172 registers, 84 KB: one block) at 5,312 training rows: dW_ih 0.66 ->
// 0.58 ms, dW_hh 0.15 -> 0.10, d_a3 0.61 -> 0.58.  The conv weight gradients run one block per CU at their f32 split counts
// (conv3 0.28 ms against 0.24 in f32), two at twice the splits (learner_plan.h: kX6SplitMul).
using Tile6Rows = gemm3::TileCfg<64, 64, 2, 4, false, 3>;
using Tile6Wg = Tile6W64;

// The tiles of one GEMM shape: f32 | two-part | three-part.  void: that arithmetic never reaches the shape -- no kernel is
// instantiated for it, and a plan that asks for it is an internal error.
template <class F32, class X2, class X3>
struct TileSet {
  using f32 = F32;
  using x2 = X2;
  using x3 = X3;
};
using SetDgrad = TileSet<TileDgrad, Tile3Dgrad, Tile6Dgrad>;  // dgrad rows (heads, fc)
using SetWfc = TileSet<TileWfc, Tile3Wfc, Tile6Wfc>;          // fc weight gradient
using SetW64 = TileSet<TileW64, Tile3W64, Tile6W64>;          // 64-channel weight gradients (conv2, conv3)
using SetW32 = TileSet<TileW32, Tile3W32, Tile6W32>;          // 32-row head weight gradients
using SetW1 = TileSet<TileW1, void, Tile6W32U8>;              // conv1 weight gradient
using SetWg = TileSet<TileWg, void, Tile6Wg>;                 // R2D2: dW_hh, dW_ih
using SetRows = TileSet<TileRows, void, Tile6Rows>;           // R2D2: the input-side data gradient
using SetSeqHeadRows = TileSet<TileRows, void, void>;         // R2D2: the heads' data gradient and ...
using SetSeqHeadW32 = TileSet<TileW32r, void, void>;          // ... weight gradients (measured slower in three parts)

// the one way a learner GEMM is launched: the slot of `arith` in the shape's set (split-K, stream, names as launch_gemm)
template <class Set, class P>
int launch_gemm_as(GemmArith arith, const P& p, int splits, hipStream_t s, const char* name) {
  if constexpr (!std::is_void_v<typename Set::f32>)
    if (arith == kArithF32) return launch_gemm<typename Set::f32>(p, splits, s, name), RELA_OK;
  if constexpr (!std::is_void_v<typename Set::x2>)
    if (arith == kArithBf16x2) return gemm3::launch_gemm<typename Set::x2>(p, splits, s, name);
  if constexpr (!std::is_void_v<typename Set::x3>)
    if (arith == kArithF32x3) return gemm3::launch_gemm<typename Set::x3>(p, splits, s, name);
  set_last_error("%s: no tile for arithmetic %d (internal error: the plan and the tile sets disagree)", name, (int)arith);
  return RELA_ESTATE;
}

// d_h[b][u] = relu'(h) * sum_k d_ha[b][k] * Wh[k][u]      Wh rows: 0..A-1 = fc_a.weight, 31 = fc_v.weight
struct ProbHeadDgrad : ProbBase {
  const float *d_ha, *a_w, *v_w, *h;
  float* d_h;
  int A;
  __device__ float4 fetchA(int m, int k) const { return ld4(d_ha + (size_t)min(m, M - 1) * 32 + k); }
  __device__ float4 fixA(float4 v, int m, int) const { return keep4(m < M, v); }
  __device__ float4 fetchB(int k, int n) const {  // (rows A .. 30 fetch fc_v's row and are zeroed)
    const float* row = k < A ? a_w + (size_t)k * 512 : v_w;
    return ld4(row + n);
  }
  __device__ float4 fixB(float4 v, int k, int) const { return keep4(k < A || k == 31, v); }
  __device__ void store(int, int m, int n, float v) const {
    const size_t i = (size_t)m * 512 + n;
    d_h[i] = h[i] > 0.f ? v : 0.f;
  }
};

// the same over many rows (R2D2: 5,312 training rows), split over blockIdx.z into partial tiles part[z][32][512]
// that head_wgrad_reduce sums in z order (one 32 x 512 output: without the split the GEMM is 8 blocks)
struct ProbHeadWgradPart : ProbBase {
  const float *d_ha, *h;
  float* part;
  __device__ float4 fetchA(int b, int m) const { return ld4(d_ha + (size_t)min(b, K - 1) * 32 + m); }
  __device__ float4 fetchB(int b, int n) const { return ld4(h + (size_t)min(b, K - 1) * 512 + n); }
  __device__ float4 fixA(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ float4 fixB(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ void store(int z, int m, int n, float v) const { part[((size_t)z * 32 + m) * 512 + n] = v; }
};
__global__ void head_wgrad_reduce(const float* __restrict__ part, int splits, int A, float* __restrict__ g_a_w,
                                  float* __restrict__ g_v_w) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 32 * 512) return;
  const int m = idx >> 9, n = idx & 511;
  if (m >= A && m != 31) return;
  float s = 0.f;
#pragma unroll 8
  for (int z = 0; z < splits; ++z) s += part[(size_t)z * (32 * 512) + idx];
  if (m < A) g_a_w[(size_t)m * 512 + n] = s;
  else g_v_w[n] = s;
}

// dWh[k][u] = sum_b d_ha[b][k] * h[b][u]
struct ProbHeadWgrad : ProbBase {
  const float *d_ha, *h;
  float *g_a_w, *g_v_w;
  int A;
  __device__ float4 fetchA(int b, int m) const { return ld4(d_ha + (size_t)min(b, K - 1) * 32 + m); }
  __device__ float4 fetchB(int b, int n) const { return ld4(h + (size_t)min(b, K - 1) * 512 + n); }
  __device__ float4 fixA(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ float4 fixB(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ void store(int, int m, int n, float v) const {
    if (m < A) g_a_w[(size_t)m * 512 + n] = v;
    else if (m == 31) g_v_w[n] = v;
  }
};

// d_a3[b][j] = relu'(a3) * sum_u d_h[b][u] * Wfc'[u][j]     j = pos*64 + c (channel-last)
struct ProbFcDgrad : ProbBase {
  const float *d_h, *wfcp, *a3;
  float* d_a3;
  __device__ float4 fetchA(int m, int k) const { return ld4(d_h + (size_t)min(m, M - 1) * 512 + k); }
  __device__ float4 fixA(float4 v, int m, int) const { return keep4(m < M, v); }
  __device__ float4 fetchB(int k, int n) const { return ld4(wfcp + (size_t)k * 3136 + n); }
  __device__ void store(int, int m, int n, float v) const {
    const size_t i = (size_t)m * 3136 + n;
    d_a3[i] = a3[i] > 0.f ? v : 0.f;
  }
};

// dWfc[u][c*49+pos] = sum_b d_h[b][u] * a3[b][pos*64+c]   (written in state_dict order, net.py:49)
struct ProbFcWgrad : ProbBase {
  const float *d_h, *a3;
  float* g_fc_w;
  __device__ float4 fetchA(int b, int m) const { return ld4(d_h + (size_t)min(b, K - 1) * 512 + m); }
  __device__ float4 fetchB(int b, int n) const { return ld4(a3 + (size_t)min(b, K - 1) * 3136 + n); }
  __device__ float4 fixA(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ float4 fixB(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ void store(int, int m, int n, float v) const {
    const int pos = n >> 6, c = n & 63;
    g_fc_w[(size_t)m * 3136 + c * 49 + pos] = v;
  }
};

// ---- conv3 / conv2 data gradients: the transposed convolution as ONE GEMM over the pixels of the layer's INPUT ----------
// Rows are the pixels whose gradient is wanted, k runs over (tap, output channel), and the A loader gathers the output
// pixel that the tap connects to the row's pixel (zeros outside the output image) -- index arithmetic, as im2col is in
// ProbConvWgrad::fetchB.  The ReLU mask of the layer below is applied in the epilogue: no column buffer, no col2im pass.
// A tap is two chunks of 32 k (64 output channels), and the sum is folded tap by tap (gemm_lds.h: kFoldChunks): each
// tap's 64 terms from zero in channel order, the taps added in (kh, kw) order -- the association of the column form
// this replaces (a 64-term GEMM per tap, then col2im's sum over the taps), so every element has the same bits as before.
// A tap outside the image contributes an exact zero where col2im skipped it.
// d_a2[b][y][x][c] = relu'(a2) * sum_{kh,kw,oc} d_a3[b][y-kh][x-kw][oc] * W3p[oc][(kh*3+kw)*64 + c]
//   M = frames * 81, N = 64, K = 9 * 64, k = (kh*3+kw)*64 + oc
struct ProbDgrad3 : ProbBase {
  static constexpr int kFoldChunks = 2;
  const float *d_out, *wp, *a2;  // d_out [b][49][64]; wp = w3p (permute_weight_at, ffnet_layout.h); a2 [b][81][64]
  float* d_a2;
  // the output pixel (oy, ox) of frame b that tap k >> 6 connects to row m (m clamped; oy, ox may lie outside the image)
  __device__ void tap_pixel(int m, int k, int& b, int& oy, int& ox) const {
    m = min(m, M - 1);
    b = m / 81;
    const int pix = m - b * 81, y = pix / 9, x = pix - y * 9;
    const int tap = k >> 6, kh = tap / 3, kw = tap - kh * 3;
    oy = y - kh, ox = x - kw;
  }
  __device__ float4 fetchA(int m, int k) const {
    int b, oy, ox;
    tap_pixel(m, k, b, oy, ox);
    oy = min(max(oy, 0), 6), ox = min(max(ox, 0), 6);
    return ld4(d_out + ((size_t)b * 49 + oy * 7 + ox) * 64 + (k & 63));
  }
  __device__ float4 fixA(float4 v, int m, int k) const {
    int b, oy, ox;
    tap_pixel(m, k, b, oy, ox);
    return keep4(m < M && (unsigned)oy < 7u && (unsigned)ox < 7u, v);
  }
  __device__ float4 fetchB(int k, int n) const { return ld4(wp + (size_t)(k & 63) * 576 + (k >> 6) * 64 + n); }
  __device__ void store(int, int m, int n, float v) const {
    const size_t i = (size_t)m * 64 + n;
    d_a2[i] = a2[i] > 0.f ? v : 0.f;
  }
};

// conv2 has stride 2: a pixel (y, x) of a1 meets only the taps kh = 2p + s, kw = 2q + r with (s, r) = (y & 1, x & 1), from
// the output pixel (y/2 - p, x/2 - q).  The four parity classes are four GEMMs with the SAME A operand and different
// weights, in one launch: the class is the N tile (N = 4 x 32 with BN = 32, so blockIdx.x of gemm_lds IS the class and no
// tile holds two classes); rows are the 100 pixels (yh, xh) of a class per frame.
// d_a1[b][2yh+s][2xh+r][c] = relu'(a1) * sum_{p,q,oc} d_a2[b][yh-p][xh-q][oc] * W2p[oc][((2p+s)*4 + 2q+r)*32 + c]
//   M = frames * 100, N = 4 * 32 (n = (2s+r)*32 + c), K = 4 * 64, k = (2p+q)*64 + oc
struct ProbDgrad2 : ProbBase {
  static constexpr int kFoldChunks = 2;
  const float *d_out, *wp, *a1;  // d_out [b][81][64]; wp = w2p (permute_weight_at, ffnet_layout.h); a1 [b][400][32]
  float* d_a1;
  __device__ void tap_pixel(int m, int k, int& b, int& oy, int& ox) const {  // (as ProbDgrad3's)
    m = min(m, M - 1);
    b = m / 100;
    const int pix = m - b * 100, yh = pix / 10, xh = pix - yh * 10;
    const int t = k >> 6;
    oy = yh - (t >> 1), ox = xh - (t & 1);
  }
  __device__ float4 fetchA(int m, int k) const {
    int b, oy, ox;
    tap_pixel(m, k, b, oy, ox);
    oy = min(max(oy, 0), 8), ox = min(max(ox, 0), 8);
    return ld4(d_out + ((size_t)b * 81 + oy * 9 + ox) * 64 + (k & 63));
  }
  __device__ float4 fixA(float4 v, int m, int k) const {
    int b, oy, ox;
    tap_pixel(m, k, b, oy, ox);
    return keep4(m < M && (unsigned)oy < 9u && (unsigned)ox < 9u, v);
  }
  __device__ float4 fetchB(int k, int n) const {
    const int cls = n >> 5, t = k >> 6;
    const int kh = (t & 2) + (cls >> 1), kw = 2 * (t & 1) + (cls & 1);
    return ld4(wp + (size_t)(k & 63) * 512 + (kh * 4 + kw) * 32 + (n & 31));
  }
  __device__ void store(int, int m, int n, float v) const {
    const int cls = n >> 5;
    const int b = m / 100, pix = m - b * 100;
    const int yh = pix / 10, xh = pix - yh * 10;
    const size_t i = ((size_t)b * 400 + (2 * yh + (cls >> 1)) * 20 + 2 * xh + (cls & 1)) * 32 + (n & 31);
    d_a1[i] = a1[i] > 0.f ? v : 0.f;
  }
};

// partial[z][oc][j] = sum_{(b,pos) in slice z} d_out[(b,pos)][oc] * patch(in)[(b,pos)][j]
template <int OC, int CIN, int KH, int KW, int STRIDE, int OH, int OW, int IH, int IW>
struct ProbConvWgrad : ProbBase {
  const float *d_out, *in;  // d_out [(b,pos)][OC]; in [b][IH][IW][CIN] channel-last
  float* part;
  __device__ float4 fetchA(int k, int m) const { return ld4(d_out + (size_t)min(k, K - 1) * OC + m); }
  __device__ float4 fixA(float4 v, int k, int) const { return keep4(k < K, v); }
  __device__ float4 fixB(float4 v, int k, int) const { return keep4(k < K, v); }
  __device__ float4 fetchB(int k, int n) const {
    k = min(k, K - 1);
    const int b = k / (OH * OW), pos = k - b * (OH * OW);
    const int oy = pos / OW, ox = pos - oy * OW;
    const int r = n / CIN, c = n - r * CIN;
    const int kh = r / KW, kw = r - kh * KW;
    return ld4(in + (((size_t)b * IH + oy * STRIDE + kh) * IW + ox * STRIDE + kw) * CIN + c);
  }
  __device__ void store(int z, int m, int n, float v) const { part[((size_t)z * M + m) * N + n] = v; }
};
using ProbW3 = ProbConvWgrad<64, 64, 3, 3, 1, 7, 7, 9, 9>;
using ProbW2 = ProbConvWgrad<64, 32, 4, 4, 2, 9, 9, 20, 20>;

// conv1: the input is the u8 frame stack [b][4][84][84]; j = (c,kh,kw) = state_dict order.
// The forward folds s/255 into the weights (net.py:46), so dW1 = (d_a1'^T x im2col(u8)) / 255,
// applied by reduce_splits.
struct ProbW1 : ProbBase {
  const float* d_out;  // [(b,pos)][32]
  const uint8_t* obs;
  float* part;
  using StageB = uint32_t;  // four u8 pixels as fetched: converted when the chunk goes to LDS
  __device__ float4 fetchA(int k, int m) const { return ld4(d_out + (size_t)min(k, K - 1) * 32 + m); }
  __device__ float4 fixA(float4 v, int k, int) const { return keep4(k < K, v); }
  __device__ uint32_t fetchB(int k, int n) const {
    k = min(k, K - 1);
    const int b = k / 400, pos = k - b * 400;
    const int oy = pos / 20, ox = pos - oy * 20;
    const int c = n >> 6, kh = (n >> 3) & 7, kw = n & 7;
    return *reinterpret_cast<const uint32_t*>(obs + (size_t)b * 28224 + c * 7056 + (oy * 4 + kh) * 84 + ox * 4 + kw);
  }
  __device__ float4 fixB(uint32_t d, int k, int) const {
    return keep4(k < K,
                 make_float4((float)(d & 0xff), (float)((d >> 8) & 0xff), (float)((d >> 16) & 0xff), (float)(d >> 24)));
  }
  __device__ void store(int z, int m, int n, float v) const { part[((size_t)z * M + m) * N + n] = v; }
};


// ---- split-K reduction, written in state_dict order -----------------------------------------
enum { kRedConv1 = 0, kRedConv2 = 1, kRedConv3 = 2 };
__global__ void reduce_splits(const float* __restrict__ part, int splits, int M, int N, int mode,
                              float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * N) return;
  const int m = idx / N, n = idx - m * N;
  float s = 0.f;
#pragma unroll 8  // (the adds stay in z order; eight loads in flight instead of one)
  for (int z = 0; z < splits; ++z) s += part[((size_t)z * M + m) * N + n];
  if (mode == kRedConv1) {
    out[(size_t)m * N + n] = s / 255.0f;
  } else if (mode == kRedConv2) {  // n = (kh*4+kw)*32 + c -> [oc][c][kh][kw]
    const int c = n & 31, r = n >> 5;
    out[((size_t)(m * 32 + c) * 4 + (r >> 2)) * 4 + (r & 3)] = s;
  } else {  // n = (kh*3+kw)*64 + c -> [oc][c][kh][kw]
    const int c = n & 63, r = n >> 6;
    out[((size_t)(m * 64 + c) * 3 + r / 3) * 3 + r % 3] = s;
  }
}

// ---- column sums (bias gradients): two deterministic stages ----------------------------------
constexpr int kColsumBlocks = 256;
// src [rows][C], C in {32, 64, 512}: a thread owns one float4 of columns and every L-th row of the
// block's row slice (coalesced 16-byte loads), LDS reduction over the L row lanes
__global__ __launch_bounds__(kLT) void colsum_partial(const float* __restrict__ src, int64_t rows, int C,
                                                      float* __restrict__ part) {
  __shared__ float4 sm[kLT];
  const int G = C / 4, L = kLT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
  float4 s = zero4();
  for (int64_t r = r0 + rl; r < r1; r += L) {
    const float4 v = ld4(src + r * C + cg * 4);
    s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0) {
    for (int l = 1; l < L; ++l) {
      const float4 v = sm[cg + l * G];
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    *reinterpret_cast<float4*>(part + (size_t)blockIdx.x * C + cg * 4) = s;
  }
}
// one block per float4 of columns: thread b holds partial b, fixed-shape tree reduction in LDS
__global__ __launch_bounds__(kColsumBlocks) void colsum_final(const float* __restrict__ part, int C,
                                                              float* __restrict__ out) {
  __shared__ float4 sm[kColsumBlocks];
  const int cg = blockIdx.x;
  sm[threadIdx.x] = ld4(part + (size_t)threadIdx.x * C + cg * 4);
  __syncthreads();
  for (int o = kColsumBlocks / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const float4 v = sm[threadIdx.x + o];
      float4& d = sm[threadIdx.x];
      d.x += v.x, d.y += v.y, d.z += v.z, d.w += v.w;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *reinterpret_cast<float4*>(out + cg * 4) = sm[0];
}
// several column sums in ONE launch pair (the five bias gradients of a learner step were ten ~7 us launches):
// blockIdx.y selects the job; every job keeps the two-stage order of colsum_partial / colsum_final, so the results
// are bit-identical to separate launches.
constexpr int kMaxColsumJobs = 6;
struct ColsumJobs {
  const float* src[kMaxColsumJobs];
  float* out[kMaxColsumJobs];
  float* part[kMaxColsumJobs];  // kColsumBlocks * C floats each
  int64_t rows[kMaxColsumJobs];
  int C[kMaxColsumJobs];
  int n = 0;
  void add(const float* s, int64_t r, int c, float* o) { src[n] = s, rows[n] = r, C[n] = c, out[n] = o, ++n; }
};
__global__ __launch_bounds__(kLT) void colsum_partial_multi(ColsumJobs jobs) {
  __shared__ float4 sm[kLT];
  const int j = blockIdx.y;
  const float* src = jobs.src[j];
  const int64_t rows = jobs.rows[j];
  const int C = jobs.C[j];
  const int G = C / 4, L = kLT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
  float4 s = zero4();
  // eight row loads in flight per thread (one at a time left the 26 MB of d_a1 latency-bound: 47 us per step); the
  // adds keep their order, so the sums are bit-identical to the one-load loop
  int64_t r = r0 + rl;
  for (; r + 7 * (int64_t)L < r1; r += 8 * (int64_t)L) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ld4(src + (r + u * (int64_t)L) * C + cg * 4);
#pragma unroll
    for (int u = 0; u < 8; ++u) s.x += v[u].x, s.y += v[u].y, s.z += v[u].z, s.w += v[u].w;
  }
  for (; r < r1; r += L) {
    const float4 v = ld4(src + r * C + cg * 4);
    s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0) {
    for (int l = 1; l < L; ++l) {
      const float4 v = sm[cg + l * G];
      s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    *reinterpret_cast<float4*>(jobs.part[j] + (size_t)blockIdx.x * C + cg * 4) = s;
  }
}
__global__ __launch_bounds__(kColsumBlocks) void colsum_final_multi(ColsumJobs jobs) {
  __shared__ float4 sm[kColsumBlocks];
  const int j = blockIdx.y, cg = blockIdx.x, C = jobs.C[j];
  if (cg >= C / 4) return;  // (whole block)
  sm[threadIdx.x] = ld4(jobs.part[j] + (size_t)threadIdx.x * C + cg * 4);
  __syncthreads();
  for (int o = kColsumBlocks / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const float4 v = sm[threadIdx.x + o];
      float4& d = sm[threadIdx.x];
      d.x += v.x, d.y += v.y, d.z += v.z, d.w += v.w;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *reinterpret_cast<float4*>(jobs.out[j] + cg * 4) = sm[0];
}
__global__ void head_bias_grad(const float* __restrict__ s32, int A, float* __restrict__ g_a_b,
                               float* __restrict__ g_v_b) {
  const int k = threadIdx.x;
  if (k < A) g_a_b[k] = s32[k];
  if (k == 31) g_v_b[0] = s32[31];
}

// ---- loss: smooth_l1(err) * w, mean over the batch (apex.py:87, main.py:228), and its gradient
// through the dueling head  q = v + a*legal - mean_A(a*legal)  (net.py:33-39) --------------------
__global__ __launch_bounds__(kLT) void learner_loss_grad(const float* __restrict__ td, const float* __restrict__ w,
                                                         const int64_t* __restrict__ act,
                                                         const float* __restrict__ legal, int Bn, int A,
                                                         float* __restrict__ d_ha, float* __restrict__ loss_out) {
  __shared__ float red[kLT];
  float lsum = 0.f;
  const float inv_b = 1.0f / (float)Bn, inv_a = 1.0f / (float)A;
  for (int i = threadIdx.x; i < Bn; i += kLT) {
    const float e = td[i], ae = fabsf(e);
    lsum += (ae < 1.0f ? 0.5f * e * e : ae - 0.5f) * w[i];
    // err = target - q[a]:  d mean(loss*w) / d q[a] = -w * clamp(err, -1, 1) / B
    const float g = -(w[i] * fminf(fmaxf(e, -1.0f), 1.0f)) * inv_b;
    const int a = (int)act[i];
    float* row = d_ha + (size_t)i * 32;
    for (int k = 0; k < 32; ++k) {
      float v = 0.f;
      if (k < A) v = legal[(size_t)i * A + k] * (g * ((k == a ? 1.0f : 0.0f) - inv_a));
      if (k == 31) v = g;
      row[k] = v;
    }
  }
  red[threadIdx.x] = lsum;
  __syncthreads();
  for (int o = kLT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[0] = red[0] * inv_b;
}

// td_err (apex.py:30-45: batch-global q.min() of greedy_act(next_obs), double-DQN target, un-fused arithmetic as
// agent_ops.hip's td_kernel) + the loss kernel above in ONE single-workgroup launch (two latency-bound launches
// before: 15 + 19 us).  Same arithmetic in the same order, so priorities, loss and d_ha are bit-identical.
__global__ __launch_bounds__(1024) void learner_td_loss_grad(int Bn, int A, const float* __restrict__ q,
                                                             const float* __restrict__ qno, const float* __restrict__ qnt,
                                                             const float* __restrict__ nlegal,
                                                             const int64_t* __restrict__ act,
                                                             const float* __restrict__ reward,
                                                             const float* __restrict__ bootstrap, float gamma_n,
                                                             float vr_eps, const float* __restrict__ w,
                                                             const float* __restrict__ legal,
                                                             float* __restrict__ td, float* __restrict__ prio,
                                                             float* __restrict__ d_ha, float* __restrict__ loss_out) {
  __shared__ float red[1024];
  float m = INFINITY;
  for (int i = threadIdx.x; i < Bn * A; i += 1024) m = fminf(m, qno[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const float qmin = red[0];
  __syncthreads();
  float lsum = 0.f;
  const float inv_b = 1.0f / (float)Bn, inv_a = 1.0f / (float)A;
  for (int i = threadIdx.x; i < Bn; i += 1024) {
    int na = 0;
    float bv = -INFINITY;
#pragma unroll 6  // (the loads of several actions in flight: one at a time this loop was most of the kernel's 19 us)
    for (int j = 0; j < A; ++j) {  // greedy_act(next_obs): first maximal index of (1 + q - qmin) * legal (apex.py:51)
      const float lq = __fmul_rn(__fsub_rn(__fadd_rn(1.0f, qno[(size_t)i * A + j]), qmin), nlegal[(size_t)i * A + j]);
      if (lq > bv) bv = lq, na = j;
    }
    const int a = (int)act[i];
    const float qa = q[(size_t)i * A + a];
    const float bq = qnt[(size_t)i * A + na];
    float tgt;  // detached: with value rescaling (value_rescale.h) only the target changes, the Huber seed below keeps its formula
    if (vr_eps > 0.0f)
      tgt = rela_vr::h(__fadd_rn(reward[i], __fmul_rn(__fmul_rn(bootstrap[i], gamma_n), rela_vr::h_inv(bq, vr_eps))), vr_eps);
    else
      tgt = __fadd_rn(reward[i], __fmul_rn(__fmul_rn(bootstrap[i], gamma_n), bq));
    const float e = __fsub_rn(tgt, qa), ae = fabsf(e);
    td[i] = e;
    prio[i] = ae;
    lsum += (ae < 1.0f ? 0.5f * e * e : ae - 0.5f) * w[i];
    const float g = -(w[i] * fminf(fmaxf(e, -1.0f), 1.0f)) * inv_b;
    float4* row = reinterpret_cast<float4*>(d_ha + (size_t)i * 32);
    float v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      v[k] = 0.f;
      if (k < A) v[k] = legal[(size_t)i * A + k] * (g * ((k == a ? 1.0f : 0.0f) - inv_a));
      if (k == 31) v[k] = g;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  }
  // the same tree as learner_loss_grad's kLT = 512 lanes when Bn <= 512: lanes >= 512 hold zeros and fold in first
  red[threadIdx.x] = lsum;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[0] = red[0] * inv_b;
}

// ---- clip_grad_norm_ + optimiser over the flat buffers ----------------------------------------
constexpr int kNormBlocks = 256;
__global__ __launch_bounds__(256) void sumsq_partial(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
  // n is a multiple of 4 (every segment of the flat buffer is padded to 4 floats) and g is 16-byte aligned: float4
  // loads, four in flight per thread; fixed association (deterministic), f64 accumulation as before
  __shared__ double red[256];
  double s = 0.0;
  const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = g4[i + u * stride];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      s += (double)v[u].x * (double)v[u].x + (double)v[u].y * (double)v[u].y + (double)v[u].z * (double)v[u].z +
           (double)v[u].w * (double)v[u].w;
  }
  for (; i < n4; i += stride) {
    const float4 v = g4[i];
    s += (double)v.x * (double)v.x + (double)v.y * (double)v.y + (double)v.z * (double)v.z + (double)v.w * (double)v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) s += (double)g[(n4 << 2) + threadIdx.x] * (double)g[(n4 << 2) + threadIdx.x];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
// out[0] = total 2-norm, out[1] = min(1, max_norm / (norm + 1e-6))   (torch clip_grad_norm_)
// `abort_word` (may be NULL): a device word that is non-zero when the gradients of this step must not be applied (the
// R2D2 learner's grid-barrier timeout word): the coefficient becomes -1 and the update kernels leave everything alone.
// `skipped` (may be NULL): a device counter of the applies skipped that way, which the host takes off its Adam step
// number (rela_r2d2_learner_check); this thread is its only writer and the launches are stream-ordered.
// A NaN norm gives a NaN coefficient (torch's clamp propagates it): the update kernels then make every weight NaN.
__global__ __launch_bounds__(256) void clip_coef(const double* __restrict__ part, int nblk, float max_norm,
                                                 float* __restrict__ out, const unsigned* __restrict__ abort_word,
                                                 unsigned* __restrict__ skipped) {
  // one block of 256 threads: fixed-order tree over the (at most 256) partial sums (a single thread walking them took
  // 20 us of every learner step)
  __shared__ double red[256];
  red[threadIdx.x] = (int)threadIdx.x < nblk ? part[threadIdx.x] : 0.0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double s = red[0];
  const float norm = (float)sqrt(s);
  out[0] = norm;
  const float c = max_norm / (norm + 1e-6f);
  out[1] = c >= 1.0f ? 1.0f : c;
  if (abort_word && *abort_word != 0) {
    out[1] = -1.0f;
    if (skipped) *skipped += 1;
  }
}
// torch.optim.RMSprop (momentum 0, not centred): sq = alpha*sq + (1-alpha)*g*g; p -= lr * g / (sqrt(sq) + eps)
// (four elements per thread: 16-byte accesses; n4 = ceil(n / 4), the flat buffers are padded to 4 floats)
__global__ void rmsprop_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, int64_t n4,
                               float lr, float alpha, float eps, const float* __restrict__ coef) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float cf = coef[1];
  if (i >= n4 || cf < 0.f) return;
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 sv = reinterpret_cast<float4*>(sq)[i], pv = reinterpret_cast<float4*>(p)[i];
  auto upd = [&](float gi, float& s, float& pi) {
    gi = gi * cf;
    s = alpha * s + (1.0f - alpha) * gi * gi;
    pi -= lr * (gi / (sqrtf(s) + eps));
  };
  upd(gv.x, sv.x, pv.x), upd(gv.y, sv.y, pv.y), upd(gv.z, sv.z, pv.z), upd(gv.w, sv.w, pv.w);
  reinterpret_cast<float4*>(sq)[i] = sv;
  reinterpret_cast<float4*>(p)[i] = pv;
}
// torch.optim.RMSprop(centered=True) (momentum 0): sq as above, av = alpha*av + (1-alpha)*g (the gradient average), and the
// step divides by sqrt(sq - av*av) + eps.  One departure from torch, on purpose: sq - av*av is clamped at 0 before the square
// root.  In float32 the difference goes negative once alpha^k has dropped below the rounding unit (an element whose gradient
// barely changes: sq and av*av then agree to the last bit or two), and torch's float32 sqrt of it makes the weight NaN for good.
// The clamp is a comparison, not fmaxf: a NaN variance stays NaN, so a NaN gradient still shows in its weight.
__global__ void rmsprop_centered_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                        float* __restrict__ av, int64_t n4, float lr, float alpha, float eps,
                                        const float* __restrict__ coef) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float cf = coef[1];
  if (i >= n4 || cf < 0.f) return;
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 sv = reinterpret_cast<float4*>(sq)[i], mv = reinterpret_cast<float4*>(av)[i], pv = reinterpret_cast<float4*>(p)[i];
  auto upd = [&](float gi, float& s, float& m, float& pi) {
    gi = gi * cf;
    s = alpha * s + (1.0f - alpha) * gi * gi;
    m = alpha * m + (1.0f - alpha) * gi;
    float v = s - m * m;
    v = v < 0.0f ? 0.0f : v;
    pi -= lr * (gi / (sqrtf(v) + eps));
  };
  upd(gv.x, sv.x, mv.x, pv.x), upd(gv.y, sv.y, mv.y, pv.y), upd(gv.z, sv.z, mv.z, pv.z), upd(gv.w, sv.w, mv.w, pv.w);
  reinterpret_cast<float4*>(sq)[i] = sv;
  reinterpret_cast<float4*>(av)[i] = mv;
  reinterpret_cast<float4*>(p)[i] = pv;
}
// soft (Polyak) target update over the flat buffers: pt = pt + tau * (p - pt); the pads stay +0 (0 + tau * (0 - 0))
__global__ void target_lerp(float* __restrict__ pt, const float* __restrict__ p, int64_t n4, float tau) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 pv = reinterpret_cast<const float4*>(p)[i];
  float4 tv = reinterpret_cast<float4*>(pt)[i];
  tv.x = tv.x + tau * (pv.x - tv.x), tv.y = tv.y + tau * (pv.y - tv.y);
  tv.z = tv.z + tau * (pv.z - tv.z), tv.w = tv.w + tau * (pv.w - tv.w);
  reinterpret_cast<float4*>(pt)[i] = tv;
}
// torch.optim.Adam (no amsgrad, no weight decay); bias corrections computed on the host per step
__global__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m1,
                            float* __restrict__ m2, int64_t n4, float lr, float b1, float b2, float eps, float bc1,
                            float bc2_sqrt, const float* __restrict__ coef) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float cf = coef[1];
  if (i >= n4 || cf < 0.f) return;
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 av = reinterpret_cast<float4*>(m1)[i], bv = reinterpret_cast<float4*>(m2)[i], pv = reinterpret_cast<float4*>(p)[i];
  auto upd = [&](float gi, float& a, float& b, float& pi) {
    gi = gi * cf;
    a = b1 * a + (1.0f - b1) * gi;
    b = b2 * b + (1.0f - b2) * gi * gi;
    pi -= (lr / bc1) * (a / (sqrtf(b) / bc2_sqrt + eps));
  };
  upd(gv.x, av.x, bv.x, pv.x), upd(gv.y, av.y, bv.y, pv.y), upd(gv.z, av.z, bv.z, pv.z), upd(gv.w, av.w, bv.w, pv.w);
  reinterpret_cast<float4*>(m1)[i] = av;
  reinterpret_cast<float4*>(m2)[i] = bv;
  reinterpret_cast<float4*>(p)[i] = pv;
}


// ---- backward pass of the conv trunk (net.{0,2,4}), shared by both learners ---------------------
// (which kernels run, their split counts and thresholds: plan_trunk_backward, learner_plan.h)
// the largest partial buffer: conv3's split-K tiles, or one tile per block of the bf16 conv1 ([32][256]) / conv2
// ([64][512]) gradients
constexpr size_t kTrunkPartFloats = (size_t)w3fast::kMaxBlocks * 64 * 576;
static_assert(kTrunkPartFloats * 4 >= dgfast::kFrag3Bytes && kTrunkPartFloats * 4 >= dgfast::kFrag2Bytes, "frag scratch");
static_assert(kTrunkPartFloats >= (size_t)kSplitW3 * kMaxSplitMul * 64 * 576, "part size (split multiplier up to kMaxSplitMul)");
static_assert(kTrunkPartFloats >= (size_t)kSplitW3 * 64 * 576 && kTrunkPartFloats >= (size_t)w1fast::kMaxBlocks * 32 * 256 &&
                  kTrunkPartFloats >= (size_t)w2fast::kMaxBlocks * 64 * 512,
              "part size");
static_assert(kSplitW3 * 64 * 576 >= kSplitW2 * 64 * 512 && kSplitW3 * 64 * 576 >= kSplitW1 * 32 * 256, "part size");
static_assert(kWgrad1Blocks == w1fast::kMaxBlocks && kWgrad1BlocksTwoLanes <= w1fast::kMaxBlocks, "the plan's block caps");

// the most frames of one trunk_backward call: the data gradients put frames * 100 / 64 (conv2) and frames * 81 / 64
// (conv3) tiles on the grid's y axis
constexpr int kTrunkMaxFrames = 32768;
static_assert(((size_t)kTrunkMaxFrames * 100 + TileDgrad2::BM - 1) / TileDgrad2::BM <= 65535 &&
                  ((size_t)kTrunkMaxFrames * 81 + TileDgrad3::BM - 1) / TileDgrad3::BM <= 65535, "grid y extent of the data gradients");
struct TrunkBwd {
  int Bn;              // frames
  const uint8_t* obs;  // [Bn][4][84][84] u8
  const float *a1, *a2;  // relu(conv1), relu(conv2), channel-last (ffnet_layout.h)
  const float* d_a3;   // [Bn][49][64] gradient w.r.t. relu(conv3), ALREADY masked by a3 > 0
  float *d_a2, *d_a1;  // scratch [Bn][81][64], [Bn][400][32]
  float* part;         // scratch, kTrunkPartFloats
  float* cpart;        // scratch, kColsumBlocks * 512
  const float *w2p, *w3p;  // conv2 / conv3 weights in dgrad k order (permute_weight_at, ffnet_layout.h)
  float *g_c1w, *g_c1b, *g_c2w, *g_c2b, *g_c3w, *g_c3b;  // gradients, state_dict layout
  // What runs: the learner's TrunkArith for Bn frames (learner_plan.h).  bf16x2: the weight gradients on the dedicated bf16
  // kernels (conv2 / conv3 from kFastWgradMinFrames frames), the data gradients on dgrad_conv_bf16.h.  f32x3: the weight-gradient
  // GEMMs (contraction over batch x positions) on the bf16 MFMA with three-part operands, f32 accuracy (r4 at 512 frames, us
  // f32 -> three-part: conv3 49 -> 35, conv2 63 -> 52, conv1 110 -> 102).
  TrunkBwdPlan plan;
  // Two-lane form (the Ape-X learner): conv3's and conv2's weight gradients, and the column sums of every tensor that
  // exists by then (the caller's pending jobs, d_a3, d_a2), run on `side` next to the data-gradient chain on the
  // caller's stream; the caller's stream waits for the side lane before trunk_backward returns.  Every kernel computes
  // what it computes on one lane (same grids, same summation orders): the results are bit-identical.
  hipStream_t side = nullptr;
  hipEvent_t ev_da3 = nullptr, ev_da2 = nullptr, ev_side = nullptr;
  float *part_side = nullptr, *cpart_side = nullptr;  // the side lane's own `part` / `cpart`
  const void *frag2 = nullptr, *frag3 = nullptr;  // dgrad weight fragments packed ahead (else per call, into `part`)
  const float* s32 = nullptr;                     // (side lane) head_bias_grad after the column sums
  float *g_a_b = nullptr, *g_v_b = nullptr;
  int A = 0;
};
// `to` continues only after everything queued on `from` so far
inline void lane_dep(hipEvent_t ev, hipStream_t from, hipStream_t to) {
  (void)hipEventRecord(ev, from);
  (void)hipStreamWaitEvent(to, ev, 0);
}

// all queued jobs in one launch pair; cpart must hold kColsumBlocks * (sum of the jobs' C) floats
inline void colsum_multi_launch(ColsumJobs& jobs, float* cpart, hipStream_t s) {
  if (jobs.n == 0) return;
  int maxC = 0;
  size_t off = 0;
  for (int j = 0; j < jobs.n; ++j) {
    jobs.part[j] = cpart + off;
    off += (size_t)kColsumBlocks * jobs.C[j];
    maxC = jobs.C[j] > maxC ? jobs.C[j] : maxC;
  }
  ProfScope prof("learner_colsum", s);
  hipLaunchKernelGGL(colsum_partial_multi, dim3(kColsumBlocks, jobs.n), dim3(kLT), 0, s, jobs);
  hipLaunchKernelGGL(colsum_final_multi, dim3(maxC / 4, jobs.n), dim3(kColsumBlocks), 0, s, jobs);
}

inline void colsum_launch(const float* src, int64_t rows, int C, float* cpart, float* out, hipStream_t s) {
  ProfScope prof("learner_colsum", s);
  hipLaunchKernelGGL(colsum_partial, dim3(kColsumBlocks), dim3(kLT), 0, s, src, rows, C, cpart);
  hipLaunchKernelGGL(colsum_final, dim3(C / 4), dim3(kColsumBlocks), 0, s, (const float*)cpart, C, out);
}

// One conv weight gradient as its WgradPlan says: the dedicated bf16 kernel (`fast`: (int* blocks) -> its launch) or the
// split-K GEMM of Problem `p` in the plan's arithmetic, into partial tiles p.part [slices][p.M][p.N]; then reduce_splits sums
// the slices in order into `out` (state_dict layout, `red`: kRedConv1 / 2 / 3).
template <class Set, class P, class Fast>
int conv_wgrad(const WgradPlan& w, const P& p, Fast fast, int red, float* out, hipStream_t s, const char* name) {
  int slices = w.splits;
  if (w.bf16_kernel) {
    ProfScope prof(name, s);
    (void)fast(&slices);
  } else if (int rc = launch_gemm_as<Set>(w.arith, p, slices, s, name)) {
    return rc;
  }
  hipLaunchKernelGGL(reduce_splits, dim3(ceil_div(p.M * p.N, 256)), dim3(256), 0, s, (const float*)p.part, slices, p.M, p.N,
                     red, out);
  return RELA_OK;
}

// `jobs`: the caller's pending column sums; the three bias gradients of the trunk are queued behind them and the
// whole queue goes out in one launch pair at the end (t.cpart: kColsumBlocks * (sum of all queued C) floats)
inline int trunk_backward(const TrunkBwd& t, hipStream_t s, ColsumJobs* pending = nullptr) {
  const int Bn = t.Bn;
  const TrunkBwdPlan& plan = t.plan;
  ColsumJobs own;
  ColsumJobs& jobs = pending ? *pending : own;
  const bool lanes = t.side != nullptr;
  hipStream_t sw = lanes ? t.side : s;  // the lane of conv3's / conv2's weight gradients
  float* partw = lanes ? t.part_side : t.part;
  if (lanes) lane_dep(t.ev_da3, s, sw);  // d_a3 (and everything the pending jobs read) is ready
  {  // conv3: dW3, db3, d_a2
    ProbW3 p{};
    p.M = 64, p.N = 576, p.K = Bn * 49;
    p.d_out = t.d_a3, p.in = t.a2, p.part = partw;
    auto fast = [&](int* blocks) { return w3fast::launch(t.a2, t.d_a3, Bn, partw, sw, blocks); };
    if (int rc = conv_wgrad<SetW64>(plan.w3, p, fast, kRedConv3, t.g_c3w, sw, "learner_wgrad_conv3")) return rc;
  }
  jobs.add(t.d_a3, (int64_t)Bn * 49, 64, t.g_c3b);
  if (plan.dgrad_bf16) {  // transposed convolution on bf16 MFMA, ReLU mask fused, no column buffer (dgrad_conv_bf16.h)
    ProfScope prof("learner_dgrad_conv3", s);
    (void)dgfast::launch_conv3(t.d_a3, t.w3p, t.a2, t.d_a2, Bn, t.part, s, t.frag3);
  } else {
    ProbDgrad3 p{};  // (f32x3 too: exact f32, one launch, no column buffer)
    p.M = Bn * 81, p.N = 64, p.K = 576;
    p.d_out = t.d_a3, p.wp = t.w3p, p.a2 = t.a2, p.d_a2 = t.d_a2;
    launch_gemm<TileDgrad3>(p, 1, s, "learner_dgrad_conv3");
  }
  if (lanes) lane_dep(t.ev_da2, s, sw);  // d_a2 is ready
  {  // conv2: dW2, db2, d_a1
    ProbW2 p{};
    p.M = 64, p.N = 512, p.K = Bn * 81;
    p.d_out = t.d_a2, p.in = t.a1, p.part = partw;
    auto fast = [&](int* blocks) { return w2fast::launch(t.a1, t.d_a2, Bn, partw, sw, blocks); };
    if (int rc = conv_wgrad<SetW64>(plan.w2, p, fast, kRedConv2, t.g_c2w, sw, "learner_wgrad_conv2")) return rc;
  }
  jobs.add(t.d_a2, (int64_t)Bn * 81, 64, t.g_c2b);
  if (lanes) {  // the side lane ends here: the column sums of everything but d_a1, then the head biases
    colsum_multi_launch(jobs, t.cpart_side, sw);
    if (t.s32) hipLaunchKernelGGL(head_bias_grad, dim3(1), dim3(32), 0, sw, t.s32, t.A, t.g_a_b, t.g_v_b);
    jobs.n = 0;
  }
  if (plan.dgrad_bf16) {
    ProfScope prof("learner_dgrad_conv2", s);
    (void)dgfast::launch_conv2(t.d_a2, t.w2p, t.a1, t.d_a1, Bn, t.part, s, t.frag2);
  } else {
    ProbDgrad2 p{};  // the four parity classes in one launch
    p.M = Bn * 100, p.N = 4 * 32, p.K = 256;
    p.d_out = t.d_a2, p.wp = t.w2p, p.a1 = t.a1, p.d_a1 = t.d_a1;
    launch_gemm<TileDgrad2>(p, 1, s, "learner_dgrad_conv2");
  }
  {  // conv1: dW1, db1 (no gradient flows into the frames)
    ProbW1 p{};
    p.M = 32, p.N = 256, p.K = Bn * 400;
    p.d_out = t.d_a1, p.obs = t.obs, p.part = t.part;
    auto fast = [&](int* blocks) { return w1fast::launch(t.obs, t.d_a1, Bn, t.part, s, blocks, plan.w1_max_blocks); };
    if (int rc = conv_wgrad<SetW1>(plan.w1, p, fast, kRedConv1, t.g_c1w, s, "learner_wgrad_conv1")) return rc;
  }
  jobs.add(t.d_a1, (int64_t)Bn * 400, 32, t.g_c1b);
  colsum_multi_launch(jobs, t.cpart, s);
  if (lanes) lane_dep(t.ev_side, sw, s);
  return RELA_OK;
}

// ---- clip_grad_norm_ + optimiser over flat parameter / gradient / state buffers -------------------
struct OptimState {
  int optimizer = 0;  // 0 RMSprop, 1 Adam
  float lr = 0.f, eps = 0.f, clip = 0.f;
  int64_t adam_t = 0;
  // torch's defaults; *_learner_set_rmsprop / _set_adam_betas change them while the state is the zero state
  float alpha = 0.99f;    // RMSprop's decay
  bool centered = false;  // RMSprop: S2 = the gradient average, rmsprop_centered_update (else S2 is never touched)
  float b1 = 0.9f, b2 = 0.999f;  // Adam's betas
};
// the ranges of the option setters and of rela_debug_optimizer_apply_opts (a NaN fails every comparison)
inline bool rmsprop_options_ok(float alpha, int centered) { return alpha > 0.f && alpha < 1.f && (centered == 0 || centered == 1); }
inline bool adam_betas_ok(float b1, float b2) { return b1 >= 0.f && b1 < 1.f && b2 > 0.f && b2 < 1.f; }
// adam_t counts every Adam apply launched; one that the device skipped (abort_word) adds one to *skipped, which the
// owner of abort_word takes off adam_t again once it has read the word.  census: rela_debug_optimizer_apply counts its
// three launches (the learners' steps do not: their censuses are recorded ones).
inline void optimizer_apply(OptimState& o, float* P, const float* G, float* S1, float* S2, int64_t n, double* npart,
                            float* norm, hipStream_t s, const unsigned* abort_word = nullptr, unsigned* skipped = nullptr,
                            bool census = false) {
  ProfScope prof("learner_optimizer", s);
  hipLaunchKernelGGL(sumsq_partial, dim3(kNormBlocks), dim3(256), 0, s, G, n, npart);
  hipLaunchKernelGGL(clip_coef, dim3(1), dim3(256), 0, s, (const double*)npart, kNormBlocks, o.clip, norm, abort_word,
                     skipped);
  if (census) {
    note_launch("sumsq_partial"), note_launch("clip_coef");
    note_launch(o.optimizer != 0 ? "adam_update" : o.centered ? "rmsprop_centered_update" : "rmsprop_update");
  }
  if (o.optimizer == 0 && o.centered) {
    hipLaunchKernelGGL(rmsprop_centered_update, dim3(ceil_div(n / 4, 256)), dim3(256), 0, s, P, G, S1, S2, n / 4, o.lr,
                       o.alpha, o.eps, (const float*)norm);
  } else if (o.optimizer == 0) {
    hipLaunchKernelGGL(rmsprop_update, dim3(ceil_div(n / 4, 256)), dim3(256), 0, s, P, G, S1, n / 4, o.lr, o.alpha, o.eps,
                       (const float*)norm);
  } else {
    o.adam_t += 1;
    const float b1 = o.b1, b2 = o.b2;
    const float bc1 = 1.0f - (float)pow((double)b1, (double)o.adam_t);
    const float bc2s = (float)sqrt(1.0 - pow((double)b2, (double)o.adam_t));
    hipLaunchKernelGGL(adam_update, dim3(ceil_div(n / 4, 256)), dim3(256), 0, s, P, G, S1, S2, n / 4, o.lr, b1, b2, o.eps,
                       bc1, bc2s, (const float*)norm);
  }
}

// ---- what the two learners share on the host ------------------------------------------------------------------------
// The flat store: P (online), PT (target), G (gradients), S1 / S2 (optimiser state), each off[nseg] floats with the
// net's tensors at off[i] (param_layout.h).  The functions are the bodies of the rela_*_learner_* entry points, which
// check their handle, select the device, pass their own name (`who` leads every message) and re-pack the
// kernel-layout weight copies afterwards (each learner's own repack).
struct LearnerCore {
  int device = 0;
  int A = 0, Bmax = 0;
  float gamma_n = 0.f;
  float vr_eps = 0.f;        // value rescaling of the TD target (set_value_rescale), 0 = off
  bool loss_called = false;  // ... which is fixed from the first loss on
  OptimState opt;
  bool applied = false;  // an apply was launched since create / the last load: S1 / S2 are no longer the zero state
  int nseg = 0;
  int64_t cnt[kLstmNetSegs] = {0};      // elements per tensor
  int64_t off[kLstmNetSegs + 1] = {0};  // segment offsets, off[nseg] = total
  float *P = nullptr, *PT = nullptr, *G = nullptr, *S1 = nullptr, *S2 = nullptr;
  double* npart = nullptr;
  float* norm = nullptr;  // [0] grad norm, [1] clip coefficient
  float* loss = nullptr;
  bool loaded = false;
  DevBuffers mem;  // every device buffer of the learner

  // counts: ffnet_param_counts / lstmnet_param_counts (param_layout.h) with their kFFNetSegs / kLstmNetSegs
  int alloc_flat(int nseg_, void (*counts)(int, int64_t*), int num_action) {
    nseg = nseg_;
    counts(num_action, cnt);
    flat_offsets(cnt, nseg, off);
    for (float** p : {&P, &PT, &G, &S1, &S2})
      if (int rc = mem.alloc(p, (size_t)off[nseg], true)) return rc;
    if (int rc = mem.alloc(&npart, kNormBlocks, false)) return rc;
    if (int rc = mem.alloc(&norm, 2, true)) return rc;  // (zeroed: stats before the first apply reads zeros)
    return mem.alloc(&loss, 1, true);
  }
  // online / target: the net's params struct, nseg pointers (target may be null: the online tensors twice)
  int load(const char* who, const void* online, const void* target, int on_device, hipStream_t s) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float* const* fo = static_cast<const float* const*>(online);
    const float* const* ft = static_cast<const float* const*>(target ? target : online);
    for (int i = 0; i < nseg; ++i) {
      RELA_CHECK(fo[i] && ft[i], RELA_EINVAL, "%s: parameter %d is NULL", who, i);
      RELA_HIP(hipMemcpyAsync(P + off[i], fo[i], sizeof(float) * cnt[i], kind, s));
      RELA_HIP(hipMemcpyAsync(PT + off[i], ft[i], sizeof(float) * cnt[i], kind, s));
    }
    if (!on_device) RELA_HIP(hipStreamSynchronize(s));  // the host buffers may go away
    const size_t nb = sizeof(float) * (size_t)off[nseg];
    RELA_HIP(hipMemsetAsync(S1, 0, nb, s));
    RELA_HIP(hipMemsetAsync(S2, 0, nb, s));
    opt.adam_t = 0;
    applied = false;  // (the options and the learning rate stay)
    return RELA_OK;
  }
  int copy_online_to_target(hipStream_t s) {  // apex.py:27
    RELA_HIP(hipMemcpyAsync(PT, P, sizeof(float) * (size_t)off[nseg], hipMemcpyDeviceToDevice, s));
    return RELA_OK;
  }
  // Polyak update of the target net: PT += tau * (P - PT) over the whole flat buffer; tau == 1 is the copy, bit for bit
  int soft_update_target(float tau, hipStream_t s) {
    if (tau == 1.0f) return copy_online_to_target(s);
    const int64_t n4 = off[nseg] / 4;
    hipLaunchKernelGGL(target_lerp, dim3(ceil_div(n4, 256)), dim3(256), 0, s, PT, (const float*)P, n4, tau);
    RELA_LAUNCH_CHECK();
    return RELA_OK;
  }
  // the checks of rela_*_learner_soft_update_target; the caller then selects the device, calls soft_update_target and re-packs
  int check_soft_update(const char* who, float tau) const {
    RELA_CHECK(tau > 0.f && tau <= 1.f, RELA_EINVAL, "%s: tau must be in (0, 1] (got %g)", who, (double)tau);
    RELA_CHECK(loaded, RELA_ESTATE, "%s: parameters were never loaded", who);
    return RELA_OK;
  }
  int set_lr(const char* who, float lr) {
    RELA_CHECK(lr >= 0.f && lr <= 3.402823466e+38f, RELA_EINVAL, "%s: lr must be finite and >= 0 (got %g)", who, (double)lr);
    opt.lr = lr;  // the next apply passes it to its update kernel; no state, no step number
    return RELA_OK;
  }
  int get_lr(const char* who, float* out) const {
    RELA_CHECK(out, RELA_EINVAL, "%s: bad arguments", who);
    *out = opt.lr;
    return RELA_OK;
  }
  // The two option setters: only while S1 / S2 are the zero state (after create or a load, before the first apply since):
  // S2 changes its meaning with `centered`, and a decay that changes under a running average has no counterpart in torch.
  int set_rmsprop(const char* who, float alpha, int centered) {
    RELA_CHECK(opt.optimizer == 0, RELA_EINVAL, "%s: this learner's optimiser is Adam, not RMSprop", who);
    RELA_CHECK(rmsprop_options_ok(alpha, centered), RELA_EINVAL, "%s: alpha must be in (0, 1) and centered 0 or 1 (got %g, %d)",
               who, (double)alpha, centered);
    RELA_CHECK(!applied, RELA_ESTATE, "%s: call it before the first apply after create or load", who);
    opt.alpha = alpha, opt.centered = centered != 0;
    return RELA_OK;
  }
  int set_adam_betas(const char* who, float b1, float b2) {
    RELA_CHECK(opt.optimizer == 1, RELA_EINVAL, "%s: this learner's optimiser is RMSprop, not Adam", who);
    RELA_CHECK(adam_betas_ok(b1, b2), RELA_EINVAL, "%s: betas must be in [0, 1) and (0, 1) (got %g, %g)", who, (double)b1,
               (double)b2);
    RELA_CHECK(!applied, RELA_ESTATE, "%s: call it before the first apply after create or load", who);
    opt.b1 = b1, opt.b2 = b2;
    return RELA_OK;
  }
  // params_out: the net's params struct; its nseg pointers into the flat buffer at `base`
  void params_at(const float* base, void* params_out) const {
    const float** f = static_cast<const float**>(params_out);
    for (int i = 0; i < nseg; ++i) f[i] = base + off[i];
  }
  int flat(float** params_dev, float** grads_dev, int64_t* count) const {
    if (params_dev) *params_dev = P;
    if (grads_dev) *grads_dev = G;
    if (count) *count = off[nseg];
    return RELA_OK;
  }
  int set_value_rescale(const char* who, float eps) {
    RELA_CHECK(eps == eps, RELA_EINVAL, "%s: bad arguments", who);
    RELA_CHECK(!loss_called, RELA_ESTATE, "%s: call it before the first loss", who);
    vr_eps = eps > 0.f ? eps : 0.f;
    return RELA_OK;
  }
  void apply(hipStream_t s, const unsigned* abort_word = nullptr, unsigned* skipped = nullptr) {
    optimizer_apply(opt, P, G, S1, S2, off[nseg], npart, norm, s, abort_word, skipped);
    applied = true;  // (also when the device skips it on the abort word: the host cannot know yet)
  }
  int debug_optim(const char* who, float** s1_dev, float** s2_dev, int64_t* adam_t) const {
    RELA_CHECK(s1_dev && s2_dev && adam_t, RELA_EINVAL, "%s: bad arguments", who);
    *s1_dev = S1, *s2_dev = S2, *adam_t = opt.adam_t;
    return RELA_OK;
  }
};

}  // namespace
}  // namespace rela_amd
