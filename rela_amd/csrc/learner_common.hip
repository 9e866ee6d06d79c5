// learner_common.hip -- the one compiled copy of what the Ape-X and the R2D2 learner step share (interface:
// learner_common.h): the backward pass of the conv trunk as gemm_lds / gemm_bf16x3 Problems and the dedicated bf16
// kernels (wgrad_conv{1,2,3}_bf16.h, dgrad_conv_bf16.h) with its split-K reduction, the column sums, the heads' one-GEMM
// weight gradient and bias gradients, global-norm clipping with the three optimiser kernels, and the Polyak update.
// The kernels sit in this unit's anonymous namespace behind the launchers learner_common.h declares; at the end, the
// test taps that run this code one call at a time.
#include "learner_common.h"

#include "dgrad_conv_bf16.h"
#include "wgrad_conv1_bf16.h"
#include "wgrad_conv2_bf16.h"
#include "wgrad_conv3_bf16.h"

namespace rela_amd {
namespace {

// ---- the tiles only the conv trunk uses (the others: learner_common.h) ----------------------------------------------
// conv2 / conv3 weight gradients (M = 64 channels).  The 64 x 64 tiles stay at S = 1 (stages of one chunk per barrier): at
// S = 2 the f32 tile measured 4 us (512 frames) and 3 - 11 us (5,312) BEHIND; the three-part tile then fits one block on a CU
// instead of two and conv2 / conv3 measured 8 / 7 us behind.
using TileW64 = TileCfg<64, 64, 2, 4, true>;
using Tile3W64 = gemm3::TileCfg<64, 64, 2, 4, true>;
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
using SetW64 = TileSet<TileW64, Tile3W64, Tile6W64>;  // 64-channel weight gradients (conv2, conv3)
using SetW1 = TileSet<TileW1, void, Tile6W32U8>;      // conv1 weight gradient

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
// several column sums in ONE launch pair (ColsumJobs, learner_common.h)
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

// ---- clip_grad_norm_ + optimiser over the flat buffers ----------------------------------------
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

// ---- the constants of learner_common.h against what they were derived from -------------------------------------------
static_assert(kTrunkPartFloats == (size_t)w3fast::kMaxBlocks * 64 * 576, "part size: one conv3 tile per block of wgrad_conv3_bf16");
static_assert(kFrag2Bytes == dgfast::kFrag2Bytes && kFrag3Bytes == dgfast::kFrag3Bytes, "frag sizes");
static_assert(kTrunkPartFloats * 4 >= dgfast::kFrag3Bytes && kTrunkPartFloats * 4 >= dgfast::kFrag2Bytes, "frag scratch");
static_assert(kTrunkPartFloats >= (size_t)kSplitW3 * kMaxSplitMul * 64 * 576, "part size (split multiplier up to kMaxSplitMul)");
static_assert(kTrunkPartFloats >= (size_t)kSplitW3 * 64 * 576 && kTrunkPartFloats >= (size_t)w1fast::kMaxBlocks * 32 * 256 &&
                  kTrunkPartFloats >= (size_t)w2fast::kMaxBlocks * 64 * 512,
              "part size");
static_assert(kSplitW3 * 64 * 576 >= kSplitW2 * 64 * 512 && kSplitW3 * 64 * 576 >= kSplitW1 * 32 * 256, "part size");
static_assert(kWgrad1Blocks == w1fast::kMaxBlocks && kWgrad1BlocksTwoLanes <= w1fast::kMaxBlocks, "the plan's block caps");
static_assert(((size_t)kTrunkMaxFrames * 100 + TileDgrad2::BM - 1) / TileDgrad2::BM <= 65535 &&
                  ((size_t)kTrunkMaxFrames * 81 + TileDgrad3::BM - 1) / TileDgrad3::BM <= 65535, "grid y extent of the data gradients");

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

}  // namespace

void colsum_multi_launch(ColsumJobs& jobs, float* cpart, hipStream_t s) {
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

void colsum_launch(const float* src, int64_t rows, int C, float* cpart, float* out, hipStream_t s) {
  ProfScope prof("learner_colsum", s);
  hipLaunchKernelGGL(colsum_partial, dim3(kColsumBlocks), dim3(kLT), 0, s, src, rows, C, cpart);
  hipLaunchKernelGGL(colsum_final, dim3(C / 4), dim3(kColsumBlocks), 0, s, (const float*)cpart, C, out);
}

void launch_head_bias_grad(const float* s32, int A, float* g_a_b, float* g_v_b, hipStream_t s) {
  hipLaunchKernelGGL(head_bias_grad, dim3(1), dim3(32), 0, s, s32, A, g_a_b, g_v_b);
}

int launch_head_wgrad(GemmArith arith, int rows, int A, const float* d_ha, const float* h, float* g_a_w, float* g_v_w,
                      hipStream_t s) {
  ProbHeadWgrad p{};
  p.M = 32, p.N = 512, p.K = rows;
  p.d_ha = d_ha, p.h = h, p.g_a_w = g_a_w, p.g_v_w = g_v_w, p.A = A;
  return launch_gemm_as<SetW32>(arith, p, 1, s, "learner_wgrad_heads");
}

void pack_dgrad_frags(const float* w2p, const float* w3p, void* frag2, void* frag3, hipStream_t s) {
  dgfast::pack_frags(w2p, w3p, frag2, frag3, s);
}

int trunk_backward(const TrunkBwd& t, hipStream_t s, ColsumJobs* pending) {
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
    if (t.s32) launch_head_bias_grad(t.s32, t.A, t.g_a_b, t.g_v_b, sw);
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

void optimizer_apply(OptimState& o, float* P, const float* G, float* S1, float* S2, int64_t n, double* npart, float* norm,
                     hipStream_t s, const unsigned* abort_word, unsigned* skipped, bool census) {
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

void launch_target_lerp(float* pt, const float* p, int64_t n4, float tau, hipStream_t s) {
  hipLaunchKernelGGL(target_lerp, dim3(ceil_div(n4, 256)), dim3(256), 0, s, pt, p, n4, tau);
}

int permute_weight(int mode, const float* src, float* dst, hipStream_t s) {
  return pack_one(kPackPermute, src, nullptr, dst, mode, 0, kPermFloats[mode], s);
}

}  // namespace rela_amd

using namespace rela_amd;

// Test tap: trunk_backward on its own, with the activations and the masked d_a3 as inputs of the call.
// Everything the learners keep across steps (scratch, the permuted weight copies, the side lane) lives for this one call.
extern "C" int rela_debug_trunk_backward(int frames, int mode, int lanes, int fast_wgrad_min_frames, const uint8_t* obs,
                                         const float* a1, const float* a2, const float* d_a3, const float* conv2_w,
                                         const float* conv3_w, float* g_c1w, float* g_c1b, float* g_c2w, float* g_c2b,
                                         float* g_c3w, float* g_c3b, float* d_a2, float* d_a1, void* stream_) {
  RELA_CHECK(frames >= 1 && frames <= kTrunkMaxFrames && mode >= 0 && mode <= 2 && (lanes == 0 || lanes == 1), RELA_EINVAL,
             "rela_debug_trunk_backward: bad arguments (frames %d, mode %d, lanes %d)", frames, mode, lanes);
  RELA_CHECK(obs && a1 && a2 && d_a3 && conv2_w && conv3_w && g_c1w && g_c1b && g_c2w && g_c2b && g_c3w && g_c3b && d_a2 &&
                 d_a1,
             RELA_EINVAL, "rela_debug_trunk_backward: a pointer is NULL");
  hipStream_t s = (hipStream_t)stream_;
  TrunkTapScratch sc;
  const size_t cpart_floats = (size_t)kColsumBlocks * (32 + 512 + 64 + 64 + 32);  // as the learners size it
  float *w2p = nullptr, *w3p = nullptr;
  if (int rc = sc.mem.alloc(&w2p, kPermFloats[kPermConv2], false)) return rc;
  if (int rc = sc.mem.alloc(&w3p, kPermFloats[kPermConv3], false)) return rc;
  if (int rc = permute_weight(kPermConv2, conv2_w, w2p, s)) return rc;
  if (int rc = permute_weight(kPermConv3, conv3_w, w3p, s)) return rc;
  TrunkBwd t{};
  t.Bn = frames, t.obs = obs, t.a1 = a1, t.a2 = a2, t.d_a3 = d_a3, t.d_a2 = d_a2, t.d_a1 = d_a1;
  t.w2p = w2p, t.w3p = w3p;
  t.g_c1w = g_c1w, t.g_c1b = g_c1b, t.g_c2w = g_c2w, t.g_c2b = g_c2b, t.g_c3w = g_c3w, t.g_c3b = g_c3b;
  t.plan = plan_apex_backward(mode, lanes != 0)
               .trunk.plan(frames, fast_wgrad_min_frames > 0 ? fast_wgrad_min_frames : kFastWgradMinFrames);
  if (int rc = sc.mem.alloc(&t.part, kTrunkPartFloats, false)) return rc;
  if (int rc = sc.mem.alloc(&t.cpart, cpart_floats, false)) return rc;
  if (lanes) {  // as rela_apex_learner_grad fills it; else one lane, as the R2D2 learner (and RELA_LEARNER_LANES=1)
    RELA_HIP(hipStreamCreateWithFlags(&sc.side, hipStreamNonBlocking));
    for (hipEvent_t& e : sc.ev) RELA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    t.side = sc.side, t.ev_da3 = sc.ev[0], t.ev_da2 = sc.ev[1], t.ev_side = sc.ev[2];
    if (int rc = sc.mem.alloc(&t.part_side, kTrunkPartFloats, false)) return rc;
    if (int rc = sc.mem.alloc(&t.cpart_side, cpart_floats, false)) return rc;
    if (t.plan.dgrad_bf16) {  // the data-gradient weight fragments packed ahead, as the Ape-X learner's repack() does
      uint8_t *frag2 = nullptr, *frag3 = nullptr;
      if (int rc = sc.mem.alloc(&frag2, kFrag2Bytes, false)) return rc;
      if (int rc = sc.mem.alloc(&frag3, kFrag3Bytes, false)) return rc;
      pack_dgrad_frags(w2p, w3p, frag2, frag3, s);
      t.frag2 = frag2, t.frag3 = frag3;
    }
  }
  const int rc = trunk_backward(t, s);
  const hipError_t launched = hipGetLastError();
  // (the scratch goes away with `sc`: both lanes must be done with it whatever happened)
  const hipError_t done = hipStreamSynchronize(s);
  if (sc.side) (void)hipStreamSynchronize(sc.side);
  if (rc != RELA_OK) return rc;
  RELA_HIP(launched);
  RELA_HIP(done);
  return RELA_OK;
}

// Test tap: optimizer_apply itself on the caller's flat buffers: the norm, the clip coefficient and one
// RMSprop / Adam update.  The OptimState, the 256 partial sums, the abort word and the skip counter live for this one call.
// (`who`: rela_debug_optimizer_apply, whose options are OptimState's defaults, or rela_debug_optimizer_apply_opts)
static int debug_optimizer_apply(const char* who, const OptimState& options, int optimizer, float lr, float eps, float clip,
                                 int64_t adam_steps_done, int64_t n, float* p, const float* g, float* s1, float* s2,
                                 float* stats_out, int abort, unsigned* skipped_out, void* stream_) {
  RELA_CHECK((optimizer == 0 || optimizer == 1) && adam_steps_done >= 0 && n > 0 && n % 4 == 0 && (abort == 0 || abort == 1),
             RELA_EINVAL, "%s: bad arguments (optimizer %d, steps done %lld, n %lld, abort %d)", who, optimizer,
             (long long)adam_steps_done, (long long)n, abort);
  RELA_CHECK(p && g && s1 && s2 && stats_out, RELA_EINVAL, "%s: a pointer is NULL", who);
  for (const void* b : {(const void*)p, (const void*)g, (const void*)s1, (const void*)s2})
    RELA_CHECK(((uintptr_t)b & 15) == 0, RELA_EINVAL, "%s: a buffer is not 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream_;
  struct Scratch {
    DevBuffers mem;
    ~Scratch() { mem.free_all(); }
  } sc;
  double* npart = nullptr;
  unsigned* words = nullptr;  // [0] the abort word, [1] the skip counter
  if (int rc = sc.mem.alloc(&npart, kNormBlocks, false)) return rc;
  if (int rc = sc.mem.alloc(&words, 2, true)) return rc;
  if (abort) RELA_HIP(hipMemsetD32Async((hipDeviceptr_t)words, 1, 1, s));
  OptimState o = options;
  o.optimizer = optimizer, o.lr = lr, o.eps = eps, o.clip = clip, o.adam_t = adam_steps_done;
  optimizer_apply(o, p, g, s1, s2, n, npart, stats_out, s, words, words + 1, true);
  const hipError_t launched = hipGetLastError();
  const hipError_t done = hipStreamSynchronize(s);  // (the scratch goes away with `sc`)
  RELA_HIP(launched);
  RELA_HIP(done);
  if (skipped_out) RELA_HIP(hipMemcpy(skipped_out, words + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  return RELA_OK;
}

extern "C" int rela_debug_optimizer_apply(int optimizer, float lr, float eps, float clip, int64_t adam_steps_done, int64_t n,
                                          float* p, const float* g, float* s1, float* s2, float* stats_out, int abort,
                                          unsigned* skipped_out, void* stream_) {
  return debug_optimizer_apply("rela_debug_optimizer_apply", OptimState(), optimizer, lr, eps, clip, adam_steps_done, n, p, g,
                               s1, s2, stats_out, abort, skipped_out, stream_);
}

// Test tap: as rela_debug_optimizer_apply, with the options of rela_*_learner_set_rmsprop / _set_adam_betas
extern "C" int rela_debug_optimizer_apply_opts(int optimizer, float lr, float eps, float clip, int64_t adam_steps_done,
                                               int64_t n, float* p, const float* g, float* s1, float* s2, float* stats_out,
                                               int abort, unsigned* skipped_out, float alpha, int centered, float b1, float b2,
                                               void* stream_) {
  RELA_CHECK(rmsprop_options_ok(alpha, centered) && adam_betas_ok(b1, b2), RELA_EINVAL,
             "rela_debug_optimizer_apply_opts: bad options (alpha %g, centered %d, betas %g / %g)", (double)alpha, centered,
             (double)b1, (double)b2);
  OptimState options;
  options.alpha = alpha, options.centered = centered != 0, options.b1 = b1, options.b2 = b2;
  return debug_optimizer_apply("rela_debug_optimizer_apply_opts", options, optimizer, lr, eps, clip, adam_steps_done, n, p, g,
                               s1, s2, stats_out, abort, skipped_out, stream_);
}

// Test tap: target_lerp, the kernel of rela_*_learner_soft_update_target, on the caller's flat buffers
extern "C" int rela_debug_target_lerp(int64_t n, float tau, float* pt, const float* p, void* stream_) {
  RELA_CHECK(n > 0 && n % 4 == 0 && tau > 0.f && tau <= 1.f, RELA_EINVAL, "rela_debug_target_lerp: bad arguments (n %lld, tau %g)",
             (long long)n, (double)tau);
  RELA_CHECK(pt && p, RELA_EINVAL, "rela_debug_target_lerp: a pointer is NULL");
  RELA_CHECK((((uintptr_t)pt | (uintptr_t)p) & 15) == 0, RELA_EINVAL, "rela_debug_target_lerp: a buffer is not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream_;
  note_launch("target_lerp");
  launch_target_lerp(pt, p, n / 4, tau, s);
  const hipError_t launched = hipGetLastError();
  const hipError_t done = hipStreamSynchronize(s);
  RELA_HIP(launched);
  RELA_HIP(done);
  return RELA_OK;
}
