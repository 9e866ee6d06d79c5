// conv_f32.h -- the conv trunk of the exact f32 mode (kTrunkF32): conv1_bf16x3, conv_mfma / conv_mfma_bstat<Conv2 | Conv3>.
// Included by ffnet.hip only: the kernels live in rela_amd::(anonymous).
//
// s u8[N,4,84,84] -> conv 8x8s4 (4->32) -> conv 4x4s2 (32->64) -> conv 3x3s1 (64->64)
//   -> fc 3136->512 -> {fc_v 512->1, fc_a 512->A} -> dueling (net.py:33-39).
// 9,352,704 MAC = 18.7 MFLOP per sample: MFMA-bound, not HBM-bound
// (660 FLOP per input byte), so every contraction runs on the matrix cores in exact fp32:
// v_mfma_f32_16x16x4_f32 is bit-for-bit a k-ordered fmaf chain (guide: FP32-input MFMA), which
// keeps Q-values within fp32 round-off of the reference (tests use 1e-4 abs+rel).
//
// Formulation: implicit GEMM  Out[m = (sample, oy, ox)][n = out channel] = sum_k A[m][k] W[k][n]
//   MFMA A operand = im2col row, read straight out of an LDS copy of the input tile
//                    (no im2col matrix is ever materialised); lane (i = l&15, kk = l>>4)
//                    supplies A[row i][k0 + kk],
//   MFMA B operand = weights, pre-packed at load time in FRAGMENT ORDER
//                    Bfrag[(col_tile*KS + kstep)*64 + lane] so a wavefront's B load is one
//                    coalesced 256-byte read that stays L2-resident,
//   accumulators   = 16x16 tiles, 4 VGPRs each; one wave owns one 16-channel column tile
//                    and several row tiles, so each B fragment is reused across all of them.
// Activations are channel-last f32 ([N][pos][C]) between layers; fc weights are permuted
// at load time to match (k = pos*64 + c instead of torch's c*49 + pos).  LDS pixel strides
// are padded (33 / 66 floats) so the 16 rows of a fragment hit distinct banks.
// conv1 is special: its inputs are u8 frames, which are EXACT in bf16, and an fp32 weight is
// exactly the sum of three bf16 pieces (24-bit significand = 3 x 8).  So conv1 runs on
// v_mfma_f32_16x16x32_bf16 (16x the fp32 MFMA rate) as three passes hi/mid/lo with fp32
// accumulation: every product is exact and the result is fp32-accurate, while the layer drops
// from MFMA-bound to HBM-bound (28 KB in + 51 KB out per sample).  The /255 of net.py:46 is
// folded into conv1's weights at load time.  The dense layers of this mode are in gemm_f32.h.
#pragma once
#include "ffnet_kern.h"
#include "prof.h"

namespace rela_amd {
namespace {

template <int CIN_, int IH_, int IW_, int KH_, int KW_, int STRIDE_, int OH_, int OW_, int OC_, int S_, bool U8_>
struct ConvCfg {
  static constexpr int CIN = CIN_, IH = IH_, IW = IW_, KH = KH_, KW = KW_, STRIDE = STRIDE_, OH = OH_, OW = OW_,
                       OC = OC_, S = S_;
  static constexpr bool U8 = U8_;
  static constexpr int P = OH * OW;
  static constexpr int M = S * P;
  static constexpr int RT = (M + 15) / 16;
  static constexpr int CT = OC / 16;
  static constexpr int RG = kWaves / CT;
  static constexpr int RPW = (RT + RG - 1) / RG;
  static constexpr int K = CIN * KH * KW;
  static constexpr int KS = K / 4;
  // LDS image of one f32 sample: pixel stride PIX floats, row stride ROW, sample stride SAMP, padded
  // so that the dword address of output position p (flattened over the samples of the block) is
  // 2*p + const (mod 32): the 16 rows x 2 k-lanes of a ds_read_b32 group then hit 32 distinct banks.
  //   STRIDE*PIX = 2 (mod 32);  STRIDE*ROW = 2*OW (mod 32);  SAMP = 2*OH*OW (mod 32)
  static constexpr int PIX = U8 ? 0 : (CIN + (STRIDE == 2 ? 1 : 2));  // floats per LDS pixel
  static constexpr int ROW_RAW = IW * PIX;
  static constexpr int ROW_NEED = STRIDE == 2 ? OW : 2 * OW;            // ROW mod (STRIDE == 2 ? 16 : 32)
  static constexpr int ROW_MOD = STRIDE == 2 ? 16 : 32;
  static constexpr int ROW = U8 ? 0 : ROW_RAW + ((ROW_NEED - ROW_RAW % ROW_MOD) % ROW_MOD + ROW_MOD) % ROW_MOD;
  static constexpr int SAMP_RAW = IH * ROW;
  static constexpr int SAMP = U8 ? 0 : SAMP_RAW + ((2 * OH * OW - SAMP_RAW) % 32 + 32) % 32;
  static constexpr int IN_ELEMS = CIN * IH * IW;                        // per sample
  static constexpr int LDS_BYTES = U8 ? S * IN_ELEMS : S * SAMP * 4;
  static constexpr bool BSTAT = !U8 && K / 4 <= 128;  // weight column tile fits the register budget
};

// Samples per block: conv2 keeps ONE sample resident (53 KB of LDS -> 3 blocks per CU, so one block's
// staging phase overlaps the others' MFMA phase; measured 458 -> 388 us per 6400 against S = 2 despite
// 81 -> 96 row padding); conv3 keeps four (S = 2 measured the same).
using Conv2 = ConvCfg<32, 20, 20, 4, 4, 2, 9, 9, 64, 1, false>;
using Conv3 = ConvCfg<64, 9, 9, 3, 3, 1, 7, 7, 64, 3, false>;

template <class C>
__global__ __launch_bounds__(kThreads) void conv_mfma(const void* __restrict__ in_, const float* __restrict__ Bfrag,
                                                      const float* __restrict__ bias, float* __restrict__ out,
                                                      int N) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * C::S;
  const int ns = min(C::S, N - n0);

  // ---- stage the input tile of S samples in LDS -----------------------------------------
  if constexpr (C::U8) {
    const uint4* src = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(in_) + (size_t)n0 * C::IN_ELEMS);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    constexpr int per = C::IN_ELEMS / 16;
    // all loads of the tile in flight before the first LDS write (one HBM round trip, not IT)
    constexpr int IT = (C::S * per + kThreads - 1) / kThreads;
    uint4 v[IT];
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int i = tid + j * kThreads;
      v[j] = (i < ns * per) ? src[i] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int i = tid + j * kThreads;
      if (i < C::S * per) dst[i] = v[j];
    }
  } else {
    const float4* src = reinterpret_cast<const float4*>(static_cast<const float*>(in_) + (size_t)n0 * C::IN_ELEMS);
    float* dst = reinterpret_cast<float*>(smem);
    constexpr int cq_n = C::CIN / 4;
    constexpr int per = C::IN_ELEMS / 4;
    // all loads of the tile in flight before the first LDS write (one HBM round trip, not IT)
    constexpr int IT = (C::S * per + kThreads - 1) / kThreads;
    float4 v[IT];
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int i = tid + j * kThreads;
      v[j] = (i < ns * per) ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int i = tid + j * kThreads;
      if (i < C::S * per) {
        const int pixel = i / cq_n, cq = i - pixel * cq_n;
        const int smp = pixel / (C::IH * C::IW), pin = pixel - smp * (C::IH * C::IW);
        const int y = pin / C::IW, x = pin - y * C::IW;
        float* d = dst + smp * C::SAMP + y * C::ROW + x * C::PIX + cq * 4;
        d[0] = v[j].x;
        d[1] = v[j].y;
        d[2] = v[j].z;
        d[3] = v[j].w;
      }
    }
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int ct = wave % C::CT, rg = wave / C::CT;
  const int li = lane & 15, kk = lane >> 4;

  int abase[C::RPW];
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) {
    const int m = (rg + t * C::RG) * 16 + li;
    const int mm = (m < C::M) ? m : 0;
    const int s = mm / C::P, pos = mm - s * C::P;
    const int oy = pos / C::OW, ox = pos - oy * C::OW;
    if constexpr (C::U8)
      abase[t] = s * C::IN_ELEMS + oy * C::STRIDE * C::IW + ox * C::STRIDE + kk;
    else
      abase[t] = (s * C::SAMP + oy * C::STRIDE * C::ROW + ox * C::STRIDE * C::PIX + kk) * 4;
  }

  f32x4 acc[C::RPW];
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* bptr = Bfrag + (size_t)ct * C::KS * 64 + lane;

  if constexpr (C::U8) {
    // k = (c, kh, kw), kw fastest: one k-step = 4 consecutive bytes of one input row
    for (int c = 0; c < C::CIN; ++c) {
#pragma unroll 2
      for (int kh = 0; kh < C::KH; ++kh) {
#pragma unroll
        for (int q = 0; q < C::KW / 4; ++q) {
          const int ks = (c * C::KH + kh) * (C::KW / 4) + q;
          const int koff = c * C::IH * C::IW + kh * C::IW + q * 4;
          const float b = bptr[(size_t)ks * 64];
#pragma unroll
          for (int t = 0; t < C::RPW; ++t) {
            const float a = (float)smem[abase[t] + koff];
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
          }
        }
      }
    }
  } else {
    // k = (kh, kw, c), c fastest: one k-step = 4 consecutive channels of one input pixel.
    // The B fragments of one (kh, kw) chunk are fetched (L2) a whole chunk ahead of their use.
    constexpr int CQ = C::CIN / 4, NCH = C::KH * C::KW;
    float bcur[CQ], bnext[CQ];
#pragma unroll
    for (int cq = 0; cq < CQ; ++cq) bcur[cq] = bptr[(size_t)cq * 64];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int kh = ch / C::KW, kw = ch - kh * C::KW;
      if (ch + 1 < NCH) {
#pragma unroll
        for (int cq = 0; cq < CQ; ++cq) bnext[cq] = bptr[(size_t)((ch + 1) * CQ + cq) * 64];
      }
#pragma unroll
      for (int cq = 0; cq < CQ; ++cq) {
        const int koff = (kh * C::ROW + kw * C::PIX + cq * 4) * 4;
#pragma unroll
        for (int t = 0; t < C::RPW; ++t) {
          const float a = *reinterpret_cast<const float*>(smem + abase[t] + koff);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bcur[cq], acc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int cq = 0; cq < CQ; ++cq) bcur[cq] = bnext[cq];
    }
  }

  // ---- epilogue: bias + ReLU, channel-last store ------------------------------------------
  const int col = ct * 16 + li;
  const float bv = bias[col];
  const int mlim = ns * C::P;
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) {
    const int rt = rg + t * C::RG;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = rt * 16 + kk * 4 + r;
      if (m < mlim) {
        const float v = acc[t][r] + bv;
        out[((size_t)n0 * C::P + m) * C::OC + col] = v > 0.f ? v : 0.f;
      }
    }
  }
}

// ---- B-stationary persistent variant for large batches -------------------------------------
// Ablation of conv_mfma at N = 6400 (conv2: 372 us with, 306 us without the per-k-step B-fragment
// loads) shows the weight fetches, not the LDS reads or the tile staging, stall the MFMA stream.
// One column tile of the weights is K x 16 floats = KS registers per lane (128 / 144), so here
// every wave keeps ITS column tile in registers for the whole launch and the block (one per CU,
// 2 waves per SIMD) walks over its share of the samples with a double-buffered LDS input tile:
// the global loads of group g+1 are issued before the k-loop of group g and written to the other
// buffer halfway through it.  The k-loop then touches only LDS (A) and registers (B).
template <class C>
__global__ __launch_bounds__(kThreads) void conv_mfma_bstat(const float* __restrict__ in,
                                                            const float* __restrict__ Bfrag,
                                                            const float* __restrict__ bias,
                                                            float* __restrict__ out, int N) {
  static_assert(!C::U8, "f32 channel-last input only");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int ct = wave % C::CT, rg = wave / C::CT;
  const int li = lane & 15, kk = lane >> 4;
  const int ngroups = (N + C::S - 1) / C::S;

  float breg[C::KS];
  {
    const float* bptr = Bfrag + (size_t)ct * C::KS * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) breg[ks] = bptr[(size_t)ks * 64];
  }

  int abase[C::RPW];
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) {
    const int m = (rg + t * C::RG) * 16 + li;
    const int mm = (m < C::M) ? m : 0;
    const int sm = mm / C::P, pos = mm - sm * C::P;
    const int oy = pos / C::OW, ox = pos - oy * C::OW;
    abase[t] = (sm * C::SAMP + oy * C::STRIDE * C::ROW + ox * C::STRIDE * C::PIX + kk) * 4;
  }
  const int col = ct * 16 + li;
  const float bv = bias[col];

  // staging in two phases of IT2 float4 per thread (keeps the live set below 256 registers)
  constexpr int cq_n = C::CIN / 4;
  constexpr int per = C::IN_ELEMS / 4;
  constexpr int IT = (C::S * per + kThreads - 1) / kThreads;
  constexpr int IT2 = (IT + 1) / 2;
  float4 v[IT2];
  auto stage_load = [&](int g, int phase) {
    const int n0 = g * C::S;
    const int ns = min(C::S, N - n0);
    const float4* src = reinterpret_cast<const float4*>(in + (size_t)n0 * C::IN_ELEMS);
#pragma unroll
    for (int j = 0; j < IT2; ++j) {
      const int i = tid + (phase * IT2 + j) * kThreads;
      v[j] = (i < ns * per) ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stage_store = [&](int buf, int phase) {
    float* dst = reinterpret_cast<float*>(smem + buf * C::LDS_BYTES);
#pragma unroll
    for (int j = 0; j < IT2; ++j) {
      const int i = tid + (phase * IT2 + j) * kThreads;
      if (i < C::S * per) {
        const int pixel = i / cq_n, cq = i - pixel * cq_n;
        const int sm = pixel / (C::IH * C::IW), pin = pixel - sm * (C::IH * C::IW);
        const int y = pin / C::IW, x = pin - y * C::IW;
        float* d = dst + sm * C::SAMP + y * C::ROW + x * C::PIX + cq * 4;
        d[0] = v[j].x;
        d[1] = v[j].y;
        d[2] = v[j].z;
        d[3] = v[j].w;
      }
    }
  };

  int g = blockIdx.x;
  if (g >= ngroups) return;
  stage_load(g, 0);
  stage_store(0, 0);
  stage_load(g, 1);
  stage_store(0, 1);
  __syncthreads();
  int buf = 0;
  constexpr int CQ = C::CIN / 4, NCH = C::KH * C::KW;
  for (; g < ngroups; g += gridDim.x) {
    const bool has_next = g + (int)gridDim.x < ngroups;
    if (has_next) stage_load(g + gridDim.x, 0);
    const uint8_t* tile = smem + buf * C::LDS_BYTES;
    f32x4 acc[C::RPW];
#pragma unroll
    for (int t = 0; t < C::RPW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int kh = ch / C::KW, kw = ch - kh * C::KW;
#pragma unroll
      for (int cq = 0; cq < CQ; ++cq) {
        const int koff = (kh * C::ROW + kw * C::PIX + cq * 4) * 4;
#pragma unroll
        for (int t = 0; t < C::RPW; ++t) {
          const float a = *reinterpret_cast<const float*>(tile + abase[t] + koff);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, breg[ch * CQ + cq], acc[t], 0, 0, 0);
        }
      }
      // the other buffer was last read one group ago (barrier since): fill it while this group computes
      if (has_next) {
        if (ch == NCH / 3) {
          stage_store(buf ^ 1, 0);
          stage_load(g + gridDim.x, 1);
        } else if (ch == (2 * NCH) / 3) {
          stage_store(buf ^ 1, 1);
        }
      }
    }
    const int n0 = g * C::S;
    const int mlim = min(C::S, N - n0) * C::P;
#pragma unroll
    for (int t = 0; t < C::RPW; ++t) {
      const int rt = rg + t * C::RG;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = rt * 16 + kk * 4 + r;
        if (m < mlim) {
          const float o = acc[t][r] + bv;
          out[((size_t)n0 * C::P + m) * C::OC + col] = o > 0.f ? o : 0.f;
        }
      }
    }
    __syncthreads();
    buf ^= 1;
  }
}

// Picks the B-stationary kernel once every CU gets at least two sample groups.  conv3 stays on
// conv_mfma: its 144 + 20 accumulator registers spill under the 256-register budget and with one
// block per CU the 2134 groups of N = 6400 quantise to 9 rounds (measured 259 us against 227 us).
// Splitting K over two wave groups (72 weight registers + 40 accumulators per wave, halves summed
// through LDS) removes the spills of the hot loop but measured 318 us: with one block per CU two
// waves per SIMD do not hide the LDS latency of ten row tiles.  Tried and dropped in round 1.
template <class C>
void launch_conv(const float* in, const float* Bfrag, const float* bias, float* out, int N, hipStream_t s) {
  const int ngroups = ceil_div(N, C::S);
  note_launch(C::K == 512 ? "conv_mfma<Conv2> (f32)" : "conv_mfma<Conv3> (f32)");
  if (C::BSTAT && ngroups >= 2 * kNumCU)
    hipLaunchKernelGGL(conv_mfma_bstat<C>, dim3(kNumCU), dim3(kThreads), 2 * C::LDS_BYTES, s, in, Bfrag, bias, out, N);
  else
    hipLaunchKernelGGL(conv_mfma<C>, dim3(ngroups), dim3(kThreads), C::LDS_BYTES, s, (const void*)in, Bfrag, bias,
                       out, N);
}

// ---- conv1 on bf16 MFMA, exact-weight split ------------------------------------------------
struct Conv1B {
  static constexpr int S = 2, P = 400, M = S * P, RT = M / 16, OC = 32, CT = 2, KS = 8;
  static constexpr int RPW = (RT + kWaves - 1) / kWaves;  // 7 row tiles per wave (last ones masked)
  static constexpr int IN_ELEMS = 4 * 84 * 84;
  static constexpr int LDS_BYTES = S * IN_ELEMS;
  static constexpr int FRAG_UINT4 = 3 * CT * KS * 64;  // [piece][ct][ks][lane] x 8 bf16
};

// 8 consecutive input bytes -> 8 bf16 (exact): v_cvt_f32_ubyteN + v_perm_b32 taking the high halves
__device__ __forceinline__ uint4 u8x8_to_bf16x8(uint32_t d0, uint32_t d1) {
  auto pk = [](uint32_t d, int lo) -> uint32_t {
    const float f0 = (float)((d >> (8 * lo)) & 0xff), f1 = (float)((d >> (8 * lo + 8)) & 0xff);
    return __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
  };
  return make_uint4(pk(d0, 0), pk(d0, 2), pk(d1, 0), pk(d1, 2));
}

__global__ __launch_bounds__(kThreads) void conv1_bf16x3(const uint8_t* __restrict__ in,
                                                         const uint4* __restrict__ Bfrag,
                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                         int N) {
  using C = Conv1B;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x;
  const int n0 = blockIdx.x * C::S;
  const int ns = min(C::S, N - n0);
  {
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)n0 * C::IN_ELEMS);
    uint4* dst = reinterpret_cast<uint4*>(smem);
    constexpr int per = C::IN_ELEMS / 16;
    // all loads of the tile in flight before the first LDS write (one HBM round trip, not IT)
    constexpr int IT = (C::S * per + kThreads - 1) / kThreads;
    uint4 v[IT];
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int i = tid + j * kThreads;
      v[j] = (i < ns * per) ? src[i] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < IT; ++j) {
      const int i = tid + j * kThreads;
      if (i < C::S * per) dst[i] = v[j];
    }
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;

  // k = (c, kh, kw): a k-step of 32 = 4 kernel rows x 8 columns of one channel; lane group g
  // owns kernel row 4*(ks&1) + g, its 8 k's are 8 CONSECUTIVE input bytes (4-byte aligned).
  int abase[C::RPW];
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) {
    const int rt = wave + t * kWaves;
    const int m = ((rt < C::RT) ? rt : 0) * 16 + li;
    const int s = m / C::P, pos = m - s * C::P;
    const int oy = pos / 20, ox = pos - oy * 20;
    abase[t] = s * C::IN_ELEMS + (4 * oy + g) * 84 + 4 * ox;
  }
  f32x4 acc[C::RPW][C::CT];
#pragma unroll
  for (int t = 0; t < C::RPW; ++t)
#pragma unroll
    for (int c = 0; c < C::CT; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Tried in round 1 without gain (157 us either way): a register double buffer for the weight fragments
  // (146 VGPRs: loses the second block per CU, 206 us) and staging them per k-step through LDS.  The kernel
  // moves 511 MB per 6,400 samples (3.2 TB/s), most of it the f32 output in 64-byte partial rows.
  // A persistent weight-stationary form (96 weight registers + 52 accumulators per wave, double-buffered
  // u8 tile) spills under the 256-register budget and measured 357-431 us.
#pragma unroll 1
  for (int ks = 0; ks < C::KS; ++ks) {
    const int koff = (ks >> 1) * 84 * 84 + (ks & 1) * 4 * 84;
    bf16x8 b[3][C::CT];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int c = 0; c < C::CT; ++c)
        b[p][c] = __builtin_bit_cast(bf16x8, Bfrag[((p * C::CT + c) * C::KS + ks) * 64 + lane]);
#pragma unroll
    for (int t = 0; t < C::RPW; ++t) {
      const uint32_t* ap = reinterpret_cast<const uint32_t*>(smem + abase[t] + koff);
      const bf16x8 a = __builtin_bit_cast(bf16x8, u8x8_to_bf16x8(ap[0], ap[1]));
#pragma unroll
      for (int c = 0; c < C::CT; ++c) {
        // smallest piece first so the big one is added last.  Operands swapped (weights as the MFMA's A operand): a
        // lane ends up with FOUR CONSECUTIVE CHANNELS of one pixel -- one 16-byte store where the pixel-major tile
        // took four 4-byte ones (r4: the f32 output is two thirds of this kernel's HBM bytes)
        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[2][c], a, acc[t][c], 0, 0, 0);
        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[1][c], a, acc[t][c], 0, 0, 0);
        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[0][c], a, acc[t][c], 0, 0, 0);
      }
    }
  }

  const int mlim = ns * C::P;
#pragma unroll
  for (int t = 0; t < C::RPW; ++t) {
    const int rt = wave + t * kWaves;
    if (rt >= C::RT) continue;
    const int m = rt * 16 + li;  // this lane's pixel; its channels: 16 c + 4 g .. + 3
    if (m >= mlim) continue;
#pragma unroll
    for (int c = 0; c < C::CT; ++c) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c * 16 + 4 * g);
      f32x4 v = acc[t][c] + bv;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.f;
      *reinterpret_cast<f32x4*>(out + ((size_t)n0 * C::P + m) * C::OC + c * 16 + 4 * g) = v;
    }
  }
}

inline void launch_conv1_bf16x3(const uint8_t* frames, const uint4* B1, const float* b1, float* a1, int N, hipStream_t s) {
  note_launch("conv1_bf16x3");
  hipLaunchKernelGGL(conv1_bf16x3, dim3(ceil_div(N, Conv1B::S)), dim3(kThreads), Conv1B::LDS_BYTES, s, frames, B1, b1, a1, N);
}

inline int opt_in_lds_conv_f32() {
  const LdsOptIn ks[] = {
      {reinterpret_cast<const void*>(&conv1_bf16x3), Conv1B::LDS_BYTES},
      {reinterpret_cast<const void*>(&conv_mfma<Conv2>), Conv2::LDS_BYTES},
      {reinterpret_cast<const void*>(&conv_mfma<Conv3>), Conv3::LDS_BYTES},
      {reinterpret_cast<const void*>(&conv_mfma_bstat<Conv2>), 2 * Conv2::LDS_BYTES},
      {reinterpret_cast<const void*>(&conv_mfma_bstat<Conv3>), 2 * Conv3::LDS_BYTES},
  };
  return opt_in(ks);
}

}  // namespace
}  // namespace rela_amd
