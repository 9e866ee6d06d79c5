// gemm_f32.h -- the dense layers of the exact f32 mode on v_mfma_f32_16x16x4_f32: gemm_mfma (fc, the LSTM gates with the
// fused cell, the AtariLSTMNet's heads), dueling_kernel, the small-batch fc as a split-K gemm_lds, and fc_reduce.
// Included by ffnet.hip only: the kernels live in rela_amd::(anonymous).  The tiling is conv_f32.h's.
#pragma once
#include "ffnet_kern.h"
#include "gemm_lds.h"
#include "prof.h"

namespace rela_amd {
namespace {

// Dense layer  out[N][OC] = act(A[N][K] * W + bias)  on the same MFMA tiling.
// Block = BM rows x (CTB*16) columns; A is staged through LDS in K-chunks of 32 (double
// buffered, row stride 34 floats -> conflict-free fragment reads), B fragments stream from L2.
enum GemmEpilogue { kEpiBias = 0, kEpiBiasRelu = 1, kEpiLstmCell = 2 };

// K1_ = leading part of K that comes from the first A matrix ([N][K1]); the rest comes from a
// second matrix ([N][K-K1]) -- the LSTM gate GEMM reads [conv features | previous h].
// KSS / KSO: k-steps per column tile of the fragment array and the first one this GEMM uses (a GEMM over a k-range of a
// larger packed operand); INIT: the accumulators start from a [N][OC] tensor passed in A2's place
template <int K_, int OC_, int BM_, int EPI_, int K1_ = K_, int KSS_ = K_ / 4, int KSO_ = 0, bool INIT_ = false>
struct GemmCfg {
  static constexpr int K = K_, OC = OC_, BM = BM_, EPI = EPI_, K1 = K1_, KSS = KSS_, KSO = KSO_;
  static constexpr bool INIT = INIT_;
  static constexpr bool RELU = EPI_ == kEpiBiasRelu;
  static constexpr int CT = OC / 16;
  static constexpr int CTB = CT < kWaves ? CT : kWaves;  // column tiles per block
  static constexpr int RGB = kWaves / CTB;               // row groups per block
  static constexpr int RT = BM / 16;
  static constexpr int RPW = RT / RGB;
  static constexpr int KC = 32;
  static constexpr int NCH = K / KC;
  static constexpr int KS = K / 4;
  static constexpr int LDA = 34;
  static constexpr int V4 = BM * KC / 4;                       // float4 per chunk
  static constexpr int VPT = (V4 + kThreads - 1) / kThreads;  // per thread (the last one may be partial)
};

// Block height is picked per launch (launch_gemm_bm below): 400 half-height fc blocks at N = 6400 sit
// two-deep on 144 CUs and one-deep on 112; 232 blocks of 112 rows fill one round.
using GemmFc = GemmCfg<3136, 512, 64, kEpiBiasRelu>;
using GemmFc112 = GemmCfg<3136, 512, 112, kEpiBiasRelu>;
using GemmHeads = GemmCfg<512, 32, 128, kEpiBias>;
// LSTM gates: [x(3136) | h(512)] x [3648][2048]; columns permuted to 4*unit + gate (i,f,g,o) so the
// four gates of a hidden unit sit in four adjacent lanes of one accumulator tile.
using GemmLstm = GemmCfg<3648, 2048, 128, kEpiLstmCell, 3136>;
using GemmLstm112 = GemmCfg<3648, 2048, 112, kEpiLstmCell, 3136>;
// bf16x2 mode of the actors' LSTM step: the x part of the gates comes from the split-bf16 GEMM (gemm_bf16s.h) and
// this GEMM adds h x W_hh (k-steps 784 .. 911 of the same fragment array) and runs the cell
using GemmLstmH = GemmCfg<512, 2048, 128, kEpiLstmCell, 512, 912, 784, true>;
using GemmLstmH112 = GemmCfg<512, 2048, 112, kEpiLstmCell, 512, 912, 784, true>;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

template <class G>
__global__ __launch_bounds__(kThreads) void gemm_mfma(const float* __restrict__ A, const float* __restrict__ A2,
                                                      const float* __restrict__ Bfrag,
                                                      const float* __restrict__ bias, float* __restrict__ out,
                                                      const float* __restrict__ c_in, float* __restrict__ c_out,
                                                      int N) {
  __shared__ __attribute__((aligned(16))) float sA[2][G::BM * G::LDA];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kk = lane >> 4;
  const int ctw = wave % G::CTB, rg = wave / G::CTB;
  const int ct = blockIdx.x * G::CTB + ctw;
  const int row0 = blockIdx.y * G::BM;

  float4 stage[G::VPT];
  auto load_chunk = [&](int ch) {
#pragma unroll
    for (int v = 0; v < G::VPT; ++v) {
      const int idx = tid + v * kThreads;
      if (G::V4 % kThreads != 0 && idx >= G::V4) break;
      const int r = idx >> 3, q = idx & 7;  // KC/4 == 8 float4 per row
      const int row = row0 + r;
      const int k = ch * G::KC + q * 4;
      const float* src = (G::K1 == G::K || k < G::K1) ? A + (size_t)row * G::K1 + k
                                                        : A2 + (size_t)row * (G::K - G::K1) + (k - G::K1);
      stage[v] = (row < N) ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int v = 0; v < G::VPT; ++v) {
      const int idx = tid + v * kThreads;
      if (G::V4 % kThreads != 0 && idx >= G::V4) break;
      const int r = idx >> 3, q = idx & 7;
      float* d = &sA[buf][r * G::LDA + q * 4];
      *reinterpret_cast<float2*>(d) = make_float2(stage[v].x, stage[v].y);
      *reinterpret_cast<float2*>(d + 2) = make_float2(stage[v].z, stage[v].w);
    }
  };

  f32x4 acc[G::RPW];
#pragma unroll
  for (int t = 0; t < G::RPW; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (G::INIT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + (rg * G::RPW + t) * 16 + kk * 4 + r;
        if (row < N) acc[t][r] = A2[(size_t)row * G::OC + blockIdx.x * G::CTB * 16 + ctw * 16 + li];
      }
    }
  }

  const float* bptr = Bfrag + ((size_t)ct * G::KSS + G::KSO) * 64 + lane;

  load_chunk(0);
  store_chunk(0);
  // B fragments stream from L2 one K-chunk AHEAD of their use (register double buffer), so the
  // MFMAs of a chunk never wait on the fragment loads issued in the same chunk
  float bnext[G::KC / 4];
#pragma unroll
  for (int j = 0; j < G::KC / 4; ++j) bnext[j] = bptr[(size_t)j * 64];
  __syncthreads();
  for (int ch = 0; ch < G::NCH; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < G::NCH) load_chunk(ch + 1);
    float bfr[G::KC / 4];
#pragma unroll
    for (int j = 0; j < G::KC / 4; ++j) bfr[j] = bnext[j];
    if (ch + 1 < G::NCH) {
#pragma unroll
      for (int j = 0; j < G::KC / 4; ++j) bnext[j] = bptr[(size_t)((ch + 1) * (G::KC / 4) + j) * 64];
    }
#pragma unroll
    for (int j = 0; j < G::KC / 4; ++j) {
#pragma unroll
      for (int t = 0; t < G::RPW; ++t) {
        const int r = (rg * G::RPW + t) * 16 + li;
        const float a = sA[buf][r * G::LDA + j * 4 + kk];
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bfr[j], acc[t], 0, 0, 0);
      }
    }
    if (ch + 1 < G::NCH) store_chunk(buf ^ 1);
    __syncthreads();
  }

  const int col = ct * 16 + li;
  const float bv = bias[col];
#pragma unroll
  for (int t = 0; t < G::RPW; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + (rg * G::RPW + t) * 16 + kk * 4 + r;
      if constexpr (G::EPI == kEpiLstmCell) {
        // torch LSTM cell (gate order i,f,g,o): c' = sig(f)*c + sig(i)*tanh(g); h' = sig(o)*tanh(c')
        const float pre = acc[t][r] + bv;
        const int base = lane & ~3;
        const float gi = __shfl(pre, base + 0, 64), gf = __shfl(pre, base + 1, 64);
        const float gg = __shfl(pre, base + 2, 64), go = __shfl(pre, base + 3, 64);
        if ((li & 3) == 0 && row < N) {
          const int unit = col >> 2;
          const float cp = c_in[(size_t)row * (G::OC / 4) + unit];
          const float c = sigmoidf_(gf) * cp + sigmoidf_(gi) * tanhf(gg);
          c_out[(size_t)row * (G::OC / 4) + unit] = c;
          out[(size_t)row * (G::OC / 4) + unit] = sigmoidf_(go) * tanhf(c);
        }
      } else if (row < N) {
        float v = acc[t][r] + bv;
        if (G::RELU) v = v > 0.f ? v : 0.f;
        out[(size_t)row * G::OC + col] = v;
      }
    }
  }
}

// gemm_mfma block height: makespan estimate = rounds over the CUs x rows per block; 112-row blocks win
// when they save a round (fc at N = 6400: 232 blocks in one round instead of 400 in two)
inline bool prefer_bm112(int N, int colgroups, int bm_default) {
  auto cost = [&](int bm) {
    const int64_t blocks = (int64_t)ceil_div(N, bm) * colgroups;
    return ((blocks + kNumCU - 1) / kNumCU) * bm;
  };
  return cost(112) < cost(bm_default);
}

// gemm_mfma with the block height prefer_bm112 picks; census: the launch-census name of G
template <class G, class G112>
void launch_gemm_bm(const char* census, const float* A, const float* A2, const float* Bfrag, const float* bias, float* out,
                    const float* c_in, float* c_out, int N, hipStream_t s) {
  note_launch(census);
  if (prefer_bm112(N, G::CT / G::CTB, G::BM))
    hipLaunchKernelGGL(gemm_mfma<G112>, dim3(G112::CT / G112::CTB, ceil_div(N, G112::BM)), dim3(kThreads), 0, s, A, A2,
                       Bfrag, bias, out, c_in, c_out, N);
  else
    hipLaunchKernelGGL(gemm_mfma<G>, dim3(G::CT / G::CTB, ceil_div(N, G::BM)), dim3(kThreads), 0, s, A, A2, Bfrag, bias,
                       out, c_in, c_out, N);
}

// ---- fc forward for small batches (kFcSplitBelow, fc_splits: ffnet_plan.h) ------------------------------------------
using TileFcSmall = gemm::TileCfg<128, 64, 4, 2, false>;
struct ProbFcFwd : gemm::ProbBase {
  const float *a3, *wt;  // a3 [N][3136] (k = pos*64+c), wt [3136][512]
  float* part;           // [splits][N][512]
  __device__ float4 fetchA(int m, int k) const { return gemm::ld4(a3 + (size_t)min(m, M - 1) * 3136 + k); }
  __device__ float4 fixA(float4 v, int m, int) const { return gemm::keep4(m < M, v); }
  __device__ float4 fetchB(int k, int n) const { return gemm::ld4(wt + (size_t)k * 512 + n); }
  __device__ void store(int z, int m, int n, float v) const { part[((size_t)z * M + m) * 512 + n] = v; }
};

// the split-K fcs of all three arithmetics end here
__global__ void fc_reduce(const float* __restrict__ part, int splits, int N, const float* __restrict__ bias,
                          float* __restrict__ h) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // one float4 of h
  if (idx >= N * 128) return;
  const int n4 = (idx & 127) * 4;
  const size_t off = (size_t)(idx >> 7) * 512 + n4;
  float4 s = *reinterpret_cast<const float4*>(bias + n4);
  for (int z = 0; z < splits; ++z) {
    const float4 v = *reinterpret_cast<const float4*>(part + (size_t)z * N * 512 + off);
    s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
  }
  *reinterpret_cast<float4*>(h + off) =
      make_float4(s.x > 0.f ? s.x : 0.f, s.y > 0.f ? s.y : 0.f, s.z > 0.f ? s.z : 0.f, s.w > 0.f ? s.w : 0.f);
}

// h = relu(bias + the slices of part, added in slice order)
inline void launch_fc_reduce(const float* part, int slices, int N, const float* bias, float* h, hipStream_t s) {
  note_launch("fc_reduce");
  hipLaunchKernelGGL(fc_reduce, dim3(ceil_div(N * 128, 256)), dim3(256), 0, s, part, slices, N, bias, h);
}
// h = relu(a3 [N][3136] f32 x BfT + bf) as `slices` slices of gemm_lds (timed as `label`) and fc_reduce
inline void launch_fc_f32_splitk(const float* a3, const float* BfT, const float* bf, float* part, float* h, int N, int slices,
                                 const char* label, hipStream_t s) {
  ProbFcFwd p{};
  p.M = N, p.N = 512, p.K = 3136;
  p.a3 = a3, p.wt = BfT, p.part = part;
  gemm::launch_gemm<TileFcSmall>(p, slices, s, label);
  launch_fc_reduce(part, slices, N, bf, h, s);
}

// duel(): q = v + a*legal - mean_A(a*legal)   net.py:33-39 (mean over A, not over #legal)
// adv (optional) receives the raw fc_a outputs, which AtariLSTMNet.act ranks (net.py:119-123)
__global__ void dueling_kernel(const float* __restrict__ ha, const float* __restrict__ legal, float* __restrict__ q,
                               float* __restrict__ adv, int N, int A) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* row = ha + (size_t)n * 32;
  const float v = row[31];
  float la[31];
  float sum = 0.f;
  for (int j = 0; j < A; ++j) {
    if (adv) adv[(size_t)n * A + j] = row[j];
    la[j] = row[j] * legal[(size_t)n * A + j];
    sum += la[j];
  }
  const float mean = sum / (float)A;
  if (q)
    for (int j = 0; j < A; ++j) q[(size_t)n * A + j] = (v + la[j]) - mean;
}

// The AtariLSTMNet's heads: h [N][512] x Bh -> ha [N][32] (cols 0..A-1 = fc_a, col 31 = fc_v), then dueling_kernel -> q
// (and adv).  Timed as label / label_duel, or the pair as `label` where label_duel is NULL.  (Not in the launch census.)
inline void launch_heads_f32(const float* h, const float* Bh, const float* bh, const float* legal, float* ha, float* q,
                             float* adv, int N, int A, const char* label, const char* label_duel, hipStream_t s) {
  const auto duel = [&] {
    hipLaunchKernelGGL(dueling_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, s, (const float*)ha, legal, q, adv, N, A);
  };
  {
    ProfScope prof(label, s);
    hipLaunchKernelGGL(gemm_mfma<GemmHeads>, dim3(GemmHeads::CT / GemmHeads::CTB, ceil_div(N, GemmHeads::BM)),
                       dim3(kThreads), 0, s, h, (const float*)nullptr, Bh, bh, ha, (const float*)nullptr, (float*)nullptr, N);
    if (!label_duel) duel();
  }
  if (label_duel) {
    ProfScope prof(label_duel, s);
    duel();
  }
}

}  // namespace
}  // namespace rela_amd
