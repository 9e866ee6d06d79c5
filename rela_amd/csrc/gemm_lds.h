// gemm_lds.h -- generic LDS-tiled MFMA GEMM (v_mfma_f32_16x16x4_f32, f32 throughout), both
// operands staged through LDS by loader functors, optional split-K over blockIdx.z.
// Used by the learner's backward pass (learner.hip) and the small-batch fc forward (ffnet.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "common.h"
#include "prof.h"

namespace rela_amd {
namespace gemm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kLT = 512;  // 8 wavefronts
constexpr int BK = 32;    // K chunk staged per barrier (8 MFMA k-steps)

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// a fix-up's zero: a select on a value that is already in registers (see the loader contract below)
__device__ __forceinline__ float4 keep4(bool in_range, float4 v) {
  return make_float4(in_range ? v.x : 0.f, in_range ? v.y : 0.f, in_range ? v.z : 0.f, in_range ? v.w : 0.f);
}

// ---- generic LDS-tiled MFMA GEMM:  C[M][N] = sum_k A(m,k) * B(k,n) ---------------------------
// A arrives either k-contiguous (AMC = false: A(m, k) -> A[m][k..k+3]) or m-contiguous
// (AMC = true: A(k, m) -> A[m..m+3][k], the transposed operand of a weight gradient);
// B is always n-contiguous: B(k, n) -> B[k][n..n+3].
//
// The loader contract (this kernel and gemm_bf16x3.h): a Problem delivers an operand element in TWO steps.
//   fetchA(i, j) / fetchB(k, n) -> StageA / StageB   one load from an address that is ALWAYS valid: rows, k and image
//       coordinates are clamped into range, nothing is decided and nothing is computed on the result.  The kernel
//       calls it when it issues a chunk's loads; the value stays in a register ring until the chunk is consumed.
//   fixA(v, i, j) / fixB(v, k, n) -> float4          applied when the chunk goes to LDS, with the indices of the fetch:
//       the zero of an element out of range -- a SELECT, never a multiplication: a clamped fetch may have returned
//       anything, NaN and Inf included -- and any conversion (ProbW1: StageB is the raw u8 word).
// A `cond ? load : zero` in the loader makes hipcc branch around the load (s_cbranch_execz) and, unable to count loads
// across the join, wait s_waitcnt vmcnt(0) at every use: a ring of chunks "in flight" then holds nothing but the loads of
// the current step.  With unconditional fetches the waits are counted and D - 1 chunks stay outstanding.
// ProbBase supplies the defaults: float4 stages and identity fix-ups.
//
// S (1, 2, 4) = the stage depth: the chunks of 32 k that are fetched, stored and multiplied per barrier.  A stage's LDS
// image is S chunk images one behind the other, each with the strides below, and its S chunks are multiplied one after
// the other in k order: every accumulator sees the MFMAs of the S = 1 kernel in the same order, so the sums keep their
// bits; splits, kslice and kFoldChunks stay counted in chunks.  Per barrier a block then pays the fixed costs of a step --
// the wait for the ring, the LDS round trip, the barrier -- once for S x 32 k.
template <int BM_, int BN_, int WM_, int WN_, bool AMC_, int S_ = 1>
struct TileCfg {
  static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, S = S_;
  static constexpr bool AMC = AMC_;
  static_assert(S == 1 || S == 2 || S == 4, "stage depth");
  static_assert(WM * WN == 8, "8 wavefronts per block");
  static constexpr int TM = BM / 16 / WM, TN = BN / 16 / WN;  // 16x16 tiles per wave
  static_assert(TM >= 1 && TN >= 1, "tile too small for the wave grid");
  // leading dimensions = 16 (mod 32) floats, or k+2: a fragment read (16 rows x 4 k) touches
  // every bank exactly twice, the minimum for 64 lanes
  static constexpr int LDA = AMC ? BM + 16 : BK + 2;
  static constexpr int A_CHUNK = AMC ? BK * LDA : BM * LDA;  // floats of one chunk's image
  static constexpr int A_FLOATS = S * A_CHUNK;
  static constexpr int LDB = BN + 16;
  static constexpr int B_CHUNK = BK * LDB;
  static constexpr int B_FLOATS = S * B_CHUNK;
  static constexpr int A_V4C = BM * BK / 4, B_V4C = BN * BK / 4;  // float4s of one chunk
  static constexpr int A_V4 = S * A_V4C, B_V4 = S * B_V4C;
  static constexpr int A_IT = (A_V4 + kLT - 1) / kLT, B_IT = (B_V4 + kLT - 1) / kLT;
  static constexpr int LDS_BYTES = 2 * (A_FLOATS + B_FLOATS) * 4;
  static constexpr bool DYN_LDS = LDS_BYTES > 64 * 1024;  // past the static limit: dynamic LDS, sized at the launch
};

// Optional (compile time): a Problem with a member `static constexpr int kFoldChunks = F` gets its sum in GROUPS of F
// chunks -- after every F chunks the accumulator is added to a running total and cleared, so an element is
// ((0 + g0) + g1) + ... with each group summed from zero in k order: bit for bit what F-chunk GEMMs per group followed by
// a sum over the groups in order give.  For launches without split-K whose chunk count is a multiple of F.
template <class P, class = void>
struct fold_chunks {
  static constexpr int value = 0;
};
template <class P>
struct fold_chunks<P, std::void_t<decltype(P::kFoldChunks)>> {
  static constexpr int value = P::kFoldChunks;
};

// ---- the chunk pipeline of gemm_lds and gemm_bf16x3 ----------------------------------------------------------------------
// D register sets, two LDS buffers.  Chunk c of the block's slice [c0, c1) lives in set (c - c0) % D and is multiplied from
// LDS buffer (c - c0) & 1.  A step: refill the set of the current chunk (it went to LDS a step ago) with chunk cur + D,
// multiply chunk cur, store chunk cur + 1 (fetched D - 1 steps ago) into the other buffer, barrier.  The loop is unrolled
// by D so that the sets are named statically, and its body has no branch: a refill past the slice's end re-reads the last
// chunk (never stored), and the last 1 .. D chunks run in a peeled tail that fetches nothing.
//   gload(chunk, set)   issue the chunk's fetches into register set `set` (std::integral_constant)
//   sstore(buf, chunk, set)   fix up and write set `set`, holding `chunk`, into LDS buffer buf
//   mma(buf, chunk, full)   multiply the chunk in LDS buffer buf; `full` (std::bool_constant) is true in the loop, whose
//                       chunks all lie before the slice's last one
// Needs c0 < c1; every condition is block-uniform.
// With a stage depth S > 1 (TileCfg) what the ring counts are STAGES of S chunks, numbered from 0 within the block's
// slice; only the last stage of a slice can be short, and it is always multiplied in the tail (full = false).
//
// store_point(): an integer zero the compiler cannot see through (an empty asm statement: one scalar move), added to the
// indices a fix-up gets.  A fix-up is a select on a fetched value and nothing else ties it to the store: hipcc evaluated
// the selects of all D sets at the top of a round, right behind the refill issued there, and waited for that refill at
// once.  A predicate that exists only from the store on keeps the select, and with it the wait, at the store.
__device__ __forceinline__ int store_point() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return z;
}
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int D, class Load, class Store, class Mma>
__device__ __forceinline__ void chunk_ring(int c0, int c1, Load&& gload, Store&& sstore, Mma&& mma) {
  using Sets = std::make_integer_sequence<int, D>;
  static_for([&](auto j) { gload(min(c0 + j.value, c1 - 1), j); }, Sets{});
  sstore(0, c0, std::integral_constant<int, 0>{});
  __syncthreads();
  int base = c0;
  for (; base + D < c1; base += D) {
    static_for(
        [&](auto j) {
          const int cur = base + j.value, buf = (cur - c0) & 1;
          gload(min(cur + D, c1 - 1), j);
          __builtin_amdgcn_sched_barrier(0);  // (the refill is issued before anything waits)
          mma(buf, cur, std::true_type{});
          __builtin_amdgcn_sched_barrier(0);
          sstore(buf ^ 1, cur + 1, std::integral_constant<int, (j.value + 1) % D>{});
          __syncthreads();
          // the body is one basic block: without this, hipcc hoists the fix-up arithmetic of the NEXT steps' stores over
          // the barrier and with it their waits, draining the ring in the first step of every round
          __builtin_amdgcn_sched_barrier(0);
        },
        Sets{});
  }
  static_for(
      [&](auto j) {
        const int cur = base + j.value, buf = (cur - c0) & 1;
        if (cur < c1) {
          mma(buf, cur, std::false_type{});
          if (cur + 1 < c1) sstore(buf ^ 1, cur + 1, std::integral_constant<int, (j.value + 1) % D>{});
          __syncthreads();
        }
      },
      Sets{});
}

constexpr int kRing = 2;  // register sets of gemm_lds: one chunk outstanding behind the one being multiplied (measured: 2 < 3 < 4)

template <class T, class P>
__global__ __launch_bounds__(kLT) void gemm_lds(const P p) {
  constexpr int S = T::S;
  // static LDS ends at 64 KB: a deeper stage's images come from the launch's dynamic LDS (the static arrays then hold
  // one vector each and are not used)
  __shared__ __attribute__((aligned(16))) float sA_[2][T::DYN_LDS ? 4 : T::A_FLOATS];
  __shared__ __attribute__((aligned(16))) float sB_[2][T::DYN_LDS ? 4 : T::B_FLOATS];
  extern __shared__ __attribute__((aligned(16))) float gemm_lds_dyn[];
  auto pA = [&](int buf, int off) -> float* {
    if constexpr (T::DYN_LDS) return gemm_lds_dyn + buf * T::A_FLOATS + off;
    else return &sA_[buf][off];
  };
  auto pB = [&](int buf, int off) -> float* {
    if constexpr (T::DYN_LDS) return gemm_lds_dyn + (2 * T::A_FLOATS + buf * T::B_FLOATS) + off;
    else return &sB_[buf][off];
  };
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, kk = lane >> 4;
  const int wm = wave / T::WN, wn = wave % T::WN;
  const int bm0 = blockIdx.y * T::BM, bn0 = blockIdx.x * T::BN;
  const int nch = (p.K + BK - 1) / BK;
  const int c0 = blockIdx.z * p.kslice;
  const int c1 = min(nch, c0 + p.kslice);
  // what chunk_ring counts: chunks [c0, c1) at S = 1, else the slice's stages [0, ns) of S chunks (the last may be short)
  const int r0 = S == 1 ? c0 : 0, r1 = S == 1 ? c1 : (c1 - c0 + S - 1) / S;
  // first k of chunk `sub` of ring item `it`.  A short last stage repeats the slice's last chunk in its surplus chunks
  // (as a ring refill past the slice's end does): no fetch leaves the slice, and those chunks are never multiplied.
  auto kbase = [&](int it, int sub) { return S == 1 ? it * BK : min(c0 + it * S + sub, c1 - 1) * BK; };

  // (idx clamped, not predicated: a surplus thread repeats its neighbour's fetch and LDS write)
  typename P::StageA ra[kRing][T::A_IT];
  typename P::StageB rb[kRing][T::B_IT];
  auto gload = [&](int ch, auto set) {
    constexpr int R = decltype(set)::value;
    const int m0 = bm0, n0 = bn0;
#pragma unroll
    for (int j = 0; j < T::A_IT; ++j) {
      const int idx = min(tid + j * kLT, T::A_V4 - 1);
      const int sub = S == 1 ? 0 : idx / T::A_V4C, ic = S == 1 ? idx : idx % T::A_V4C;
      const int k0 = kbase(ch, sub);
      if constexpr (T::AMC) {
        const int kr = ic / (T::BM / 4), q = ic % (T::BM / 4);
        ra[R][j] = p.fetchA(k0 + kr, m0 + 4 * q);
      } else {
        const int r = ic >> 3, q = ic & 7;
        ra[R][j] = p.fetchA(m0 + r, k0 + 4 * q);
      }
    }
#pragma unroll
    for (int j = 0; j < T::B_IT; ++j) {
      const int idx = min(tid + j * kLT, T::B_V4 - 1);
      const int sub = S == 1 ? 0 : idx / T::B_V4C, ic = S == 1 ? idx : idx % T::B_V4C;
      const int kr = ic / (T::BN / 4), q = ic % (T::BN / 4);
      rb[R][j] = p.fetchB(kbase(ch, sub) + kr, n0 + 4 * q);
    }
  };
  auto sstore = [&](int buf, int ch, auto set) {
    constexpr int R = decltype(set)::value;
    const int z = store_point();
    const int k00 = kbase(ch, 0) + z, m0 = bm0 + z, n0 = bn0 + z;
#pragma unroll
    for (int j = 0; j < T::A_IT; ++j) {
      const int idx = min(tid + j * kLT, T::A_V4 - 1);
      const int sub = S == 1 ? 0 : idx / T::A_V4C, ic = S == 1 ? idx : idx % T::A_V4C;
      const int k0 = S == 1 ? k00 : kbase(ch, sub) + z;
      if constexpr (T::AMC) {
        const int kr = ic / (T::BM / 4), q = ic % (T::BM / 4);
        *reinterpret_cast<float4*>(pA(buf, sub * T::A_CHUNK + kr * T::LDA + 4 * q)) = p.fixA(ra[R][j], k0 + kr, m0 + 4 * q);
      } else {
        const int r = ic >> 3, q = ic & 7;
        const float4 v = p.fixA(ra[R][j], m0 + r, k0 + 4 * q);
        float* d = pA(buf, sub * T::A_CHUNK + r * T::LDA + 4 * q);
        *reinterpret_cast<float2*>(d) = make_float2(v.x, v.y);
        *reinterpret_cast<float2*>(d + 2) = make_float2(v.z, v.w);
      }
    }
#pragma unroll
    for (int j = 0; j < T::B_IT; ++j) {
      const int idx = min(tid + j * kLT, T::B_V4 - 1);
      const int sub = S == 1 ? 0 : idx / T::B_V4C, ic = S == 1 ? idx : idx % T::B_V4C;
      const int kr = ic / (T::BN / 4), q = ic % (T::BN / 4);
      *reinterpret_cast<float4*>(pB(buf, sub * T::B_CHUNK + kr * T::LDB + 4 * q)) =
          p.fixB(rb[R][j], (S == 1 ? k00 : kbase(ch, sub) + z) + kr, n0 + 4 * q);
    }
  };

  f32x4 acc[T::TM][T::TN];
#pragma unroll
  for (int t = 0; t < T::TM; ++t)
#pragma unroll
    for (int u = 0; u < T::TN; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int FOLD = fold_chunks<P>::value;
  f32x4 tot[FOLD ? T::TM : 1][FOLD ? T::TN : 1];
  if constexpr (FOLD > 0) {
#pragma unroll
    for (int t = 0; t < T::TM; ++t)
#pragma unroll
      for (int u = 0; u < T::TN; ++u) tot[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  auto mma = [&](int buf, int ch, auto full) {
    const int left = c1 - c0 - ch * S;  // (S > 1, the tail) chunks of the slice from this stage on
#pragma unroll
    for (int sub = 0; sub < S; ++sub) {
      // (block-uniform) a short last stage: the chunks past the slice's end belong to nobody and are not multiplied
      if (S == 1 || decltype(full)::value || sub < left) {
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
          float a[T::TM], b[T::TN];
#pragma unroll
          for (int t = 0; t < T::TM; ++t) {
            const int row = (wm * T::TM + t) * 16 + li;
            a[t] = *pA(buf, sub * T::A_CHUNK + (T::AMC ? (4 * ks + kk) * T::LDA + row : row * T::LDA + 4 * ks + kk));
          }
#pragma unroll
          for (int u = 0; u < T::TN; ++u) b[u] = *pB(buf, sub * T::B_CHUNK + (4 * ks + kk) * T::LDB + (wn * T::TN + u) * 16 + li);
#pragma unroll
          for (int t = 0; t < T::TM; ++t)
#pragma unroll
            for (int u = 0; u < T::TN; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[u], acc[t][u], 0, 0, 0);
        }
        if constexpr (FOLD > 0) {
          const int done = S == 1 ? ch - c0 + 1 : ch * S + sub + 1;  // chunks of the slice multiplied so far
          if (done % FOLD == 0) {  // (block-uniform) a group is complete
#pragma unroll
            for (int t = 0; t < T::TM; ++t)
#pragma unroll
              for (int u = 0; u < T::TN; ++u) {
                tot[t][u] += acc[t][u];
                acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
              }
          }
        }
      }
    }
  };
  // (a block whose slice is empty fetches nothing and stores its zeros: the split reductions read every split)
  if (c0 < c1) chunk_ring<kRing>(r0, r1, gload, sstore, mma);

#pragma unroll
  for (int t = 0; t < T::TM; ++t)
#pragma unroll
    for (int u = 0; u < T::TN; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = bm0 + (wm * T::TM + t) * 16 + kk * 4 + r;
        const int n = bn0 + (wn * T::TN + u) * 16 + li;
        if (m < p.M && n < p.N) {
          if constexpr (FOLD > 0) p.store(blockIdx.z, m, n, tot[t][u][r]);
          else p.store(blockIdx.z, m, n, acc[t][u][r]);
        }
      }
}

struct ProbBase {
  int M, N, K, kslice;
  using StageA = float4;
  using StageB = float4;
  __device__ float4 fixA(float4 v, int, int) const { return v; }
  __device__ float4 fixB(float4 v, int, int) const { return v; }
};

template <class T, class P>
void launch_gemm(P p, int splits, hipStream_t s, const char* name) {
  const int nch = ceil_div(p.K, BK);
  p.kslice = ceil_div(nch, splits);
  ProfScope prof(name, s);
  note_launch("gemm_lds (f32)");
  static_assert(T::LDS_BYTES <= 160 * 1024, "two stages must fit the CU's LDS");
  if constexpr (T::DYN_LDS) {
    static const hipError_t attr_set = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_lds<T, P>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, T::LDS_BYTES);
    (void)attr_set;
  }
  hipLaunchKernelGGL((gemm_lds<T, P>), dim3(ceil_div(p.N, T::BN), ceil_div(p.M, T::BM), splits), dim3(kLT),
                     T::DYN_LDS ? T::LDS_BYTES : 0, s, p);
}

}  // namespace gemm
}  // namespace rela_amd
