// ffnet_kern.h -- what every kernel family of the forward (conv_f32.h, gemm_f32.h, conv_bf16s.h, conv12_i8.h, fc_bf16s.h,
// heads_duel.h) shares: the block shape, the vector types, the persistent grids and the dynamic-LDS opt-in.  Included by
// ffnet.hip only: the names below the vector types live in rela_amd::(anonymous), as the kernels of those headers do.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "common.h"

namespace rela_amd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the *_stamps diagnostics: shader-clock stamps [2 waves][kStampFrames][kStampPoints] u64
constexpr int kStampFrames = 8, kStampPoints = 12;

constexpr int kNumCU = 256;
// Blocks of a PERSISTENT kernel (one block per CU, each walking its share of the frames): a grid of exactly 256 has no
// slack -- one CU held by another stream's small kernel (the replay's single-workgroup chain, a learner GEMM) when the
// launch starts delays one block by that kernel's whole duration, and with it the launch.  RELA_CU_RESERVE = r leaves r
// CUs out of such grids (default below; 0 = the full chip).
// (One copy per including translation unit: rela_runtime_set_cu_reserve, ffnet.hip, sets the only one there is.)
std::atomic<int> g_cu_reserve{-1};  // -1: not set (RELA_CU_RESERVE, else 0)
inline int persistent_blocks(int n) {
  int r = g_cu_reserve.load(std::memory_order_relaxed);
  if (r < 0) {
    const char* e = std::getenv("RELA_CU_RESERVE");
    r = e ? std::atoi(e) : 0;
    r = r < 0 ? 0 : (r > 128 ? 128 : r);
    g_cu_reserve.store(r, std::memory_order_relaxed);
  }
  return std::min(kNumCU - r, n);
}

// A kernel's opt-in to more than 64 KB of dynamic LDS.  Every family header lists its own kernels in an opt_in_lds_*
// function, which the nets' create calls once (ffnet.hip: opt_in_dynamic_lds).
struct LdsOptIn {
  const void* kernel;
  int bytes;
};
template <int N>
int opt_in(const LdsOptIn (&ks)[N]) {
  for (const LdsOptIn& k : ks) RELA_HIP(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
  return RELA_OK;
}

}  // namespace
}  // namespace rela_amd
