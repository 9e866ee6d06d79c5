// pow_aten.h -- torch::pow(tensor, exponent) on the device, as the replay (replay.hip) and the TD kernel that writes a
// block's weights itself (agent_ops.hip: td_kernel_insert) evaluate it: one routine, so both give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "sleef_powf_core.h"

namespace rela_amd {

// torch::pow(tensor, exponent) as ATen's CPU kernel evaluates it for a float tensor of n elements and a
// float exponent held in a double Scalar (rela/prioritized_replay.h:188,239,321): the vectorised loop takes
// 2 * Vec::size() = 32 floats per iteration through SLEEF's powf (u10) with the exponent as float; the
// remaining n % 32 elements go through the scalar lambda, std::pow(float, double) -> double pow, rounded to
// float.  Exponent 1 is a copy.  pos = index inside that tensor, n_ref = its length.
__device__ __forceinline__ float pow_aten(float p, float ex, int pos, int n_ref) {
  if (ex == 1.0f) return p;
  // exponents ATen evaluates without pow (pow_tensor_scalar_optimized_kernel); beta = 1 gives the reciprocal.
  // (+-0.5 go through ATen's vectorised sqrt, which is not the IEEE square root in the last bit on every input:
  // the device uses the IEEE one; no BASELINE config uses those exponents and they are not pinned.)
  if (ex == -1.0f) return __fdiv_rn(1.0f, p);
  if (ex == 0.5f) return __fsqrt_rn(p);
  if (ex == 2.0f) return __fmul_rn(p, p);
  if (ex == 3.0f) return __fmul_rn(__fmul_rn(p, p), p);
  if (ex == -0.5f) return __fdiv_rn(1.0f, __fsqrt_rn(p));
  if (ex == -2.0f) return __fdiv_rn(1.0f, __fmul_rn(p, p));
  if (pos < n_ref - (n_ref & 31)) return sleef::powf_u10(p, ex);
  return (float)pow((double)p, (double)ex);
}

}  // namespace rela_amd
