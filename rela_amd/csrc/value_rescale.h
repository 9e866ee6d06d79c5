// value_rescale.h -- the invertible value rescaling of R2D2 (Kapturowski et al., ICLR 2019, after Pohlen et al. 2018)
//   h(x)     = sign(x) * (sqrt(|x| + 1) - 1) + eps * x
//   h_inv(x) = sign(x) * (((sqrt(1 + 4 eps (|x| + 1 + eps)) - 1) / (2 eps))^2 - 1)
// as ONE fixed float32 recipe, shared by every kernel that forms a TD target (agent_ops.hip: td_kernel, learner.hip:
// learner_td_loss_grad, learner_r2d2.hip: seq_td_loss) and by the host restatement (tests/cpu_shims/value_rescale_host.cpp),
// which are therefore bit-identical.  The reference has no counterpart (it clips rewards in its env instead).
//
// Neither function is evaluated in the textbook form above, because both cancel in float32:
//   h:      sqrt(a + 1) - 1 for small a = |x| loses every bit below ulp(1); written as
//             a / (sqrt(a + 1) + 1)                                          (multiply by the conjugate),
//           a quotient of positive terms.
//   h_inv:  with u = sqrt(y + 1), y = h_inv(a), the definition of h reads  eps t^2 + (1 + 2 eps) t - a = 0  for
//           t = u - 1 >= 0.  The textbook form is the root  (-(1 + 2 eps) + r) / (2 eps), r = sqrt((1 + 2 eps)^2 + 4 eps a)
//           = sqrt(1 + 4 eps (a + 1 + eps)), which subtracts two numbers near 1 and then squares and subtracts 1 again.
//           The same root written from the other side (Vieta: the product of the roots is -a / eps),
//             t = 2 a / ((1 + 2 eps) + r),
//           has only positive terms, so u - 1 comes without any subtraction, and
//             y = u^2 - 1 = (u - 1) (u + 1) = t (t + 2).
// Both results carry the sign of x (copysign) and are sums / products of same-signed terms: the relative error stays at a
// few ulp for every |x| (measured: DESIGN.md, "Value rescaling").  Only +, *, correctly rounded division and sqrtf are
// used (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; no __fsqrt_rn / __fdividef, which may map to the
// approximate instructions), and no FMA contraction anywhere, so host and device agree bit for bit.
// eps must be > 0 here: the callers' "off" (eps <= 0) never reaches these functions.
// Plain C++ apart from the HIP qualifiers: g++ compiles it for the host restatement.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RELA_VR_HD __host__ __device__
#else
#define RELA_VR_HD
#endif

namespace rela_vr {

RELA_VR_HD inline float h(float x, float eps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = fabsf(x);
  const float s = sqrtf(a + 1.0f);
  const float m = a / (s + 1.0f);  // sqrt(a + 1) - 1
  return copysignf(m, x) + eps * x;
}

RELA_VR_HD inline float h_inv(float x, float eps) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float a = fabsf(x);
  const float c = 1.0f + 2.0f * eps;
  const float r = sqrtf(c * c + (4.0f * eps) * a);
  const float t = (2.0f * a) / (c + r);  // sqrt(y + 1) - 1
  return copysignf(t * (t + 2.0f), x);
}

}  // namespace rela_vr
