// CPU shim: the host build of rela_amd/csrc/value_rescale.h (the same source the kernels compile), for
// tests/test_value_rescale_host.py and as the host side of the bit-for-bit GPU tests.  TEST INFRASTRUCTURE.
// With -DVALUE_RESCALE_MAIN it is a stand-alone program (a sweep with a round-trip check) for a host-only sanitizer run:
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -DVALUE_RESCALE_MAIN value_rescale_host.cpp && ./a.out
#include "../../rela_amd/csrc/value_rescale.h"

extern "C" void shim_value_rescale(const float* x, int n, float eps, float* h_out, float* hinv_out) {
  for (int i = 0; i < n; ++i) {
    if (h_out) h_out[i] = rela_vr::h(x[i], eps);
    if (hinv_out) hinv_out[i] = rela_vr::h_inv(x[i], eps);
  }
}

#ifdef VALUE_RESCALE_MAIN
#include <stdio.h>

#include <vector>

int main() {
  const float eps = 1e-3f;
  std::vector<float> x;
  x.push_back(0.0f);
  for (float a = 1e-6f; a <= 1e5f; a *= 1.01f) {
    x.push_back(a);
    x.push_back(-a);
  }
  std::vector<float> hx(x.size()), back(x.size());
  shim_value_rescale(x.data(), (int)x.size(), eps, hx.data(), nullptr);
  shim_value_rescale(hx.data(), (int)hx.size(), eps, nullptr, back.data());
  double worst = 0.0;
  for (size_t i = 0; i < x.size(); ++i) {
    const double d = fabs((double)back[i] - (double)x[i]), s = fabs((double)x[i]);
    const double r = s > 0.0 ? d / s : d;
    if (r > worst) worst = r;
  }
  printf("value_rescale_host: %zu points, worst round-trip relative error %.3g\n", x.size(), worst);
  return worst < 1e-5 ? 0 : 1;
}
#endif
