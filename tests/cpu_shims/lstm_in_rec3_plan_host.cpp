// CPU shim for tests/test_lstm_in_rec3_plan_host.py: the R2D2 learner's backward plan (rela_amd/csrc/learner_plan.h) with its
// lstm_in_rec3 option behind a C ABI.  Built by the test with g++.  TEST INFRASTRUCTURE -- not part of the product library.
#include "../../rela_amd/csrc/learner_plan.h"

using namespace rela_amd;

// with_arg = 0: the call as it was before the option (two or three arguments).  out, 11 ints: heads, head_wgrad_splits,
// lstm_in_rec64, lstm_in, trunk (arith, split_mul x 3, two_lanes, dgrad_x3), lstm_in_rec3
extern "C" void shim_r2d2_plan_rec3(int precision, int rows, int dgrad_x3, int with_arg, int lstm_in_rec3, int* out) {
  const R2d2BwdPlan p = with_arg ? plan_r2d2_backward(precision, rows, dgrad_x3 != 0, lstm_in_rec3 != 0)
                                 : plan_r2d2_backward(precision, rows, dgrad_x3 != 0);
  const int v[11] = {p.heads, p.head_wgrad_splits, p.lstm_in_rec64, p.lstm_in, p.trunk.arith, p.trunk.split_mul[0],
                     p.trunk.split_mul[1], p.trunk.split_mul[2], p.trunk.two_lanes, p.trunk.dgrad_x3, p.lstm_in_rec3};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
}
