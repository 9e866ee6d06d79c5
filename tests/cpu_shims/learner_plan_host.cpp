// CPU shim for the host logic tests: the backward plan of the two learners (rela_amd/csrc/learner_plan.h is plain C++: the
// SAME functions rela_apex_learner_grad, rela_r2d2_learner_grad and the backward taps call before they launch anything)
// behind a C ABI.  Built by tests/test_learner_plan_host.py with g++.
// TEST INFRASTRUCTURE -- not part of the product library.
#include "../../rela_amd/csrc/learner_plan.h"

using namespace rela_amd;

namespace {
// 11 ints: per layer conv3, conv2, conv1 (bf16_kernel, arith, splits), then w1_max_blocks, dgrad_bf16
void put_trunk(const TrunkBwdPlan& p, int* out) {
  const WgradPlan* w[3] = {&p.w3, &p.w2, &p.w1};
  for (int i = 0; i < 3; ++i) out[3 * i] = w[i]->bf16_kernel, out[3 * i + 1] = w[i]->arith, out[3 * i + 2] = w[i]->splits;
  out[9] = p.w1_max_blocks, out[10] = p.dgrad_bf16;
}
}  // namespace

extern "C" {

void shim_plan_trunk_backward(int arith, int frames, int fast_wgrad_min_frames, int mul1, int mul2, int mul3, int two_lanes,
                              int* out) {
  const int mul[3] = {mul1, mul2, mul3};
  put_trunk(plan_trunk_backward((GemmArith)arith, frames, fast_wgrad_min_frames, mul, two_lanes != 0), out);
}

// out: heads_fc, then the trunk of `frames` frames as put_trunk
void shim_plan_apex_backward(int precision, int two_lanes, int frames, int* out) {
  const ApexBwdPlan p = plan_apex_backward(precision, two_lanes != 0);
  out[0] = p.heads_fc;
  put_trunk(p.trunk.plan(frames), out + 1);
}

// out: heads, head_wgrad_splits, lstm_in_rec64, lstm_in, then the trunk of `rows` frames as put_trunk
void shim_plan_r2d2_backward(int precision, int rows, int* out) {
  const R2d2BwdPlan p = plan_r2d2_backward(precision, rows);
  out[0] = p.heads, out[1] = p.head_wgrad_splits, out[2] = p.lstm_in_rec64, out[3] = p.lstm_in;
  put_trunk(p.trunk.plan(rows), out + 4);
}

// the constants, in the order tests/test_learner_plan_host.py names them
void shim_constants(int* out) {
  out[0] = kArithF32, out[1] = kArithBf16x2, out[2] = kArithF32x3, out[3] = kMaxSplitMul, out[4] = kFastWgradMinFrames;
}
}
