// CPU shim for tests/test_wgrad_x3_plan_host.py: the learners' backward plan (rela_amd/csrc/learner_plan.h) with its wgrad_x3
// option behind a C ABI, beside learner_plan_host.cpp, which covers the plan without it.  Built by the test with g++.
// TEST INFRASTRUCTURE -- not part of the product library.
#include "../../rela_amd/csrc/learner_plan.h"

using namespace rela_amd;

// learner 0: the Ape-X learner's trunk (precision 0..2, one or two lanes) | 1: the R2D2 learner's (precision 0..3, one lane)
// out, 15 ints: per layer conv3, conv2, conv1 (bf16_kernel, arith, splits), then w1_max_blocks, dgrad_bf16, dgrad_x3,
// wgrad_x3, w1_x3_blocks, w2_x3_blocks
extern "C" void shim_trunk_plan_wx3(int learner, int precision, int two_lanes, int frames, int dgrad_x3, int wgrad_x3, int* out) {
  const TrunkBwdPlan p = learner == 0
                             ? plan_apex_backward(precision, two_lanes != 0, dgrad_x3 != 0, wgrad_x3 != 0).trunk.plan(frames)
                             : plan_r2d2_backward(precision, frames, dgrad_x3 != 0, false, wgrad_x3 != 0).trunk.plan(frames);
  const WgradPlan* w[3] = {&p.w3, &p.w2, &p.w1};
  for (int i = 0; i < 3; ++i) out[3 * i] = w[i]->bf16_kernel, out[3 * i + 1] = w[i]->arith, out[3 * i + 2] = w[i]->splits;
  out[9] = p.w1_max_blocks, out[10] = p.dgrad_bf16, out[11] = p.dgrad_x3;
  out[12] = p.wgrad_x3, out[13] = p.w1_x3_blocks, out[14] = p.w2_x3_blocks;
}
extern "C" int shim_wgrad1_x3_blocks(int frames, int two_lanes) { return plan_wgrad1_x3_blocks(frames, two_lanes != 0); }
extern "C" int shim_wgrad2_x3_blocks(int frames) { return plan_wgrad2_x3_blocks(frames); }
