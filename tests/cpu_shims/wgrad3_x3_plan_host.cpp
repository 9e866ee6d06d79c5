// CPU shim for tests/test_wgrad3_x3_plan_host.py: the learners' backward plan (rela_amd/csrc/learner_plan.h) with its
// wgrad3_x3 option behind a C ABI, beside wgrad_x3_plan_host.cpp, which covers the plan without it.  Built by the test with g++.
// TEST INFRASTRUCTURE -- not part of the product library.
#include "../../rela_amd/csrc/learner_plan.h"

using namespace rela_amd;

static void put(const TrunkBwdPlan& p, int* out) {
  const WgradPlan* w[3] = {&p.w3, &p.w2, &p.w1};
  for (int i = 0; i < 3; ++i) out[3 * i] = w[i]->bf16_kernel, out[3 * i + 1] = w[i]->arith, out[3 * i + 2] = w[i]->splits;
  out[9] = p.w1_max_blocks, out[10] = p.dgrad_bf16, out[11] = p.dgrad_x3;
  out[12] = p.wgrad_x3, out[13] = p.w1_x3_blocks, out[14] = p.w2_x3_blocks;
  out[15] = p.wgrad3_x3, out[16] = p.w3_x3_blocks;
}

// learner 0: Ape-X | 1: R2D2.  opts: bit 0 dgrad_x3, 1 wgrad_x3, 2 wgrad3_x3, 3 (R2D2) lstm_in_rec3.  out: 17 ints
extern "C" void shim_trunk_plan_w3x3(int learner, int precision, int two_lanes, int frames, int opts, int* out) {
  const bool d = opts & 1, w = opts & 2, w3 = opts & 4, rec3 = opts & 8;
  put(learner == 0 ? plan_apex_backward(precision, two_lanes != 0, d, w, w3).trunk.plan(frames)
                   : plan_r2d2_backward(precision, frames, d, rec3, w, w3).trunk.plan(frames), out);
}
// the same plan through the calls as they were before the option: no argument for it
extern "C" void shim_trunk_plan_before(int learner, int precision, int two_lanes, int frames, int opts, int* out) {
  const bool d = opts & 1, w = opts & 2, rec3 = opts & 8;
  put(learner == 0 ? plan_apex_backward(precision, two_lanes != 0, d, w).trunk.plan(frames)
                   : plan_r2d2_backward(precision, frames, d, rec3, w).trunk.plan(frames), out);
}
extern "C" int shim_wgrad3_x3_blocks(int frames) { return plan_wgrad3_x3_blocks(frames); }
