// The three-part conv weight gradients (wgrad_conv_x3.h) as a translation unit of their own, compiled once for both
// learners, so that the compiler's account of the two kernels can be checked by compiling this file alone
// (tests/test_wgrad_x3_plan_host.py).  learner_common.hip reaches the kernels through these two functions.
#include "wgrad_conv_x3.h"

#include "learner_common.h"

namespace rela_amd {

static_assert(kWgradX3MaxBlocks == wgx3::kMaxBlocks, "the plan's block caps");
static_assert(kTrunkPartFloats >= (size_t)wgx3::kMaxBlocks * 64 * 512, "part size: one conv2 tile per block");

int launch_wgrad_conv1_x3(const uint8_t* obs, const float* d_a1, int frames, float* part, int blocks, hipStream_t s) {
  return wgx3::launch_conv1(obs, d_a1, frames, part, blocks, s);
}
int launch_wgrad_conv2_x3(const float* a1, const float* d_a2, int frames, float* part, int blocks, hipStream_t s) {
  return wgx3::launch_conv2(a1, d_a2, frames, part, blocks, s);
}

}  // namespace rela_amd
