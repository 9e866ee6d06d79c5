// The three-part conv3 weight gradient (wgrad_conv3_x3.h) as a translation unit of its own, compiled once for both
// learners, so that the compiler's account of the kernel can be checked by compiling this file alone
// (tests/test_wgrad3_x3_plan_host.py).  learner_common.hip reaches the kernel through this function.
#include "wgrad_conv3_x3.h"

#include "learner_common.h"

namespace rela_amd {

static_assert(kWgrad3X3MaxBlocks == wg3x3::kMaxBlocks, "the plan's block cap");
static_assert(kTrunkPartFloats >= (size_t)wg3x3::kMaxBlocks * 64 * 576, "part size: one conv3 tile per block");

int launch_wgrad_conv3_x3(const float* a2, const float* d_a3, int frames, float* part, int blocks, hipStream_t s) {
  return wg3x3::launch(a2, d_a3, frames, part, blocks, s);
}

}  // namespace rela_amd
