// The three-part conv data gradients (dgrad_conv_x3.h) as a translation unit of their own: the build compiles it without
// packed f32 arithmetic (rela_amd/build.py: EXTRA_HIP_FLAGS), so the operand splits and the epilogue's sums are plain
// v_sub_f32 / v_add_f32 beside the MFMAs.  learner_common.hip reaches the kernels through these three functions.
#include "dgrad_conv_x3.h"

#include "learner_common.h"

namespace rela_amd {

static_assert(kFrag2X3Bytes == dgx3::kFrag2Bytes && kFrag3X3Bytes == dgx3::kFrag3Bytes, "frag sizes");
static_assert(kTrunkPartFloats * 4 >= dgx3::kFrag2Bytes + dgx3::kFrag3Bytes, "frag scratch");

void pack_dgrad_x3_frags(const float* w2p, const float* w3p, void* frag2, void* frag3, hipStream_t s) {
  dgx3::pack_frags(w2p, w3p, frag2, frag3, s);
}
int launch_dgrad_conv3_x3(const float* d_a3, const float* w3p, const float* a2, float* d_a2, int frames, void* scratch,
                          hipStream_t s, const void* frags) {
  return dgx3::launch_conv3(d_a3, w3p, a2, d_a2, frames, scratch, s, frags);
}
int launch_dgrad_conv2_x3(const float* d_a2, const float* w2p, const float* a1, float* d_a1, int frames, void* scratch,
                          hipStream_t s, const void* frags) {
  return dgx3::launch_conv2(d_a2, w2p, a1, d_a1, frames, scratch, s, frags);
}

}  // namespace rela_amd
