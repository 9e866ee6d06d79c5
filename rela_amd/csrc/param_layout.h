// param_layout.h -- the parameter tensors of the two nets, in rela_ffnet_params / rela_lstmnet_params (= state_dict)
// order, and the flat f32 buffer the learners keep them in.  The one place for these tables: the nets' loads
// (ffnet.hip), both learners and, through tests/cpu_shims/param_layout_host.cpp, the check against the Python layout
// (rela_amd/learner.py: SHAPES, ffnet_flat_layout, lstmnet_flat_layout) that actor-only ranks cut the buffer up with.
// Plain C++: no HIP include.
#pragma once
#include <cstdint>

namespace rela_amd {

constexpr int kFFNetSegs = 12, kLstmNetSegs = 14;

// conv1 w/b, conv2 w/b, conv3 w/b, fc w/b, fc_v w/b, fc_a w/b     (AtariFFNet, net.py:8-55)
inline void ffnet_param_counts(int A, int64_t cnt[kFFNetSegs]) {
  const int64_t c[kFFNetSegs] = {32 * 256, 32, 64 * 512, 64, 64 * 576, 64, (int64_t)512 * 3136, 512, 512, 1,
                                 (int64_t)A * 512, A};
  for (int i = 0; i < kFFNetSegs; ++i) cnt[i] = c[i];
}

// conv1 w/b, conv2 w/b, conv3 w/b, lstm w_ih, w_hh, b_ih, b_hh, fc_v w/b, fc_a w/b     (AtariLSTMNet)
inline void lstmnet_param_counts(int A, int64_t cnt[kLstmNetSegs]) {
  const int64_t c[kLstmNetSegs] = {32 * 256, 32, 64 * 512, 64, 64 * 576, 64, (int64_t)2048 * 3136, (int64_t)2048 * 512,
                                   2048, 2048, 512, 1, (int64_t)A * 512, A};
  for (int i = 0; i < kLstmNetSegs; ++i) cnt[i] = c[i];
}

// the flat buffer: every segment padded to 4 floats (16-byte aligned tensors, float4 optimiser kernels);
// off[nseg] = total length
inline void flat_offsets(const int64_t* cnt, int nseg, int64_t* off) {
  off[0] = 0;
  for (int i = 0; i < nseg; ++i) off[i + 1] = off[i] + (cnt[i] + 3) / 4 * 4;
}

}  // namespace rela_amd
