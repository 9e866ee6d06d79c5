// Which kernels the backward pass of a learner step runs (csrc/learner.hip, learner_r2d2.hip, the shared conv trunk in
// learner_common.hip): the arithmetic of every GEMM, the split-K counts and the frame / row thresholds, as pure host
// functions of the learner's precision mode.  No HIP in here: learner_common.h includes this header, and
// tests/cpu_shims/learner_plan_host.cpp compiles it with a plain C++ compiler so that the decision table is checked where
// there is no GPU (tests/test_learner_plan_host.py).  The two *_grad entry points and the four backward taps take their
// plan from plan_apex_backward / plan_r2d2_backward and from nowhere else: a new variant is a row in here.
#pragma once

namespace rela_amd {

// the arithmetic of one learner GEMM (launch_gemm_as, learner_common.h, picks the kernel family and the tile)
enum GemmArith {
  kArithF32 = 0,     // gemm_lds: f32 MFMA
  kArithBf16x2 = 1,  // gemm_bf16x3, PARTS = 2: operands as bf16 hi + lo, three products
  kArithF32x3 = 2,   // gemm_bf16x3, PARTS = 3: three bf16 parts, six products, f32 accuracy
};

// ---- the conv trunk (net.{0,2,4}), shared by both learners ----------------------------------------------------------
constexpr int kSplitW3 = 28, kSplitW2 = 27, kSplitW1 = 64;  // split-K slices of the weight-gradient GEMMs
// conv2 / conv3 up to this many frames: 3 x the splits = 3-4 blocks per CU instead of one (a block alone on its CU waits
// out every chunk's load latency with two waves per SIMD; flat between 2 and 4 in the r3 sweep).  conv1 keeps kSplitW1 at
// every frame count: more splits measured 105 -> 69-75 us at 512 frames, but another split count is another association
// of g_c1w and with it other bits of a step.
constexpr int kSmallTrunkMaxFrames = 1024, kSmallTrunkSplitMul = 3;
// the most a split multiplier may be: what kTrunkPartFloats (learner_common.h) leaves room for
constexpr int kMaxSplitMul = 8;
static_assert(kSmallTrunkSplitMul <= kMaxSplitMul, "part size");
// conv2 / conv3 on wgrad_conv{2,3}_bf16 only from this many frames (R2D2: T * B): at 512 frames their per-block fixed
// costs (LDS zero fill, 256 partial tiles of 128 / 144 KB for reduce_splits) cancel the gain (Ape-X: step 0.83 -> 0.91 ms)
constexpr int kFastWgradMinFrames = 2048;
// blocks of wgrad_conv1_bf16: all of them on one lane (w1fast::kMaxBlocks), half with a second lane to leave CUs to it
constexpr int kWgrad1Blocks = 256, kWgrad1BlocksTwoLanes = 128;

struct WgradPlan {
  bool bf16_kernel;  // wgrad_conv{1,2,3}_bf16.h (one partial tile per block), else a split-K GEMM:
  GemmArith arith;
  int splits;
};
struct TrunkBwdPlan {
  WgradPlan w3, w2, w1;
  int w1_max_blocks;  // of wgrad_conv1_bf16
  bool dgrad_bf16;    // the data gradients on dgrad_conv_bf16.h, else the f32 GEMM (f32x3 too: exact f32, one launch)
};

// conv3 / conv2: `base` slices, tripled for few frames; above, times the multiplier of the three-part GEMM
inline WgradPlan plan_wgrad23(GemmArith arith, int frames, int fast_wgrad_min_frames, int base, int split_mul) {
  if (arith == kArithBf16x2 && frames >= fast_wgrad_min_frames) return {true, arith, 0};
  const int mul = frames <= kSmallTrunkMaxFrames ? kSmallTrunkSplitMul : (arith == kArithF32x3 ? split_mul : 1);
  return {false, arith, base * mul};
}

// split_mul: multipliers on the split counts of conv1's / conv2's / conv3's THREE-PART weight gradients (conv1 at every
// frame count, conv2 / conv3 above kSmallTrunkMaxFrames).  Another split count is another association of the sum, so the
// modes that existed before the R2D2 learner's mode 3 keep 1.  fast_wgrad_min_frames: kFastWgradMinFrames in both learners;
// rela_debug_trunk_backward lowers it so that small ragged frame counts reach wgrad_conv{2,3}_bf16.
inline TrunkBwdPlan plan_trunk_backward(GemmArith arith, int frames, int fast_wgrad_min_frames, const int split_mul[3],
                                        bool two_lanes) {
  TrunkBwdPlan p{};
  p.w3 = plan_wgrad23(arith, frames, fast_wgrad_min_frames, kSplitW3, split_mul[2]);
  p.w2 = plan_wgrad23(arith, frames, fast_wgrad_min_frames, kSplitW2, split_mul[1]);
  if (arith == kArithBf16x2) p.w1 = {true, arith, 0};  // exact u8 frames x (hi + lo) gradients
  else p.w1 = {false, arith, kSplitW1 * (arith == kArithF32x3 ? split_mul[0] : 1)};
  p.w1_max_blocks = two_lanes ? kWgrad1BlocksTwoLanes : kWgrad1Blocks;
  p.dgrad_bf16 = arith == kArithBf16x2;
  return p;
}

// what a learner's plan says about its trunk; the frame count of the call makes a TrunkBwdPlan of it
struct TrunkArith {
  GemmArith arith;
  int split_mul[3];  // conv1, conv2, conv3
  bool two_lanes;
  TrunkBwdPlan plan(int frames, int fast_wgrad_min_frames = kFastWgradMinFrames) const {
    return plan_trunk_backward(arith, frames, fast_wgrad_min_frames, split_mul, two_lanes);
  }
};

// ---- Ape-X (rela_apex_learner_set_precision: 0 f32 | 1 bf16x2 | 2 f32x3) --------------------------------------------
struct ApexBwdPlan {
  GemmArith heads_fc;  // the four GEMMs of head_fc_backward
  TrunkArith trunk;
};
inline ApexBwdPlan plan_apex_backward(int precision, bool two_lanes) {
  const GemmArith arith = precision == 1 ? kArithBf16x2 : precision == 2 ? kArithF32x3 : kArithF32;
  return {arith, {arith, {1, 1, 1}, two_lanes}};
}

// ---- R2D2 (rela_r2d2_learner_set_precision: 0 f32 | 1 bf16x2 | 2 f32x3 | 3 f32x3_bwd) -------------------------------
// Mode 2 is a forward mode: its backward is mode 0's.  Mode 3 moves the large GEMMs over all training rows at once (dW_hh,
// dW_ih, d_a3, the conv weight gradients) to three-part operands; the heads' GEMMs (K = 32, M = 32: 11 / 10 us in three
// parts against 10 / 8 us), the recurrence, the cell kernels and the conv data gradients stay what they are in mode 0.
constexpr int kSplitHeads = 32;
constexpr int kSeqHeadSplitRows = 1024;  // from here the head weight gradient is split-K: 256 blocks instead of 8
// twice the splits in mode 3: conv1 0.35 -> 0.28 ms, conv2 0.31 -> 0.25, conv3 0.28 -> 0.15 at 5,312 rows (four times: the same)
constexpr int kX6SplitMul = 2;
static_assert(kX6SplitMul <= kMaxSplitMul, "part size");

struct R2d2BwdPlan {
  GemmArith heads;        // seq_head_backward's two GEMMs
  int head_wgrad_splits;  // 1: one GEMM straight into the gradient | kSplitHeads: partial tiles + head_wgrad_reduce
  bool lstm_in_rec64;     // lstm_input_backward on the rec64 path (gemm_bf16s.h), else three GEMMs in:
  GemmArith lstm_in;
  TrunkArith trunk;       // one lane
};
inline R2d2BwdPlan plan_r2d2_backward(int precision, int rows) {
  R2d2BwdPlan p{};
  p.heads = kArithF32;
  p.head_wgrad_splits = rows >= kSeqHeadSplitRows ? kSplitHeads : 1;
  p.lstm_in_rec64 = precision == 1;
  p.lstm_in = precision == 3 ? kArithF32x3 : kArithF32;
  if (precision == 1) p.trunk = {kArithBf16x2, {1, 1, 1}, false};
  else if (precision == 3) p.trunk = {kArithF32x3, {kX6SplitMul, kX6SplitMul, kX6SplitMul}, false};
  else p.trunk = {kArithF32, {1, 1, 1}, false};
  return p;
}

}  // namespace rela_amd
