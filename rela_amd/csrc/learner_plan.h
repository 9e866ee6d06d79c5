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
// ---- the wgrad_x3 option: conv1's / conv2's weight gradients on wgrad_conv_x3.h.  A block is a partial tile, so the block
// counts are functions of the frame count (and, for conv1, of the lane form) alone: a result's bits depend on `frames`
// through these two functions only.
constexpr int kWgradX3MaxBlocks = 256;  // one persistent block per CU
// conv1: a frame per block up to the cap of wgrad_conv1_bf16 (its tile is 32 KB: 256 of them cost reduce_splits 8 MB)
inline int plan_wgrad1_x3_blocks(int frames, bool two_lanes) {
  const int cap = two_lanes ? kWgrad1BlocksTwoLanes : kWgrad1Blocks;
  return frames < cap ? frames : cap;
}
// conv2: a frame per block up to one block per CU at every frame count.  A block pays the zero fill of 138 KB of LDS and a
// partial tile of 128 KB that reduce_splits reads back (256 tiles: 32 MB), the cost that keeps wgrad_conv2_bf16 off below
// kFastWgradMinFrames -- but a frame costs this kernel far more than that: at 512 frames a cap of 64 / 128 / 256 blocks
// measured 114 / 62 / 42 us on one lane and 152 / 99 / 78 us on two (profiles/wgrad_x3_ab.md), so fewer blocks for few
// frames were tried and dropped.
inline int plan_wgrad2_x3_blocks(int frames) { return frames < kWgradX3MaxBlocks ? frames : kWgradX3MaxBlocks; }
// ---- the wgrad3_x3 option: conv3's weight gradient on wgrad_conv3_x3.h.  A frame per block up to one block per CU (its
// tile is 144 KB: kTrunkPartFloats is exactly 256 of them); the result's bits depend on `frames` through this function only.
constexpr int kWgrad3X3MaxBlocks = 256;
inline int plan_wgrad3_x3_blocks(int frames) { return frames < kWgrad3X3MaxBlocks ? frames : kWgrad3X3MaxBlocks; }

struct WgradPlan {
  bool bf16_kernel;  // wgrad_conv{1,2,3}_bf16.h (one partial tile per block), else a split-K GEMM:
  GemmArith arith;
  int splits;
};
struct TrunkBwdPlan {
  WgradPlan w3, w2, w1;
  int w1_max_blocks;  // of wgrad_conv1_bf16
  bool dgrad_bf16;    // the data gradients on dgrad_conv_bf16.h, else the f32 GEMM (f32x3 too: exact f32, one launch)
  bool dgrad_x3;      // ... unless this is set: both on dgrad_conv_x3.h (three-part bf16 operands, f32 accuracy), in every mode
  // conv1's / conv2's weight gradients on wgrad_conv_x3.h (three-part operands, f32 accuracy) with this many blocks,
  // whatever w1 / w2 say, in every mode
  bool wgrad_x3;
  int w1_x3_blocks, w2_x3_blocks;
  // conv3's weight gradient on wgrad_conv3_x3.h (likewise) with this many blocks, whatever w3 says, in every mode
  bool wgrad3_x3;
  int w3_x3_blocks;
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
// dgrad_x3: the learners' option of that name (rela_*_learner_set_dgrad_x3); it changes nothing but the plan's member.
// wgrad_x3: likewise (rela_*_learner_set_wgrad_x3); it sets its member and the two block counts and nothing else.
// wgrad3_x3: likewise (rela_*_learner_set_wgrad3_x3); its member and its block count.
inline TrunkBwdPlan plan_trunk_backward(GemmArith arith, int frames, int fast_wgrad_min_frames, const int split_mul[3],
                                        bool two_lanes, bool dgrad_x3 = false, bool wgrad_x3 = false, bool wgrad3_x3 = false) {
  TrunkBwdPlan p{};
  p.w3 = plan_wgrad23(arith, frames, fast_wgrad_min_frames, kSplitW3, split_mul[2]);
  p.w2 = plan_wgrad23(arith, frames, fast_wgrad_min_frames, kSplitW2, split_mul[1]);
  if (arith == kArithBf16x2) p.w1 = {true, arith, 0};  // exact u8 frames x (hi + lo) gradients
  else p.w1 = {false, arith, kSplitW1 * (arith == kArithF32x3 ? split_mul[0] : 1)};
  p.w1_max_blocks = two_lanes ? kWgrad1BlocksTwoLanes : kWgrad1Blocks;
  p.dgrad_bf16 = arith == kArithBf16x2;
  p.dgrad_x3 = dgrad_x3;
  p.wgrad_x3 = wgrad_x3;
  p.w1_x3_blocks = wgrad_x3 ? plan_wgrad1_x3_blocks(frames, two_lanes) : 0;
  p.w2_x3_blocks = wgrad_x3 ? plan_wgrad2_x3_blocks(frames) : 0;
  p.wgrad3_x3 = wgrad3_x3;
  p.w3_x3_blocks = wgrad3_x3 ? plan_wgrad3_x3_blocks(frames) : 0;
  return p;
}

// what a learner's plan says about its trunk; the frame count of the call makes a TrunkBwdPlan of it
struct TrunkArith {
  GemmArith arith;
  int split_mul[3];  // conv1, conv2, conv3
  bool two_lanes;
  bool dgrad_x3 = false;
  bool wgrad_x3 = false;
  bool wgrad3_x3 = false;
  TrunkBwdPlan plan(int frames, int fast_wgrad_min_frames = kFastWgradMinFrames) const {
    return plan_trunk_backward(arith, frames, fast_wgrad_min_frames, split_mul, two_lanes, dgrad_x3, wgrad_x3, wgrad3_x3);
  }
};

// ---- Ape-X (rela_apex_learner_set_precision: 0 f32 | 1 bf16x2 | 2 f32x3) --------------------------------------------
struct ApexBwdPlan {
  GemmArith heads_fc;  // the four GEMMs of head_fc_backward
  TrunkArith trunk;
};
inline ApexBwdPlan plan_apex_backward(int precision, bool two_lanes, bool dgrad_x3 = false, bool wgrad_x3 = false,
                                      bool wgrad3_x3 = false) {
  const GemmArith arith = precision == 1 ? kArithBf16x2 : precision == 2 ? kArithF32x3 : kArithF32;
  return {arith, {arith, {1, 1, 1}, two_lanes, dgrad_x3, wgrad_x3, wgrad3_x3}};
}

// ---- R2D2 (rela_r2d2_learner_set_precision: 0 f32 | 1 bf16x2 | 2 f32x3 | 3 f32x3_bwd) -------------------------------
// Mode 2 is a forward mode: its backward is mode 0's.  Mode 3 moves the large GEMMs over all training rows at once (dW_hh,
// dW_ih, d_a3, the conv weight gradients) to three-part operands; the heads' GEMMs (K = 32, M = 32: 11 / 10 us in three
// parts against 10 / 8 us), the recurrence, the cell kernels and the conv data gradients stay what they are in mode 0
// (the data gradients unless dgrad_x3 moves them to dgrad_conv_x3.h, in any mode; wgrad_x3 moves conv1's / conv2's weight
// gradients to wgrad_conv_x3.h and wgrad3_x3 conv3's to wgrad_conv3_x3.h, in any mode).
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
  bool lstm_in_rec3;      // ... unless this is set: the three GEMMs on gemm_rec3.h (three-part records, f32 accuracy), in every mode
  TrunkArith trunk;       // one lane
};
// lstm_in_rec3: the learner's option of that name (rela_r2d2_learner_set_lstm_in_rec3); it changes nothing but the plan's member.
inline R2d2BwdPlan plan_r2d2_backward(int precision, int rows, bool dgrad_x3 = false, bool lstm_in_rec3 = false,
                                      bool wgrad_x3 = false, bool wgrad3_x3 = false) {
  R2d2BwdPlan p{};
  p.heads = kArithF32;
  p.head_wgrad_splits = rows >= kSeqHeadSplitRows ? kSplitHeads : 1;
  p.lstm_in_rec64 = precision == 1;
  p.lstm_in = precision == 3 ? kArithF32x3 : kArithF32;
  p.lstm_in_rec3 = lstm_in_rec3;
  if (precision == 1) p.trunk = {kArithBf16x2, {1, 1, 1}, false};
  else if (precision == 3) p.trunk = {kArithF32x3, {kX6SplitMul, kX6SplitMul, kX6SplitMul}, false};
  else p.trunk = {kArithF32, {1, 1, 1}, false};
  p.trunk.dgrad_x3 = dgrad_x3;
  p.trunk.wgrad_x3 = wgrad_x3;
  p.trunk.wgrad3_x3 = wgrad3_x3;
  return p;
}

}  // namespace rela_amd
