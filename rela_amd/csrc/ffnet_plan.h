// Which kernels a forward of N rows runs (csrc/ffnet.hip): the batch thresholds of the three precision modes and the
// decision they drive, as pure host functions.  No HIP in here: ffnet.hip includes this header, and
// tests/cpu_shims/ffnet_plan_host.cpp compiles it with a plain C++ compiler so that the decision table is checked where
// there is no GPU (tests/test_ffnet_plan_host.py, against the tables the GPU tests assert through the launch census).
#pragma once
#include <cstdint>

namespace rela_amd {

// ---- batch thresholds ---------------------------------------------------------------------------------------------
constexpr int kFastMinN = 1024;  // below this fc_bf16s has too few blocks and the f32 split-K fc is faster
constexpr int kFastTrunkMinN = 128;  // from here up the split-bf16 convolutions beat the f32 ones
// f32-accurate bf16 mode (precision 2: the f32x3 arithmetic of gemm_f32emu.h).  r5: from kEmuConvMinN rows the whole trunk
// runs on pre-split activations ("split3 records", gemm_s3.h): conv1 -> conv2 fused per frame (conv12_s3.h), conv3 as an
// image kernel with resident weights (conv_img_s3.h), fc as an LDS-DMA GEMM over records (gemm_s3.h); smaller batches
// run the exact f32 MFMA kernels (same accuracy, channel-last f32).  Byte offsets inside the records are 32-bit.
constexpr int kEmuConvMinN = 512, kEmuFcMinN = 512, kEmuMaxN = 80000;
// Below kFcSplitBelow rows gemm_mfma<GemmFc> launches fewer than 128 blocks, each walking all 98
// K-chunks (123 us at N = 512, the same at N = 80).  There the product runs as a split-K instance of
// gemm_lds (gemm_lds.h) over ~256 blocks; fc_reduce sums the partial tiles in a fixed order and
// applies bias + ReLU.  The partial tiles live in the caller's workspace behind `ha`.
constexpr int kFcSplitBelow = 2048;
constexpr int kFcPartRows = 8192;  // splits * N <= 8192 rows of partial sums (f32 split-K: <= 4096)
constexpr int64_t kFcPartFloats = (int64_t)kFcPartRows * 512;
// what the slicing of the bf16 split-K fc counts with (ffnet.hip asserts them against the kernels' own): the rows of a
// block of fc_bf16s (FcFast::BM), the 7 x 7 positions of a3 its contraction is sliced over (FcFast::NPOS), the CUs
constexpr int kFcBf16BlockRows = 112, kFcPositions = 49, kPlanCUs = 256;

// ---- forward modes ------------------------------------------------------------------------------------------------
// ffnet_forward_mode's `mode`: the net's own precision, one of the three precisions whatever the net says, or the
// learner's f32x3 pass that also leaves a1 / a2 / a3 in channel-last f32 for the backward kernels
enum FfnetMode { kModeNet = -1, kModeF32 = 0, kModeBf16x2 = 1, kModeF32x3 = 2, kModeF32x3KeepF32 = 3 };

enum TrunkKind {
  kTrunkF32 = 0,   // conv1_bf16x3 -> conv_mfma<Conv2> -> conv_mfma<Conv3>: channel-last f32
  kTrunkBf16 = 1,  // conv12_i8 -> conv_bf16s<Conv3F>: split-bf16 records in a2 / a3's places, a1 not produced
  kTrunkS3 = 2,    // conv12_s3 -> conv3_img_s3: split3 records in the record scratch
};
enum FcKind {
  kFcF32SplitK = 0,   // gemm_lds split-K over BfT + fc_reduce (N < kFcSplitBelow)
  kFcF32Gemm = 1,     // gemm_mfma<GemmFc>
  kFcBf16 = 2,        // fc_bf16s over a3's records
  kFcBf16SplitK = 3,  // fc_bf16s<split> over fc_slices slices of fc_per positions + fc_reduce
  kFcS3 = 4,          // gemm_s3<fc>, one slice
  kFcS3SplitK = 5,    // gemm_s3<fc>, free to split K: s3::plan picks the slices (fc_reduce if more than one)
};

// ---- weight layouts -------------------------------------------------------------------------------------------------
// The kernel-layout copies a net holds of its weights; the index is the row of the layout table (ffnet.hip: names,
// sizes, pack bodies).  Both nets hold the rows below kLayShared, an AtariFFNet adds [kLayShared, kLayFFNetEnd), an
// AtariLSTMNet [kLayFFNetEnd, kLayCount).
enum Layout {
  kLayB1, kLayb1, kLayB2, kLayb2, kLayB3, kLayb3, kLayBh, kLaybh, kLayW1d, kLayB2f, kLayB3f, kLayB2e, kLayB3e, kLayShared,
  kLayBf = kLayShared, kLayBfT, kLaybf, kLayBhp, kLayBff, kLayBfe, kLayFFNetEnd,
  kLayBl = kLayFFNetEnd, kLaybl, kLayWrec, kLayWx3, kLayCount
};
constexpr uint32_t lay_bit(int layout) { return 1u << layout; }

// does a net whose owner declared max_rows (0: no limit) pack the bf16 fc fragments (Bff)?
inline bool packs_bf16_fc(int max_rows) { return !(max_rows > 0 && max_rows < kFastTrunkMinN); }

// The layouts a load of an AtariFFNet packs.  A net whose owner never runs more than max_rows rows (a learner, which
// re-packs after every step) skips the fc layouts only larger batches read -- Bf (f32 fragments, N >= kFcSplitBelow),
// Bff (bf16 fragments, the split-K fc_bf16s serves 128 rows and up) -- and the layouts of the f32x3 mode its batches are
// too small for.  BfT (the f32 split-K fc's weights, 6.4 MB) of such a net in the split-bf16 mode: no kernel of that
// mode reads it from 128 rows up, so a load from device pointers leaves it out and the f32 path packs it on demand from
// the owner's buffer, which outlives the load (ffnet_forward_mode).
inline bool ffnet_bft_on_demand(int max_rows, int precision, bool on_device) {
  return max_rows >= kFastTrunkMinN && on_device && precision == kModeBf16x2;
}
inline uint32_t ffnet_pack_set(int max_rows, int precision, bool on_device) {
  uint32_t set = lay_bit(kLayFFNetEnd) - 1;
  const bool limited = max_rows > 0;
  if (limited && max_rows < kEmuConvMinN) set &= ~(lay_bit(kLayB2e) | lay_bit(kLayB3e));
  if (limited && max_rows < kEmuFcMinN) set &= ~lay_bit(kLayBfe);
  if (limited && max_rows < kFcSplitBelow) set &= ~lay_bit(kLayBf);
  if (!packs_bf16_fc(max_rows)) set &= ~lay_bit(kLayBff);
  if (ffnet_bft_on_demand(max_rows, precision, on_device)) set &= ~lay_bit(kLayBfT);
  return set;
}

// slices of the f32 split-K fc
inline int fc_splits(int N) {
  const int rb = (N + 127) / 128;
  const int sp = 32 / rb;
  return sp < 1 ? 1 : sp;
}

// slices of the bf16 split-K fc (~256 blocks; the partial tiles hold kFcPartRows rows); *per: positions per slice
inline int fc_bf16_slices(int N, int* per) {
  const int rb = (N + kFcBf16BlockRows - 1) / kFcBf16BlockRows;
  int slices = kPlanCUs / (4 * rb);
  slices = slices < kFcPositions ? slices : kFcPositions;
  slices = slices > 1 ? slices : 1;
  slices = slices < kFcPartRows / N ? slices : kFcPartRows / N;
  *per = (kFcPositions + slices - 1) / slices;
  return (kFcPositions + *per - 1) / *per;
}

struct FfnetPlan {
  int precision;    // the arithmetic that runs: 0 f32 | 1 bf16x2 | 2 f32x3
  TrunkKind trunk;
  FcKind fc;
  bool keep_f32;    // kModeF32x3KeepF32: a kTrunkS3 trunk writes a1 / a2 / a3 as f32 too
  bool unsplit_a3;  // kTrunkBf16 in front of an f32 fc: a3's records are turned back into f32 in place
  int fc_slices, fc_per;  // kFcF32SplitK: slices | kFcBf16SplitK: slices and positions per slice | else 1, 0
};

// the layouts the kernels of a plan read (ffnet_forward_mode refuses a plan whose layouts the net's load did not pack):
// the biases of conv2, conv3, fc and the heads with Bhp always, then by TrunkKind (conv1's bias is folded into W1d's tail)
// and by FcKind
inline uint32_t ffnet_plan_reads(const FfnetPlan& p) {
  const uint32_t trunk[3] = {lay_bit(kLayB1) | lay_bit(kLayb1) | lay_bit(kLayB2) | lay_bit(kLayB3),
                             lay_bit(kLayW1d) | lay_bit(kLayB2f) | lay_bit(kLayB3f),
                             lay_bit(kLayW1d) | lay_bit(kLayB2e) | lay_bit(kLayB3e)};
  const int fc[6] = {kLayBfT, kLayBf, kLayBff, kLayBff, kLayBfe, kLayBfe};
  return lay_bit(kLayb2) | lay_bit(kLayb3) | lay_bit(kLaybf) | lay_bit(kLayBhp) | lay_bit(kLaybh) | trunk[p.trunk] | lay_bit(fc[p.fc]);
}

// mode: an FfnetMode; net_precision: what rela_ffnet_set_precision left; max_rows: the rows limit of the call -- the
// net's own (ffnet_set_max_rows, 0: no limit) unless the caller of ffnet_forward_mode passes another
inline FfnetPlan plan_ffnet_forward(int mode, int net_precision, int N, int max_rows) {
  FfnetPlan p{};
  p.keep_f32 = mode == kModeF32x3KeepF32;
  p.precision = mode < 0 ? net_precision : (mode == kModeF32x3KeepF32 ? (int)kModeF32x3 : mode);
  p.fc_slices = 1;
  // (a net packed for small batches only has no bf16 fc fragments: it keeps the f32 fc whatever the threshold says)
  const int fast_min_n = (max_rows > 0 && max_rows < kFastMinN) ? max_rows + 1 : kFastMinN;
  if (p.precision == kModeBf16x2 && N >= fast_min_n) {
    // split-bf16 fast path: a2 / a3 hold split records (same bytes as the f32 tensors they replace)
    p.trunk = kTrunkBf16, p.fc = kFcBf16;
    return p;
  }
  if (p.precision == kModeBf16x2 && N >= kFastTrunkMinN) {
    // Between kFastTrunkMinN and kFastMinN rows the convolutions still win on split-bf16 MFMA (N = 512: 39 us against
    // 90 us in f32) but fc_bf16s has too few blocks (55 us against the 24 us of the f32 split-K GEMM): fc runs as a
    // split-K launch of fc_bf16s straight from a3's records (r3; the f32 split-K GEMM after an unsplit pass took
    // 21 + 6 + 6 us at 512 rows) ...
    p.trunk = kTrunkBf16;
    if (packs_bf16_fc(max_rows)) {
      p.fc = kFcBf16SplitK;
      p.fc_slices = fc_bf16_slices(N, &p.fc_per);
      return p;
    }
    p.unsplit_a3 = true;  // ... or, in a net without the bf16 fc fragments, a3 goes back to f32 and fc takes the f32 path
  } else if (p.precision == kModeF32x3 && N >= kEmuConvMinN && N <= kEmuMaxN && !(max_rows > 0 && max_rows < kEmuConvMinN)) {
    // f32x3: the trunk on split3 records, fc as gemm_s3 (small batches: the contraction split over blocks, as far as
    // the partial tiles' space goes)
    p.trunk = kTrunkS3;
    p.fc = (N < kFcSplitBelow && (int64_t)8 * N <= kFcPartRows) ? kFcS3SplitK : kFcS3;
    return p;
  } else {
    p.trunk = kTrunkF32;
  }
  if (N < kFcSplitBelow) {
    p.fc = kFcF32SplitK;
    p.fc_slices = fc_splits(N);
  } else {
    p.fc = kFcF32Gemm;
  }
  return p;
}

// conv trunk of an AtariLSTMNet.  fast: split-bf16 asked for | emu: f32x3 asked for | has_rec_scratch: the caller has
// N * (kRec2Bytes + kRec3Bytes) bytes for split3 records | want_records: a3 may stay in split-bf16 records
struct LstmTrunkPlan {
  TrunkKind trunk;
  bool a3_records;  // a3 is left as records: split3 at the scratch's a3 part (kTrunkS3), split-bf16 in a3's place (kTrunkBf16)
};
inline LstmTrunkPlan plan_lstm_trunk(bool fast, bool emu, bool has_rec_scratch, int N, bool want_records) {
  if (emu && has_rec_scratch && N >= kEmuConvMinN && N <= kEmuMaxN) return {kTrunkS3, true};
  if (fast && N >= kFastTrunkMinN) return {kTrunkBf16, want_records};
  // (f32x3 without record scratch, or below its batch threshold: the exact f32 kernels -- same accuracy)
  return {kTrunkF32, false};
}

// batches the Ape-X learner's merged split-bf16 forward serves (ffnet_learner_forward: 2 B rows through the online net)
inline bool learner_merged_rows(int B) { return B >= kFastTrunkMinN && 2 * B < kFcSplitBelow; }

}  // namespace rela_amd
