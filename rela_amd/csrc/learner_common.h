// learner_common.h -- the interface of what the two hand-written learner steps share (learner.hip: Ape-X / AtariFFNet;
// learner_r2d2.hip: R2D2 / AtariLSTMNet), and the templates both use for GEMMs of their own: the tile sets and the one
// dispatch that obeys the backward plan (learner_plan.h).  The shared kernels -- the conv trunk's backward pass, column
// sums, the heads' weight gradient, global-norm clipping, the optimisers, the Polyak update -- are compiled once, in
// learner_common.hip; here are their launchers' prototypes, the structs they take and the constants their callers size
// buffers with.  Host side, at the end: LearnerCore, the base of rela_apex_learner and rela_r2d2_learner: the flat
// parameter / gradient / optimiser-state store and what the entry points do with it (its device buffers belong to a
// DevBuffers, common.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"
#include "ffnet_layout.h"
#include "gemm_lds.h"
#include "gemm_bf16x3.h"
#include "learner_plan.h"
#include "param_layout.h"
#include "prof.h"
#include "weight_pack.h"

namespace rela_amd {

using namespace gemm;

// ---- the tiles of the learners' GEMMs, by shape and arithmetic --------------------------------------------------------
// A shape's f32 tile runs on gemm_lds (f32 MFMA).  The two-part tile runs on the bf16 matrix cores (gemm_bf16x3.h: operands
// split into bf16 hi + lo on the way into LDS, three MFMAs per product): the learners' bf16x2 mode.  The three-part tile
// (PARTS = 3, six products) has f32 accuracy on the bf16 MFMA: the f32x3 modes.
// (the tiles only the conv trunk uses: learner_common.hip; the R2D2 learner's: learner_r2d2.hip)
using TileDgrad = TileCfg<128, 64, 4, 2, false>;  // M = batch rows, A k-contiguous
using Tile3Dgrad = gemm3::TileCfg<128, 64, 4, 2, false>;
using Tile6Dgrad = gemm3::TileCfg<128, 64, 4, 2, false, 3>;
using TileWfc = TileCfg<128, 64, 4, 2, true>;     // fc weight gradient (M = 512 units)
using Tile3Wfc = gemm3::TileCfg<128, 64, 4, 2, true>;
using Tile6Wfc = gemm3::TileCfg<128, 64, 4, 2, true, 3>;
// the three-part 64 x 64 tile of the conv2 / conv3 weight gradients (SetW64, learner_common.hip) and of the R2D2
// learner's dW_hh / dW_ih (Tile6Wg, learner_r2d2.hip)
using Tile6W64 = gemm3::TileCfg<64, 64, 2, 4, true, 3>;
using TileW32 = TileCfg<32, 64, 2, 4, true>;      // head weight gradients (M = 32)
using Tile3W32 = gemm3::TileCfg<32, 64, 2, 4, true>;
using Tile6W32 = gemm3::TileCfg<32, 64, 2, 4, true, 3>;

// The tiles of one GEMM shape: f32 | two-part | three-part.  void: that arithmetic never reaches the shape -- no kernel is
// instantiated for it, and a plan that asks for it is an internal error.
template <class F32, class X2, class X3>
struct TileSet {
  using f32 = F32;
  using x2 = X2;
  using x3 = X3;
};
using SetDgrad = TileSet<TileDgrad, Tile3Dgrad, Tile6Dgrad>;  // dgrad rows (heads, fc)
using SetWfc = TileSet<TileWfc, Tile3Wfc, Tile6Wfc>;          // fc weight gradient
using SetW32 = TileSet<TileW32, Tile3W32, Tile6W32>;          // 32-row head weight gradients

// the one way a learner GEMM is launched: the slot of `arith` in the shape's set (split-K, stream, names as launch_gemm)
template <class Set, class P>
int launch_gemm_as(GemmArith arith, const P& p, int splits, hipStream_t s, const char* name) {
  if constexpr (!std::is_void_v<typename Set::f32>)
    if (arith == kArithF32) return launch_gemm<typename Set::f32>(p, splits, s, name), RELA_OK;
  if constexpr (!std::is_void_v<typename Set::x2>)
    if (arith == kArithBf16x2) return gemm3::launch_gemm<typename Set::x2>(p, splits, s, name);
  if constexpr (!std::is_void_v<typename Set::x3>)
    if (arith == kArithF32x3) return gemm3::launch_gemm<typename Set::x3>(p, splits, s, name);
  set_last_error("%s: no tile for arithmetic %d (internal error: the plan and the tile sets disagree)", name, (int)arith);
  return RELA_ESTATE;
}

// ---- column sums (bias gradients): two deterministic stages ----------------------------------
constexpr int kColsumBlocks = 256;
// several column sums in ONE launch pair (the five bias gradients of a learner step were ten ~7 us launches):
// blockIdx.y selects the job; every job keeps the two-stage order of colsum_partial / colsum_final, so the results
// are bit-identical to separate launches.
constexpr int kMaxColsumJobs = 6;
struct ColsumJobs {
  const float* src[kMaxColsumJobs];
  float* out[kMaxColsumJobs];
  float* part[kMaxColsumJobs];  // kColsumBlocks * C floats each
  int64_t rows[kMaxColsumJobs];
  int C[kMaxColsumJobs];
  int n = 0;
  void add(const float* s, int64_t r, int c, float* o) { src[n] = s, rows[n] = r, C[n] = c, out[n] = o, ++n; }
};
// all queued jobs in one launch pair; cpart must hold kColsumBlocks * (sum of the jobs' C) floats
void colsum_multi_launch(ColsumJobs& jobs, float* cpart, hipStream_t s);
// one column sum of src [rows][C], C in {32, 64, 512, 2048}; cpart: kColsumBlocks * C floats
void colsum_launch(const float* src, int64_t rows, int C, float* cpart, float* out, hipStream_t s);
// the heads' bias gradients from the 32 column sums of d_ha: g_a_b[0..A-1] = s32[0..A-1], g_v_b[0] = s32[31]
void launch_head_bias_grad(const float* s32, int A, float* g_a_b, float* g_v_b, hipStream_t s);
// the heads' weight gradient in one GEMM: dWh[k][u] = sum_b d_ha[b][k] * h[b][u] over `rows` rows, rows 0..A-1 into
// g_a_w, row 31 into g_v_w (SetW32 in `arith`; named "learner_wgrad_heads")
int launch_head_wgrad(GemmArith arith, int rows, int A, const float* d_ha, const float* h, float* g_a_w, float* g_v_w,
                      hipStream_t s);

// ---- backward pass of the conv trunk (net.{0,2,4}), shared by both learners ---------------------
// (which kernels run, their split counts and thresholds: plan_trunk_backward, learner_plan.h)
// the largest partial buffer: conv3's split-K tiles, or one tile per block of the bf16 conv1 ([32][256]) / conv2
// ([64][512]) gradients (256 blocks at the most; learner_common.hip checks it against the kernels' own constants)
constexpr size_t kTrunkPartFloats = (size_t)256 * 64 * 576;
// the conv2 / conv3 data-gradient weight fragments of the bf16x2 mode (dgrad_conv_bf16.h), for a caller that keeps them
// across steps: pack_dgrad_frags when the weights change, TrunkBwd::frag2 / frag3
constexpr size_t kFrag2Bytes = (size_t)4 * 2 * 8 * 2 * 64 * 16, kFrag3Bytes = (size_t)4 * 18 * 2 * 64 * 16;
void pack_dgrad_frags(const float* w2p, const float* w3p, void* frag2, void* frag3, hipStream_t s);

// the most frames of one trunk_backward call: the data gradients put frames * 100 / 64 (conv2) and frames * 81 / 64
// (conv3) tiles on the grid's y axis
constexpr int kTrunkMaxFrames = 32768;
struct TrunkBwd {
  int Bn;              // frames
  const uint8_t* obs;  // [Bn][4][84][84] u8
  const float *a1, *a2;  // relu(conv1), relu(conv2), channel-last (ffnet_layout.h)
  const float* d_a3;   // [Bn][49][64] gradient w.r.t. relu(conv3), ALREADY masked by a3 > 0
  float *d_a2, *d_a1;  // scratch [Bn][81][64], [Bn][400][32]
  float* part;         // scratch, kTrunkPartFloats
  float* cpart;        // scratch, kColsumBlocks * 512
  const float *w2p, *w3p;  // conv2 / conv3 weights in dgrad k order (permute_weight_at, ffnet_layout.h)
  float *g_c1w, *g_c1b, *g_c2w, *g_c2b, *g_c3w, *g_c3b;  // gradients, state_dict layout
  // What runs: the learner's TrunkArith for Bn frames (learner_plan.h).  bf16x2: the weight gradients on the dedicated bf16
  // kernels (conv2 / conv3 from kFastWgradMinFrames frames), the data gradients on dgrad_conv_bf16.h.  f32x3: the weight-gradient
  // GEMMs (contraction over batch x positions) on the bf16 MFMA with three-part operands, f32 accuracy (r4 at 512 frames, us
  // f32 -> three-part: conv3 49 -> 35, conv2 63 -> 52, conv1 110 -> 102).
  TrunkBwdPlan plan;
  // Two-lane form (the Ape-X learner): conv3's and conv2's weight gradients, and the column sums of every tensor that
  // exists by then (the caller's pending jobs, d_a3, d_a2), run on `side` next to the data-gradient chain on the
  // caller's stream; the caller's stream waits for the side lane before trunk_backward returns.  Every kernel computes
  // what it computes on one lane (same grids, same summation orders): the results are bit-identical.
  hipStream_t side = nullptr;
  hipEvent_t ev_da3 = nullptr, ev_da2 = nullptr, ev_side = nullptr;
  float *part_side = nullptr, *cpart_side = nullptr;  // the side lane's own `part` / `cpart`
  const void *frag2 = nullptr, *frag3 = nullptr;  // dgrad weight fragments packed ahead (else per call, into `part`)
  const float* s32 = nullptr;                     // (side lane) head_bias_grad after the column sums
  float *g_a_b = nullptr, *g_v_b = nullptr;
  int A = 0;
};
// `to` continues only after everything queued on `from` so far
inline void lane_dep(hipEvent_t ev, hipStream_t from, hipStream_t to) {
  (void)hipEventRecord(ev, from);
  (void)hipStreamWaitEvent(to, ev, 0);
}
// `jobs`: the caller's pending column sums; the three bias gradients of the trunk are queued behind them and the
// whole queue goes out in one launch pair at the end (t.cpart: kColsumBlocks * (sum of all queued C) floats)
int trunk_backward(const TrunkBwd& t, hipStream_t s, ColsumJobs* pending = nullptr);

// what a backward tap keeps for its one call (rela_debug_trunk_backward here, rela_debug_head_fc_backward in learner.hip):
// scratch, and the side lane with its events
struct TrunkTapScratch {
  DevBuffers mem;
  hipStream_t side = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~TrunkTapScratch() {
    mem.free_all();
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (side) (void)hipStreamDestroy(side);
  }
};
// one of the dgrad operand copies on its own, as a pack list of one segment (the learners' re-pack makes them in its launch)
int permute_weight(int mode, const float* src, float* dst, hipStream_t s);

// ---- clip_grad_norm_ + optimiser over flat parameter / gradient / state buffers -------------------
constexpr int kNormBlocks = 256;
struct OptimState {
  int optimizer = 0;  // 0 RMSprop, 1 Adam
  float lr = 0.f, eps = 0.f, clip = 0.f;
  int64_t adam_t = 0;
  // torch's defaults; *_learner_set_rmsprop / _set_adam_betas change them while the state is the zero state
  float alpha = 0.99f;    // RMSprop's decay
  bool centered = false;  // RMSprop: S2 = the gradient average, rmsprop_centered_update (else S2 is never touched)
  float b1 = 0.9f, b2 = 0.999f;  // Adam's betas
};
// the ranges of the option setters and of rela_debug_optimizer_apply_opts (a NaN fails every comparison)
inline bool rmsprop_options_ok(float alpha, int centered) { return alpha > 0.f && alpha < 1.f && (centered == 0 || centered == 1); }
inline bool adam_betas_ok(float b1, float b2) { return b1 >= 0.f && b1 < 1.f && b2 > 0.f && b2 < 1.f; }
// adam_t counts every Adam apply launched; one that the device skipped (abort_word) adds one to *skipped, which the
// owner of abort_word takes off adam_t again once it has read the word.  census: rela_debug_optimizer_apply counts its
// three launches (the learners' steps do not: their censuses are recorded ones).  npart: kNormBlocks doubles.
void optimizer_apply(OptimState& o, float* P, const float* G, float* S1, float* S2, int64_t n, double* npart, float* norm,
                     hipStream_t s, const unsigned* abort_word = nullptr, unsigned* skipped = nullptr, bool census = false);
// soft (Polyak) target update over flat buffers of 4 * n4 floats: pt = pt + tau * (p - pt)
void launch_target_lerp(float* pt, const float* p, int64_t n4, float tau, hipStream_t s);

// ---- what the two learners share on the host ------------------------------------------------------------------------
// The flat store: P (online), PT (target), G (gradients), S1 / S2 (optimiser state), each off[nseg] floats with the
// net's tensors at off[i] (param_layout.h).  The functions are the bodies of the rela_*_learner_* entry points, which
// check their handle, select the device, pass their own name (`who` leads every message) and re-pack the
// kernel-layout weight copies afterwards (each learner's own repack).
struct LearnerCore {
  int device = 0;
  int A = 0, Bmax = 0;
  float gamma_n = 0.f;
  float vr_eps = 0.f;        // value rescaling of the TD target (set_value_rescale), 0 = off
  bool loss_called = false;  // ... which is fixed from the first loss on
  OptimState opt;
  bool applied = false;  // an apply was launched since create / the last load: S1 / S2 are no longer the zero state
  int nseg = 0;
  int64_t cnt[kLstmNetSegs] = {0};      // elements per tensor
  int64_t off[kLstmNetSegs + 1] = {0};  // segment offsets, off[nseg] = total
  float *P = nullptr, *PT = nullptr, *G = nullptr, *S1 = nullptr, *S2 = nullptr;
  double* npart = nullptr;
  float* norm = nullptr;  // [0] grad norm, [1] clip coefficient
  float* loss = nullptr;
  bool loaded = false;
  DevBuffers mem;  // every device buffer of the learner

  // counts: ffnet_param_counts / lstmnet_param_counts (param_layout.h) with their kFFNetSegs / kLstmNetSegs
  int alloc_flat(int nseg_, void (*counts)(int, int64_t*), int num_action) {
    nseg = nseg_;
    counts(num_action, cnt);
    flat_offsets(cnt, nseg, off);
    for (float** p : {&P, &PT, &G, &S1, &S2})
      if (int rc = mem.alloc(p, (size_t)off[nseg], true)) return rc;
    if (int rc = mem.alloc(&npart, kNormBlocks, false)) return rc;
    if (int rc = mem.alloc(&norm, 2, true)) return rc;  // (zeroed: stats before the first apply reads zeros)
    return mem.alloc(&loss, 1, true);
  }
  // online / target: the net's params struct, nseg pointers (target may be null: the online tensors twice)
  int load(const char* who, const void* online, const void* target, int on_device, hipStream_t s) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const float* const* fo = static_cast<const float* const*>(online);
    const float* const* ft = static_cast<const float* const*>(target ? target : online);
    for (int i = 0; i < nseg; ++i) {
      RELA_CHECK(fo[i] && ft[i], RELA_EINVAL, "%s: parameter %d is NULL", who, i);
      RELA_HIP(hipMemcpyAsync(P + off[i], fo[i], sizeof(float) * cnt[i], kind, s));
      RELA_HIP(hipMemcpyAsync(PT + off[i], ft[i], sizeof(float) * cnt[i], kind, s));
    }
    if (!on_device) RELA_HIP(hipStreamSynchronize(s));  // the host buffers may go away
    const size_t nb = sizeof(float) * (size_t)off[nseg];
    RELA_HIP(hipMemsetAsync(S1, 0, nb, s));
    RELA_HIP(hipMemsetAsync(S2, 0, nb, s));
    opt.adam_t = 0;
    applied = false;  // (the options and the learning rate stay)
    return RELA_OK;
  }
  int copy_online_to_target(hipStream_t s) {  // apex.py:27
    RELA_HIP(hipMemcpyAsync(PT, P, sizeof(float) * (size_t)off[nseg], hipMemcpyDeviceToDevice, s));
    return RELA_OK;
  }
  // Polyak update of the target net: PT += tau * (P - PT) over the whole flat buffer; tau == 1 is the copy, bit for bit
  int soft_update_target(float tau, hipStream_t s) {
    if (tau == 1.0f) return copy_online_to_target(s);
    launch_target_lerp(PT, P, off[nseg] / 4, tau, s);
    RELA_LAUNCH_CHECK();
    return RELA_OK;
  }
  // the checks of rela_*_learner_soft_update_target; the caller then selects the device, calls soft_update_target and re-packs
  int check_soft_update(const char* who, float tau) const {
    RELA_CHECK(tau > 0.f && tau <= 1.f, RELA_EINVAL, "%s: tau must be in (0, 1] (got %g)", who, (double)tau);
    RELA_CHECK(loaded, RELA_ESTATE, "%s: parameters were never loaded", who);
    return RELA_OK;
  }
  int set_lr(const char* who, float lr) {
    RELA_CHECK(lr >= 0.f && lr <= 3.402823466e+38f, RELA_EINVAL, "%s: lr must be finite and >= 0 (got %g)", who, (double)lr);
    opt.lr = lr;  // the next apply passes it to its update kernel; no state, no step number
    return RELA_OK;
  }
  int get_lr(const char* who, float* out) const {
    RELA_CHECK(out, RELA_EINVAL, "%s: bad arguments", who);
    *out = opt.lr;
    return RELA_OK;
  }
  // The two option setters: only while S1 / S2 are the zero state (after create or a load, before the first apply since):
  // S2 changes its meaning with `centered`, and a decay that changes under a running average has no counterpart in torch.
  int set_rmsprop(const char* who, float alpha, int centered) {
    RELA_CHECK(opt.optimizer == 0, RELA_EINVAL, "%s: this learner's optimiser is Adam, not RMSprop", who);
    RELA_CHECK(rmsprop_options_ok(alpha, centered), RELA_EINVAL, "%s: alpha must be in (0, 1) and centered 0 or 1 (got %g, %d)",
               who, (double)alpha, centered);
    RELA_CHECK(!applied, RELA_ESTATE, "%s: call it before the first apply after create or load", who);
    opt.alpha = alpha, opt.centered = centered != 0;
    return RELA_OK;
  }
  int set_adam_betas(const char* who, float b1, float b2) {
    RELA_CHECK(opt.optimizer == 1, RELA_EINVAL, "%s: this learner's optimiser is RMSprop, not Adam", who);
    RELA_CHECK(adam_betas_ok(b1, b2), RELA_EINVAL, "%s: betas must be in [0, 1) and (0, 1) (got %g, %g)", who, (double)b1,
               (double)b2);
    RELA_CHECK(!applied, RELA_ESTATE, "%s: call it before the first apply after create or load", who);
    opt.b1 = b1, opt.b2 = b2;
    return RELA_OK;
  }
  // params_out: the net's params struct; its nseg pointers into the flat buffer at `base`
  void params_at(const float* base, void* params_out) const {
    const float** f = static_cast<const float**>(params_out);
    for (int i = 0; i < nseg; ++i) f[i] = base + off[i];
  }
  int flat(float** params_dev, float** grads_dev, int64_t* count) const {
    if (params_dev) *params_dev = P;
    if (grads_dev) *grads_dev = G;
    if (count) *count = off[nseg];
    return RELA_OK;
  }
  int set_value_rescale(const char* who, float eps) {
    RELA_CHECK(eps == eps, RELA_EINVAL, "%s: bad arguments", who);
    RELA_CHECK(!loss_called, RELA_ESTATE, "%s: call it before the first loss", who);
    vr_eps = eps > 0.f ? eps : 0.f;
    return RELA_OK;
  }
  void apply(hipStream_t s, const unsigned* abort_word = nullptr, unsigned* skipped = nullptr) {
    optimizer_apply(opt, P, G, S1, S2, off[nseg], npart, norm, s, abort_word, skipped);
    applied = true;  // (also when the device skips it on the abort word: the host cannot know yet)
  }
  int debug_optim(const char* who, float** s1_dev, float** s2_dev, int64_t* adam_t) const {
    RELA_CHECK(s1_dev && s2_dev && adam_t, RELA_EINVAL, "%s: bad arguments", who);
    *s1_dev = S1, *s2_dev = S2, *adam_t = opt.adam_t;
    return RELA_OK;
  }
};

}  // namespace rela_amd
