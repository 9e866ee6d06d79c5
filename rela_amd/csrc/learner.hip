// Ape-X learner step on the device: pyrela/main.py:206-251 with ApexAgent.loss (apex.py:80-91),
// i.e.  sample -> td_err -> smooth_l1 * IS weight -> mean -> backward -> clip_grad_norm_ ->
// RMSprop -> (update_priority by the caller).  Replaces PyTorch autograd on the hot path
// (SURVEY 8f-2); AtariFFNet only (net.py:8-55).
//
//   forward   three rela_ffnet_forward calls (csrc/ffnet.hip); the online(obs) pass leaves its
//             activations a1/a2/a3/h in the workspace (ffnet_layout.h) for the backward pass
//   loss      rela_apex_td_from_q (signed TD error, batch-global q.min() as in apex.py:51) +
//             learner_loss_grad: Huber' * w / B pushed through the dueling head -> d_ha [B][32]
//   backward  every contraction is one instance of gemm_lds (both operands staged through LDS,
//             v_mfma_f32_16x16x4_f32, f32 throughout):
//               dgrad  d_h   = d_ha  x Wh            (relu mask in the epilogue)
//                      d_a3  = d_h   x Wfc'          (Wfc' = fc weight in channel-last k order)
//                      d_a2  = convT(d_a3, W3'), d_a1 = convT_stride2(d_a2, W2'): rows = the layer's input pixels,
//                              k = (tap, output channel), the gather of the output pixels in the A loader
//               wgrad  dWh   = d_ha^T x h,  dWfc = d_h^T x a3,
//                      dW3 = d_a3'^T x im2col(a2), dW2 = d_a2'^T x im2col(a1), dW1 = d_a1'^T x im2col(s)
//                      (im2col is index arithmetic in the B loader; the long reductions over
//                      B*pos are split over blockIdx.z into partial tiles that reduce_splits sums
//                      in a fixed order -- deterministic, no atomics)
//             bias gradients are column sums (colsum_*).
//   update    one flat parameter / gradient / optimiser-state buffer in state_dict order:
//             global 2-norm -> clip coefficient -> RMSprop (torch defaults alpha = 0.99), then the
//             kernel-layout copies of the new weights are re-packed.
// The gradient buffer is exposed (rela_apex_learner_flat) so data-parallel learners all-reduce
// it between rela_apex_learner_backward and rela_apex_learner_apply.
#include "learner_common.h"
#include "value_rescale.h"

using namespace rela_amd;

namespace rela_amd {
namespace {

// ---- the Problems of this learner's own GEMMs (heads and fc; the tiles: learner_common.h) -----------------------------
// d_h[b][u] = relu'(h) * sum_k d_ha[b][k] * Wh[k][u]      Wh rows: 0..A-1 = fc_a.weight, 31 = fc_v.weight
struct ProbHeadDgrad : ProbBase {
  const float *d_ha, *a_w, *v_w, *h;
  float* d_h;
  int A;
  __device__ float4 fetchA(int m, int k) const { return ld4(d_ha + (size_t)min(m, M - 1) * 32 + k); }
  __device__ float4 fixA(float4 v, int m, int) const { return keep4(m < M, v); }
  __device__ float4 fetchB(int k, int n) const {  // (rows A .. 30 fetch fc_v's row and are zeroed)
    const float* row = k < A ? a_w + (size_t)k * 512 : v_w;
    return ld4(row + n);
  }
  __device__ float4 fixB(float4 v, int k, int) const { return keep4(k < A || k == 31, v); }
  __device__ void store(int, int m, int n, float v) const {
    const size_t i = (size_t)m * 512 + n;
    d_h[i] = h[i] > 0.f ? v : 0.f;
  }
};

// d_a3[b][j] = relu'(a3) * sum_u d_h[b][u] * Wfc'[u][j]     j = pos*64 + c (channel-last)
struct ProbFcDgrad : ProbBase {
  const float *d_h, *wfcp, *a3;
  float* d_a3;
  __device__ float4 fetchA(int m, int k) const { return ld4(d_h + (size_t)min(m, M - 1) * 512 + k); }
  __device__ float4 fixA(float4 v, int m, int) const { return keep4(m < M, v); }
  __device__ float4 fetchB(int k, int n) const { return ld4(wfcp + (size_t)k * 3136 + n); }
  __device__ void store(int, int m, int n, float v) const {
    const size_t i = (size_t)m * 3136 + n;
    d_a3[i] = a3[i] > 0.f ? v : 0.f;
  }
};

// dWfc[u][c*49+pos] = sum_b d_h[b][u] * a3[b][pos*64+c]   (written in state_dict order, net.py:49)
struct ProbFcWgrad : ProbBase {
  const float *d_h, *a3;
  float* g_fc_w;
  __device__ float4 fetchA(int b, int m) const { return ld4(d_h + (size_t)min(b, K - 1) * 512 + m); }
  __device__ float4 fetchB(int b, int n) const { return ld4(a3 + (size_t)min(b, K - 1) * 3136 + n); }
  __device__ float4 fixA(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ float4 fixB(float4 v, int b, int) const { return keep4(b < K, v); }
  __device__ void store(int, int m, int n, float v) const {
    const int pos = n >> 6, c = n & 63;
    g_fc_w[(size_t)m * 3136 + c * 49 + pos] = v;
  }
};

// ---- loss: smooth_l1(err) * w, mean over the batch (apex.py:87, main.py:228), and its gradient
// through the dueling head  q = v + a*legal - mean_A(a*legal)  (net.py:33-39) --------------------
__global__ __launch_bounds__(kLT) void learner_loss_grad(const float* __restrict__ td, const float* __restrict__ w,
                                                         const int64_t* __restrict__ act,
                                                         const float* __restrict__ legal, int Bn, int A,
                                                         float* __restrict__ d_ha, float* __restrict__ loss_out) {
  __shared__ float red[kLT];
  float lsum = 0.f;
  const float inv_b = 1.0f / (float)Bn, inv_a = 1.0f / (float)A;
  for (int i = threadIdx.x; i < Bn; i += kLT) {
    const float e = td[i], ae = fabsf(e);
    lsum += (ae < 1.0f ? 0.5f * e * e : ae - 0.5f) * w[i];
    // err = target - q[a]:  d mean(loss*w) / d q[a] = -w * clamp(err, -1, 1) / B
    const float g = -(w[i] * fminf(fmaxf(e, -1.0f), 1.0f)) * inv_b;
    const int a = (int)act[i];
    float* row = d_ha + (size_t)i * 32;
    for (int k = 0; k < 32; ++k) {
      float v = 0.f;
      if (k < A) v = legal[(size_t)i * A + k] * (g * ((k == a ? 1.0f : 0.0f) - inv_a));
      if (k == 31) v = g;
      row[k] = v;
    }
  }
  red[threadIdx.x] = lsum;
  __syncthreads();
  for (int o = kLT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[0] = red[0] * inv_b;
}

// td_err (apex.py:30-45: batch-global q.min() of greedy_act(next_obs), double-DQN target, un-fused arithmetic as
// agent_ops.hip's td_kernel) + the loss kernel above in ONE single-workgroup launch (two latency-bound launches
// before: 15 + 19 us).  Same arithmetic in the same order, so priorities, loss and d_ha are bit-identical.
__global__ __launch_bounds__(1024) void learner_td_loss_grad(int Bn, int A, const float* __restrict__ q,
                                                             const float* __restrict__ qno, const float* __restrict__ qnt,
                                                             const float* __restrict__ nlegal,
                                                             const int64_t* __restrict__ act,
                                                             const float* __restrict__ reward,
                                                             const float* __restrict__ bootstrap, float gamma_n,
                                                             float vr_eps, const float* __restrict__ w,
                                                             const float* __restrict__ legal,
                                                             float* __restrict__ td, float* __restrict__ prio,
                                                             float* __restrict__ d_ha, float* __restrict__ loss_out) {
  __shared__ float red[1024];
  float m = INFINITY;
  for (int i = threadIdx.x; i < Bn * A; i += 1024) m = fminf(m, qno[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + off]);
    __syncthreads();
  }
  const float qmin = red[0];
  __syncthreads();
  float lsum = 0.f;
  const float inv_b = 1.0f / (float)Bn, inv_a = 1.0f / (float)A;
  for (int i = threadIdx.x; i < Bn; i += 1024) {
    int na = 0;
    float bv = -INFINITY;
#pragma unroll 6  // (the loads of several actions in flight: one at a time this loop was most of the kernel's 19 us)
    for (int j = 0; j < A; ++j) {  // greedy_act(next_obs): first maximal index of (1 + q - qmin) * legal (apex.py:51)
      const float lq = __fmul_rn(__fsub_rn(__fadd_rn(1.0f, qno[(size_t)i * A + j]), qmin), nlegal[(size_t)i * A + j]);
      if (lq > bv) bv = lq, na = j;
    }
    const int a = (int)act[i];
    const float qa = q[(size_t)i * A + a];
    const float bq = qnt[(size_t)i * A + na];
    float tgt;  // detached: with value rescaling (value_rescale.h) only the target changes, the Huber seed below keeps its formula
    if (vr_eps > 0.0f)
      tgt = rela_vr::h(__fadd_rn(reward[i], __fmul_rn(__fmul_rn(bootstrap[i], gamma_n), rela_vr::h_inv(bq, vr_eps))), vr_eps);
    else
      tgt = __fadd_rn(reward[i], __fmul_rn(__fmul_rn(bootstrap[i], gamma_n), bq));
    const float e = __fsub_rn(tgt, qa), ae = fabsf(e);
    td[i] = e;
    prio[i] = ae;
    lsum += (ae < 1.0f ? 0.5f * e * e : ae - 0.5f) * w[i];
    const float g = -(w[i] * fminf(fmaxf(e, -1.0f), 1.0f)) * inv_b;
    float4* row = reinterpret_cast<float4*>(d_ha + (size_t)i * 32);
    float v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      v[k] = 0.f;
      if (k < A) v[k] = legal[(size_t)i * A + k] * (g * ((k == a ? 1.0f : 0.0f) - inv_a));
      if (k == 31) v[k] = g;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  }
  // the same tree as learner_loss_grad's kLT = 512 lanes when Bn <= 512: lanes >= 512 hold zeros and fold in first
  red[threadIdx.x] = lsum;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_out[0] = red[0] * inv_b;
}

}  // namespace
}  // namespace rela_amd

// flat parameter layout: rela_ffnet_params order (LearnerCore, learner_common.h)
static_assert(sizeof(rela_ffnet_params) == kFFNetSegs * sizeof(float*), "rela_ffnet_params is kFFNetSegs pointers");
struct rela_apex_learner : LearnerCore {
  rela_ffnet *online = nullptr, *target = nullptr;
  float *w2p = nullptr, *w3p = nullptr, *wfcp = nullptr;  // dgrad operand copies
  uint8_t *ws_on = nullptr, *ws_tmp = nullptr;
  int64_t ws_bytes = 0;
  float *q = nullptr;  // [3][B][A]
  float *td = nullptr, *d_ha = nullptr, *d_h = nullptr, *d_a3 = nullptr, *d_a2 = nullptr, *d_a1 = nullptr;
  float *part = nullptr;   // split-K partial tiles
  float *cpart = nullptr;  // colsum partials [64][512]
  float *s32 = nullptr;
  // batch of the last rela_apex_learner_loss, until rela_apex_learner_grad consumes it
  int pend_B = 0, last_B = 0;
  int pend_rows = 0;  // rows of the ffnet_ws layout the last forward used for ws_on (B, or 2 B for the merged forward)
  const uint8_t* pend_obs = nullptr;
  // The side lane of the backward pass (TrunkBwd in learner_common.h): the weight gradients of heads, fc, conv3 and
  // conv2, the column sums and the records -> f32 conversion of the forward's activations run on `side` next to the
  // data-gradient chain on the caller's stream; RELA_LEARNER_LANES=1 keeps everything on the caller's stream.
  hipStream_t side = nullptr;
  hipEvent_t ev[8] = {nullptr};  // 0 forward done | 1 unsplit done | 2 d_ha | 3 d_h | 4 d_a3 | 5 d_a2 | 6 side lane done
  float *part_side = nullptr, *cpart_side = nullptr;
  uint8_t *frag2 = nullptr, *frag3 = nullptr;  // conv2 / conv3 data-gradient weight fragments, re-packed with the weights
};

namespace {
rela_ffnet_params params_at(const rela_apex_learner* l, const float* base) {
  rela_ffnet_params p;
  l->params_at(base, &p);
  return p;
}

int repack(rela_apex_learner* l, bool online, bool target, hipStream_t s) {
  if (online) {
    const rela_ffnet_params p = params_at(l, l->P);
    ExtraPacks extra;  // the dgrad operand copies ride along in the re-pack launch
    extra.w2p = l->w2p, extra.w3p = l->w3p, extra.wfcp = l->wfcp;
    int rc = ffnet_load_extra(l->online, &p, s, extra);
    if (rc != RELA_OK) return rc;
    if (l->frag2) pack_dgrad_frags(l->w2p, l->w3p, l->frag2, l->frag3, s);
  }
  if (target) {
    const rela_ffnet_params p = params_at(l, l->PT);
    int rc = rela_ffnet_load(l->target, &p, 1, s);
    if (rc != RELA_OK) return rc;
  }
  return RELA_OK;
}

// ---- loss and head gradient d_ha from the three Q tables: what rela_apex_learner_loss launches after its forwards ----
// fused: learner_td_loss_grad, one workgroup (the learner: batch <= kFusedLossMaxBatch); else td_from_q + learner_loss_grad
constexpr int kFusedLossMaxBatch = 1024;
int launch_loss_grad(int Bn, int A, bool fused, const float* q_on, const float* q_no, const float* q_nt, const float* nlegal,
                     const int64_t* act, const float* reward, const float* boot, float gamma_n, float vr_eps,
                     const float* weight, const float* legal, float* td, float* prio, float* d_ha, float* loss, hipStream_t s) {
  if (fused) {
    ProfScope prof("learner_loss_grad", s);
    note_launch("learner_td_loss_grad");
    hipLaunchKernelGGL(learner_td_loss_grad, dim3(1), dim3(1024), 0, s, Bn, A, q_on, q_no, q_nt, nlegal, act, reward, boot,
                       gamma_n, vr_eps, weight, legal, td, prio, d_ha, loss);
  } else {
    int rc = td_from_q(Bn, A, 0, q_on, q_no, q_nt, nlegal, act, reward, boot, gamma_n, vr_eps, td, prio, s);
    if (rc != RELA_OK) return rc;
    note_launch("td_kernel");
    ProfScope prof("learner_loss_grad", s);
    note_launch("learner_loss_grad");
    hipLaunchKernelGGL(learner_loss_grad, dim3(1), dim3(kLT), 0, s, (const float*)td, weight, act, legal, Bn, A, d_ha, loss);
  }
  return RELA_OK;
}

// ---- the backward pass between d_ha and d_a3: the dueling heads and the fc layer, four GEMMs and two column sums ------
struct HeadFcBwd {
  int Bn, A;
  const float* d_ha;            // [Bn][32] from the loss kernel: columns 0..A-1 = fc_a, 31 = fc_v
  const float *h, *a3;          // relu(fc) [Bn][512], relu(conv3) [Bn][49][64] channel-last (ffnet_layout.h)
  const float *a_w, *v_w;       // fc_a.weight [A][512], fc_v.weight [512] (state_dict layout)
  const float* wfcp;            // the fc weight in a3's column order (permute_weight_at, kPermFc)
  float *d_h, *d_a3;            // out: [Bn][512] masked by h > 0, [Bn][49][64] masked by a3 > 0
  float *g_a_w, *g_v_w, *g_fc_w, *g_fc_b;  // out: gradients, state_dict layout
  float* s32;                   // the column sums of d_ha, for head_bias_grad after the queued sums have run
  GemmArith arith;              // of the four GEMMs (ApexBwdPlan::heads_fc, learner_plan.h)
  hipEvent_t ev_dh = nullptr;   // (two lanes) d_h is ready
};
// s: the data-gradient chain; sw: the lane of the weight gradients (== s: one lane).  The two bias gradients' column
// sums are queued on `sums` for the launch pair at the end of trunk_backward.
int head_fc_backward(const HeadFcBwd& t, hipStream_t s, hipStream_t sw, ColsumJobs* sums) {
  const int Bn = t.Bn;
  // heads: d_h, dWh, db
  {
    ProbHeadDgrad p{};
    p.M = Bn, p.N = 512, p.K = 32;
    p.d_ha = t.d_ha, p.a_w = t.a_w, p.v_w = t.v_w, p.h = t.h, p.d_h = t.d_h, p.A = t.A;
    if (int rc = launch_gemm_as<SetDgrad>(t.arith, p, 1, s, "learner_dgrad_heads")) return rc;
  }
  if (int rc = launch_head_wgrad(t.arith, Bn, t.A, t.d_ha, t.h, t.g_a_w, t.g_v_w, sw)) return rc;
  sums->add(t.d_ha, Bn, 32, t.s32);
  if (sw != s) lane_dep(t.ev_dh, s, sw);  // d_h is ready
  // fc: d_a3, dWfc, db
  {
    ProbFcDgrad p{};
    p.M = Bn, p.N = 3136, p.K = 512;
    p.d_h = t.d_h, p.wfcp = t.wfcp, p.a3 = t.a3, p.d_a3 = t.d_a3;
    if (int rc = launch_gemm_as<SetDgrad>(t.arith, p, 1, s, "learner_dgrad_fc")) return rc;
  }
  {
    ProbFcWgrad p{};
    p.M = 512, p.N = 3136, p.K = Bn;
    p.d_h = t.d_h, p.a3 = t.a3, p.g_fc_w = t.g_fc_w;
    if (int rc = launch_gemm_as<SetWfc>(t.arith, p, 1, sw, "learner_wgrad_fc")) return rc;
  }
  sums->add(t.d_h, Bn, 512, t.g_fc_b);
  return RELA_OK;
}
}  // namespace

namespace {
// everything rela_apex_learner_create allocates; a failure leaves a half-built learner for rela_apex_learner_destroy
int build_learner(rela_apex_learner* l, int num_action, int max_batch, int multi_step, float gamma, int optimizer, float lr,
                  float eps, float grad_clip, int device) {
  l->device = device;
  l->A = num_action;
  l->Bmax = max_batch;
  l->gamma_n = (float)pow((double)gamma, (double)multi_step);  // apex.py:44
  l->opt.optimizer = optimizer, l->opt.lr = lr, l->opt.eps = eps, l->opt.clip = grad_clip;
  if (int rc = l->alloc_flat(kFFNetSegs, ffnet_param_counts, num_action)) return rc;
  const size_t B = (size_t)max_batch, A = (size_t)num_action;
  if (int rc = rela_ffnet_create(&l->online, num_action, device)) return rc;
  if (int rc = rela_ffnet_create(&l->target, num_action, device)) return rc;
  ffnet_label_as_learner(l->online);
  ffnet_label_as_learner(l->target);
  ffnet_set_max_rows(l->online, max_batch);
  ffnet_set_max_rows(l->target, max_batch);
  DevBuffers& m = l->mem;
  if (int rc = m.alloc(&l->w2p, kPermFloats[kPermConv2], false)) return rc;
  if (int rc = m.alloc(&l->w3p, kPermFloats[kPermConv3], false)) return rc;
  if (int rc = m.alloc(&l->wfcp, kPermFloats[kPermFc], false)) return rc;
  // (the merged split-bf16 forward runs the online net over 2 x batch rows: [s ; s'])
  l->ws_bytes = std::max(rela_ffnet_workspace_bytes(nullptr, max_batch), rela_ffnet_workspace_bytes(nullptr, 2 * max_batch));
  if (int rc = m.alloc(&l->ws_on, (size_t)l->ws_bytes, false)) return rc;
  if (int rc = m.alloc(&l->ws_tmp, (size_t)l->ws_bytes, false)) return rc;
  if (int rc = m.alloc(&l->q, 3 * B * A, false)) return rc;
  if (int rc = m.alloc(&l->td, B, false)) return rc;
  if (int rc = m.alloc(&l->d_ha, B * 32, false)) return rc;
  if (int rc = m.alloc(&l->d_h, B * 512, false)) return rc;
  if (int rc = m.alloc(&l->d_a3, B * kA3, false)) return rc;
  if (int rc = m.alloc(&l->d_a2, B * kA2, false)) return rc;
  if (int rc = m.alloc(&l->d_a1, B * kA1, false)) return rc;
  const size_t cpart_floats = (size_t)kColsumBlocks * (32 + 512 + 64 + 64 + 32);  // all five jobs
  if (int rc = m.alloc(&l->part, kTrunkPartFloats, false)) return rc;
  if (int rc = m.alloc(&l->cpart, cpart_floats, false)) return rc;
  if (int rc = m.alloc(&l->s32, 32, false)) return rc;
  static const bool lanes = !(getenv("RELA_LEARNER_LANES") && atoi(getenv("RELA_LEARNER_LANES")) == 1);
  if (lanes) {
    RELA_HIP(hipStreamCreateWithFlags(&l->side, hipStreamNonBlocking));
    for (hipEvent_t& e : l->ev) RELA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (int rc = m.alloc(&l->part_side, kTrunkPartFloats, false)) return rc;
    if (int rc = m.alloc(&l->cpart_side, cpart_floats, false)) return rc;
    if (int rc = m.alloc(&l->frag2, kFrag2Bytes, false)) return rc;
    if (int rc = m.alloc(&l->frag3, kFrag3Bytes, false)) return rc;
  }
  return RELA_OK;
}
}  // namespace

extern "C" int rela_apex_learner_create(rela_apex_learner** out, int num_action, int max_batch, int multi_step,
                                        float gamma, int optimizer, float lr, float eps, float grad_clip,
                                        int device) {
  RELA_CHECK(out && num_action >= 1 && num_action <= 31 && max_batch >= 1 && max_batch <= kTrunkMaxFrames && multi_step >= 1 &&
                 (optimizer == 0 || optimizer == 1),
             RELA_EINVAL, "rela_apex_learner_create: bad arguments (A=%d batch=%d n=%d optimizer=%d)", num_action,
             max_batch, multi_step, optimizer);
  if (int rc = check_device(device, "rela_apex_learner_create")) return rc;
  DeviceGuard g(device);
  auto* l = new rela_apex_learner();
  const int rc = build_learner(l, num_action, max_batch, multi_step, gamma, optimizer, lr, eps, grad_clip, device);
  if (rc != RELA_OK) {
    rela_apex_learner_destroy(l);  // the one exit of a failed create: *out stays untouched
    return rc;
  }
  *out = l;
  return RELA_OK;
}

// (also the end of a half-built learner: null nets, stream and events are skipped, l->mem holds what was allocated)
extern "C" void rela_apex_learner_destroy(rela_apex_learner* l) {
  if (!l) return;
  DeviceGuard g(l->device);
  (void)hipDeviceSynchronize();
  l->mem.free_all();
  for (hipEvent_t e : l->ev)
    if (e) (void)hipEventDestroy(e);
  if (l->side) (void)hipStreamDestroy(l->side);
  rela_ffnet_destroy(l->online);
  rela_ffnet_destroy(l->target);
  delete l;
}

extern "C" int rela_apex_learner_load(rela_apex_learner* l, const rela_ffnet_params* online,
                                      const rela_ffnet_params* target, int on_device, void* stream_) {
  RELA_CHECK(l && online, RELA_EINVAL, "rela_apex_learner_load: bad arguments");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(l->device);
  if (int rc = l->load("rela_apex_learner_load", online, target, on_device, s)) return rc;
  if (int rc = repack(l, true, true, s)) return rc;
  l->loaded = true;
  return RELA_OK;
}

extern "C" int rela_apex_learner_set_value_rescale(rela_apex_learner* l, float eps) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_set_value_rescale: bad arguments");
  return l->set_value_rescale("rela_apex_learner_set_value_rescale", eps);
}

extern "C" int rela_apex_learner_set_precision(rela_apex_learner* l, int mode) {
  RELA_CHECK(l && mode >= 0 && mode <= 2, RELA_EINVAL, "rela_apex_learner_set_precision: mode must be 0, 1 or 2");
  int rc = rela_ffnet_set_precision(l->online, mode);
  if (rc != RELA_OK) return rc;
  return rela_ffnet_set_precision(l->target, mode);
}

extern "C" int rela_apex_learner_sync_target(rela_apex_learner* l, void* stream_) {
  RELA_CHECK(l && l->loaded, RELA_ESTATE, "rela_apex_learner_sync_target: parameters were never loaded");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(l->device);
  if (int rc = l->copy_online_to_target(s)) return rc;
  return repack(l, false, true, s);
}

extern "C" int rela_apex_learner_soft_update_target(rela_apex_learner* l, float tau, void* stream_) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_soft_update_target: bad arguments");
  if (int rc = l->check_soft_update("rela_apex_learner_soft_update_target", tau)) return rc;
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(l->device);
  if (int rc = l->soft_update_target(tau, s)) return rc;
  return repack(l, false, true, s);
}

extern "C" int rela_apex_learner_set_lr(rela_apex_learner* l, float lr) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_set_lr: bad arguments");
  return l->set_lr("rela_apex_learner_set_lr", lr);
}

extern "C" int rela_apex_learner_lr(rela_apex_learner* l, float* out) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_lr: bad arguments");
  return l->get_lr("rela_apex_learner_lr", out);
}

extern "C" int rela_apex_learner_set_rmsprop(rela_apex_learner* l, float alpha, int centered) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_set_rmsprop: bad arguments");
  return l->set_rmsprop("rela_apex_learner_set_rmsprop", alpha, centered);
}

extern "C" int rela_apex_learner_set_adam_betas(rela_apex_learner* l, float b1, float b2) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_set_adam_betas: bad arguments");
  return l->set_adam_betas("rela_apex_learner_set_adam_betas", b1, b2);
}

extern "C" int rela_apex_learner_params(rela_apex_learner* l, rela_ffnet_params* online_out,
                                        rela_ffnet_params* target_out) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_params: bad arguments");
  if (online_out) l->params_at(l->P, online_out);
  if (target_out) l->params_at(l->PT, target_out);
  return RELA_OK;
}

extern "C" int rela_apex_learner_grads(rela_apex_learner* l, rela_ffnet_params* grads_out) {
  RELA_CHECK(l && grads_out, RELA_EINVAL, "rela_apex_learner_grads: bad arguments");
  l->params_at(l->G, grads_out);
  return RELA_OK;
}

extern "C" int rela_apex_learner_flat(rela_apex_learner* l, float** params_dev, float** grads_dev, int64_t* count) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_flat: bad arguments");
  return l->flat(params_dev, grads_dev, count);
}

extern "C" const float* rela_apex_learner_stats_dev(const rela_apex_learner* l) { return l ? l->norm : nullptr; }

extern "C" int rela_apex_learner_debug_activations(rela_apex_learner* l, float** a1, float** a2, float** a3, float** h,
                                                   int* batch) {
  RELA_CHECK(l && l->last_B > 0, RELA_ESTATE, "rela_apex_learner_debug_activations: no rela_apex_learner_loss yet");
  const FFNetWs w = ffnet_ws(l->ws_on, l->pend_rows);
  if (a1) *a1 = w.a1;
  if (a2) *a2 = w.a2;
  if (a3) *a3 = w.a3;
  if (h) *h = w.h;
  if (batch) *batch = l->last_B;
  return RELA_OK;
}

extern "C" int rela_apex_learner_backward(rela_apex_learner* l, int batch, const void* const* rows_dev,
                                          const float* weight_dev, float* priority_dev, float* loss_dev,
                                          void* stream_) {
  int rc = rela_apex_learner_loss(l, batch, rows_dev, weight_dev, priority_dev, loss_dev, stream_);
  if (rc != RELA_OK) return rc;
  return rela_apex_learner_grad(l, stream_);
}

// The forward half of the step: the three forwards of td_err, the priorities and the loss (with the head gradient
// d_ha the loss kernel leaves).  `priority_dev` is final when this returns' work is done, so a caller may hand it to
// update_priority and ask for the next batch while rela_apex_learner_grad still runs (the replay is not touched by
// the backward pass); the batch's `s` rows must stay untouched until then (conv1's weight gradient reads them).
// RELA_LEARNER_MERGE_ONLINE=0: the two online forwards of the f32x3 step as two launches per layer again (A/B switch)
static bool merge_online_forwards() {
  static const bool on = [] {
    const char* e = getenv("RELA_LEARNER_MERGE_ONLINE");
    return !(e && e[0] == '0');
  }();
  return on;
}

extern "C" int rela_apex_learner_loss(rela_apex_learner* l, int batch, const void* const* rows_dev,
                                      const float* weight_dev, float* priority_dev, float* loss_dev, void* stream_) {
  RELA_CHECK(l && l->loaded, RELA_ESTATE, "rela_apex_learner_loss: parameters were never loaded");
  RELA_CHECK(batch >= 1 && batch <= l->Bmax && rows_dev && weight_dev && priority_dev, RELA_EINVAL,
             "rela_apex_learner_loss: bad arguments (batch %d, max %d)", batch, l->Bmax);
  l->pend_B = 0;
  l->loss_called = true;
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(l->device);
  const int Bn = batch, A = l->A;
  // FFTransition fields in the order rela_replay_sample fills them (types.h:18-51)
  const uint8_t* obs = static_cast<const uint8_t*>(rows_dev[0]);
  const uint8_t* nobs = static_cast<const uint8_t*>(rows_dev[1]);
  const float* legal = static_cast<const float*>(rows_dev[4]);
  const float* nlegal = static_cast<const float*>(rows_dev[5]);
  const int64_t* act = static_cast<const int64_t*>(rows_dev[6]);
  const float* reward = static_cast<const float*>(rows_dev[7]);
  const float* boot = static_cast<const float*>(rows_dev[9]);
  RELA_CHECK(obs && nobs && legal && nlegal && act && reward && boot, RELA_EINVAL,
             "rela_apex_learner_loss: a batch field is NULL");
  float* q_on = l->q;
  float* q_no = l->q + (size_t)Bn * A;
  float* q_nt = l->q + 2 * (size_t)Bn * A;
  // td_err (apex.py:30-45): greedy_act(next_obs) and target_net(next_obs) carry no gradient
  int rc;
  bool unsplit_side = false;
  l->pend_rows = Bn;
  if (rela_ffnet_precision(l->online) == 1 && ffnet_learner_forward_ok(l->online, l->target, Bn)) {
    // bf16x2: all three forwards on split-bf16 MFMA, one launch per layer (online over [s ; s'], target over s'); the
    // backward then reads the activations -- and the ReLU masks -- of THIS forward (turned back into f32 below)
    rc = ffnet_learner_forward(l->online, l->target, Bn, obs, nobs, legal, nlegal, q_on, q_no, q_nt, l->ws_on, l->ws_tmp,
                               l->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    if (l->side) lane_dep(l->ev[0], s, l->side);  // (the loss kernel below reads Q only: the conversion runs next to it)
    rc = ffnet_learner_unsplit(Bn, l->ws_on, l->side ? l->side : s);
    if (rc != RELA_OK) return rc;
    unsplit_side = l->side != nullptr;
    l->pend_rows = 2 * Bn;  // the workspace layout the backward must address
  } else if (rela_ffnet_precision(l->online) == 2 && Bn >= 512 && merge_online_forwards() &&
             nobs == obs + (size_t)Bn * 28224 && nlegal == legal + (size_t)Bn * A) {
    // f32x3 (r5): the two ONLINE forwards as one launch per layer over [s ; s'] when the caller's batch has s' right behind s
    // and the legal moves likewise (rela_amd.replay.FFReplay's output buffers do).  Same-box A/B at B = 512: 2.033 against
    // 2.045 ms per bench step, 0.729 against 0.733 ms learner-only (profiles/r05_ab_merge_online.log) -- half a percent;
    // a caller with separate buffers keeps the three launches (staging copies would cost more than that).
    const uint8_t* in2 = obs;
    const float* legal2 = legal;
    rc = rela_ffnet_forward(l->target, Bn, nobs, nlegal, q_nt, l->ws_tmp, l->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    // (the net's declared batch limit only says which weight layouts its loads pack; the three-part ones this launch reads
    // are packed from 512 rows up, and the workspaces are sized for 2 x the batch: the call brings its own limit)
    rc = ffnet_forward_mode(l->online, 2 * Bn, in2, legal2, q_on, l->ws_on, l->ws_bytes, s, 3, 2 * l->Bmax);  // q_no = q_on + Bn * A
    if (rc != RELA_OK) return rc;
    l->pend_rows = 2 * Bn;  // the workspace layout the backward must address (it reads the first Bn rows)
  } else {
    rc = rela_ffnet_forward(l->online, Bn, nobs, nlegal, q_no, l->ws_tmp, l->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    rc = rela_ffnet_forward(l->target, Bn, nobs, nlegal, q_nt, l->ws_tmp, l->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    // f32 activations for the backward, which reads a1..h (the f32x3 mode keeps that layout: it may serve this pass too)
    rc = ffnet_forward_mode(l->online, Bn, obs, legal, q_on, l->ws_on, l->ws_bytes, s, rela_ffnet_precision(l->online) == 2 ? 3 : 0);
    if (rc != RELA_OK) return rc;
  }
  rc = launch_loss_grad(Bn, A, Bn <= kFusedLossMaxBatch, q_on, q_no, q_nt, nlegal, act, reward, boot, l->gamma_n, l->vr_eps,
                        weight_dev, legal, l->td, priority_dev, l->d_ha, l->loss, s);
  if (rc != RELA_OK) return rc;
  if (loss_dev) RELA_HIP(dev_copy2(loss_dev, l->loss, sizeof(float), nullptr, nullptr, 0, s));  // (a kernel, not a blit: common.h)
  if (unsplit_side) lane_dep(l->ev[1], l->side, s);  // the caller's stream owns the workspace again from here
  RELA_LAUNCH_CHECK();
  l->pend_B = l->last_B = Bn;
  l->pend_obs = obs;
  return RELA_OK;
}

// The backward half: gradients of the last rela_apex_learner_loss into the flat gradient buffer.
extern "C" int rela_apex_learner_grad(rela_apex_learner* l, void* stream_) {
  RELA_CHECK(l && l->loaded && l->pend_B > 0, RELA_ESTATE, "rela_apex_learner_grad: no rela_apex_learner_loss to differentiate");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(l->device);
  const int Bn = l->pend_B, A = l->A;
  const uint8_t* obs = l->pend_obs;
  l->pend_B = 0;

  const FFNetWs w = ffnet_ws(l->ws_on, l->pend_rows);
  const rela_ffnet_params P = params_at(l, l->P);
  float* Gm[kFFNetSegs];  // gradient tensors in rela_ffnet_params order
  for (int i = 0; i < kFFNetSegs; ++i) Gm[i] = l->G + l->off[i];

  ColsumJobs sums;  // the five bias gradients: queued here, one launch pair at the end of trunk_backward
  const bool lanes = l->side != nullptr;
  const ApexBwdPlan plan = plan_apex_backward(rela_ffnet_precision(l->online), lanes);
  hipStream_t sw = lanes ? l->side : s;  // the weight-gradient lane
  if (lanes) lane_dep(l->ev[2], s, sw);  // d_ha and the forward's activations are ready

  {  // heads and fc: d_h, dWh, d_a3, dWfc; their bias gradients queued on `sums`
    HeadFcBwd t{};
    t.Bn = Bn, t.A = A, t.d_ha = l->d_ha, t.h = w.h, t.a3 = w.a3, t.a_w = P.a_w, t.v_w = P.v_w, t.wfcp = l->wfcp;
    t.d_h = l->d_h, t.d_a3 = l->d_a3, t.g_a_w = Gm[10], t.g_v_w = Gm[8], t.g_fc_w = Gm[6], t.g_fc_b = Gm[7], t.s32 = l->s32;
    t.arith = plan.heads_fc, t.ev_dh = l->ev[3];
    if (int rc = head_fc_backward(t, s, sw, &sums)) return rc;
  }
  {
    TrunkBwd t{};
    t.Bn = Bn, t.obs = obs, t.a1 = w.a1, t.a2 = w.a2, t.d_a3 = l->d_a3, t.d_a2 = l->d_a2, t.d_a1 = l->d_a1;
    t.part = l->part, t.cpart = l->cpart, t.w2p = l->w2p, t.w3p = l->w3p;
    t.g_c1w = Gm[0], t.g_c1b = Gm[1], t.g_c2w = Gm[2], t.g_c2b = Gm[3], t.g_c3w = Gm[4], t.g_c3b = Gm[5];
    t.plan = plan.trunk.plan(Bn);
    if (lanes) {
      t.side = sw, t.ev_da3 = l->ev[4], t.ev_da2 = l->ev[5], t.ev_side = l->ev[6];
      t.part_side = l->part_side, t.cpart_side = l->cpart_side;
      if (t.plan.dgrad_bf16) t.frag2 = l->frag2, t.frag3 = l->frag3;
      t.s32 = l->s32, t.A = A, t.g_a_b = Gm[11], t.g_v_b = Gm[9];
    }
    if (int rc = trunk_backward(t, s, &sums)) return rc;
    if (!lanes) launch_head_bias_grad(l->s32, A, Gm[11], Gm[9], s);
  }
  RELA_LAUNCH_CHECK();
  return RELA_OK;
}

// Test tap: launch_loss_grad on its own, the three Q tables and the batch's fields as inputs of the call.
extern "C" int rela_debug_loss_grad(int batch, int A, int form, const float* q, const float* qno, const float* qnt,
                                    const float* nlegal, const int64_t* act, const float* reward, const float* bootstrap,
                                    float gamma_n, float vr_eps, const float* weight, const float* legal, float* td,
                                    float* prio, float* d_ha, float* loss, void* stream_) {
  RELA_CHECK(batch >= 1 && batch <= kTrunkMaxFrames && A >= 1 && A <= 31 && form >= 0 && form <= 2, RELA_EINVAL,
             "rela_debug_loss_grad: bad arguments (batch %d, A %d, form %d)", batch, A, form);
  RELA_CHECK(q && qno && qnt && nlegal && act && reward && bootstrap && weight && legal && td && prio && d_ha && loss,
             RELA_EINVAL, "rela_debug_loss_grad: a pointer is NULL");
  hipStream_t s = (hipStream_t)stream_;
  const bool fused = form == 0 ? batch <= kFusedLossMaxBatch : form == 1;
  if (int rc = launch_loss_grad(batch, A, fused, q, qno, qnt, nlegal, act, reward, bootstrap, gamma_n, vr_eps, weight, legal,
                                td, prio, d_ha, loss, s))
    return rc;
  RELA_LAUNCH_CHECK();
  RELA_HIP(hipStreamSynchronize(s));
  return RELA_OK;
}

// Test tap: head_fc_backward on its own, then the two queued column sums and head_bias_grad as the learner's lanes run
// them (the side lane's launch pair at the end of trunk_backward's side lane, or the caller's stream with one lane).
extern "C" int rela_debug_head_fc_backward(int batch, int A, int mode, int lanes, const float* d_ha, const float* h,
                                           const float* a3, const float* fc_a_w, const float* fc_v_w, const float* fc_w,
                                           float* g_fc_a_w, float* g_fc_a_b, float* g_fc_v_w, float* g_fc_v_b, float* g_fc_w,
                                           float* g_fc_b, float* d_h, float* d_a3, void* stream_) {
  RELA_CHECK(batch >= 1 && batch <= kTrunkMaxFrames && A >= 1 && A <= 31 && mode >= 0 && mode <= 2 &&
                 (lanes == 0 || lanes == 1),
             RELA_EINVAL, "rela_debug_head_fc_backward: bad arguments (batch %d, A %d, mode %d, lanes %d)", batch, A, mode,
             lanes);
  RELA_CHECK(d_ha && h && a3 && fc_a_w && fc_v_w && fc_w && g_fc_a_w && g_fc_a_b && g_fc_v_w && g_fc_v_b && g_fc_w && g_fc_b &&
                 d_h && d_a3,
             RELA_EINVAL, "rela_debug_head_fc_backward: a pointer is NULL");
  hipStream_t s = (hipStream_t)stream_;
  TrunkTapScratch sc;
  float *wfcp = nullptr, *cpart = nullptr, *s32 = nullptr;
  if (int rc = sc.mem.alloc(&wfcp, kPermFloats[kPermFc], false)) return rc;
  if (int rc = sc.mem.alloc(&cpart, (size_t)kColsumBlocks * (32 + 512), false)) return rc;
  if (int rc = sc.mem.alloc(&s32, 32, false)) return rc;
  if (int rc = permute_weight(kPermFc, fc_w, wfcp, s)) return rc;
  hipStream_t sw = s;
  if (lanes) {  // as rela_apex_learner_grad: the weight gradients and the column sums on a side lane
    RELA_HIP(hipStreamCreateWithFlags(&sc.side, hipStreamNonBlocking));
    for (hipEvent_t& e : sc.ev) RELA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    sw = sc.side;
    lane_dep(sc.ev[0], s, sw);  // the inputs (and wfcp) are ready
  }
  HeadFcBwd t{};
  t.Bn = batch, t.A = A, t.d_ha = d_ha, t.h = h, t.a3 = a3, t.a_w = fc_a_w, t.v_w = fc_v_w, t.wfcp = wfcp;
  t.d_h = d_h, t.d_a3 = d_a3, t.g_a_w = g_fc_a_w, t.g_v_w = g_fc_v_w, t.g_fc_w = g_fc_w, t.g_fc_b = g_fc_b, t.s32 = s32;
  t.arith = plan_apex_backward(mode, lanes != 0).heads_fc, t.ev_dh = sc.ev[1];
  ColsumJobs sums;
  const int rc = head_fc_backward(t, s, sw, &sums);
  if (rc == RELA_OK) {
    colsum_multi_launch(sums, cpart, sw);
    launch_head_bias_grad(s32, A, g_fc_a_b, g_fc_v_b, sw);
  }
  if (lanes) lane_dep(sc.ev[2], sw, s);
  const hipError_t launched = hipGetLastError();
  // (the scratch goes away with `sc`: both lanes must be done with it whatever happened)
  const hipError_t done = hipStreamSynchronize(s);
  if (sc.side) (void)hipStreamSynchronize(sc.side);
  if (rc != RELA_OK) return rc;
  RELA_HIP(launched);
  RELA_HIP(done);
  return RELA_OK;
}

extern "C" int rela_apex_learner_debug_head_grads(rela_apex_learner* l, float** d_ha, float** d_h, float** d_a3) {
  RELA_CHECK(l && d_ha && d_h && d_a3, RELA_EINVAL, "rela_apex_learner_debug_head_grads: bad arguments");
  RELA_CHECK(l->last_B > 0, RELA_ESTATE, "rela_apex_learner_debug_head_grads: no rela_apex_learner_loss yet");
  *d_ha = l->d_ha, *d_h = l->d_h, *d_a3 = l->d_a3;
  return RELA_OK;
}

extern "C" int rela_apex_learner_debug_optim(rela_apex_learner* l, float** s1_dev, float** s2_dev, int64_t* adam_t) {
  RELA_CHECK(l, RELA_EINVAL, "rela_apex_learner_debug_optim: bad arguments");
  return l->debug_optim("rela_apex_learner_debug_optim", s1_dev, s2_dev, adam_t);
}

extern "C" int rela_apex_learner_apply(rela_apex_learner* l, void* stream_) {
  RELA_CHECK(l && l->loaded, RELA_ESTATE, "rela_apex_learner_apply: parameters were never loaded");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(l->device);
  l->apply(s);
  RELA_LAUNCH_CHECK();
  return repack(l, true, false, s);
}
