// actor_r2d2.hip -- device-resident R2D2 actor shard (C ABI: rela_r2d2_actor_*).
//
// Restates what BasicThreadLoop (rela/thread_loop.h:74-105) drives through R2D2Actor
// (rela/r2d2_actor.h:189-353):
//   act        :221-249  historyHidden_.push_back(hidden_); TorchScript "act" (r2d2.py:58-73 ->
//                        net.py:110-124): conv trunk + one LSTM step, greedy over the raw advantages
//                        shifted by their batch minimum, eps-greedy; hidden_ <- new state
//   post_step  :252-302  push (r,t); zero the hidden state of finished envs (:258-267); n-step pop
//                        (dqn_actor.h:58-106); per-step priority (r2d2.py:76-100: online(s_t,h_t),
//                        online.act(s_t+n,h_t+n), target(s_t+n,h_t+n)); R2D2TransitionBuffer::push
//                        (:29-87); on canPop popTransition (:93-170) + aggregate_priority
//                        (r2d2.py:103-120) + replay add (:301)
// The integer bookkeeping of the sequence windows is r2d2_seq_core.h (host); this file owns the HBM
// side: per env one window of T = burn_in + seq_len + multi_step slots PER FIELD, laid out so a whole
// window is exactly one replay row of that field -- emitting a sequence is a plain row copy.
#include <cmath>
#include <cstring>

#include "actor_shard.h"
#include "prof.h"
#include "r2d2_seq_core.h"

using namespace rela_amd;

namespace {

constexpr int kHid = 512;
constexpr int kT = 256;

struct Windows {
  uint8_t* s;     // [R][T][28224]   (null with de-duplication)
  int32_t* sref;  // [R][T][ups]     de-duplication (rela_r2d2_actor_set_dedup): references instead of frames, -1 = pad
  float* eps;     // [R][T]
  float* legal;   // [R][T][A]
  int64_t* a;     // [R][T]
  float* reward;  // [R][T]
  uint8_t* term;  // [R][T]
  float* boot;    // [R][T]
  float* prio;    // [R][seq+n]   per-step priorities (batchSeqPriority_)
  float *h0, *c0, *nh0, *nc0;  // [R][512]  batchH0_ / batchNextH0_
  int T, A, seq, burn, n;
  int ups;  // 0: frames in `s`; 1 / 4: references in `sref`
};

__device__ __forceinline__ void block_copy16(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t bytes) {
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int64_t i = threadIdx.x; i < (bytes >> 4); i += blockDim.x) d4[i] = s4[i];
}
__device__ __forceinline__ void block_zero16(uint8_t* __restrict__ dst, int64_t bytes) {
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (int64_t i = threadIdx.x; i < (bytes >> 4); i += blockDim.x) d4[i] = make_uint4(0, 0, 0, 0);
}

// R2D2TransitionBuffer::push :51-71 for every env: write this step's transition into its window slot
__global__ __launch_bounds__(kT) void r2d2_write_step(Windows w, const int32_t* __restrict__ slot,
                                                     const uint8_t* __restrict__ flags,
                                                     const uint8_t* __restrict__ obs, const float* __restrict__ eps,
                                                     const float* __restrict__ legal, const int64_t* __restrict__ act,
                                                     const float* __restrict__ reward,
                                                     const uint8_t* __restrict__ term, const float* __restrict__ boot,
                                                     const float* __restrict__ prio_step,
                                                     const float* __restrict__ hid_h, const float* __restrict__ hid_c,
                                                     const int32_t* __restrict__ refs) {
  const int i = blockIdx.x;
  const int j = slot[i];
  const int64_t o = (int64_t)i * w.T + j;
  if (w.ups > 0) {
    for (int k = threadIdx.x; k < w.ups; k += blockDim.x) w.sref[o * w.ups + k] = refs[(int64_t)i * w.ups + k];
  } else {
    block_copy16(w.s + o * kObs, obs + (int64_t)i * kObs, kObs);
  }
  for (int k = threadIdx.x; k < w.A; k += blockDim.x) w.legal[o * w.A + k] = legal[(int64_t)i * w.A + k];
  if (threadIdx.x == 0) {
    w.eps[o] = eps[i];
    w.a[o] = act[i];
    w.reward[o] = reward[i];
    w.term[o] = term[i];
    w.boot[o] = boot[i];
    w.prio[(int64_t)i * (w.seq + w.n) + (j - w.burn)] = prio_step[i];
  }
  const uint8_t f = flags[i];
  if (f & 1)  // batchH0_[i] <- hid :41
    for (int k = threadIdx.x; k < kHid; k += blockDim.x) {
      w.h0[(int64_t)i * kHid + k] = hid_h[(int64_t)i * kHid + k];
      w.c0[(int64_t)i * kHid + k] = hid_c[(int64_t)i * kHid + k];
    }
  if (f & 2)  // batchNextH0_[i] <- hid :65-68
    for (int k = threadIdx.x; k < kHid; k += blockDim.x) {
      w.nh0[(int64_t)i * kHid + k] = hid_h[(int64_t)i * kHid + k];
      w.nc0[(int64_t)i * kHid + k] = hid_c[(int64_t)i * kHid + k];
    }
}

// padLike (types.cc:69-80) over slot ranges: zeros everywhere, terminal = 1, optional priority 0
__global__ __launch_bounds__(kT) void r2d2_pad(Windows w, const int32_t* __restrict__ ranges /*[n][4]*/) {
  const int env = ranges[blockIdx.x * 4 + 0], begin = ranges[blockIdx.x * 4 + 1], end = ranges[blockIdx.x * 4 + 2];
  const int zero_prio = ranges[blockIdx.x * 4 + 3];
  const int j = begin + blockIdx.y;
  if (j >= end) return;
  const int64_t o = (int64_t)env * w.T + j;
  if (w.ups > 0) {
    for (int k = threadIdx.x; k < w.ups; k += blockDim.x) w.sref[o * w.ups + k] = -1;  // the all-zero unit
  } else {
    block_zero16(w.s + o * kObs, kObs);
  }
  for (int k = threadIdx.x; k < w.A; k += blockDim.x) w.legal[o * w.A + k] = 0.f;
  if (threadIdx.x == 0) {
    w.eps[o] = 0.f;
    w.a[o] = 0;
    w.reward[o] = 0.f;
    w.term[o] = 1;
    w.boot[o] = 0.f;
    if (zero_prio) w.prio[(int64_t)env * (w.seq + w.n) + (j - w.burn)] = 0.f;
  }
}

// carry-over :119-139: slots [seq, seq+burn+n) -> [0, burn+n) in ascending order (the ranges may
// overlap when burn+n > seq), priorities by the reference's effective rule, h0 <- next_h0
__global__ __launch_bounds__(kT) void r2d2_carry(Windows w, const int32_t* __restrict__ envs) {
  const int env = envs[blockIdx.x];
  const int64_t base = (int64_t)env * w.T;
  for (int j = 0; j < w.burn + w.n; ++j) {
    const int64_t d = base + j, s = base + w.seq + j;
    if (w.ups > 0) {
      for (int k = threadIdx.x; k < w.ups; k += blockDim.x) w.sref[d * w.ups + k] = w.sref[s * w.ups + k];
    } else {
      block_copy16(w.s + d * kObs, w.s + s * kObs, kObs);
    }
    for (int k = threadIdx.x; k < w.A; k += blockDim.x) w.legal[d * w.A + k] = w.legal[s * w.A + k];
    if (threadIdx.x == 0) {
      w.eps[d] = w.eps[s];
      w.a[d] = w.a[s];
      w.reward[d] = w.reward[s];
      w.term[d] = w.term[s];
      w.boot[d] = w.boot[s];
    }
    __syncthreads();
  }
  float* p = w.prio + (int64_t)env * (w.seq + w.n);
  if (threadIdx.x == 0)
    for (int j = w.burn; j < w.n; ++j) p[j] = p[w.seq + j];  // see r2d2_seq_core.h on the stale entries
  for (int k = threadIdx.x; k < kHid; k += blockDim.x) {
    w.h0[(int64_t)env * kHid + k] = w.nh0[(int64_t)env * kHid + k];
    w.c0[(int64_t)env * kHid + k] = w.nc0[(int64_t)env * kHid + k];
  }
}

// priority rows + lengths of every emitted sequence, read from the PRE-carry windows
__global__ void r2d2_collect(Windows w, const int32_t* __restrict__ emits /*[n][3] env,len,second*/, int nseq,
                             float* __restrict__ prow, float* __restrict__ lens) {
  const int q = blockIdx.x;
  if (q >= nseq) return;
  const int env = emits[q * 3], len = emits[q * 3 + 1], second = emits[q * 3 + 2];
  const float* p = w.prio + (int64_t)env * (w.seq + w.n);
  for (int j = threadIdx.x; j < w.seq; j += blockDim.x) {
    float v;
    if (!second) v = p[j];
    else if (j < w.n) v = (j >= w.burn) ? p[w.seq + j] : p[j];
    else v = 0.f;
    prow[(int64_t)q * w.seq + j] = v;
  }
  if (threadIdx.x == 0) lens[q] = (float)len;
}

// R2D2Agent.aggregate_priority  r2d2.py:103-120 (one lane per sequence; seq_len <= a few hundred)
__global__ void r2d2_aggregate(const float* __restrict__ prow, const float* __restrict__ lens, int nseq, int seq,
                               int burn, float eta, float one_minus_eta, float* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nseq) return;
  float sum = 0.f, mx = -INFINITY;
  for (int t = 0; t < seq; ++t) {
    const float m = ((float)t < lens[q]) ? 1.f : 0.f;
    const float v = prow[(int64_t)q * seq + t] * m;
    sum += v;
    mx = fmaxf(mx, v);
  }
  const float mean = sum / (lens[q] - (float)burn);
  out[q] = __fadd_rn(__fmul_rn(eta, mx), __fmul_rn(one_minus_eta, mean));
}

// setRewardAndTerminal :258-267: finished envs restart from the zero state
__global__ void r2d2_reset_hidden(const uint8_t* __restrict__ term, int R, float* __restrict__ h, float* __restrict__ c) {
  const int i = blockIdx.x;
  if (i >= R || !term[i]) return;
  for (int k = threadIdx.x; k < kHid; k += blockDim.x) {
    h[(int64_t)i * kHid + k] = 0.f;
    c[(int64_t)i * kHid + k] = 0.f;
  }
}

// priorities of the sequences a piece keeps (de-duplication drops those that contain an unstored tick)
__global__ void r2d2_pick(const float* __restrict__ agg, const int32_t* __restrict__ qs, int m, float* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m) out[k] = agg[qs[k]];
}

constexpr int64_t kPadTick = -1, kLostTick = -2;  // de-duplication: window entries that are padding / an unstored tick

}  // namespace

struct rela_r2d2_actor : ActorShardBase {
  int seq = 0, burn = 0, T = 0;
  float gamma = 0.f, gamma_n = 0.f, eta = 0.f, one_minus_eta = 0.f;
  uint64_t seed = 0;
  // hidden history (r2d2_actor.h:345) next to the n-step ring
  float *hist_h = nullptr, *hist_c = nullptr;  // [n+1][R][512]
  float *hid_h = nullptr, *hid_c = nullptr, *tmp_h = nullptr, *tmp_c = nullptr;  // [R][512]
  // q: adv(act), q_online, adv_next, q_target; weights the advantages in q[0] (written by act, slot q_slot) belong to
  const rela_lstmnet* q_net = nullptr;
  uint64_t q_version = 0;
  float* prio_step = nullptr;  // [R]
  Windows w{};
  float *prow = nullptr, *lens = nullptr, *agg = nullptr;  // [2R][seq], [2R], [2R]
  int32_t *d_slot = nullptr, *d_ranges = nullptr, *d_emits = nullptr, *d_envs = nullptr;
  int32_t* d_gather = nullptr;  // [2][3R]: destination offsets, source envs and emit indices of one batch
  uint8_t* d_flags = nullptr;
  void* ws = nullptr;
  int64_t ws_bytes = 0;
  std::vector<uint8_t> h_term;  // [n+1][R] host copy: the bookkeeping needs the flags
  SeqBook* book = nullptr;
  SeqPlan plan;
  // frame-stack de-duplication: ref_hist is the n-step ring of the stacks' references, and the windows (w.sref) receive
  // those of obs_t.  tick_seq has tick_win entries; for an unstored tick it holds a lower bound.
  int tick_win = 0;                  // T + n + 8 ticks: the oldest unit a sequence emitted now can refer to is T + n + 3 back
  int64_t seq_hint = 0;              // the unit sequence number after this shard's last reservation
  std::vector<int64_t> win_tick;     // [R][T] host: the tick each window entry holds (kPadTick, kLostTick)
  float* agg_kept = nullptr;         // [2R] priorities of the kept sequences of one piece
  int32_t* d_kept = nullptr;         // [2R]
  HostStage stage;  // pinned staging of the per-tick index plans (one segment per post_step)
};

extern "C" int rela_r2d2_actor_create(rela_r2d2_actor** out, int rows, int group_rows, int num_action, int multi_step,
                                      float gamma, int seq_len, int burn_in, double eta, rela_replay* replay,
                                      uint64_t seed, int device) {
  RELA_CHECK(out && rows >= 1 && group_rows >= 1 && rows % group_rows == 0 && num_action >= 1 && num_action <= 31 &&
                 multi_step >= 1 && seq_len >= 1 && burn_in >= 0,
             RELA_EINVAL, "rela_r2d2_actor_create: bad arguments");
  RELA_CHECK(burn_in <= seq_len && multi_step <= seq_len, RELA_EINVAL,
             "rela_r2d2_actor_create: needs burn_in <= seq_len and multi_step <= seq_len");  // r2d2_actor.h:25-26
  int rc = check_device(device, "rela_r2d2_actor_create");
  if (rc != RELA_OK) return rc;
  DeviceGuard g(device);
  auto* a = new rela_r2d2_actor();
  a->device = device;
  a->R = rows;
  a->K = group_rows;
  a->A = num_action;
  a->n = multi_step;
  a->seq = seq_len;
  a->burn = burn_in;
  a->T = burn_in + seq_len + multi_step;
  a->gamma = gamma;
  a->gamma_n = (float)pow((double)gamma, (double)multi_step);
  a->eta = (float)eta;
  a->one_minus_eta = (float)(1.0 - eta);  // TorchScript folds (1.0 - self.eta) in double, r2d2.py:119
  a->replay = replay;
  a->seed = seed;
  const size_t H = (size_t)multi_step + 1, R = (size_t)rows, A = (size_t)num_action, T = (size_t)a->T;
  rc = shard_alloc_ring(a);
  if (rc != RELA_OK) return rc;
  RELA_ALLOC(a->hist_h, H * R * kHid * sizeof(float));
  RELA_ALLOC(a->hist_c, H * R * kHid * sizeof(float));
  RELA_ALLOC(a->hid_h, R * kHid * sizeof(float));
  RELA_ALLOC(a->hid_c, R * kHid * sizeof(float));
  RELA_ALLOC(a->tmp_h, R * kHid * sizeof(float));
  RELA_ALLOC(a->tmp_c, R * kHid * sizeof(float));
  RELA_ALLOC(a->prio_step, R * sizeof(float));
  Windows& w = a->w;
  w.T = a->T;
  w.A = num_action;
  w.seq = seq_len;
  w.burn = burn_in;
  w.n = multi_step;
  RELA_ALLOC(w.s, R * T * kObs);
  RELA_ALLOC(w.eps, R * T * sizeof(float));
  RELA_ALLOC(w.legal, R * T * A * sizeof(float));
  RELA_ALLOC(w.a, R * T * sizeof(int64_t));
  RELA_ALLOC(w.reward, R * T * sizeof(float));
  RELA_ALLOC(w.term, R * T);
  RELA_ALLOC(w.boot, R * T * sizeof(float));
  RELA_ALLOC(w.prio, R * (size_t)(seq_len + multi_step) * sizeof(float));
  RELA_ALLOC(w.h0, R * kHid * sizeof(float));
  RELA_ALLOC(w.c0, R * kHid * sizeof(float));
  RELA_ALLOC(w.nh0, R * kHid * sizeof(float));
  RELA_ALLOC(w.nc0, R * kHid * sizeof(float));
  RELA_ALLOC(a->prow, 2 * R * (size_t)seq_len * sizeof(float));
  RELA_ALLOC(a->lens, 2 * R * sizeof(float));
  RELA_ALLOC(a->agg, 2 * R * sizeof(float));
  RELA_ALLOC(a->d_slot, R * sizeof(int32_t));
  RELA_ALLOC(a->d_flags, R);
  RELA_ALLOC(a->d_ranges, 2 * R * 4 * sizeof(int32_t));
  RELA_ALLOC(a->d_emits, 2 * R * 3 * sizeof(int32_t));
  RELA_ALLOC(a->d_gather, 2 * R * 3 * sizeof(int32_t));
  RELA_ALLOC(a->d_envs, R * sizeof(int32_t));
  a->ws_bytes = rela_lstmnet_workspace_bytes(nullptr, rows);
  RELA_HIP(hipMalloc(&a->ws, (size_t)a->ws_bytes));
  a->h_term.assign(H * R, 0);
  rc = a->stage.init(R * 320 + 4096);
  RELA_CHECK(rc == RELA_OK, rc, "rela_r2d2_actor_create: pinned staging buffer");
  a->book = new SeqBook(rows, multi_step, seq_len, burn_in);
  *out = a;
  return RELA_OK;
}

extern "C" void rela_r2d2_actor_destroy(rela_r2d2_actor* a) {
  if (!a) return;
  DeviceGuard g(a->device);
  (void)hipDeviceSynchronize();
  shard_free(a);
  void* ps[] = {a->hist_h, a->hist_c, a->hid_h,  a->hid_c,  a->tmp_h,  a->tmp_c,    a->prio_step, a->w.s,     a->w.sref,
                a->w.eps,  a->w.legal, a->w.a,   a->w.reward, a->w.term, a->w.boot, a->w.prio,    a->w.h0,    a->w.c0,
                a->w.nh0,  a->w.nc0,  a->prow,   a->lens,   a->agg,    a->d_slot,   a->d_flags,   a->d_ranges, a->d_emits,
                a->d_gather, a->d_envs, a->ws,   a->agg_kept, a->d_kept};
  for (void* p : ps) (void)hipFree(p);
  a->stage.destroy();
  delete a->book;
  delete a;
}

extern "C" void* rela_r2d2_actor_obs_slot(rela_r2d2_actor* a) { return shard_obs_slot(a); }
extern "C" void* rela_r2d2_actor_plane_stage(rela_r2d2_actor* a) { return shard_plane_stage(a); }
extern "C" int rela_r2d2_actor_slide_stacks(rela_r2d2_actor* a, const uint8_t* restart_host, void* stream_) {
  return shard_slide_stacks(a, restart_host, (hipStream_t)stream_, "rela_r2d2_actor_slide_stacks", "rela_r2d2_actor_plane_stage");
}
extern "C" int rela_r2d2_actor_set_screen_input(rela_r2d2_actor* a, int height, int width) {
  return shard_set_screen_input(a, height, width, 3, "rela_r2d2_actor_set_screen_input");
}
extern "C" int rela_r2d2_actor_set_screen_input_indexed(rela_r2d2_actor* a, int height, int width) {
  return shard_set_screen_input(a, height, width, 1, "rela_r2d2_actor_set_screen_input_indexed");
}
extern "C" void* rela_r2d2_actor_palette_stage(rela_r2d2_actor* a) { return a ? a->palettes : nullptr; }
extern "C" void* rela_r2d2_actor_screen_stage(rela_r2d2_actor* a) { return a ? a->screens : nullptr; }
extern "C" int rela_r2d2_actor_screens_to_stacks(rela_r2d2_actor* a, const uint8_t* restart_host, void* stream_) {
  return shard_screens_to_stacks(a, restart_host, (hipStream_t)stream_, "rela_r2d2_actor_screens_to_stacks");
}
extern "C" int rela_r2d2_actor_set_value_rescale(rela_r2d2_actor* a, float eps) {
  return shard_set_value_rescale(a, eps, "rela_r2d2_actor_set_value_rescale");
}
extern "C" int rela_r2d2_actor_set_reuse(rela_r2d2_actor* a, int on) {
  return shard_set_reuse(a, on, "rela_r2d2_actor_set_reuse");
}
extern "C" int rela_r2d2_actor_set_dedup(rela_r2d2_actor* a, int units_per_stack) {
  const int rc = shard_set_dedup_common(a, units_per_stack, a ? a->T : 1, "rela_r2d2_actor_set_dedup");
  if (rc != RELA_OK) return rc;
  DeviceGuard g(a->device);
  const size_t R = (size_t)a->R, T = (size_t)a->T, ups = (size_t)a->dd_ups;
  RELA_HIP(hipMalloc(&a->w.sref, R * T * ups * sizeof(int32_t)));
  RELA_HIP(hipMemset(a->w.sref, 0xff, R * T * ups * sizeof(int32_t)));  // -1: padding
  RELA_HIP(hipMalloc(&a->agg_kept, 2 * R * sizeof(float)));
  RELA_HIP(hipMalloc(&a->d_kept, 2 * R * sizeof(int32_t)));
  RELA_HIP(hipFree(a->w.s));  // the frame windows ([R][T][28,224] B) are no longer needed
  a->w.s = nullptr;
  a->w.ups = a->dd_ups;
  a->tick_win = a->T + a->n + 8;
  a->tick_seq.assign((size_t)a->tick_win, 0);
  a->win_tick.assign(R * T, kPadTick);
  return RELA_OK;
}
extern "C" int64_t rela_r2d2_actor_num_act(const rela_r2d2_actor* a) { return a ? a->num_act.load() : 0; }
extern "C" const float* rela_r2d2_actor_hidden_dev(const rela_r2d2_actor* a, int which) {
  return a ? (which ? a->hid_c : a->hid_h) : nullptr;
}
extern "C" const float* rela_r2d2_actor_last_priority_dev(const rela_r2d2_actor* a) { return a ? a->prio_step : nullptr; }

extern "C" int rela_r2d2_actor_act(rela_r2d2_actor* a, const rela_lstmnet* online, const uint8_t* obs_host,
                                   const float* eps_host, const float* legal_host, int64_t* action_host,
                                   const int64_t** action_dev_out, void* stream_) {
  RELA_CHECK(a && online, RELA_EINVAL, "rela_r2d2_actor_act: bad arguments");
  RELA_CHECK(rela_lstmnet_num_action(online) == a->A, RELA_EINVAL, "rela_r2d2_actor_act: net has %d actions, actor %d",
             rela_lstmnet_num_action(online), a->A);
  RELA_CHECK(a->count <= a->n, RELA_ESTATE, "rela_r2d2_actor_act: act() twice without post_step()");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(a->device);
  ActSlot sl;
  int rc = shard_begin_act(a, obs_host, eps_host, legal_host, s, &sl);
  if (rc != RELA_OK) return rc;
  const size_t R = (size_t)a->R, HB = R * kHid * sizeof(float);
  // historyHidden_.push_back(hidden_) :226-228
  RELA_HIP(dev_copy2(a->hist_h + (size_t)sl.slot * R * kHid, a->hid_h, HB, a->hist_c + (size_t)sl.slot * R * kHid, a->hid_c, HB, s));
  rc = shard_snapshot_consts(a, sl, s);
  if (rc != RELA_OK) return rc;
  // (the dueling Q of this step goes to the slot's table: compute_priority's online_net(obs, hid) n ticks from now)
  a->qh_net[sl.slot] = nullptr;
  rc = rela_lstmnet_step(online, a->R, sl.obs, sl.legal, a->hid_h, a->hid_c, a->tmp_h, a->tmp_c, sl.q, a->q, a->ws,
                         a->ws_bytes, s);
  if (rc != RELA_OK) return rc;
  a->qh_net[sl.slot] = online;
  a->qh_version[sl.slot] = rela_lstmnet_version(online);
  std::swap(a->hid_h, a->tmp_h);  // hidden_ <- new state :241
  std::swap(a->hid_c, a->tmp_c);
  rc = rela_apex_act_from_q(a->R, a->A, a->K, a->q, sl.legal, sl.eps, a->seed, a->act_calls * (uint64_t)a->R, sl.act, s);
  if (rc != RELA_OK) return rc;
  a->q_net = online;
  a->q_version = rela_lstmnet_version(online);
  return shard_finish_act(a, sl, action_host, action_dev_out, s);
}

namespace {
int upload_ranges(rela_r2d2_actor* a, const std::vector<SeqRange>& rs, hipStream_t s) {
  if (rs.empty()) return RELA_OK;
  std::vector<int32_t> flat;
  int maxlen = 0;
  for (const auto& r : rs) {
    flat.insert(flat.end(), {r.env, r.begin, r.end, r.zero_prio});
    maxlen = std::max(maxlen, r.end - r.begin);
  }
  RELA_HIP(a->stage.h2d(a->d_ranges, flat.data(), flat.size() * sizeof(int32_t), s));
  hipLaunchKernelGGL(r2d2_pad, dim3((unsigned)rs.size(), (unsigned)maxlen), dim3(kT), 0, s, a->w, a->d_ranges);
  RELA_LAUNCH_CHECK();
  return RELA_OK;  // `flat` may die: the upload reads the pinned copy
}

// de-duplication: store this tick's stack (shard_dedup_store), then this shard's window of unit sequence numbers: a
// stored tick's first unit, an unstored tick's lower bound (no unit of a later tick is older than seq_hint)
int dedup_store(rela_r2d2_actor* a, int nonblocking, hipStream_t s) {
  DedupStored st;
  const int rc = shard_dedup_store(a, nonblocking, s, &st);
  if (rc != RELA_OK) return rc;
  if (st.stored) a->seq_hint = st.seq + st.count;
  a->tick_seq[(size_t)(st.tick % a->tick_win)] = st.stored ? st.seq : a->seq_hint;
  return RELA_OK;
}

void win_mark(rela_r2d2_actor* a, const std::vector<SeqRange>& rs) {
  for (const auto& r : rs)
    for (int j = r.begin; j < r.end; ++j) a->win_tick[(size_t)r.env * a->T + j] = kPadTick;
}
}  // namespace

extern "C" int rela_r2d2_actor_post_step(rela_r2d2_actor* a, const float* reward_host, const uint8_t* terminal_host,
                                         const rela_lstmnet* online, const rela_lstmnet* target, int nonblocking,
                                         int* n_sequences, void* stream_) {
  RELA_CHECK(a && reward_host && terminal_host && online && target, RELA_EINVAL,
             "rela_r2d2_actor_post_step: bad arguments");
  RELA_CHECK(a->replay, RELA_ESTATE, "rela_r2d2_actor_post_step: evaluation actor has no replay");
  RELA_CHECK(a->cur >= 0, RELA_ESTATE, "rela_r2d2_actor_post_step: no act() to attach the reward to");
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(a->device);
  if (n_sequences) *n_sequences = 0;
  const size_t R = (size_t)a->R;
  const int H = a->n + 1;
  struct StageCall {  // one pinned segment per call, released (event) on every return path
    HostStage& st;
    hipStream_t s;
    StageCall(HostStage& st_, hipStream_t s_) : st(st_), s(s_) { st.begin(); }
    ~StageCall() { st.end(s); }
  } stage_call(a->stage, s);
  RELA_HIP(a->stage.h2d(a->rew + (size_t)a->cur * R, reward_host, R * sizeof(float), s));
  RELA_HIP(a->stage.h2d(a->term + (size_t)a->cur * R, terminal_host, R, s));
  memcpy(&a->h_term[(size_t)a->cur * R], terminal_host, R);
  hipLaunchKernelGGL(r2d2_reset_hidden, dim3(a->R), dim3(128), 0, s, a->term + (size_t)a->cur * R, a->R, a->hid_h,
                     a->hid_c);
  if (a->dd_ups > 0) {
    const int rc = dedup_store(a, nonblocking, s);
    if (rc != RELA_OK) return rc;
  }
  a->cur = -1;
  a->count += 1;
  if (a->count < H) return RELA_OK;  // multiStepBuffer_.canPop :276-279

  const int first = a->head, last = (a->head + a->n) % H;
  int rc = rela_nstep_return(a->n, a->R, a->gamma, first, a->rew, a->term, a->out_r, a->out_b, a->out_t, s);
  if (rc != RELA_OK) return rc;
  const uint8_t* obs_t = a->obs + (size_t)first * R * kObs;
  const uint8_t* obs_n = a->obs + (size_t)last * R * kObs;
  const float *h_t = a->hist_h + (size_t)first * R * kHid, *c_t = a->hist_c + (size_t)first * R * kHid;
  const float *h_n = a->hist_h + (size_t)last * R * kHid, *c_n = a->hist_c + (size_t)last * R * kHid;
  const size_t QA = R * a->A;
  const float* legal_t = a->legal_hist + (size_t)first * R * a->A;
  const float* legal_n = a->legal_hist + (size_t)last * R * a->A;
  const float* eps_t = a->eps_hist + (size_t)first * R;
  // compute_priority  r2d2.py:76-100
  // online_net(obs, hid) :89 is the step act() ran n ticks ago on the same frames with the same recurrent state
  // (historyHidden_.front()) and legal mask: with unchanged weights its Q table in q_hist[first] is reused
  const float* q_online_t = a->q_hist + (size_t)first * QA;
  if (!(a->reuse_mode == 1 && a->qh_net[first] == online && a->qh_version[first] == rela_lstmnet_version(online))) {
    rc = rela_lstmnet_step(online, a->R, obs_t, legal_t, h_t, c_t, a->tmp_h, a->tmp_c, a->q + QA, nullptr, a->ws,
                           a->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    q_online_t = a->q + QA;
  }
  // online_net.act(next_obs, next_hid) :91 is the very step act() ran on this tick (same frames, same
  // recurrent state, same legal mask): with unchanged weights its advantages in q[0] are reused
  const float* adv_next = a->q;
  if (!(a->reuse_mode != 0 && a->q_net == online && a->q_version == rela_lstmnet_version(online) && a->q_slot == last)) {
    rc = rela_lstmnet_step(online, a->R, obs_n, legal_n, h_n, c_n, a->tmp_h, a->tmp_c, nullptr, a->q + 2 * QA, a->ws,
                           a->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    adv_next = a->q + 2 * QA;
  }
  rc = rela_lstmnet_step(target, a->R, obs_n, legal_n, h_n, c_n, a->tmp_h, a->tmp_c, a->q + 3 * QA, nullptr, a->ws,
                         a->ws_bytes, s);  // target_net(next_obs, next_hid, next_action) :93
  if (rc != RELA_OK) return rc;
  const int64_t* act_t = a->act + (size_t)first * R;
  rc = td_from_q(a->R, a->A, a->K, q_online_t, adv_next, a->q + 3 * QA, legal_n, act_t, a->out_r, a->out_b, a->gamma_n,
                 a->vr_eps, nullptr, a->prio_step, s);
  if (rc != RELA_OK) return rc;

  // r2d2Buffer_.push(transition, priority, hid) :289
  SeqPlan& plan = a->plan;
  a->book->step(&a->h_term[(size_t)first * R], &plan);
  rc = upload_ranges(a, plan.front_pad, s);
  if (rc != RELA_OK) return rc;
  RELA_HIP(a->stage.h2d(a->d_slot, plan.write_slot.data(), R * sizeof(int32_t), s));
  RELA_HIP(a->stage.h2d(a->d_flags, plan.flags.data(), R, s));
  const bool dd = a->dd_ups > 0;
  const int32_t* refs_t = dd ? a->ref_hist + (size_t)first * R * a->dd_ups : nullptr;
  hipLaunchKernelGGL(r2d2_write_step, dim3(a->R), dim3(kT), 0, s, a->w, a->d_slot, a->d_flags, obs_t, eps_t, legal_t,
                     act_t, a->out_r, a->out_t, a->out_b, a->prio_step, h_t, c_t, refs_t);
  RELA_LAUNCH_CHECK();
  rc = upload_ranges(a, plan.tail_pad, s);
  if (rc != RELA_OK) return rc;
  // de-duplication: the host mirror of the windows' ticks (which entries are padding, which hold an unstored tick)
  const int64_t t_first = a->tick - 1 - a->n;  // the tick obs_t was acted on
  if (dd) {
    win_mark(a, plan.front_pad);
    const int64_t v = a->refs_valid[first] ? t_first : kLostTick;
    for (int i = 0; i < a->R; ++i) a->win_tick[(size_t)i * a->T + plan.write_slot[i]] = v;
    win_mark(a, plan.tail_pad);
  }

  if (plan.can_pop) {  // :292-301
    const int nseq = (int)plan.emits.size();
    std::vector<int32_t> em;
    for (const auto& e : plan.emits) em.insert(em.end(), {e.env, e.len, e.second});
    RELA_HIP(a->stage.h2d(a->d_emits, em.data(), em.size() * sizeof(int32_t), s));
    hipLaunchKernelGGL(r2d2_collect, dim3(nseq), dim3(128), 0, s, a->w, a->d_emits, nseq, a->prow, a->lens);
    hipLaunchKernelGGL(r2d2_aggregate, dim3(ceil_div(nseq, 64)), dim3(64), 0, s, a->prow, a->lens, nseq, a->seq, a->burn,
                       a->eta, a->one_minus_eta, a->agg);
    RELA_LAUNCH_CHECK();
    // A pop of a large shard can exceed what a blocking append can ever get (ring - capacity slots:
    // sample() evicts down to capacity only).  The pop therefore goes in pieces of at most that many
    // sequences, cut at env boundaries (an env's second, short sequence directly follows its first):
    // reserve, write the first sequences, carry those envs' windows, write their second sequences, commit.
    int cap = 0, ring = 0;
    rc = rela_replay_limits(a->replay, &cap, &ring);
    if (rc != RELA_OK) return rc;
    const int max_block = ring - cap > 1 ? ring - cap : 1;
    const Windows& w = a->w;
    int inserted = 0, dropped = 0;
    // de-duplication: a sequence is kept only if every stack of its window was stored (keep[q]), and its block declares
    // the oldest unit it may refer to.  For that bound: a window spans at most T consecutive ticks up to t_first, and a
    // plane-unit stack reaches 3 ticks further back -- never across an unstored tick (a keyframe follows it).  The bound
    // is the same for every sequence of this tick and grows with the tick, so the slots' bounds stay in FIFO order.
    std::vector<uint8_t> keep((size_t)nseq, 1);
    int64_t min_seq = 0;
    if (dd) {
      std::vector<uint8_t> carries(R, 0);
      for (int e : plan.carry_env) carries[(size_t)e] = 1;
      std::vector<int> pad_of(R, -1);
      for (size_t k = 0; k < plan.carry_pad.size(); ++k) pad_of[(size_t)plan.carry_pad[k].env] = (int)k;
      auto stored = [&](int env) {
        const int64_t* wt = &a->win_tick[(size_t)env * a->T];
        for (int j = 0; j < a->T; ++j)
          if (wt[j] == kLostTick) return false;
        return true;
      };
      for (int q = 0; q < nseq; ++q) {  // in emission order, with the carry-over replayed between an env's two sequences
        const int env = plan.emits[q].env;
        keep[(size_t)q] = stored(env) ? 1 : 0;
        if (plan.emits[q].second || !carries[(size_t)env]) continue;
        int64_t* wt = &a->win_tick[(size_t)env * a->T];
        for (int j = 0; j < a->burn + a->n; ++j) wt[j] = wt[a->seq + j];
        if (pad_of[(size_t)env] >= 0) win_mark(a, {plan.carry_pad[(size_t)pad_of[(size_t)env]]});
      }
      int64_t oldest = t_first - (a->T - 1) - (a->dd_ups == 4 ? 3 : 0);
      if (oldest < 0) oldest = 0;
      min_seq = a->tick_seq[(size_t)(oldest % a->tick_win)];  // (tick - oldest <= T + n + 3 < tick_win)
    }
    size_t ci = 0, pi = 0;  // cursors into carry_env / carry_pad (both ascending in env)
    for (int q0 = 0; q0 < nseq && rc == RELA_OK;) {
      int q1 = nseq - q0 <= max_block ? nseq : q0 + max_block;
      if (q1 < nseq && plan.emits[q1].second) q1 = (q1 - 1 > q0) ? q1 - 1 : q1 + 1;  // keep a pair together
      int cnt = q1 - q0;
      const int env_hi = plan.emits[q1 - 1].env;
      std::vector<int32_t> carry;
      while (ci < plan.carry_env.size() && plan.carry_env[ci] <= env_hi) carry.push_back(plan.carry_env[ci++]);
      std::vector<SeqRange> pads;
      while (pi < plan.carry_pad.size() && plan.carry_pad[pi].env <= env_hi) pads.push_back(plan.carry_pad[pi++]);
      auto carry_piece = [&]() -> int {
        if (carry.empty()) return RELA_OK;
        RELA_HIP(a->stage.h2d(a->d_envs, carry.data(), carry.size() * sizeof(int32_t), s));
        hipLaunchKernelGGL(r2d2_carry, dim3((unsigned)carry.size()), dim3(kT), 0, s, a->w, a->d_envs);
        RELA_LAUNCH_CHECK();
        return upload_ranges(a, pads, s);
      };
      std::vector<int32_t> kept;  // (de-duplication) the sequences of this piece that are stored
      if (dd) {
        for (int q = q0; q < q1; ++q)
          if (keep[(size_t)q]) kept.push_back(q);
        if ((int)kept.size() < cnt) dropped = 1;
        cnt = (int)kept.size();
        if (cnt == 0) {  // the windows advance as if stored
          rc = carry_piece();
          q0 = q1;
          continue;
        }
      }
      int slot0 = 0;
      rc = rela_replay_begin_add(a->replay, cnt, nonblocking, &slot0);
      if (rc == RELA_EWOULDBLOCK) {
        // dropped piece: the windows must still advance exactly as if it had been stored
        dropped = 1;
        rc = carry_piece();
        q0 = q1;
        continue;
      }
      if (rc != RELA_OK) break;
      if (dd) {
        rc = rela_replay_set_block_min_unit(a->replay, slot0, cnt, min_seq);
        if (rc != RELA_OK) {
          (void)rela_replay_abort_add(a->replay, slot0, cnt);
          break;
        }
      }
      // all sequences of one kind leave in ONE gathered write per field: destination offset q - q0 (de-duplication: the
      // rank among the kept ones), source row = the env's window (lens is indexed by q itself)
      auto emit_batch = [&](bool second) -> int {
        std::vector<int32_t> dst, envs, qs;
        int rank = 0;
        for (int q = q0; q < q1; ++q) {
          if (dd && !keep[(size_t)q]) continue;
          if ((plan.emits[q].second != 0) == second) {
            dst.push_back(dd ? rank : q - q0);
            envs.push_back(plan.emits[q].env);
            qs.push_back(q);
          }
          ++rank;
        }
        const int m = (int)dst.size();
        if (m == 0) return RELA_OK;
        int32_t* d_dst = a->d_gather + (second ? 3 * (size_t)a->R : 0);
        int32_t* d_env = d_dst + m;
        int32_t* d_q = d_env + m;
        std::vector<int32_t> all(dst);
        all.insert(all.end(), envs.begin(), envs.end());
        all.insert(all.end(), qs.begin(), qs.end());
        RELA_HIP(a->stage.h2d(d_dst, all.data(), all.size() * sizeof(int32_t), s));  // pinned copy: `all` may die
        const void* stacks = dd ? (const void*)w.sref : (const void*)w.s;
        const void* bases[10] = {stacks, w.eps, w.legal, w.a, w.reward, w.term, w.boot, w.h0, w.c0, a->lens};
        const int32_t* idx[10] = {d_env, d_env, d_env, d_env, d_env, d_env, d_env, d_env, d_env, d_q};
        return rela_replay_write_rows_gather(a->replay, slot0, m, d_dst, bases, idx, s);
      };
      rc = emit_batch(false);
      if (rc == RELA_OK) rc = carry_piece();
      if (rc == RELA_OK) rc = emit_batch(true);
      const float* prio = a->agg + q0;
      if (rc == RELA_OK && dd && cnt < q1 - q0) {  // the priorities of the kept sequences, in slot order
        rc = a->stage.h2d(a->d_kept, kept.data(), kept.size() * sizeof(int32_t), s) == hipSuccess ? RELA_OK : RELA_ENODEV;
        if (rc == RELA_OK) {
          hipLaunchKernelGGL(r2d2_pick, dim3(ceil_div(cnt, 256)), dim3(256), 0, s, (const float*)a->agg, a->d_kept, cnt,
                             a->agg_kept);
          prio = a->agg_kept;
        }
      }
      if (rc == RELA_OK) rc = rela_replay_commit_add(a->replay, slot0, cnt, prio, s);
      if (rc == RELA_OK) inserted += cnt;
      else (void)rela_replay_abort_add(a->replay, slot0, cnt);  // never leave a reservation uncommitted
      q0 = q1;
    }
    if (rc != RELA_OK) return rc;
    if (n_sequences) *n_sequences = inserted;
    if (dropped) rc = RELA_EWOULDBLOCK;
    if (rc != RELA_OK && rc != RELA_EWOULDBLOCK) return rc;
  }
  a->head = (a->head + 1) % H;  // multiStepBuffer_ / historyHidden_ pop_front :283-286
  a->count -= 1;
  return plan.can_pop && rc == RELA_EWOULDBLOCK ? RELA_EWOULDBLOCK : RELA_OK;
}
