// actor_shard.h -- the part of a device-resident actor shard the Ape-X shard (actor.hip, rela_apex_actor_*) and the R2D2
// shard (actor_r2d2.hip, rela_r2d2_actor_*) share: the n-step ring of MultiStepTransitionBuffer (rela/dqn_actor.h:15-124)
// in HBM, the screen / sliding-stack input of the observation slot, and the per-tick store of frame-stack
// de-duplication.  rela_apex_actor and rela_r2d2_actor derive from ActorShardBase; their extern "C" entry points forward
// here with their own name (`who`), which leads every message.
#pragma once
#include <atomic>
#include <vector>

#include "common.h"
#include "dedup_refs.h"

namespace rela_amd {

constexpr int64_t kObs = 4 * 84 * 84;  // bytes of one frame stack
constexpr int64_t kPlane = 84 * 84;    // ... and of one of its planes

struct ActorShardBase {
  int device = 0;
  int R = 0, K = 0, A = 0, n = 0;  // rows, rows per group, actions, multi_step
  rela_replay* replay = nullptr;   // null: evaluation shard
  uint64_t act_calls = 0;
  std::atomic<int64_t> num_act{0};
  // n-step ring of n+1 history slots (the deque of dqn_actor.h:120-123; "pop_front" is a head increment)
  int head = 0, count = 0, cur = -1;  // oldest slot, slots in use, slot of an act() that awaits its post_step()
  uint8_t* obs = nullptr;             // [n+1][R][28224]
  int64_t* act = nullptr;             // [n+1][R]
  float* rew = nullptr;               // [n+1][R]
  uint8_t* term = nullptr;            // [n+1][R]
  float* eps = nullptr;               // [R]      current values (callers may write them on the device) ...
  float* legal = nullptr;             // [R][A]
  float* eps_hist = nullptr;          // [n+1][R]     ... snapshotted per history slot by act(), because the
  float* legal_hist = nullptr;        // [n+1][R][A]  transition's obs side carries those of time t-n (:84-90)
  float* q = nullptr;                 // [4][R][A]   scratch tables of post_step (each shard's own layout)
  float* q_hist = nullptr;            // [n+1][R][A] act()'s own Q table of every history slot
  float *out_r = nullptr, *out_b = nullptr;  // [R] n-step return and bootstrap flag of the popped transition
  uint8_t* out_t = nullptr;                  // [R] ... and its terminal
  // net (rela_ffnet / rela_lstmnet) and weight version act() evaluated every history slot with (q_hist[slot])
  std::vector<const void*> qh_net;
  std::vector<uint64_t> qh_version;
  int q_slot = -1;     // slot of the last act()
  int reuse_mode = 1;  // 0: recompute everything, 1: reuse both act() forwards, 2: only the one of s_t+n
  // Ape-X shard (*_set_fused_insert): the target forward stores into the reserved replay rows itself: 1 next_obs, 2 next_obs
  // and obs, 0 neither
  int fused_insert = 2;
  float vr_eps = 0.f;  // value rescaling of the priority's TD target (*_set_value_rescale; value_rescale.h), 0 = off
  // sliding-stack and screen input of the observation slot
  uint8_t* restart = nullptr;       // [R] *_slide_stacks / *_screens_to_stacks: 1 = the row's stack restarts with its new plane
  uint8_t* fresh_planes = nullptr;  // [R][7056] staging of the newest plane of every row (*_plane_stage)
  uint8_t* screens = nullptr;       // [R][2][scr_h][scr_w][3] screen pairs (*_set_screen_input), or
                                    // [R][2][scr_h][scr_w] palette indices (*_set_screen_input_indexed)
  uint8_t* palettes = nullptr;      // [R][256][3] RGB table of every row: indexed screens only
  uint8_t* screen_prev = nullptr;   // [R][28224] evaluation shard (no replay): copy of the one slot it acts on
  int scr_h = 0, scr_w = 0;
  // frame-stack de-duplication (*_set_dedup; replay side: rela_replay_set_schema_dedup / _seq_dedup): every tick the
  // stack acted on enters the replay's unit ring once, and transitions / windows refer to it
  int dd_ups = 0;                   // 0 = off, 1 = one unit per stack, 4 = one unit per 84x84 plane
  int64_t dd_cap = 0;               // units in the replay's ring
  int32_t* ref_hist = nullptr;      // [n+1][R][ups] unit indices of every history slot's stack
  std::vector<uint8_t> refs_valid;  // [n+1] the slot's units were stored
  std::vector<int64_t> tick_seq;    // first unit sequence number of the last ticks (ring by tick; each shard's own size)
  int64_t tick = 0;                 // ticks that went through the store so far
};

namespace {

template <class P>
inline int shard_alloc(P** p, size_t bytes) {  // a zero-filled device buffer
  RELA_HIP(hipMalloc(reinterpret_cast<void**>(p), bytes));
  RELA_HIP(hipMemset(*p, 0, bytes));
  return RELA_OK;
}
#define RELA_ALLOC(ptr, bytes)                          \
  do {                                                  \
    int _rc = ::rela_amd::shard_alloc(&(ptr), (bytes)); \
    if (_rc != RELA_OK) return _rc;                     \
  } while (0)

// the ring of R, A, n (set by the caller, on the caller's device): zero-filled, legal_move all ones
inline int shard_alloc_ring(ActorShardBase* a) {
  const size_t H = (size_t)a->n + 1, R = (size_t)a->R, A = (size_t)a->A;
  RELA_ALLOC(a->obs, H * R * kObs);
  RELA_ALLOC(a->act, H * R * sizeof(int64_t));
  RELA_ALLOC(a->rew, H * R * sizeof(float));
  RELA_ALLOC(a->term, H * R);
  RELA_ALLOC(a->eps, R * sizeof(float));
  RELA_ALLOC(a->legal, R * A * sizeof(float));
  RELA_ALLOC(a->eps_hist, H * R * sizeof(float));
  RELA_ALLOC(a->legal_hist, H * R * A * sizeof(float));
  RELA_ALLOC(a->q, 4 * R * A * sizeof(float));
  RELA_ALLOC(a->q_hist, H * R * A * sizeof(float));
  RELA_ALLOC(a->out_r, R * sizeof(float));
  RELA_ALLOC(a->out_b, R * sizeof(float));
  RELA_ALLOC(a->out_t, R);
  a->qh_net.assign(H, nullptr);
  a->qh_version.assign(H, 0);
  std::vector<float> ones(R * A, 1.0f);
  RELA_HIP(hipMemcpy(a->legal, ones.data(), R * A * sizeof(float), hipMemcpyHostToDevice));
  return RELA_OK;
}

inline void shard_free(ActorShardBase* a) {
  void* ps[] = {a->obs,   a->act,   a->rew,      a->term,    a->eps,          a->legal,   a->eps_hist, a->legal_hist,
                a->q,     a->q_hist, a->out_r,   a->out_b,   a->out_t,        a->restart, a->fresh_planes,
                a->screens, a->palettes, a->screen_prev, a->ref_hist};
  for (void* p : ps) (void)hipFree(p);
}

inline int shard_next_slot(const ActorShardBase* a) { return (a->head + a->count) % (a->n + 1); }
inline uint8_t* shard_obs_at(const ActorShardBase* a, int slot) { return a->obs + (size_t)slot * a->R * kObs; }

inline void* shard_obs_slot(ActorShardBase* a) { return a ? shard_obs_at(a, shard_next_slot(a)) : nullptr; }

inline void* shard_plane_stage(ActorShardBase* a) {
  if (!a) return nullptr;
  if (!a->fresh_planes) {
    DeviceGuard g(a->device);
    if (hipMalloc(&a->fresh_planes, (size_t)a->R * kPlane) != hipSuccess) a->fresh_planes = nullptr;
  }
  return a->fresh_planes;
}

// stage_fn: the name of the shard's *_plane_stage, for the message
inline int shard_slide_stacks(ActorShardBase* a, const uint8_t* restart_host, hipStream_t s, const char* who,
                              const char* stage_fn) {
  RELA_CHECK(a && restart_host, RELA_EINVAL, "%s: bad arguments", who);
  RELA_CHECK(a->fresh_planes, RELA_ESTATE, "%s: no plane was staged (%s)", who, stage_fn);
  RELA_CHECK(a->act_calls > 0, RELA_ESTATE, "%s: the first observation must be uploaded whole", who);
  RELA_CHECK(a->count <= a->n, RELA_ESTATE, "%s: act() twice without post_step()", who);
  DeviceGuard g(a->device);
  if (!a->restart) RELA_HIP(hipMalloc(&a->restart, (size_t)a->R));
  RELA_HIP(hipMemcpyAsync(a->restart, restart_host, (size_t)a->R, hipMemcpyHostToDevice, s));
  const int H = a->n + 1, slot = shard_next_slot(a), prev = (slot + H - 1) % H;
  return slide_stacks(shard_obs_at(a, slot), shard_obs_at(a, prev), a->fresh_planes, a->restart, a->R, s);
}

// channels: 3 = RGB screens, 1 = palette indices (a zeroed palette stage comes with them)
inline int shard_set_screen_input(ActorShardBase* a, int height, int width, int channels, const char* who) {
  RELA_CHECK(a && height >= 2 && height <= 512 && width >= 2 && width <= 512, RELA_EINVAL,
             "%s: bad arguments (screens must be 2..512 x 2..512)", who);
  RELA_CHECK(a->act_calls == 0 && !a->screens, RELA_ESTATE,
             "%s: call it once, before the first act() (a shard takes RGB or indexed screens, not both)", who);
  DeviceGuard g(a->device);
  RELA_ALLOC(a->screens, (size_t)a->R * 2 * height * width * channels);
  if (channels == 1) RELA_ALLOC(a->palettes, (size_t)a->R * 768);
  RELA_CHECK(shard_plane_stage(a), RELA_ENOMEM, "%s: plane stage", who);
  if (!a->replay) RELA_HIP(hipMalloc(&a->screen_prev, (size_t)a->R * kObs));
  a->scr_h = height;
  a->scr_w = width;
  return RELA_OK;
}

inline int shard_screens_to_stacks(ActorShardBase* a, const uint8_t* restart_host, hipStream_t s, const char* who) {
  RELA_CHECK(a, RELA_EINVAL, "%s: bad arguments", who);
  RELA_CHECK(a->count <= a->n, RELA_ESTATE, "%s: act() twice without post_step()", who);
  DeviceGuard g(a->device);
  const int slot = shard_next_slot(a), prev = a->q_slot >= 0 ? a->q_slot : slot;  // the stacks of the last act()
  return screens_to_stacks(a->screens, a->palettes, a->scr_h, a->scr_w, a->fresh_planes, &a->restart, restart_host,
                           a->act_calls == 0, shard_obs_at(a, slot), shard_obs_at(a, prev), a->screen_prev, a->R, s, who);
}

inline int shard_set_reuse(ActorShardBase* a, int on, const char* who) {
  RELA_CHECK(a, RELA_EINVAL, "%s: bad arguments", who);
  RELA_CHECK(on >= 0 && on <= 2, RELA_EINVAL, "%s: 0 (off), 1 (on) or 2 (next_obs only)", who);
  a->reuse_mode = on;
  return RELA_OK;
}

inline int shard_set_value_rescale(ActorShardBase* a, float eps, const char* who) {
  RELA_CHECK(a && eps == eps, RELA_EINVAL, "%s: bad arguments", who);
  RELA_CHECK(a->act_calls == 0, RELA_ESTATE, "%s: call it before the first act()", who);
  a->vr_eps = eps > 0.f ? eps : 0.f;
  return RELA_OK;
}

// The part of *_set_dedup both shards share: the state guard, the replay's schema against units_per_stack, the ring of
// references.  steps: 0 = a transition replay (Ape-X); otherwise the steps per slot a sequence replay must have (R2D2).
// The caller sizes tick_seq and adds what else it keeps.
inline int shard_set_dedup_common(ActorShardBase* a, int units_per_stack, int steps, const char* who) {
  RELA_CHECK(a && a->replay && (units_per_stack == 1 || units_per_stack == 4), RELA_EINVAL,
             "%s: needs a replay and 1 (stack units) or 4 (plane units)", who);
  RELA_CHECK(a->act_calls == 0 && a->count == 0 && a->tick == 0 && a->dd_ups == 0, RELA_ESTATE,
             "%s: call it once, before the first act()", who);
  int ups = 0;
  int64_t ub = 0, cap = 0;
  const int rc = rela_replay_dedup_info(a->replay, &ups, &ub, &cap);
  if (rc != RELA_OK) return rc;
  const bool units_ok = ups == units_per_stack && ub * ups == kObs;
  if (steps > 0) {
    const int have = rela_replay_dedup_steps(a->replay);
    RELA_CHECK(units_ok && have == steps, RELA_EINVAL,
               "%s: the replay's schema has %d units of %lld bytes per stack and %d steps per slot "
               "(this shard: %d steps; needs rela_replay_set_schema_seq_dedup)", who, ups, (long long)ub, have, steps);
  } else {
    RELA_CHECK(units_ok, RELA_EINVAL, "%s: the replay's schema has %d units of %lld bytes per stack", who, ups, (long long)ub);
  }
  DeviceGuard g(a->device);
  const size_t H = (size_t)a->n + 1;
  RELA_ALLOC(a->ref_hist, H * (size_t)a->R * ups * sizeof(int32_t));
  a->dd_ups = ups;
  a->dd_cap = cap;
  a->refs_valid.assign(H, 0);
  return RELA_OK;
}

// The front of *_act after the caller's own argument checks.  shard_begin_act names the history slot this act() fills
// and queues the three optional uploads; shard_snapshot_consts copies eps / legal_move into the slot (the R2D2 shard
// copies its hidden history in between).
struct ActSlot {
  int slot;
  uint8_t* obs;        // [R][28224]
  float *eps, *legal;  // [R], [R][A]: the slot's snapshots
  float* q;            // [R][A]
  int64_t* act;        // [R]
};
inline int shard_begin_act(ActorShardBase* a, const uint8_t* obs_host, const float* eps_host, const float* legal_host,
                           hipStream_t s, ActSlot* sl) {
  const int slot = shard_next_slot(a);
  const size_t R = (size_t)a->R, RA = R * a->A;
  *sl = {slot, shard_obs_at(a, slot), a->eps_hist + slot * R, a->legal_hist + slot * RA, a->q_hist + slot * RA,
         a->act + slot * R};
  if (obs_host) RELA_HIP(hipMemcpyAsync(sl->obs, obs_host, R * kObs, hipMemcpyHostToDevice, s));
  if (eps_host) RELA_HIP(hipMemcpyAsync(a->eps, eps_host, R * sizeof(float), hipMemcpyHostToDevice, s));
  if (legal_host) RELA_HIP(hipMemcpyAsync(a->legal, legal_host, RA * sizeof(float), hipMemcpyHostToDevice, s));
  return RELA_OK;
}
inline int shard_snapshot_consts(ActorShardBase* a, const ActSlot& sl, hipStream_t s) {
  const size_t R = (size_t)a->R;
  RELA_HIP(dev_copy2(sl.eps, a->eps, R * sizeof(float), sl.legal, a->legal, R * a->A * sizeof(float), s));
  return RELA_OK;
}

// The tail of *_act: the slot's forward and its actions are queued; counters, then the actions' way out.
inline int shard_finish_act(ActorShardBase* a, const ActSlot& sl, int64_t* action_host, const int64_t** action_dev_out,
                            hipStream_t s) {
  const int64_t* act = sl.act;
  a->act_calls += 1;
  a->cur = sl.slot;
  a->q_slot = sl.slot;
  a->num_act += a->R;  // dqn_actor.h:169
  if (action_dev_out) *action_dev_out = act;
  if (action_host) {
    RELA_HIP(hipMemcpyAsync(action_host, act, (size_t)a->R * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RELA_HIP(hipStreamSynchronize(s));
  }
  return RELA_OK;
}

// De-duplicated replay: the stack acted on this tick (history slot `cur`) enters the unit ring ONCE -- one new plane, or
// all four on a keyframe (the first tick, or the first after an unstored one), or the whole stack -- and ref_hist[cur]
// receives its references; transitions refer to it (as next_obs now, as obs n ticks from now).  Ring full and
// nonblocking: the tick is not stored (stored = false) and what would refer to it is dropped.  The tick advances either
// way; the caller's window bookkeeping (tick_seq and what it keeps besides) reads `tick` as the tick just handled.
struct DedupStored {
  bool stored;
  int keyframe, count;  // all planes were stored; units reserved
  int64_t seq;          // first unit sequence number
  int64_t tick;
};
inline int shard_dedup_store(ActorShardBase* a, int nonblocking, hipStream_t s, DedupStored* out) {
  const int H = a->n + 1, cur = a->cur, prev = (cur + H - 1) % H, ups = a->dd_ups;
  const bool prev_ok = a->tick > 0 && a->refs_valid[prev];
  const int keyframe = (ups == 4 && !prev_ok) ? 1 : 0;
  const int count = keyframe ? 4 * a->R : a->R;
  int64_t seq = 0;
  int32_t idx = 0;
  int rc = rela_replay_units_reserve(a->replay, count, nonblocking, &seq, &idx);
  if (rc != RELA_OK && rc != RELA_EWOULDBLOCK) return rc;
  const bool stored = rc == RELA_OK;
  if (stored) {
    const uint8_t* stack = shard_obs_at(a, cur);
    if (ups == 1) rc = rela_replay_units_write(a->replay, seq, count, stack, kObs, s);
    else if (keyframe) rc = rela_replay_units_write(a->replay, seq, count, stack, kPlane, s);
    else rc = rela_replay_units_write(a->replay, seq, count, stack + 3 * kPlane, kObs, s);  // the newest plane
    if (rc != RELA_OK) return rc;
    hipLaunchKernelGGL(dedup_make_refs, dim3(ceil_div(a->R, 256)), dim3(256), 0, s, a->ref_hist + (size_t)cur * a->R * ups,
                       a->ref_hist + (size_t)prev * a->R * ups, a->term + (size_t)prev * a->R, a->R, ups, keyframe, idx,
                       a->dd_cap);
    RELA_LAUNCH_CHECK();
  }
  a->refs_valid[cur] = stored ? 1 : 0;
  *out = {stored, keyframe, count, seq, a->tick};
  a->tick += 1;
  return RELA_OK;
}

}  // namespace
}  // namespace rela_amd
