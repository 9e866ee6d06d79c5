// actor.hip -- device-resident Ape-X actor shard (C ABI: rela_apex_actor_*).
//
// Restates the per-step work BasicThreadLoop::mainLoop (rela/thread_loop.h:74-105) drives through
// DQNActor (rela/dqn_actor.h:126-211) and MultiStepTransitionBuffer (:15-124):
//   act        push (obs, action) :23-29,153-171      -> 1 trunk forward + eps-greedy
//   post_step  push (r, t) :31-40; canPop :46-48; popTransition :58-106; computePriority :193-203
//              (online(s_t), online(s_t+n), target(s_t+n), apex.py:30-45; online(s_t+n) is act()'s own
//              forward of this tick and online(s_t) is act()'s forward of n ticks ago: each is reused when
//              the online weights were not re-loaded in between); replay add :189
// The deque of :120-123 is a ring of multi_step+1 slots in HBM; "pop_front" is a head increment.
#include <cmath>

#include "actor_shard.h"
#include "ffnet_layout.h"

using namespace rela_amd;

struct rela_apex_actor : ActorShardBase {
  float gamma = 0.f, gamma_n = 0.f;
  uint64_t seed = 0;
  // q: tables recomputed in post_step (1: online(s_t), 2: online(s_t+n), 3: target)
  float* prio = nullptr;  // [R] priorities of the last popped transitions
  void* ws = nullptr;
  int64_t ws_bytes = 0;
  int64_t key_tick = -1;  // de-duplication: tick of the last keyframe (all planes stored)
};

namespace {
constexpr int kTickWin = 64;  // de-duplication: ticks tick_seq remembers
}

extern "C" int rela_apex_actor_create(rela_apex_actor** out, int rows, int group_rows, int num_action, int multi_step,
                                      float gamma, rela_replay* replay, uint64_t seed, int device) {
  RELA_CHECK(out && rows >= 1 && group_rows >= 1 && rows % group_rows == 0 && num_action >= 1 && num_action <= 31 &&
                 multi_step >= 1,
             RELA_EINVAL, "rela_apex_actor_create: bad arguments (rows=%d group=%d A=%d n=%d)", rows, group_rows,
             num_action, multi_step);
  int rc = check_device(device, "rela_apex_actor_create");
  if (rc != RELA_OK) return rc;
  DeviceGuard g(device);
  auto* a = new rela_apex_actor();
  a->device = device;
  a->R = rows;
  a->K = group_rows;
  a->A = num_action;
  a->n = multi_step;
  a->gamma = gamma;
  a->gamma_n = (float)pow((double)gamma, (double)multi_step);  // gamma ** multi_step, apex.py:44
  a->replay = replay;
  a->seed = seed;
  rc = shard_alloc_ring(a);
  if (rc != RELA_OK) return rc;
  RELA_ALLOC(a->prio, (size_t)rows * sizeof(float));
  a->ws_bytes = rela_ffnet_workspace_bytes(nullptr, rows);
  RELA_HIP(hipMalloc(&a->ws, (size_t)a->ws_bytes));
  *out = a;
  return RELA_OK;
}

extern "C" void rela_apex_actor_destroy(rela_apex_actor* a) {
  if (!a) return;
  DeviceGuard g(a->device);
  (void)hipDeviceSynchronize();
  shard_free(a);
  (void)hipFree(a->prio);
  (void)hipFree(a->ws);
  delete a;
}

extern "C" void* rela_apex_actor_obs_slot(rela_apex_actor* a) { return shard_obs_slot(a); }
extern "C" void* rela_apex_actor_plane_stage(rela_apex_actor* a) { return shard_plane_stage(a); }
extern "C" int rela_apex_actor_slide_stacks(rela_apex_actor* a, const uint8_t* restart_host, void* stream_) {
  return shard_slide_stacks(a, restart_host, (hipStream_t)stream_, "rela_apex_actor_slide_stacks", "rela_apex_actor_plane_stage");
}
extern "C" int rela_apex_actor_set_screen_input(rela_apex_actor* a, int height, int width) {
  return shard_set_screen_input(a, height, width, 3, "rela_apex_actor_set_screen_input");
}
extern "C" int rela_apex_actor_set_screen_input_indexed(rela_apex_actor* a, int height, int width) {
  return shard_set_screen_input(a, height, width, 1, "rela_apex_actor_set_screen_input_indexed");
}
extern "C" void* rela_apex_actor_palette_stage(rela_apex_actor* a) { return a ? a->palettes : nullptr; }
extern "C" void* rela_apex_actor_screen_stage(rela_apex_actor* a) { return a ? a->screens : nullptr; }
extern "C" int rela_apex_actor_screens_to_stacks(rela_apex_actor* a, const uint8_t* restart_host, void* stream_) {
  return shard_screens_to_stacks(a, restart_host, (hipStream_t)stream_, "rela_apex_actor_screens_to_stacks");
}
extern "C" int rela_apex_actor_set_reuse(rela_apex_actor* a, int on) {
  return shard_set_reuse(a, on, "rela_apex_actor_set_reuse");
}
extern "C" int rela_apex_actor_set_fused_insert(rela_apex_actor* a, int on) {
  RELA_CHECK(a && on >= 0 && on <= 2, RELA_EINVAL, "rela_apex_actor_set_fused_insert: 0 (off), 1 (next_obs) or 2 (next_obs and obs)");
  a->fused_insert = on;
  return RELA_OK;
}
extern "C" int rela_apex_actor_set_value_rescale(rela_apex_actor* a, float eps) {
  return shard_set_value_rescale(a, eps, "rela_apex_actor_set_value_rescale");
}
extern "C" int rela_apex_actor_set_dedup(rela_apex_actor* a, int units_per_stack) {
  const int rc = shard_set_dedup_common(a, units_per_stack, 0, "rela_apex_actor_set_dedup");
  if (rc == RELA_OK) a->tick_seq.assign(kTickWin, 0);
  return rc;
}
extern "C" float* rela_apex_actor_eps_dev(rela_apex_actor* a) { return a ? a->eps : nullptr; }
extern "C" float* rela_apex_actor_legal_dev(rela_apex_actor* a) { return a ? a->legal : nullptr; }
extern "C" int64_t rela_apex_actor_num_act(const rela_apex_actor* a) { return a ? a->num_act.load() : 0; }
extern "C" const float* rela_apex_actor_last_q_dev(const rela_apex_actor* a) {
  return a ? a->q_hist + (size_t)(a->q_slot < 0 ? 0 : a->q_slot) * a->R * a->A : nullptr;
}
extern "C" const float* rela_apex_actor_last_priority_dev(const rela_apex_actor* a) { return a ? a->prio : nullptr; }

extern "C" int rela_apex_actor_act(rela_apex_actor* a, const rela_ffnet* online, const uint8_t* obs_host,
                                   const float* eps_host, const float* legal_host, int64_t* action_host,
                                   const int64_t** action_dev_out, void* stream_) {
  RELA_CHECK(a && online, RELA_EINVAL, "rela_apex_actor_act: bad arguments");
  RELA_CHECK(rela_ffnet_num_action(online) == a->A, RELA_EINVAL, "rela_apex_actor_act: net has %d actions, actor %d",
             rela_ffnet_num_action(online), a->A);
  RELA_CHECK(a->count <= a->n, RELA_ESTATE, "rela_apex_actor_act: act() twice without post_step()");  // :24-25
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(a->device);
  ActSlot sl;
  int rc = shard_begin_act(a, obs_host, eps_host, legal_host, s, &sl);
  if (rc == RELA_OK) rc = shard_snapshot_consts(a, sl, s);
  if (rc != RELA_OK) return rc;
  a->qh_net[sl.slot] = nullptr;
  rc = rela_ffnet_forward(online, a->R, sl.obs, sl.legal, sl.q, a->ws, a->ws_bytes, s);
  if (rc != RELA_OK) return rc;
  rc = rela_apex_act_from_q(a->R, a->A, a->K, sl.q, sl.legal, sl.eps, a->seed, a->act_calls * (uint64_t)a->R, sl.act, s);
  if (rc != RELA_OK) return rc;
  a->qh_net[sl.slot] = online;
  a->qh_version[sl.slot] = rela_ffnet_version(online);
  return shard_finish_act(a, sl, action_host, action_dev_out, s);
}

extern "C" int rela_apex_actor_post_step(rela_apex_actor* a, const float* reward, const uint8_t* terminal,
                                         int on_device, const rela_ffnet* online, const rela_ffnet* target,
                                         int nonblocking, int* inserted, void* stream_) {
  RELA_CHECK(a && reward && terminal && online && target, RELA_EINVAL, "rela_apex_actor_post_step: bad arguments");
  RELA_CHECK(a->replay, RELA_ESTATE, "rela_apex_actor_post_step: evaluation actor has no replay");  // :175,182
  RELA_CHECK(a->cur >= 0, RELA_ESTATE, "rela_apex_actor_post_step: no act() to attach the reward to");  // :33
  hipStream_t s = (hipStream_t)stream_;
  DeviceGuard g(a->device);
  if (inserted) *inserted = 0;
  if (on_device) {  // one launch (common.h: dev_copy2), not two of the runtime's blit kernels
    RELA_HIP(dev_copy2(a->rew + (size_t)a->cur * a->R, reward, (size_t)a->R * sizeof(float), a->term + (size_t)a->cur * a->R, terminal,
                       (size_t)a->R, s));
  } else {
    RELA_HIP(hipMemcpyAsync(a->rew + (size_t)a->cur * a->R, reward, (size_t)a->R * sizeof(float), hipMemcpyHostToDevice, s));
    RELA_HIP(hipMemcpyAsync(a->term + (size_t)a->cur * a->R, terminal, (size_t)a->R, hipMemcpyHostToDevice, s));
  }
  const int H = a->n + 1;
  if (a->dd_ups > 0) {  // the stack acted on this tick enters the unit ring once
    DedupStored st;
    const int rc = shard_dedup_store(a, nonblocking, s, &st);
    if (rc != RELA_OK) return rc;
    if (st.stored) {
      if (st.keyframe || a->dd_ups == 1) a->key_tick = st.tick;
      a->tick_seq[(size_t)(st.tick % kTickWin)] = st.seq;
    }
  }
  a->cur = -1;
  a->count += 1;
  if (a->count < a->n + 1) return RELA_OK;  // canPop :46-48
  const int first = a->head, last = (a->head + a->n) % H;
  int rc = rela_nstep_return(a->n, a->R, a->gamma, first, a->rew, a->term, a->out_r, a->out_b, a->out_t, s);
  if (rc != RELA_OK) return rc;
  // de-duplication: both stacks of the transition must be in the unit ring; the oldest unit it refers to is
  // the first plane of obs_t, stored at most 3 ticks before tick t = (tick - 1) - n (never before a keyframe)
  bool dd_drop = false;
  int64_t dd_min_seq = 0;
  if (a->dd_ups > 0) {
    dd_drop = !(a->refs_valid[first] && a->refs_valid[last]);
    int64_t t_first = a->tick - 1 - a->n;
    int64_t oldest = a->dd_ups == 4 ? t_first - 3 : t_first;
    if (oldest < 0) oldest = 0;
    // a keyframe at or before t_first bounds the chain; a later one cannot happen while refs stay valid
    if (a->key_tick >= 0 && a->key_tick <= t_first && oldest < a->key_tick) oldest = a->key_tick;
    if (a->tick - oldest >= kTickWin) oldest = a->tick - kTickWin + 1;
    dd_min_seq = a->tick_seq[(size_t)(oldest % kTickWin)];
  }
  const uint8_t* obs_t = a->obs + (size_t)first * a->R * kObs;
  const uint8_t* obs_n = a->obs + (size_t)last * a->R * kObs;
  const size_t QA = (size_t)a->R * a->A;
  const float* legal_t = a->legal_hist + (size_t)first * a->R * a->A;
  const float* legal_n = a->legal_hist + (size_t)last * a->R * a->A;
  const float* eps_t = a->eps_hist + (size_t)first * a->R;
  const float* eps_n = a->eps_hist + (size_t)last * a->R;
  // Both online forwards of compute_priority evaluate observations act() already ran the online net on:
  // obs is history.front(), acted on n ticks ago, and next_obs is history.back(), acted on this tick
  // (dqn_actor.h:84,161).  With the same weights (no load since: rela_ffnet_version), the same legal mask and the
  // same batch such a forward is bit-identical to the table act() left in q_hist[slot]: reuse it.
  const uint64_t ver = rela_ffnet_version(online);
  auto cached = [&](int slot) { return a->qh_net[slot] == online && a->qh_version[slot] == ver; };
  const float* q_online_t = a->q_hist + (size_t)first * QA;
  if (!(a->reuse_mode == 1 && cached(first))) {
    rc = rela_ffnet_forward(online, a->R, obs_t, legal_t, a->q + QA, a->ws, a->ws_bytes, s);  // apex.py:38
    if (rc != RELA_OK) return rc;
    q_online_t = a->q + QA;
  }
  const float* q_online_n = a->q_hist + (size_t)last * QA;  // greedy_act(next_obs) :41
  if (!(a->reuse_mode != 0 && cached(last) && a->q_slot == last)) {
    rc = rela_ffnet_forward(online, a->R, obs_n, legal_n, a->q + 2 * QA, a->ws, a->ws_bytes, s);
    if (rc != RELA_OK) return rc;
    q_online_n = a->q + 2 * QA;
  }
  // One reference block per group of K rows (each batched actor thread's own add, :189).  The whole shard
  // is reserved at once when that can always be satisfied; a blocking append of more than ring - capacity
  // rows never can (sample() evicts down to capacity only), so a shard that large goes in pieces of whole
  // K-groups -- which is exactly what the reference's separate actor threads would issue.
  int cap = 0, ring = 0;
  rc = rela_replay_limits(a->replay, &cap, &ring);
  if (rc != RELA_OK) return rc;
  const int fit = ((ring - cap) / a->K) * a->K;
  const int piece = a->R <= ring - cap ? a->R : (fit > a->K ? fit : a->K);
  // Fused insert: the target forward reads every byte of obs_n, the very rows the insert copies into the replay's
  // next_obs field.  Where its trunk is conv12_s3 (f32x3, 512 rows and up) and the shard goes in as ONE block of plain
  // rows, the block is reserved here already and the forward stores the frames into its rows from the registers it stages
  // them in (conv12_s3_copy): one replay_scatter_rows launch and one read of R frames less per tick.  The rows are
  // written on `s`, behind the waits rela_replay_direct_rows puts there and ahead of the event commit_add records on `s`.
  // fused_insert == 2: the same launch passes obs_t through to the block's obs rows as well (conv12_s3_copy2; obs_t takes
  // no part in that forward's arithmetic): the insert then launches no replay_scatter_rows at all.  obs_t is the history
  // slot the NEXT act() overwrites; the forward reads it on `s` ahead of everything the next tick queues there.
  // Anything else -- de-duplicated stacks, a shard in pieces, another trunk, a reservation that would block -- takes the
  // path below unchanged; a field the forward reports it did not store is copied by write_rows.
  int fused_slot = -1, fused_copied = 0;
  if (a->fused_insert && a->dd_ups == 0 && piece == a->R && ffnet_forward_stores_frames(target, a->R)) {
    rc = rela_replay_begin_add(a->replay, a->R, nonblocking, &fused_slot);
    if (rc == RELA_EWOULDBLOCK) fused_slot = -1;
    else if (rc != RELA_OK) return rc;
  }
  if (fused_slot >= 0) {
    void* base = nullptr;
    int rows_ring = 0;
    int64_t row_bytes = 0;
    rc = rela_replay_direct_rows(a->replay, fused_slot, a->R, 1, &base, &rows_ring, &row_bytes, s);
    if (rc == RELA_OK && row_bytes != kObs) {
      set_last_error("rela_apex_actor_post_step: the replay's next_obs rows have %lld bytes, a frame stack %lld",
                     (long long)row_bytes, (long long)kObs);
      rc = RELA_EINVAL;
    }
    FrameRows fr{static_cast<uint8_t*>(base), fused_slot, rows_ring};
    if (rc == RELA_OK && a->fused_insert == 2) {
      void* base0 = nullptr;
      int ring0 = 0;
      rc = rela_replay_direct_rows(a->replay, fused_slot, a->R, 0, &base0, &ring0, &row_bytes, s);
      if (rc == RELA_OK && (row_bytes != kObs || ring0 != rows_ring)) {
        set_last_error("rela_apex_actor_post_step: the replay's obs rows have %lld bytes in a ring of %d, a frame stack %lld in %d",
                       (long long)row_bytes, ring0, (long long)kObs, rows_ring);
        rc = RELA_EINVAL;
      }
      fr.src2 = obs_t;
      fr.base2 = static_cast<uint8_t*>(base0);
      fr.first2 = fused_slot;
    }
    if (rc == RELA_OK)
      rc = ffnet_forward_store_frames(target, a->R, obs_n, legal_n, a->q + 3 * QA, a->ws, a->ws_bytes, s, fr, &fused_copied);  // :42
  } else {
    rc = rela_ffnet_forward(target, a->R, obs_n, legal_n, a->q + 3 * QA, a->ws, a->ws_bytes, s);  // :42
  }
  const int64_t* act_t = a->act + (size_t)first * a->R;
  if (rc == RELA_OK)
    rc = td_from_q(a->R, a->A, a->K, q_online_t, q_online_n, a->q + 3 * QA, legal_n, act_t, a->out_r, a->out_b, a->gamma_n,
                   a->vr_eps, nullptr, a->prio, s);
  if (rc != RELA_OK) {
    if (fused_slot >= 0) (void)rela_replay_abort_add(a->replay, fused_slot, a->R);
    return rc;
  }
  // FFTransition rows (types.h:18-51): obs{s,eps,legal_move}, next_obs{...}, action{a}, reward, terminal, bootstrap
  const void* rows[10] = {obs_t, obs_n, eps_t, eps_n, legal_t, legal_n, act_t, a->out_r, a->out_t, a->out_b};
  if (a->dd_ups > 0) {
    rows[0] = a->ref_hist + (size_t)first * a->R * a->dd_ups;
    rows[1] = a->ref_hist + (size_t)last * a->R * a->dd_ups;
  }
  // (the blocks: `piece` rows each, above; a fused insert's one block is reserved already and has its next_obs rows)
  const int64_t stack_rb = a->dd_ups > 0 ? (int64_t)sizeof(int32_t) * a->dd_ups : kObs;
  const int64_t rb[10] = {stack_rb, stack_rb, 4, 4, 4 * a->A, 4 * a->A, 8, 4, 1, 4};
  int dropped = dd_drop ? 1 : 0;
  for (int off = 0; off < a->R && !dd_drop; off += piece) {
    const int cnt = a->R - off < piece ? a->R - off : piece;
    const void* prow[10];
    for (int f = 0; f < 10; ++f) prow[f] = static_cast<const uint8_t*>(rows[f]) + (int64_t)off * rb[f];
    int slot = fused_slot;
    if (fused_slot >= 0) {  // (piece == R: this is the only block)
      if (fused_copied >= 1) prow[1] = nullptr;
      if (fused_copied >= 2) prow[0] = nullptr;
    } else {
      rc = rela_replay_begin_add(a->replay, cnt, nonblocking, &slot);
      if (rc == RELA_EWOULDBLOCK) {
        dropped = 1;
        continue;
      }
      if (rc != RELA_OK) break;
    }
    if (a->dd_ups > 0) (void)rela_replay_set_block_min_unit(a->replay, slot, cnt, dd_min_seq);
    rc = rela_replay_write_rows(a->replay, slot, 0, cnt, prow, s);
    if (rc == RELA_OK) rc = rela_replay_commit_add_grouped(a->replay, slot, cnt, a->K, a->prio + off, s);
    if (rc != RELA_OK) {  // release the reservation so later blocks of other producers can still commit
      (void)rela_replay_abort_add(a->replay, slot, cnt);
      break;
    }
  }
  a->head = (a->head + 1) % H;  // pop_front :101-104
  a->count -= 1;
  if (rc == RELA_OK && dropped) rc = RELA_EWOULDBLOCK;
  if (rc == RELA_OK && inserted) *inserted = 1;
  return rc;
}
