"""Deterministic end-to-end drive of the `rela` surface, shared by the golden generator (real
reference, CPU TorchScript actor) and the GPU test (this repo's module).

One actor thread with K synthetic envs (eps = 0) fills a tiny replay until back-pressure parks
it (ring full, prioritized_replay.h:47); the main thread then samples, lets the parked block
land, and only then updates priorities -- so every replay mutation is totally ordered and the
run is reproducible.  Each round records the sampled batch.
"""
import time

import numpy as np
import torch

CFG = dict(K=4, multi_step=3, gamma=0.997, capacity=16, alpha=1.0, beta=1.0, seed=5, episode_len=7,
           num_action=18, rounds=6, batch=8, online_seed=1001, target_seed=2002, env_seed=900)


def _wait(cond, what, timeout=120.0):
    t0 = time.time()
    while not cond():
        if time.time() - t0 > timeout:
            raise TimeoutError(what)
        time.sleep(0.002)


# the same run with an Atari-like env: ONE new plane per step, sliding stack, first frame of an episode repeated
# four times (atari/game_state.h:53-82) -- the stream a plane-level de-duplicating replay is valid for
CFG_SLIDING = dict(CFG, sliding=True, env_seed=950, rounds=8)


# r4: ONE actor thread with K = 128 envs -- the smallest shard whose forwards reach the split-bf16 kernels (from 128 rows
# up, csrc/ffnet_plan.h kFastTrunkMinN) -- at the headline's replay exponents (alpha 0.6 / beta 0.4, pyrela/main.py:60-65).
# Ring 640 = five blocks of 128.  The golden also records the smallest gap between the two best legal Q-values over
# every frame the run can see (tests/golden/make_golden.py e2e_big), so "greedy actions equal" is a checked expectation.
# The synthetic frames are noise, so the online net's two best actions (14 and 9 with these parameters) differ by
# 0.006 +- 0.0045 and ~2.5 decisions per thousand are closer than the fast mode's tolerance; a flipped greedy action
# changes the env's reward stream and the double-DQN bootstrap, i.e. everything after it.  `online_fc_a_bias_add` lifts
# action 14's advantage bias by the offset that MAXIMISES the smallest gap over the run's frames while keeping real
# variety (37 of 3,072 decisions pick action 9): smallest gap 1.39e-4 = 8 x the stated |dQ| bound at max|Q| = 0.85.
CFG_BIG = dict(K=128, multi_step=3, gamma=0.997, capacity=512, alpha=0.6, beta=0.4, seed=21, episode_len=9,
               num_action=18, rounds=5, batch=16, online_seed=1001, target_seed=2002, env_seed=4000,
               online_fc_a_bias_add=[14, 0.00427])


# the same 128 envs as a COHORT of this repo's module: 2 threads x 64 envs (one 128-row device shard, q.min() and replay
# blocks per group of 64)
CFG_COHORT = dict(CFG_BIG, K=64, threads=2)
# four threads x 128 envs: ONE 512-row shard -- the batch size from which the f32x3 mode's conv kernels run
CFG_COHORT_512 = dict(CFG_BIG, K=128, threads=4, capacity=2048, batch=64, rounds=4)


# r5: ONE actor thread with K = 512 envs -- a 512-row shard, the batch size from which EVERY layer of the f32x3 mode (the
# headline arithmetic of bench.py) runs its three-part bf16 kernels -- recorded from the REAL reference (one TorchScript
# call per 512 envs on the CPU).  Ring 2,560 = five blocks of 512.  `online_fc_a_bias_add` is the offset that maximises
# the smallest top-two gap over the run's frames (tests/golden/make_golden.py e2e_k512_scan).
CFG_K512 = dict(K=512, multi_step=3, gamma=0.997, capacity=2048, alpha=0.6, beta=0.4, seed=23, episode_len=9,
                num_action=18, rounds=4, batch=64, online_seed=1001, target_seed=2002, env_seed=6000,
                online_fc_a_bias_add=[14, 0.00554])


def frames_of_run(synth_atari, cfg, steps):
    """The observation every env of the run emits at each of its first `steps` calls (reset or step), as the thread
    loop drives it (rela/thread_loop.h:74-105: all envs share the episode length, so they reset together).  The
    synthetic env's frames and its LCG do not depend on the actions.  -> u8 [steps, K, 4, 84, 84]"""
    out = np.zeros((steps, cfg["K"], 4, 84, 84), np.uint8)
    act = {"a": torch.zeros(1, dtype=torch.int64)}
    for g in range(cfg["K"]):
        env = synth_atari.SyntheticAtariEnv(cfg["env_seed"] + g, 0.0, cfg["num_action"], cfg["episode_len"])
        t = 0
        while t < steps:
            out[t, g] = env.reset()["s"].numpy()
            t += 1
            while not env.terminated() and t < steps:
                out[t, g] = env.step(act)[0]["s"].numpy()
                t += 1
    return out


# the reference's multi-device wiring on one GPU: 2 lockers x 1 thread x 4 envs, capacity 32 = 2 partitions of 16 with
# seeds 5 and 6, batch 16 = 8 + 8.  Partition 0 sees exactly the stream of the single-replay golden (CFG).
CFG_TWO_LOCKERS = dict(CFG, threads=2, lockers=2, capacity=32, batch=16)

# the sliding-stack golden's four envs as a cohort of this repo's module (2 threads x 2 envs): the path on which only
# the newest plane of every row crosses PCIe and the device completes the stacks (rela_apex_actor_slide_stacks)
CFG_SLIDING_COHORT = dict(CFG_SLIDING, K=2, threads=2)


def run_lockstep(rela, synth_atari, agent, act_device, sample_device, cfg=CFG, prefetch=0):
    """agent: an ApexAgent-shaped module whose state_dict carries online_net.* / target_net.*."""
    ring = int(1.25 * cfg["capacity"])
    replay = rela.FFPrioritizedReplay(cfg["capacity"], cfg["seed"], cfg["alpha"], cfg["beta"], prefetch)
    # cfg["lockers"] = L > 1 (this repo's module only): the reference's multi-device wiring, one ModelLocker per act
    # device and thread t on locker t % L (pyrela/main.py:131-136,155,166) -- here all on `act_device`, so the replay
    # owns L partitions of capacity / L on one GPU; the batch is L slices of batch / L rows, partition 0 first
    L = cfg.get("lockers", 1)
    lockers = [rela.ModelLocker([agent], act_device) for _ in range(L)]
    ctx = rela.Context()
    games, actors = [], []
    # cfg["threads"] > 1 (this repo's module only: its cohort commits the members' blocks in member order, the
    # reference's threads would race for the slots): T threads x K envs, env seeds numbered through
    for t in range(cfg.get("threads", 1)):
        actor = rela.DQNActor(lockers[t % L], cfg["multi_step"], cfg["K"], cfg["gamma"], replay)
        vec = rela.VectorEnv()
        for g in range(cfg["K"]):
            seed = cfg["env_seed"] + t * cfg["K"] + g
            if cfg.get("sliding"):
                game = synth_atari.SyntheticAtariEnv(seed, 0.0, cfg["num_action"], cfg["episode_len"], True)
            else:
                game = synth_atari.SyntheticAtariEnv(seed, 0.0, cfg["num_action"], cfg["episode_len"])
            games.append(game)
            vec.append(game)
        actors.append(actor)
        ctx.push_env_thread(rela.BasicThreadLoop(actor, vec, False))
    ctx.start()
    rounds = []
    for r in range(cfg["rounds"]):
        _wait(lambda: replay.size() == ring, "actor never filled the ring")
        batch, w = replay.sample(cfg["batch"], sample_device)
        _wait(lambda: replay.size() == ring, "parked block never landed")  # append happens-before update
        s = batch.obs["s"].cpu().numpy().astype(np.int64)
        ns = batch.next_obs["s"].cpu().numpy().astype(np.int64)
        rounds.append(dict(
            s_sum=s.reshape(len(s), -1).sum(1).tolist(), s_head=s.reshape(len(s), -1)[:, :4].tolist(),
            next_s_sum=ns.reshape(len(ns), -1).sum(1).tolist(),
            s_planes=s.reshape(len(s), 4, -1).sum(2).tolist(), next_s_planes=ns.reshape(len(ns), 4, -1).sum(2).tolist(),
            a=batch.action["a"].cpu().tolist(), reward=batch.reward.cpu().tolist(),
            terminal=[int(x) for x in batch.terminal.cpu().tolist()], bootstrap=batch.bootstrap.cpu().tolist(),
            eps=batch.obs["eps"].cpu().reshape(-1).tolist(),
            legal_sum=batch.obs["legal_move"].cpu().sum(1).tolist(),
            weight=w.cpu().double().tolist(), num_add=replay.num_add()))
        newp = torch.linspace(0.5, 2.0, cfg["batch"] // L).repeat(L) * (1 + 0.25 * r)
        replay.update_priority(newp)
    ctx.terminate()
    ctx.resume()
    t0 = time.time()
    while not ctx.terminated():  # the actor may be parked on the full ring: drain until it exits
        if replay.size() >= cfg["batch"]:
            batch, w = replay.sample(cfg["batch"], sample_device)
            replay.update_priority(torch.ones(cfg["batch"]))
        time.sleep(0.005)
        if time.time() - t0 > 120:
            raise TimeoutError("context did not terminate")
    return rounds


def load_agent_params(agent, cfg=CFG):
    from synth import synth_params

    sd = {}
    for prefix, seed in (("online_net.", cfg["online_seed"]), ("target_net.", cfg["target_seed"])):
        for k, v in synth_params(cfg["num_action"], seed).items():
            sd[prefix + k] = torch.from_numpy(v)
    if cfg.get("online_fc_a_bias_add"):
        a, delta = cfg["online_fc_a_bias_add"]
        sd["online_net.fc_a.bias"] = sd["online_net.fc_a.bias"].clone()
        sd["online_net.fc_a.bias"][int(a)] += float(delta)
    agent.load_state_dict(sd)
    return agent


# ---------------------------------------------------------------------------------------------
# R2D2: same lock-step idea with sequences.  Blocks are 1..2K sequences, so "ring full" is not an
# exact size; the actor is considered parked when size() has not moved for a while.
# ---------------------------------------------------------------------------------------------
CFG_R2D2 = dict(K=2, multi_step=3, gamma=0.997, seq_len=6, burn_in=2, eta=0.9, capacity=16, alpha=1.0, beta=1.0,
                seed=11, episode_len=14, num_action=6, rounds=5, batch=4, online_seed=3003, target_seed=4004,
                env_seed=700)


def _wait_parked(replay, min_size, quiet=1.0, timeout=180.0):
    t0 = time.time()
    last, since = -1, time.time()
    while True:
        cur = replay.num_add()
        if cur != last:
            last, since = cur, time.time()
        elif replay.size() >= min_size and time.time() - since > quiet:
            return
        if time.time() - t0 > timeout:
            raise TimeoutError("actor never parked (size %d)" % replay.size())
        time.sleep(0.01)


# BASELINE config C4's sequence shape (pyrela/scripts/ref_run_r2d2.sh:12-18: seq 80 / burn-in 40 / n 3, window of
# 123 slots = 3.47 MB of frames per sequence).  The four envs cover: an episode shorter than the window
# (50 steps), a terminal inside the carried region (step 120 lands in slot 80 of the second window,
# r2d2_actor.h:119-142 -> a second, short sequence), several carries in a row (260) and a window that
# never sees a terminal (1000).  `quiet` = seconds without an add before the actor counts as parked
# (the reference's CPU actor needs ~2 s for the 80 steps between two pops).
CFG_R2D2_C4 = dict(K=4, multi_step=3, gamma=0.997, seq_len=80, burn_in=40, eta=0.9, capacity=16, alpha=1.0, beta=1.0,
                   seed=13, episode_len=0, episode_lens=[50, 121, 260, 1000], num_action=6, rounds=4, batch=4,
                   online_seed=3003, target_seed=4004, env_seed=760)


# two lockers x 1 thread x 2 envs on one GPU, as CFG_TWO_LOCKERS: 2 partitions of 16 with seeds 11 and 12, batch 8 = 4 + 4.
# Partition 0 sees exactly the stream of the single-replay golden (CFG_R2D2).
CFG_R2D2_TWO_LOCKERS = dict(CFG_R2D2, threads=2, lockers=2, capacity=2 * CFG_R2D2["capacity"], batch=2 * CFG_R2D2["batch"])


def run_lockstep_r2d2(rela, synth_atari, agent, act_device, sample_device, cfg=CFG_R2D2, quiet=1.0, prefetch=0):
    replay = rela.RNNPrioritizedReplay(cfg["capacity"], cfg["seed"], cfg["alpha"], cfg["beta"], prefetch)
    # cfg["lockers"] / cfg["threads"] (this repo's module only) as in run_lockstep: thread t on locker t % L, env seeds
    # numbered through; every thread has thread 0's episode lengths, so the partitions fill and park in step
    L = cfg.get("lockers", 1)
    lockers = [rela.ModelLocker([agent], act_device) for _ in range(L)]
    ctx = rela.Context()
    games, actors = [], []
    for t in range(cfg.get("threads", 1)):
        actor = rela.R2D2Actor(lockers[t % L], cfg["multi_step"], cfg["K"], cfg["gamma"], cfg["seq_len"], cfg["burn_in"],
                               replay)
        vec = rela.VectorEnv()
        for g in range(cfg["K"]):
            ep_len = cfg["episode_lens"][g] if cfg.get("episode_lens") else cfg["episode_len"]
            game = synth_atari.SyntheticAtariEnv(cfg["env_seed"] + t * cfg["K"] + g, 0.0, cfg["num_action"], ep_len)
            games.append(game)
            vec.append(game)
        actors.append(actor)
        ctx.push_env_thread(rela.BasicThreadLoop(actor, vec, False))
    ctx.start()
    rounds = []
    for r in range(cfg["rounds"]):
        _wait_parked(replay, cfg["batch"], quiet=quiet, timeout=180.0 + 40 * quiet)
        batch, w = replay.sample(cfg["batch"], sample_device)
        _wait_parked(replay, cfg["batch"], quiet=quiet, timeout=180.0 + 40 * quiet)  # the parked block lands first
        s = batch.obs["s"].cpu().numpy().astype(np.int64)  # [T,B,4,84,84]
        T, B = s.shape[:2]
        rounds.append(dict(
            s_sum=s.reshape(T, B, -1).sum(2).T.tolist(),
            a=batch.action["a"].cpu().T.tolist(), reward=batch.reward.cpu().T.tolist(),
            terminal=batch.terminal.cpu().long().T.tolist(), bootstrap=batch.bootstrap.cpu().T.tolist(),
            eps_sum=batch.obs["eps"].cpu().sum().item(), legal_sum=batch.obs["legal_move"].cpu().sum(2).T.tolist(),
            seq_len=batch.seq_len.cpu().tolist(),
            h0_abs=batch.h0["h0"].cpu().abs().sum(2).reshape(-1).double().tolist(),
            c0_abs=batch.h0["c0"].cpu().abs().sum(2).reshape(-1).double().tolist(),
            weight=w.cpu().double().tolist(), num_add=replay.num_add(), size=replay.size(),
            shapes=dict(s=list(s.shape), eps=list(batch.obs["eps"].shape), legal_move=list(batch.obs["legal_move"].shape),
                        a=list(batch.action["a"].shape), reward=list(batch.reward.shape),
                        terminal=list(batch.terminal.shape), bootstrap=list(batch.bootstrap.shape),
                        h0=list(batch.h0["h0"].shape), c0=list(batch.h0["c0"].shape), seq_len=list(batch.seq_len.shape),
                        weight=list(w.shape))))
        replay.update_priority(torch.linspace(0.5, 2.0, cfg["batch"] // L).repeat(L) * (1 + 0.25 * r))
    ctx.terminate()
    ctx.resume()
    t0 = time.time()
    while not ctx.terminated():
        if replay.size() >= cfg["batch"]:
            batch, w = replay.sample(cfg["batch"], sample_device)
            replay.update_priority(torch.ones(cfg["batch"]))
        time.sleep(0.005)
        if time.time() - t0 > 180:
            raise TimeoutError("context did not terminate")
    return rounds


def load_lstm_agent_params(agent, cfg=CFG_R2D2):
    from synth import synth_lstm_params

    sd = {}
    for prefix, seed in (("online_net.", cfg["online_seed"]), ("target_net.", cfg["target_seed"])):
        for k, v in synth_lstm_params(cfg["num_action"], seed).items():
            sd[prefix + k] = torch.from_numpy(v)
    agent.load_state_dict(sd)
    return agent
