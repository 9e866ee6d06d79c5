"""The device-resident Catch env (rela_amd/device_env.py over csrc/catch_env.hip) against the pure-Python restatement of
the game (tests/catch_ref.py), wired into the Ape-X and R2D2 actor shards, the de-duplicating replay, the greedy
evaluation and the engine training loop.  Nets are f32 and come from synth.synth_params."""
import numpy as np
import pytest

from catch_ref import CatchRefVec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ffnets(A):
    import torch

    from rela_amd.engine import FFNetHandle
    from synth import synth_params

    on, tg = FFNetHandle(A, DEV), FFNetHandle(A, DEV)
    on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 11).items()})
    tg.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 12).items()})
    return on, tg


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the env against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("A", [3, 18])
@pytest.mark.parametrize("rows", [1, 5, 130])  # one row; fewer rows than a wave; more than 128 and no multiple of 64
def test_device_env_equals_the_reference_every_tick(rows, A):
    """100 ticks at episode_len = 45 (episodes end mid-fall).  Even ticks take the fused launch, odd ticks the step and
    the frame as two launches: both must give the reference's stacks, rewards, terminals and state."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.device_env import DeviceCatchEnv

    seed = 2 ** 32 - 3  # row seeds cross 2^32
    env = DeviceCatchEnv(rows, A, 45, seed, DEV)
    ref = CatchRefVec(rows, A, 45, seed)
    slot = torch.full((rows + 1, 4, 84, 84), 7, dtype=torch.uint8, device=DEV)  # one guard row behind the env's
    rng = np.random.default_rng(rows * 31 + A)
    with capi.launch_census() as census:
        env.reset(slot[:rows])
        assert np.array_equal(slot[:rows].cpu().numpy(), ref.reset())
        assert np.array_equal(env.state(), ref.state())
        for t in range(100):
            actions = rng.integers(0, A, rows)
            if t % 2 == 0:
                reward, terminal = env.step(_cuda(actions), slot[:rows])
            else:
                slot[:rows].fill_(9)
                reward, terminal = env.step(_cuda(actions))
                env.render(slot[:rows])
            r_reward, r_terminal = ref.step(actions)
            assert reward.dtype == torch.float32 and terminal.dtype == torch.uint8
            assert np.array_equal(reward.cpu().numpy(), r_reward), t
            assert np.array_equal(terminal.cpu().numpy(), r_terminal), t
            assert np.array_equal(slot[:rows].cpu().numpy(), ref.obs()), t
            assert np.array_equal(env.state(), ref.state()), t
    assert census.counts.get("catch_step_render") == 50 and census.counts.get("catch_step") == 50
    assert census.counts.get("catch_render") == 50 and census.counts.get("catch_reset_render") == 1
    assert bool((slot[rows] == 7).all())  # nothing was written behind the last row
    stats = env.episode_stats()
    assert np.array_equal(env.stats_dev().cpu().numpy(), ref.stats())
    assert stats["episodes"] == 2 * rows and stats["return_sum"] == int(ref.stats()[1].sum())
    assert np.array_equal(stats["rows"]["last_len"].cpu().numpy(), np.full(rows, 45))
    env.close()


def test_create_refuses_bad_shapes():
    import ctypes as C

    from rela_amd import _capi as capi

    h = C.c_void_p()
    for rows, A, length in ((0, 18, 10), (4, 2, 10), (4, 18, 0)):
        assert capi.lib.rela_catch_create(C.byref(h), rows, A, length, 1, 0) == capi.EINVAL
    assert b"rela_catch_create" in capi.lib.rela_last_error()


# ---- 2. seeding: row r is the host env seeded seed + r -------------------------------------------------------------
def test_rows_are_the_host_envs_of_consecutive_seeds():
    import torch

    from rela_amd.device_env import DeviceCatchEnv
    from rela_amd.pyrela import create_env

    rows, A, length, seed = 8, 18, 25, 4242
    env = DeviceCatchEnv(rows, A, length, seed, DEV)
    hosts = [create_env.synth_atari.CatchEnv(seed + r, 0.0, A, length) for r in range(rows)]
    slot = torch.zeros((rows, 4, 84, 84), dtype=torch.uint8, device=DEV)
    env.reset(slot)
    obs = np.stack([h.reset()["s"].numpy() for h in hosts])
    assert np.array_equal(slot.cpu().numpy(), obs)
    rng = np.random.default_rng(8)
    for t in range(60):
        actions = rng.integers(0, A, rows)
        reward, terminal = env.step(_cuda(actions), slot)
        for r, h in enumerate(hosts):
            o, rew, term = h.step({"a": torch.tensor([actions[r]], dtype=torch.int64)})
            assert (float(reward[r]), int(terminal[r])) == (rew, int(term)), (t, r)
            if term:  # VectorEnv::reset
                o = h.reset()
            obs[r] = o["s"].numpy()
        assert np.array_equal(slot.cpu().numpy(), obs), t
        host_state = np.stack([h.state().numpy() for h in hosts])
        assert np.array_equal(env.state()[:, :7], host_state[:, :7]), t
    env.close()


# ---- 3. bad actions ---------------------------------------------------------------------------------------------------
def test_bad_actions_move_nothing_and_are_counted():
    import torch

    from rela_amd.device_env import DeviceCatchEnv

    rows, A = 6, 18
    env = DeviceCatchEnv(rows, A, 45, 5, DEV)
    ref = CatchRefVec(rows, A, 45, 5)
    slot = torch.zeros((rows, 4, 84, 84), dtype=torch.uint8, device=DEV)
    env.reset(slot)
    ref.reset()
    for actions in ([2, 0, 1, 2, 0, 1], [0, -1, 2, 1, A, 0], [1, 1, 1, 1, 1, 1]):
        before, obs_before = env.state(), slot.cpu().numpy().copy()
        reward, terminal = env.step(_cuda(np.array(actions, np.int64)), slot)  # returns normally
        r_reward, r_terminal = ref.step(actions)
        after = env.state()
        assert np.array_equal(after, ref.state()) and np.array_equal(slot.cpu().numpy(), ref.obs())
        assert np.array_equal(reward.cpu().numpy(), r_reward) and np.array_equal(terminal.cpu().numpy(), r_terminal)
        for r, a in enumerate(actions):
            if a < 0 or a >= A:
                assert np.array_equal(after[r, :7], before[r, :7]) and after[r, 7] == before[r, 7] + 1 == 1
                assert np.array_equal(slot[r].cpu().numpy(), obs_before[r]) and float(reward[r]) == 0 and int(terminal[r]) == 0
            else:
                assert after[r, 5] == before[r, 5] + 1 and after[r, 7] == before[r, 7]
    assert env.state()[:, 7].tolist() == [0, 1, 0, 0, 1, 0]
    env.close()


# ---- 4. Ape-X wiring ----------------------------------------------------------------------------------------------------
def _apex_run(device_fed, dedup, ticks, batch, sample_every=2, cap=256, length=11):
    """R = 16, K = 8, n = 3, A = 18, episode_len = `length`.  device_fed: DeviceCatchEnv steps on the device, post_step takes its
    device rewards, the frame goes into the slot post_step released; else: the reference's frames are copied into the slot
    and its rewards uploaded.  The ring has 320 slots and a sample evicts down to the capacity of 256, so a batch is
    sampled every second tick (two ticks add 32 rows); the adds are non-blocking, so a full ring would show as a block
    that was not inserted instead of a wait.  -> per tick (actions, priorities), the sampled batches"""
    import torch

    from rela_amd.device_env import DeviceCatchEnv
    from rela_amd.engine import ApexActorEngine
    from rela_amd.replay import FFReplay

    R, K, n, A, seed = 16, 8, 3, 18, 900
    on, tg = _ffnets(A)
    replay = FFReplay(cap, 7, 0.6, 0.4, 0, A, DEV, dedup=dedup, guard_units=(n + 8) * R)
    eps = np.linspace(0.0, 0.6, R).tolist()
    eng = ApexActorEngine(R, K, A, n, 0.997, replay, eps, DEV)
    if device_fed:
        env = DeviceCatchEnv(R, A, length, seed, DEV)
        env.reset(eng.next_obs_slot())
    else:
        ref = CatchRefVec(R, A, length, seed)
        eng.next_obs_slot().copy_(_cuda(ref.reset()))
    per_tick, batches = [], []
    for t in range(ticks):
        action = eng.act(on)
        if device_fed:
            reward, terminal = env.step(action)
            inserted = eng.post_step(reward, terminal, on, tg, nonblocking=True)
            env.render(eng.next_obs_slot())
        else:
            reward, terminal = ref.step(action.cpu().numpy())
            inserted = eng.post_step(_cuda(reward), _cuda(terminal), on, tg, nonblocking=True)
            eng.next_obs_slot().copy_(_cuda(ref.obs()))
        assert inserted == (t >= n), t
        per_tick.append((action.cpu().numpy().copy(), eng.prio.cpu().numpy().copy()))
        if t % sample_every == sample_every - 1 and replay.size() >= batch:
            b, w = replay.sample(batch)
            st = replay.debug_state()
            assert st["dev_error"] == 0
            batches.append(dict(s=b.obs["s"].cpu().numpy().copy(), ns=b.next_obs["s"].cpu().numpy().copy(),
                                a=b.action["a"].cpu().numpy().copy(), r=b.reward.cpu().numpy().copy(),
                                t=b.terminal.cpu().numpy().copy(), boot=b.bootstrap.cpu().numpy().copy(),
                                eps=b.obs["eps"].cpu().numpy().copy(), w=w.cpu().numpy().copy(), sum=st["sum"],
                                head=st["head"], size=st["size"], num_add=st["num_add"]))
            replay.update_priority(torch.linspace(0.3, 1.7, batch, device=DEV))
    if device_fed:
        env.close()
    eng.close()
    replay.close()
    return per_tick, batches


def _same_batches(a, b, what):
    assert len(a) == len(b) >= 1
    for i, (x, y) in enumerate(zip(a, b)):
        for key in ("a", "r", "t", "boot", "eps", "w", "s", "ns"):
            assert np.array_equal(x[key], y[key]), (what, i, key)
        assert (x["sum"], x["head"], x["size"], x["num_add"]) == (y["sum"], y["head"], y["size"], y["num_add"]), (what, i)


@pytest.mark.parametrize("length", [11, 25])  # 11: episodes end before a ball lands (every reward is 0); 25: balls land
def test_apex_shard_fed_by_the_device_env_equals_the_host_fed_shard(length):
    dev_ticks, dev_batches = _apex_run(True, None, 30, batch=8, length=length)
    ref_ticks, ref_batches = _apex_run(False, None, 30, batch=8, length=length)
    for t, ((a, p), (ra, rp)) in enumerate(zip(dev_ticks, ref_ticks)):
        assert np.array_equal(a, ra), t
        assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)), t  # bit-equal priorities
    _same_batches(dev_batches, ref_batches, "apex")
    assert dev_batches[-1]["num_add"] == (30 - 3) * 16 and len(dev_batches) >= 12


# ---- 5. dedup = "plane" fed by the device env -----------------------------------------------------------------------------
def test_plane_dedup_fed_by_the_device_env_equals_full_storage():
    """the parity definition of tests/test_dedup_gpu.py: every sampled batch (frames, small fields, importance weights,
    f64 running sum, head, size, adds) is identical to that of a replay storing s and next_s in full; 592 adds into a
    ring of 320 slots, so the slot ring wraps"""
    _, full = _apex_run(True, None, 40, batch=16)
    _, plane = _apex_run(True, "plane", 40, batch=16)
    assert len(full) >= 15
    _same_batches(full, plane, "plane")
    assert full[-1]["head"] != full[0]["head"]  # eviction happened


# ---- 6. R2D2 wiring through step_host -------------------------------------------------------------------------------------
def _r2d2_run(device_fed, ticks):
    import torch

    from rela_amd.device_env import DeviceCatchEnv
    from rela_amd.engine import LSTMNetHandle, R2D2ActorEngine
    from rela_amd.replay import RNNReplay
    from synth import synth_lstm_params

    R, K, n, A, seq, burn, length, seed = 8, 4, 3, 6, 8, 4, 11, 31
    T = burn + seq + n
    on, tg = LSTMNetHandle(A, DEV), LSTMNetHandle(A, DEV)
    on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, 1).items()})
    tg.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, 2).items()})
    replay = RNNReplay(128, 7, 0.6, 0.4, 0, A, T, DEV)
    eng = R2D2ActorEngine(R, K, A, n, 0.997, seq, burn, 0.9, replay, np.linspace(0.0, 0.5, R).tolist(), DEV)
    if device_fed:
        env = DeviceCatchEnv(R, A, length, seed, DEV)
        env.reset(eng.next_obs_slot())
    else:
        ref = CatchRefVec(R, A, length, seed)
        eng.next_obs_slot().copy_(_cuda(ref.reset()))
    n_seq, terminals = [], 0
    for t in range(ticks):
        action = eng.act(on)
        if device_fed:
            _, _, reward, terminal = env.step_host(action)
            assert reward.dtype == np.float32 and terminal.dtype == np.uint8
            n_seq.append(eng.post_step(reward, terminal, on, tg))
            env.render(eng.next_obs_slot())
        else:
            reward, terminal = ref.step(action.cpu().numpy())
            n_seq.append(eng.post_step(reward, terminal, on, tg))
            eng.next_obs_slot().copy_(_cuda(ref.obs()))
        terminals += int(terminal.sum())
    assert replay.size() >= 8 and terminals >= 2 * R  # terminals padded windows
    replay.sample(8)
    torch.cuda.synchronize()
    out = {f: v.cpu().numpy().copy() for f, v in replay._buffers(8, 0).items()}
    if device_fed:
        env.close()
    eng.close()
    replay.close()
    return n_seq, out


def test_r2d2_shard_fed_through_step_host_equals_the_host_fed_shard():
    dev_seq, dev_batch = _r2d2_run(True, 40)
    ref_seq, ref_batch = _r2d2_run(False, 40)
    assert dev_seq == ref_seq and sum(dev_seq) > 0
    assert sorted(dev_batch) == sorted(ref_batch)
    for f in dev_batch:
        assert np.array_equal(dev_batch[f], ref_batch[f]), f


# ---- 7. greedy evaluation ----------------------------------------------------------------------------------------------
def test_greedy_evaluation_scores_the_collected_rewards_and_repeats_itself():
    import torch
    from types import SimpleNamespace

    from rela_amd.device_env import DeviceCatchEnv
    from rela_amd.engine import ApexActorEngine
    from rela_amd.pyrela import train_engine

    rows, A, length, seed = 32, 18, 40, 77
    on, _ = _ffnets(A)
    eng = ApexActorEngine(rows, rows, A, 3, 0.997, None, [0.0] * rows, DEV)
    env = DeviceCatchEnv(rows, A, length, seed, DEV)
    env.reset(eng.next_obs_slot())
    total = torch.zeros(rows, device=DEV)
    for _ in range(length):
        reward, terminal = env.step(eng.act(on), eng.next_obs_slot())
        total += reward
    assert bool((terminal == 1).all())  # every row's one episode ended on the last tick
    st = env.episode_stats()
    assert st["episodes"] == rows
    assert torch.equal(st["rows"]["last_return"].float(), total)
    manual = float(total.double().mean())
    env.close()
    args = SimpleNamespace(episode_len=length)
    score1, per_row1 = train_engine.evaluate(eng, on, args, seed)
    score2, per_row2 = train_engine.evaluate(eng, on, args, seed)
    assert score1 == manual == score2 and torch.equal(per_row1, per_row2) and torch.equal(per_row1.float(), total)
    assert -2 <= manual <= 2  # 40 ticks = two landings per row
    eng.close()


# ---- 8. the engine training loop ------------------------------------------------------------------------------------------
def test_train_engine_smoke():
    import math

    from rela_amd import _capi as capi
    from rela_amd.pyrela import train_engine

    args = train_engine.parse_args(["--rows", "64", "--group_rows", "16", "--replay_buffer_size", "4096", "--batchsize", "32",
                                    "--burn_in_frames", "256", "--episode_len", "20", "--num_epoch", "2", "--epoch_len", "20",
                                    "--eval_rows", "16"])
    seen = []
    with capi.launch_census() as census:
        history = train_engine.train(args, on_epoch=seen.append)
    assert len(history) == 2 and seen == history
    for rec in history:
        assert set(train_engine.HISTORY_KEYS) <= set(rec)
        assert math.isfinite(rec["loss"]) and rec["env_steps_per_s"] > 0 and rec["grad_steps_per_s"] > 0
        assert rec["num_act"] == 64 * rec["ticks"]
        assert math.isfinite(rec["eval_return"]) and -1 <= rec["eval_return"] <= 1  # 20 ticks = one landing per row
        assert rec["weights_moved"] > 0  # the online weights differ from the initial ones
    assert [rec["updates"] for rec in history] == [20, 40]
    assert history[1]["actor_net_version"] > history[0]["actor_net_version"]  # the actors' nets were re-published
    assert history[1]["train_episodes"] > 0 and math.isfinite(history[1]["train_return"])
    assert math.isfinite(history[1]["train_return_low_eps"])
    for kernel in ("catch_step_render", "catch_step", "catch_render", "catch_reset_render"):
        assert census.counts.get(kernel, 0) > 0, census.counts
