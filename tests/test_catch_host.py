"""Catch on the host: rela_amd/csrc/catch_game.h compiled by g++ (tests/cpu_shims/catch_game_host.cpp) and the host env
synth_atari.CatchEnv against the pure-Python restatement of the specification (tests/catch_ref.py), the env selection of
create_env and the engine loop's parser.  No GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from catch_ref import CatchRef, walk_policy

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu_shims", "catch_game_host.cpp")
HDR = os.path.join(HERE, "..", "rela_amd", "csrc", "catch_game.h")
OBS = 4 * 84 * 84


@functools.lru_cache(maxsize=None)
def shim():
    so = os.path.join(HERE, "cpu_shims", "libcatch_game_host.so")
    if not os.path.exists(so) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC], check=True)
    return C.CDLL(so)


def shim_run(seed, num_action, episode_len, actions):
    n = len(actions)
    a = np.ascontiguousarray(actions, np.int64)
    obs = np.zeros((n + 1, 4, 84, 84), np.uint8)
    state = np.zeros((n + 1, 8), np.int32)
    reward, terminal, stats = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(4, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    shim().shim_catch_run(C.c_int64(seed), num_action, episode_len, p(a), n, p(obs), p(state), p(reward), p(terminal), p(stats))
    return obs, state, reward, terminal, stats


@functools.lru_cache(maxsize=None)
def runs():
    """3 seeds x 450 steps at episode_len = 45 (episodes end mid-fall: a ball needs 20 steps), random actions over all 18
    ids: per seed (actions, the shim's outputs, the reference's outputs)"""
    out = []
    for seed in (0, 1, 2 ** 31 + 5):
        actions = np.random.default_rng(100 + seed % 97).integers(0, 18, 450)
        got = shim_run(seed, 18, 45, actions)
        ref = CatchRef(seed, 18, 45, auto_reset=True)
        r_obs, r_state = [ref.reset()], [ref.state()]
        r_reward, r_term = [], []
        for a in actions:
            r, t = ref.step(a)
            r_reward.append(r)
            r_term.append(t)
            r_obs.append(ref.obs())
            r_state.append(ref.state())
        stats = [ref.episodes, ref.return_sum, ref.last_return, ref.last_len]
        out.append((actions, got, (np.stack(r_obs), np.array(r_state, np.int32), np.array(r_reward, np.int32),
                                   np.array(r_term, np.uint8), np.array(stats, np.int32))))
    return out


def test_header_equals_the_python_restatement_at_every_step():
    for actions, got, ref in runs():
        for name, g, r in zip(("obs", "state", "reward", "terminal", "stats"), got, ref):
            assert g.shape == r.shape and g.dtype == r.dtype, name
            if not np.array_equal(g, r):
                bad = int(np.argwhere(g.reshape(len(g), -1) != r.reshape(len(r), -1))[0][0])
                raise AssertionError("%s differs first at index %d" % (name, bad))
        assert got[0].shape[1:] == (4, 84, 84) and got[0][0].size == OBS  # all 28,224 bytes of every step were compared
        assert ref[4][0] == 10 and ref[3].sum() == 10  # 450 / 45 episodes
    # the runs together saw misses, catches and steps without a landing
    assert set(np.concatenate([ref[2] for _, _, ref in runs()]).tolist()) == {-1, 0, 1}


def test_stack_slides_by_one_plane_and_a_reset_repeats_the_first_frame():
    for actions, got, _ in runs():
        obs, terminal = got[0], got[3]
        assert not (obs[0, 0] != obs[0]).any()  # the first observation: four equal planes
        for t in range(1, len(obs)):
            if terminal[t - 1]:
                assert all(np.array_equal(obs[t, k], obs[t, 3]) for k in range(3)), t
            else:
                assert np.array_equal(obs[t, :3], obs[t - 1, 1:]), t
        # a frame holds exactly a ball and a paddle
        assert set(np.unique(obs)) == {0, 170, 255}
        assert ((obs == 255).sum(axis=(2, 3)) == 16).all() and ((obs == 170).sum(axis=(2, 3)) == 36).all()


def test_pixel_definition_equals_the_rectangle_rendering():
    """catch_game::pixel (what the kernel evaluates per byte) against catch_game::render (what the host env draws)"""
    for actions, got, _ in runs()[:1]:
        obs = got[0]
        for t in (0, 19, 20, 44, 45, 449):
            planes = obs[t]
            hist = []
            for k in range(4):
                by, bx = np.argwhere(planes[k] == 255)[0]
                px = np.argwhere(planes[k] == 170)[0][1]
                hist += [px, bx, by]
            h = np.array(hist, np.int32)
            out = np.zeros((4, 84, 84), np.uint8)
            shim().shim_catch_pixels(h.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
            assert np.array_equal(out, planes), t
            # ... and pixel_word, the four-pixel form the kernel stores (every coordinate is a multiple of four)
            words = np.zeros((4, 84, 21), np.uint32)
            shim().shim_catch_pixel_words(h.ctypes.data_as(C.c_void_p), words.ctypes.data_as(C.c_void_p))
            assert np.array_equal(words.view(np.uint8).reshape(4, 84, 84), planes), t
    for _, got, _ in runs():
        assert not (got[1][:, 1:3] % 4).any()  # px and bx of every state


def test_walking_towards_the_ball_catches_every_ball():
    """episode_len = 200 over 50 seeds: the policy that walks towards bx - 4 returns exactly 10 = 200 // 20"""
    ret = np.zeros(1, np.int32)
    for seed in range(50):
        shim().shim_catch_walk(C.c_int64(seed), 200, 1, ret.ctypes.data_as(C.c_void_p))
        assert ret[0] == 10, seed
        ref = CatchRef(seed, 18, 200)
        ref.reset()
        while not ref.terminal:
            ref.step(walk_policy(ref))
        assert ref.ep_return == 10, seed


def test_random_policy_scores_well_below_the_optimum():
    """the gap that makes the game learnable: uniformly random actions lose most balls"""
    rng = np.random.default_rng(5)
    total = []
    for seed in range(40):
        _, _, reward, _, _ = shim_run(seed, 18, 200, rng.integers(0, 18, 200))
        total.append(int(reward.sum()))
    assert -10 <= min(total) and np.mean(total) < -4, np.mean(total)


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "catch_game_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DCATCH_MAIN", "-o", exe, SRC], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "0 violations" in out, out


def _obs_dict_action(a):
    import torch

    return {"a": torch.tensor([a], dtype=torch.int64)}


def test_host_env_equals_the_python_restatement():
    from rela_amd.pyrela import create_env

    synth_atari = create_env.synth_atari
    for seed, A in ((3, 18), (2 ** 31 - 1, 3)):
        env = synth_atari.CatchEnv(seed, 0.25, A, 45)
        ref = CatchRef(seed, A, 45)
        assert env.terminated() and env.num_action() == A
        rng = np.random.default_rng(seed % 1000)
        for episode in range(3):
            obs = env.reset()
            assert np.array_equal(obs["s"].numpy(), ref.reset()) and not env.terminated()
            assert obs["s"].dtype.is_floating_point is False and tuple(obs["s"].shape) == (4, 84, 84)
            assert float(obs["eps"][0]) == 0.25 and tuple(obs["eps"].shape) == (1,)
            assert tuple(obs["legal_move"].shape) == (A,) and bool((obs["legal_move"] == 1).all())
            assert env.get_episode_reward() == 0
            for t in range(45):
                a = int(rng.integers(0, A))
                obs, reward, terminal = env.step(_obs_dict_action(a))
                r_reward, r_terminal = ref.step(a)
                assert (reward, terminal) == (float(r_reward), r_terminal), (episode, t)
                assert np.array_equal(obs["s"].numpy(), ref.obs()), (episode, t)
                assert env.state().tolist()[:7] == ref.state()[:7]
                assert env.terminated() == r_terminal and env.get_episode_reward() == ref.ep_return
            assert env.terminated()
        for bad in (-1, A):
            with pytest.raises(IndexError):
                env.step(_obs_dict_action(bad))


def test_create_game_selects_catch_and_the_default_is_unchanged(monkeypatch):
    from rela_amd.pyrela import create_env

    for var in ("RELA_SYNTH_ENV", "RELA_SYNTH_SCREEN", "RELA_SYNTH_SLIDING", "RELA_REPLAY_DEDUP"):
        monkeypatch.delenv(var, raising=False)
    game = create_env.create_game(4, 0.1, 30, game="catch")
    assert type(game).__name__ == "CatchEnv" and game.num_action() == create_env.NUM_ACTION
    for default in (create_env.create_game(4, 0.1, 30), create_env.create_game(4, 0.1, 30, game="synthetic"),
                    create_env.create_game(4, 0.1, 30, None)):
        assert type(default).__name__ == "SyntheticAtariEnv"
    # the very same env as before: the LCG frames of the seed
    a = create_env.create_game(4, 0.1, 30).reset()["s"]
    b = create_env.synth_atari.SyntheticAtariEnv(4, 0.1, create_env.NUM_ACTION, 30, False).reset()["s"]
    assert bool((a == b).all())


def test_engine_loop_is_apex_only(capsys):
    from rela_amd.pyrela import train_engine

    with pytest.raises(SystemExit) as e:
        train_engine.parse_args(["--algo", "r2d2"])
    assert e.value.code != 0 and "Ape-X only" in capsys.readouterr().err
    args = train_engine.parse_args([])
    assert args.algo == "apex" and args.updates_per_tick == 1 and args.lr == 6.25e-5 and args.batchsize == 512
    assert args.rows % args.group_rows == 0 and args.eval_rows > 0
