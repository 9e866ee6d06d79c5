"""GameState::computeFeature (atari/game_state.h:53-82,122-133) on the GPU: the kernel (rela_atari_features), the actor
shards' screens_to_stacks and the drop-in module's screen mode (rela/screen_env.h, synth_atari.SyntheticScreenEnv).

The kernel must be bit-identical to the host restatement synth_atari.screen_features (one fixed float32 recipe,
csrc/atari_screen.h) and, like it, within the cap of tests/test_atari_screen_cpu.py against the reference's torch ops
(every pixel within 1, at most 1e-3 of all pixels differ)."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_atari_screen_cpu import cap_check, edge_pairs, screen_pairs, torch_feature  # noqa: E402


@pytest.fixture(scope="module")
def mods():
    sys.path.insert(0, os.path.join(ROOT, "rela_amd", "pybind"))
    import torch  # noqa: F401
    import rela
    import synth_atari

    return rela, synth_atari


def host_features(synth, scr):
    """[rows][2][H][W][3] -> [rows][84][84] with synth_atari.screen_features"""
    import torch

    return np.stack([synth.screen_features(torch.from_numpy(p[0]), torch.from_numpy(p[1])).numpy() for p in scr])


def dev_features(scr):
    import torch

    from rela_amd import _capi as capi

    rows, _, H, W, _ = scr.shape
    s = torch.from_numpy(scr).to("cuda:0")
    out = torch.full((rows, 84, 84), 7, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_atari_features(C.c_void_p(s.data_ptr()), rows, H, W, C.c_void_p(out.data_ptr()), stream),
                   "rela_atari_features")
        torch.cuda.synchronize()
    assert census.counts.get("atari_features") == 1, census.counts  # all rows in one launch
    return out.cpu().numpy()


def random_screens(rows, H=210, W=160, seed=0):
    """rows pairs: alternately uniform noise and 8-colour palette screens with 10-pixel blocks"""
    pairs = screen_pairs(H, W, n=min(rows, 40), seed=seed)
    rng = np.random.default_rng(seed + 1)
    out = np.empty((rows, 2, H, W, 3), np.uint8)
    for r in range(rows):
        if r < len(pairs):
            out[r, 0], out[r, 1] = pairs[r]
        else:
            out[r] = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    return out


@pytest.mark.parametrize("rows", [1, 7, 2400])
def test_kernel_bit_identical_to_host_restatement(mods, rows):
    _, synth = mods
    scr = random_screens(rows)
    got = dev_features(scr)
    ref = host_features(synth, scr)
    assert np.array_equal(got, ref), "%d of %d pixels differ" % ((got != ref).sum(), got.size)


@pytest.mark.parametrize("shape", [(250, 160), (210, 161), (2, 2), (512, 512), (84, 84), (37, 300)])
def test_kernel_other_shapes_bit_identical(mods, shape):
    """other screen sizes, among them rows that are not a multiple of 16 bytes (byte loads) and upsampling"""
    _, synth = mods
    H, W = shape
    scr = random_screens(5, H, W, seed=4)
    scr = np.concatenate([scr, np.stack([np.stack(p) for p in edge_pairs(H, W)])])
    assert np.array_equal(dev_features(scr), host_features(synth, scr))


def test_kernel_within_cap_of_torch(mods):
    """the inputs of the CPU test (40 pairs, seed 0, 210x160) plus its edge cases, against the reference's torch ops"""
    scr = np.stack([np.stack(p) for p in screen_pairs() + edge_pairs(210, 160)])
    got = dev_features(scr)
    ref = np.stack([torch_feature(p[0], p[1]) for p in scr])
    cap_check(got, ref, "kernel vs torch, %d pairs" % len(scr))


def test_kernel_refuses_bad_shapes():
    import torch

    from rela_amd import _capi as capi

    buf = torch.zeros(2 * 513 * 513 * 3, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(84 * 84, dtype=torch.uint8, device="cuda:0")
    p, o = C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr())
    for (rows, H, W) in ((1, 1, 160), (1, 210, 1), (1, 513, 160), (1, 210, 513), (0, 210, 160)):
        assert capi.lib.rela_atari_features(p, rows, H, W, o, None) == capi.EINVAL, (rows, H, W)
    torch.cuda.synchronize()
    assert (out.cpu() == 0).all()


def _expected_stacks(feats, restart, prev):
    out = np.empty((len(feats), 4, 84, 84), np.uint8)
    for r in range(len(feats)):
        out[r] = np.stack([feats[r]] * 4) if restart[r] else np.concatenate([prev[r, 1:], feats[r][None]])
    return out


@pytest.mark.parametrize("shard", ["apex", "r2d2", "apex_eval", "r2d2_eval"])
def test_shard_screens_to_stacks(mods, shard):
    """40 ticks with random restart flags (all set on the first): every stack of the obs slot equals the stacks built
    in numpy from screen_features with the sliding and restart rule."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle, LSTMNetHandle, R2D2ActorEngine
    from rela_amd.replay import FFReplay, RNNReplay
    from synth import synth_lstm_params, synth_params

    _, synth = mods
    R, A, n, H, W = 7, 6, 3, 210, 160
    ev = shard.endswith("_eval")
    if shard.startswith("apex"):
        on, tg = FFNetHandle(A), FFNetHandle(A)
        for net, seed in ((on, 1), (tg, 2)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, seed).items()})
        replay = None if ev else FFReplay(1024, 3, 1.0, 1.0, 0, A, "cuda:0")
        eng = ApexActorEngine(R, R, A, 1 if ev else n, 0.99, replay, [0.0] * R)
        lib_set, lib_stage, lib_to = (capi.lib.rela_apex_actor_set_screen_input, capi.lib.rela_apex_actor_screen_stage,
                                      capi.lib.rela_apex_actor_screens_to_stacks)
    else:
        on, tg = LSTMNetHandle(A), LSTMNetHandle(A)
        for net, seed in ((on, 1), (tg, 2)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, seed).items()})
        seq, burn = 5, 2
        replay = None if ev else RNNReplay(256, 3, 1.0, 1.0, 0, A, burn + seq + n, "cuda:0")
        eng = R2D2ActorEngine(R, R, A, 1 if ev else n, 0.99, 1 if ev else seq, 0 if ev else burn, 0.9, replay, [0.0] * R)
        lib_set, lib_stage, lib_to = (capi.lib.rela_r2d2_actor_set_screen_input, capi.lib.rela_r2d2_actor_screen_stage,
                                      capi.lib.rela_r2d2_actor_screens_to_stacks)
    capi.check(lib_set(eng.h, H, W), "set_screen_input")
    assert lib_set(eng.h, H, W) == capi.ESTATE  # once
    from rela_amd.engine import dev_view

    stage = dev_view(lib_stage(eng.h), (R, 2, H, W, 3), torch.uint8, torch.device("cuda:0"))
    rng = np.random.default_rng(11)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    prev = None
    bad = np.zeros(R, np.uint8)
    assert lib_to(eng.h, bad.ctypes.data_as(C.c_void_p), stream) == capi.EINVAL  # the first tick must restart every row
    for t in range(40):
        scr = random_screens(R, H, W, seed=100 + t)
        restart = np.ones(R, np.uint8) if t == 0 else (rng.uniform(size=R) < 0.3).astype(np.uint8)
        stage.copy_(torch.from_numpy(scr))
        capi.check(lib_to(eng.h, restart.ctypes.data_as(C.c_void_p), stream), "screens_to_stacks")
        got = eng.next_obs_slot().cpu().numpy()
        exp = _expected_stacks(host_features(synth, scr), restart, prev)
        assert np.array_equal(got, exp), (shard, t, int((got != exp).sum()))
        prev = exp
        eng.act(on)
        torch.cuda.synchronize()
        if not ev:
            r = rng.integers(-1, 2, R).astype(np.float32)
            term = (rng.uniform(size=R) < 0.1).astype(np.uint8)
            if shard == "apex":
                eng.post_step(torch.from_numpy(r).cuda(), torch.from_numpy(term).cuda(), on, tg, nonblocking=True)
            else:
                eng.post_step(r, term, on, tg, nonblocking=True)
            torch.cuda.synchronize()
    eng.close()


# ---- the drop-in module: SyntheticScreenEnv with the stacks built on the GPU (device mode) and on the host -------------

def _shim(synth, device):
    """e2e_lockstep builds SyntheticAtariEnv(seed, eps, A, L[, sliding]): hand it the screen env in one mode"""
    return SimpleNamespace(SyntheticAtariEnv=lambda seed, eps, A, L, *rest: synth.SyntheticScreenEnv(seed, eps, A, L, device))


@pytest.fixture
def dedup_env():
    def set_(mode):
        if mode:
            os.environ["RELA_REPLAY_DEDUP"] = mode
            os.environ["RELA_REPLAY_DEDUP_GUARD"] = "4096"
        else:
            os.environ.pop("RELA_REPLAY_DEDUP", None)
            os.environ.pop("RELA_REPLAY_DEDUP_GUARD", None)
    yield set_
    set_(None)


@pytest.mark.parametrize("cfg", ["CFG", "CFG_SLIDING_COHORT"])
def test_module_apex_lockstep_device_equals_host(mods, dedup_env, cfg):
    """run_lockstep with the screen env: device-built stacks give the same rounds as host-built ones (a lone actor and a
    cohort of two threads), and so does the plane-de-duplicating replay (RELA_REPLAY_DEDUP=plane) in device mode."""
    import e2e_lockstep
    from e2e_lockstep import load_agent_params, run_lockstep
    from rela_amd import _capi as capi
    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet

    rela, synth = mods
    C_ = getattr(e2e_lockstep, cfg)
    out = {}
    for name, device, dedup in (("host", False, None), ("device", True, None), ("device_plane", True, "plane")):
        dedup_env(dedup)
        agent = load_agent_params(ApexAgent(lambda: AtariFFNet(C_["num_action"]), C_["multi_step"], C_["gamma"]), C_)
        with capi.launch_census() as census:
            out[name] = run_lockstep(rela, _shim(synth, device), agent, "cuda:0", "cuda:0", C_)
        assert ("atari_features" in census.counts) == device, (name, census.counts)
    assert out["device"] == out["host"]
    assert out["device_plane"] == out["host"]
    assert len({s for r in out["host"] for s in r["s_sum"]}) > 1  # the sampled stacks are not all alike


def test_module_r2d2_lockstep_device_equals_host(mods):
    from e2e_lockstep import CFG_R2D2, load_lstm_agent_params, run_lockstep_r2d2
    from rela_amd.pyrela.net import AtariLSTMNet
    from rela_amd.pyrela.r2d2 import R2D2Agent

    rela, synth = mods
    out = []
    for device in (False, True):
        agent = R2D2Agent(lambda dev: AtariLSTMNet(dev, CFG_R2D2["num_action"]), "cpu", CFG_R2D2["multi_step"],
                          CFG_R2D2["gamma"], CFG_R2D2["eta"], CFG_R2D2["seq_len"], CFG_R2D2["burn_in"], 0)
        out.append(run_lockstep_r2d2(rela, _shim(synth, device), load_lstm_agent_params(agent, CFG_R2D2), "cuda:0", "cuda:0",
                                     CFG_R2D2))
    assert out[0] == out[1]


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_module_eval_episode_device_equals_host(mods, algo):
    """one evaluation episode (DQNActor(locker) / R2D2Actor(locker), one env) per mode: the same reward and num_act"""
    import time

    from e2e_lockstep import CFG, CFG_R2D2, load_agent_params, load_lstm_agent_params
    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet, AtariLSTMNet
    from rela_amd.pyrela.r2d2 import R2D2Agent

    rela, synth = mods
    if algo == "apex":
        agent = load_agent_params(ApexAgent(lambda: AtariFFNet(CFG["num_action"]), CFG["multi_step"], CFG["gamma"]))
        A, actor_cls = CFG["num_action"], rela.DQNActor
    else:
        agent = load_lstm_agent_params(R2D2Agent(lambda dev: AtariLSTMNet(dev, CFG_R2D2["num_action"]), "cpu",
                                                 CFG_R2D2["multi_step"], CFG_R2D2["gamma"], CFG_R2D2["eta"],
                                                 CFG_R2D2["seq_len"], CFG_R2D2["burn_in"], 0))
        A, actor_cls = CFG_R2D2["num_action"], rela.R2D2Actor
    res = []
    for device in (False, True):
        locker = rela.ModelLocker([agent], "cuda:0")
        game = synth.SyntheticScreenEnv(77, 0.0, A, 60, device)
        vec = rela.VectorEnv()
        vec.append(game)
        actor = actor_cls(locker)
        ctx = rela.Context()
        ctx.push_env_thread(rela.BasicThreadLoop(actor, vec, True))
        ctx.start()
        t0 = time.time()
        while not ctx.terminated():
            assert time.time() - t0 < 120
            time.sleep(0.01)
        res.append((game.get_episode_reward(), actor.num_act()))
        del ctx
    print(algo, "eval (reward, num_act) host / device:", res)
    assert res[0] == res[1] and res[0][1] == 60
