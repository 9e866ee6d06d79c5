"""Indexed-colour screens on the GPU: the kernel (rela_atari_features_indexed), the actor shards' screens_to_stacks in
the indexed set-up, and the drop-in module's indexed screen mode (rela/screen_env.h: screenChannels() == 1).

The palette lookup happens in the kernel and the frame is max(pal[ia], pal[ib]) per channel, so everything equals the
RGB path on the expanded screens pal[ia], pal[ib] bit for bit: the host restatements (synth_atari.screen_features_indexed,
screen_features) and the RGB kernel (rela_atari_features)."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_atari_screen_indexed_cpu import edge_indexed  # noqa: E402


@pytest.fixture(scope="module")
def mods():
    sys.path.insert(0, os.path.join(ROOT, "rela_amd", "pybind"))
    import torch  # noqa: F401
    import rela
    import synth_atari

    return rela, synth_atari


def random_indexed(rows, H=210, W=160, seed=0):
    """[rows][2][H][W] uniform indices and [rows][256][3] uniform palettes, a different one per row"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, 2, H, W), dtype=np.uint8), rng.integers(0, 256, (rows, 256, 3), dtype=np.uint8)


def expand(idx, pal):
    """[rows][2][H][W] indices -> [rows][2][H][W][3] RGB through every row's own palette"""
    return np.stack([pal[r][idx[r]] for r in range(len(idx))])


def host_indexed(synth, idx, pal):
    import torch

    return np.stack([synth.screen_features_indexed(torch.from_numpy(idx[r, 0]), torch.from_numpy(idx[r, 1]),
                                                   torch.from_numpy(pal[r])).numpy() for r in range(len(idx))])


def host_rgb(synth, scr):
    import torch

    return np.stack([synth.screen_features(torch.from_numpy(p[0]), torch.from_numpy(p[1])).numpy() for p in scr])


def dev_indexed(idx, pal, offset=0):
    """rela_atari_features_indexed; offset: the screens start that many bytes into their (16-byte aligned) allocation"""
    import torch

    from rela_amd import _capi as capi

    rows, _, H, W = idx.shape
    buf = torch.zeros(idx.size + offset, dtype=torch.uint8, device="cuda:0")
    buf[offset:].copy_(torch.from_numpy(idx.reshape(-1)))
    assert buf.data_ptr() % 16 == 0
    p = torch.from_numpy(pal).to("cuda:0")
    out = torch.full((rows, 84, 84), 7, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_atari_features_indexed(C.c_void_p(buf.data_ptr() + offset), C.c_void_p(p.data_ptr()), rows, H, W,
                                                        C.c_void_p(out.data_ptr()), stream), "rela_atari_features_indexed")
        torch.cuda.synchronize()
    assert census.counts.get("atari_features_indexed") == 1, census.counts  # all rows in one launch
    assert "atari_features" not in census.counts, census.counts
    return out.cpu().numpy()


def dev_rgb(scr):
    import torch

    from rela_amd import _capi as capi

    rows, _, H, W, _ = scr.shape
    s = torch.from_numpy(scr).to("cuda:0")
    out = torch.full((rows, 84, 84), 9, dtype=torch.uint8, device="cuda:0")
    capi.check(capi.lib.rela_atari_features(C.c_void_p(s.data_ptr()), rows, H, W, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "rela_atari_features")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_all(synth, idx, pal, offset=0):
    got = dev_indexed(idx, pal, offset)
    scr = expand(idx, pal)
    for what, ref in (("host indexed", host_indexed(synth, idx, pal)), ("host RGB", host_rgb(synth, scr)),
                      ("RGB kernel", dev_rgb(scr))):
        assert np.array_equal(got, ref), "%s: %d of %d pixels differ" % (what, (got != ref).sum(), got.size)
    return got


@pytest.mark.parametrize("rows", [1, 7, 300])
def test_kernel_equals_host_restatement_and_rgb_kernel(mods, rows):
    _, synth = mods
    idx, pal = random_indexed(rows, seed=rows)
    got = check_all(synth, idx, pal)
    assert len(np.unique(got)) > 50


def with_edges(idx, pal, H, W):
    e = edge_indexed(H, W)
    return (np.concatenate([idx, np.stack([np.stack([a, b]) for a, b, _ in e])]),
            np.concatenate([pal, np.stack([p for _, _, p in e])]))


@pytest.mark.parametrize("shape", [(250, 160), (210, 161), (37, 300), (2, 2), (512, 512), (84, 84)])
def test_kernel_other_shapes(mods, shape):
    """both instantiations (16-byte loads: W % 16 == 0; byte loads otherwise), upsampling, the limits, a width above 256"""
    _, synth = mods
    H, W = shape
    idx, pal = with_edges(*random_indexed(5, H, W, seed=4), H, W)
    check_all(synth, idx, pal)


def test_kernel_unaligned_screens_take_the_byte_path(mods):
    """W = 160 but the screens start one byte past a 16-byte boundary: byte loads, still exact"""
    _, synth = mods
    idx, pal = with_edges(*random_indexed(5, 210, 160, seed=8), 210, 160)
    check_all(synth, idx, pal, offset=1)


def test_kernel_refuses_bad_arguments():
    import torch

    from rela_amd import _capi as capi

    buf = torch.zeros(2 * 513 * 513, dtype=torch.uint8, device="cuda:0")
    pal = torch.zeros(256 * 3, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(84 * 84, dtype=torch.uint8, device="cuda:0")
    p, q, o = C.c_void_p(buf.data_ptr()), C.c_void_p(pal.data_ptr()), C.c_void_p(out.data_ptr())
    f = capi.lib.rela_atari_features_indexed
    for (rows, H, W) in ((1, 1, 160), (1, 210, 1), (1, 513, 160), (1, 210, 513), (0, 210, 160)):
        assert f(p, q, rows, H, W, o, None) == capi.EINVAL, (rows, H, W)
    assert f(p, None, 1, 210, 160, o, None) == capi.EINVAL  # no palette
    assert f(None, q, 1, 210, 160, o, None) == capi.EINVAL
    assert f(p, q, 1, 210, 160, None, None) == capi.EINVAL
    torch.cuda.synchronize()
    assert (out.cpu() == 0).all()


def _expected_stacks(feats, restart, prev):
    out = np.empty((len(feats), 4, 84, 84), np.uint8)
    for r in range(len(feats)):
        out[r] = np.stack([feats[r]] * 4) if restart[r] else np.concatenate([prev[r, 1:], feats[r][None]])
    return out


def _make_shard(shard):
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle, LSTMNetHandle, R2D2ActorEngine
    from rela_amd.replay import FFReplay, RNNReplay
    from synth import synth_lstm_params, synth_params

    R, A, n = 7, 6, 3
    ev = shard.endswith("_eval")
    if shard.startswith("apex"):
        on, tg = FFNetHandle(A), FFNetHandle(A)
        for net, seed in ((on, 1), (tg, 2)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, seed).items()})
        replay = None if ev else FFReplay(1024, 3, 1.0, 1.0, 0, A, "cuda:0")
        eng = ApexActorEngine(R, R, A, 1 if ev else n, 0.99, replay, [0.0] * R)
        fns = {k: getattr(capi.lib, "rela_apex_actor_" + k)
               for k in ("set_screen_input", "set_screen_input_indexed", "screen_stage", "palette_stage", "screens_to_stacks")}
    else:
        on, tg = LSTMNetHandle(A), LSTMNetHandle(A)
        for net, seed in ((on, 1), (tg, 2)):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, seed).items()})
        seq, burn = 5, 2
        replay = None if ev else RNNReplay(256, 3, 1.0, 1.0, 0, A, burn + seq + n, "cuda:0")
        eng = R2D2ActorEngine(R, R, A, 1 if ev else n, 0.99, 1 if ev else seq, 0 if ev else burn, 0.9, replay, [0.0] * R)
        fns = {k: getattr(capi.lib, "rela_r2d2_actor_" + k)
               for k in ("set_screen_input", "set_screen_input_indexed", "screen_stage", "palette_stage", "screens_to_stacks")}
    return eng, on, tg, SimpleNamespace(**fns), R


@pytest.mark.parametrize("shard", ["apex", "r2d2", "apex_eval", "r2d2_eval"])
def test_shard_screens_to_stacks_indexed(mods, shard):
    """40 ticks with random restart flags (all set on the first): every stack of the obs slot equals the stacks built in
    numpy from screen_features_indexed with the sliding and restart rule.  The palette stage exists only in the indexed
    set-up, which excludes the RGB one."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import dev_view

    _, synth = mods
    H, W = 210, 160
    ev = shard.endswith("_eval")
    eng, on, tg, lib, R = _make_shard(shard)
    assert lib.palette_stage(eng.h) is None  # no screen input yet
    capi.check(lib.set_screen_input_indexed(eng.h, H, W), "set_screen_input_indexed")
    assert lib.set_screen_input_indexed(eng.h, H, W) == capi.ESTATE  # once
    assert lib.set_screen_input(eng.h, H, W) == capi.ESTATE          # and not the RGB format on top
    dev = torch.device("cuda:0")
    stage = dev_view(lib.screen_stage(eng.h), (R, 2, H, W), torch.uint8, dev)
    assert lib.palette_stage(eng.h)
    pstage = dev_view(lib.palette_stage(eng.h), (R, 256, 3), torch.uint8, dev)
    assert (pstage.cpu() == 0).all() and (stage.cpu() == 0).all()  # zero-initialised
    rng = np.random.default_rng(11)
    pal = rng.integers(0, 256, (R, 256, 3), dtype=np.uint8)
    pstage.copy_(torch.from_numpy(pal))  # once
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    prev = None
    bad = np.zeros(R, np.uint8)
    assert lib.screens_to_stacks(eng.h, bad.ctypes.data_as(C.c_void_p), stream) == capi.EINVAL  # the first tick restarts all
    for t in range(40):
        idx = rng.integers(0, 256, (R, 2, H, W), dtype=np.uint8)
        restart = np.ones(R, np.uint8) if t == 0 else (rng.uniform(size=R) < 0.3).astype(np.uint8)
        stage.copy_(torch.from_numpy(idx))
        with capi.launch_census() as census:
            capi.check(lib.screens_to_stacks(eng.h, restart.ctypes.data_as(C.c_void_p), stream), "screens_to_stacks")
        assert census.counts.get("atari_features_indexed") == 1 and "atari_features" not in census.counts, census.counts
        got = eng.next_obs_slot().cpu().numpy()
        exp = _expected_stacks(host_indexed(synth, idx, pal), restart, prev)
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


@pytest.mark.parametrize("shard", ["apex", "r2d2"])
def test_shard_rgb_set_up_has_no_palette_and_excludes_indexed(shard):
    from rela_amd import _capi as capi

    eng, _, _, lib, _ = _make_shard(shard)
    capi.check(lib.set_screen_input(eng.h, 210, 160), "set_screen_input")
    assert lib.palette_stage(eng.h) is None
    assert lib.set_screen_input_indexed(eng.h, 210, 160) == capi.ESTATE
    assert lib.palette_stage(eng.h) is None and lib.screen_stage(eng.h)
    eng.close()


# ---- the drop-in module: the indexed device env against the RGB device env and the host env ---------------------------

def _shim(synth, device, indexed):
    """e2e_lockstep builds SyntheticAtariEnv(seed, eps, A, L[, sliding]): hand it the screen env in one mode"""
    return SimpleNamespace(
        SyntheticAtariEnv=lambda seed, eps, A, L, *rest: synth.SyntheticScreenEnv(seed, eps, A, L, device, indexed))


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
def test_module_apex_lockstep_indexed_equals_rgb_and_host(mods, dedup_env, cfg):
    """run_lockstep (a lone actor, and a cohort of two threads): the indexed device env gives the rounds of the RGB
    device env and of the host env, also with the plane-de-duplicating replay, and launches only the indexed kernel."""
    import e2e_lockstep
    from e2e_lockstep import load_agent_params, run_lockstep
    from rela_amd import _capi as capi
    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet

    rela, synth = mods
    C_ = getattr(e2e_lockstep, cfg)
    out = {}
    for name, device, indexed, dedup in (("host", False, False, None), ("rgb", True, False, None),
                                         ("indexed", True, True, None), ("indexed_plane", True, True, "plane")):
        dedup_env(dedup)
        agent = load_agent_params(ApexAgent(lambda: AtariFFNet(C_["num_action"]), C_["multi_step"], C_["gamma"]), C_)
        with capi.launch_census() as census:
            out[name] = run_lockstep(rela, _shim(synth, device, indexed), agent, "cuda:0", "cuda:0", C_)
        assert ("atari_features_indexed" in census.counts) == indexed, (name, census.counts)
        assert ("atari_features" in census.counts) == (device and not indexed), (name, census.counts)
    assert out["indexed"] == out["rgb"] == out["host"]
    assert out["indexed_plane"] == out["host"]
    assert len({s for r in out["host"] for s in r["s_sum"]}) > 1  # the sampled stacks are not all alike


def test_module_r2d2_lockstep_indexed_equals_rgb_and_host(mods):
    from e2e_lockstep import CFG_R2D2, load_lstm_agent_params, run_lockstep_r2d2
    from rela_amd import _capi as capi
    from rela_amd.pyrela.net import AtariLSTMNet
    from rela_amd.pyrela.r2d2 import R2D2Agent

    rela, synth = mods
    out = []
    for device, indexed in ((False, False), (True, False), (True, True)):
        agent = R2D2Agent(lambda dev: AtariLSTMNet(dev, CFG_R2D2["num_action"]), "cpu", CFG_R2D2["multi_step"],
                          CFG_R2D2["gamma"], CFG_R2D2["eta"], CFG_R2D2["seq_len"], CFG_R2D2["burn_in"], 0)
        with capi.launch_census() as census:
            out.append(run_lockstep_r2d2(rela, _shim(synth, device, indexed), load_lstm_agent_params(agent, CFG_R2D2), "cuda:0",
                                         "cuda:0", CFG_R2D2))
        assert ("atari_features_indexed" in census.counts) == indexed, census.counts
        assert ("atari_features" in census.counts) == (device and not indexed), census.counts
    assert out[2] == out[1] == out[0]


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_module_eval_episode_indexed_equals_host(mods, algo):
    """one evaluation episode (DQNActor(locker) / R2D2Actor(locker), one env): the same reward and num_act"""
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
    for device, indexed in ((False, False), (True, True)):
        locker = rela.ModelLocker([agent], "cuda:0")
        game = synth.SyntheticScreenEnv(77, 0.0, A, 60, device, indexed)
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
    print(algo, "eval (reward, num_act) host / indexed device:", res)
    assert res[0] == res[1] and res[0][1] == 60


def test_vector_env_of_rgb_and_indexed_screen_envs_raises_at_first_reset(mods):
    """one RGB and one indexed screen env in a VectorEnv: refused at its first reset() (raised through Context)"""
    import time

    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet

    rela, synth = mods
    agent = ApexAgent(lambda: AtariFFNet(18), 3, 0.99)
    locker = rela.ModelLocker([agent], "cuda:0")
    replay = rela.FFPrioritizedReplay(64, 1, 1.0, 1.0, 0)
    vec = rela.VectorEnv()
    vec.append(synth.SyntheticScreenEnv(1, 0.0, 18, 10, True))
    vec.append(synth.SyntheticScreenEnv(2, 0.0, 18, 10, True, indexed=True))
    ctx = rela.Context()
    ctx.push_env_thread(rela.BasicThreadLoop(rela.DQNActor(locker, 3, 2, 0.99, replay), vec, False))
    ctx.start()
    t0 = time.time()
    with pytest.raises(RuntimeError, match="screen envs of different formats"):
        while not ctx.terminated():
            assert time.time() - t0 < 60
            time.sleep(0.01)
