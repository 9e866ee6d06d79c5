"""Invertible value rescaling of the TD targets on the device (csrc/value_rescale.h through every kernel that forms a
target, and up through the C ABI, the module and main.py):

  3. rela_debug_value_rescale is bit-identical to the host build of the header on the grid of the CPU test.
  4. Actor priority through an Ape-X and an R2D2 shard against a numpy float32 restatement of td_kernel that takes the
     Q tables as the device produced them and the rescaling from the host shim: bit for bit; switch off = an untouched
     shard, bit for bit.
  5. Both learners against the pyrela agent (value_rescale=1e-3) run in float64 on the CPU, at the tolerances of the
     rescale-off tests of the same shapes (tests/test_learner_gpu.py, tests/test_r2d2_learner_gpu.py).
  6. eps = 0 set explicitly = the setter never called, bit for bit.
  7. Through the module: a 2-thread x 2-env lock-step run whose sampled batches go to the HIP learner and to the torch
     agent, and the main.py entry point.
  8. A setter after the first act / loss returns RELA_ESTATE.
"""
import copy
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from value_rescale_util import (EPS, apex_agent, grid, host_h_hinv, nstep_f32, r2d2_agent, scale_rewards,
                                td_priority_f32, to_f64_cpu)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VR = 1e-3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_device_recipe_is_bit_identical_to_the_host_build():
    import torch

    from rela_amd import _capi as capi

    x = np.array(grid())
    d_x = torch.from_numpy(x).cuda()
    d_h, d_hi = torch.empty_like(d_x), torch.empty_like(d_x)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(capi.lib.rela_debug_value_rescale(x.size, d_x.data_ptr(), EPS, d_h.data_ptr(), d_hi.data_ptr(), stream),
               "rela_debug_value_rescale")
    torch.cuda.synchronize()
    h, hi = host_h_hinv(x)
    assert np.array_equal(_bits(d_h.cpu().numpy()), _bits(h))
    assert np.array_equal(_bits(d_hi.cpu().numpy()), _bits(hi))
    assert capi.lib.rela_debug_value_rescale(x.size, d_x.data_ptr(), 0.0, d_h.data_ptr(), d_hi.data_ptr(),
                                             stream) == capi.EINVAL


# ---- 4, 6 and 8 for the actors ------------------------------------------------------------------------------------
K_ENVS, N_ACT, N_STEP, TICKS, GAMMA = 4, 6, 3, 8, 0.997


def _tick_inputs(t):
    """frames, rewards of magnitude up to 1e3 and terminals of tick t, the same for every run"""
    from synth import synth_obs

    rng = np.random.default_rng(9000 + t)
    reward = (rng.uniform(-1, 1, K_ENVS) * 10.0 ** rng.uniform(-1, 3, K_ENVS)).astype(np.float32)
    term = (rng.uniform(size=K_ENVS) < 0.15).astype(np.uint8)
    return synth_obs(K_ENVS, 4100 + t), reward, term


def _gamma_n():
    return float(np.float32(float(np.float32(GAMMA)) ** N_STEP))  # (float)pow((double)gamma, n) of the shards


def _run_apex_shard(mode):
    """mode: None = the setter is never called, else its eps.  -> (priorities [pops][K] from the device, their float32
    restatement from the device's own Q tables, the setter's return code after the run)"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import ApexActorEngine, FFNetHandle
    from rela_amd.replay import FFReplay
    from synth import synth_params

    dev = "cuda:0"
    on, tg = FFNetHandle(N_ACT, dev), FFNetHandle(N_ACT, dev)
    on.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(N_ACT, 11, gain=3.0).items()})
    tg.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(N_ACT, 12, gain=3.0).items()})
    replay = FFReplay(256, 7, 1.0, 0.4, 0, N_ACT, dev)
    eng = ApexActorEngine(K_ENVS, K_ENVS, N_ACT, N_STEP, GAMMA, replay, [0.0] * K_ENVS, dev)
    if mode is not None:
        eng.set_value_rescale(mode)
    legal = torch.ones(K_ENVS, N_ACT, device=dev)
    nb = capi.lib.rela_ffnet_workspace_bytes(tg.h, K_ENVS)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hist, got, want = [], [], []
    for t in range(TICKS):
        obs, reward, term = _tick_inputs(t)
        d_obs = torch.from_numpy(obs).to(dev)
        eng.next_obs_slot().copy_(d_obs)
        act = eng.act(on).cpu().numpy().copy()
        q_on = eng.q[0].cpu().numpy().copy()
        q_tg = torch.empty(K_ENVS, N_ACT, device=dev)  # target(s_t) as post_step evaluates it n ticks from now
        capi.check(capi.lib.rela_ffnet_forward(tg.h, K_ENVS, d_obs.data_ptr(), legal.data_ptr(), q_tg.data_ptr(),
                                               ws.data_ptr(), nb, stream), "rela_ffnet_forward")
        hist.append((act, q_on, q_tg.cpu().numpy().copy(), reward, term))
        popped = eng.post_step(torch.from_numpy(reward).to(dev), torch.from_numpy(term).to(dev), on, tg)
        assert popped == (t >= N_STEP)
        if popped:
            got.append(eng.prio.cpu().numpy().copy())
            t0 = t - N_STEP
            r, b = nstep_f32(np.stack([hist[t0 + k][3] for k in range(N_STEP)]),
                             np.stack([hist[t0 + k][4] for k in range(N_STEP)]), GAMMA, N_STEP)
            want.append(td_priority_f32(hist[t0][1], hist[t][1], hist[t][2], np.ones((K_ENVS, N_ACT), np.float32),
                                        hist[t0][0], r, b, _gamma_n(), mode or 0.0))
    late = capi.lib.rela_apex_actor_set_value_rescale(eng.h, VR)
    eng.close()
    replay.close()
    on.close()
    tg.close()
    return np.array(got), np.array(want), late


def _run_r2d2_shard(mode):
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import dev_view
    from test_r2d2_actor_gpu import _net

    A, n, seq, burn, R = N_ACT, N_STEP, 6, 2, K_ENVS
    T = burn + seq + n
    dev = torch.device("cuda:0")
    online, _k1 = _net(capi, A, 1)
    target, _k2 = _net(capi, A, 2)
    replay = C.c_void_p()
    capi.check(capi.lib.rela_replay_create(C.byref(replay), 8 * R, 7, 0.9, 0.6, 0, 0), "rela_replay_create")
    rb = (C.c_int64 * 10)(T * 28224, T * 4, T * 4 * A, T * 8, T * 4, T, T * 4, 2048, 2048, 4)
    st = (C.c_int32 * 10)(T, T, T, T, T, T, T, 1, 1, 1)
    capi.check(capi.lib.rela_replay_set_schema_seq(replay, 10, rb, st), "schema")
    actor = C.c_void_p()
    capi.check(capi.lib.rela_r2d2_actor_create(C.byref(actor), R, R, A, n, GAMMA, seq, burn, 0.9, replay, 3, 0), "create")
    if mode is not None:
        capi.check(capi.lib.rela_r2d2_actor_set_value_rescale(actor, mode), "rela_r2d2_actor_set_value_rescale")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = capi.lib.rela_lstmnet_workspace_bytes(online, R)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    tmp_h, tmp_c = torch.empty(R, 512, device=dev), torch.empty(R, 512, device=dev)
    legal = np.ones((R, A), np.float32)
    d_legal = torch.from_numpy(legal).to(dev)
    eps = np.zeros(R, np.float32)

    def step(net, d_obs, h, c, want_q):
        """the shard's own call for one of the three tables of compute_priority: dueling Q or the raw advantages"""
        out = torch.empty(R, A, device=dev)
        capi.check(capi.lib.rela_lstmnet_step(net, R, d_obs.data_ptr(), d_legal.data_ptr(), h.data_ptr(), c.data_ptr(),
                                              tmp_h.data_ptr(), tmp_c.data_ptr(), out.data_ptr() if want_q else None,
                                              None if want_q else out.data_ptr(), ws.data_ptr(), nb, stream), "lstmnet_step")
        return out.cpu().numpy().copy()

    hist, got, want = [], [], []
    for t in range(TICKS):
        obs, reward, term = _tick_inputs(t)
        # the recurrent state that enters this act (historyHidden_.push_back(hidden_), r2d2_actor.h:226)
        h = dev_view(capi.lib.rela_r2d2_actor_hidden_dev(actor, 0), (R, 512), torch.float32, dev).clone()
        c = dev_view(capi.lib.rela_r2d2_actor_hidden_dev(actor, 1), (R, 512), torch.float32, dev).clone()
        act = np.zeros(R, np.int64)
        capi.check(capi.lib.rela_r2d2_actor_act(actor, online, obs.ctypes.data_as(C.c_void_p),
                                                eps.ctypes.data_as(C.c_void_p), legal.ctypes.data_as(C.c_void_p),
                                                act.ctypes.data_as(C.c_void_p), None, stream), "act")
        d_obs = torch.from_numpy(obs).to(dev)
        hist.append((act.copy(), step(online, d_obs, h, c, True), step(online, d_obs, h, c, False),
                     step(target, d_obs, h, c, True), reward, term))
        capi.check(capi.lib.rela_r2d2_actor_post_step(actor, reward.ctypes.data_as(C.c_void_p),
                                                      term.ctypes.data_as(C.c_void_p), online, target, 0, None, stream),
                   "post_step")
        torch.cuda.synchronize()
        if t >= n:
            p = dev_view(capi.lib.rela_r2d2_actor_last_priority_dev(actor), (R,), torch.float32, dev)
            got.append(p.cpu().numpy().copy())
            t0 = t - n
            r, b = nstep_f32(np.stack([hist[t0 + k][4] for k in range(n)]), np.stack([hist[t0 + k][5] for k in range(n)]),
                             GAMMA, n)
            # online_net(obs, hid) -> Q; online_net.act(next_obs, next_hid) ranks the advantages; target Q (r2d2.py:76-100)
            want.append(td_priority_f32(hist[t0][1], hist[t][2], hist[t][3], legal, hist[t0][0], r, b, _gamma_n(),
                                        mode or 0.0))
    late = capi.lib.rela_r2d2_actor_set_value_rescale(actor, VR)
    capi.lib.rela_r2d2_actor_destroy(actor)
    capi.lib.rela_replay_destroy(replay)
    capi.lib.rela_lstmnet_destroy(online)
    capi.lib.rela_lstmnet_destroy(target)
    return np.array(got), np.array(want), late


@pytest.mark.parametrize("run", [_run_apex_shard, _run_r2d2_shard], ids=["apex", "r2d2"])
def test_actor_priority_is_the_float32_restatement_bit_for_bit(run):
    from rela_amd import _capi as capi

    got_on, want_on, late = run(EPS)
    assert late == capi.ESTATE  # 8: the setter after the first act
    assert got_on.shape == (TICKS - N_STEP, K_ENVS) and np.isfinite(got_on).all()
    assert np.array_equal(_bits(got_on), _bits(want_on))
    got_bare, want_bare, _ = run(None)
    assert np.array_equal(_bits(got_bare), _bits(want_bare))  # (the restatement itself, against today's arithmetic)
    got_zero, _, _ = run(0.0)
    assert np.array_equal(_bits(got_zero), _bits(got_bare))  # 6: off = untouched
    assert np.abs(got_on - got_bare).max() > 10  # rewards up to 1e3: the rescaling matters


# ---- 5, 6 and 8 for the learners ------------------------------------------------------------------------------------
def _apex_case(B, A, agent_seed, batch_seed):
    from test_learner_gpu import make_batch

    batch, w = make_batch(B, A, batch_seed)
    scale_rewards(batch, np.random.default_rng(batch_seed))
    return apex_agent(A, agent_seed, VR), batch, w


def _f64_apex(agent, batch, w):
    import torch

    a64 = copy.deepcopy(agent).double()
    per_sample, prio = a64.loss(to_f64_cpu(batch))
    loss = (per_sample * w.cpu().double()).mean()
    loss.backward()
    return float(loss.detach()), prio.numpy(), {k: p.grad.numpy() for k, p in a64.online_net.named_parameters()}


@pytest.mark.parametrize("B,precision", [(8, "f32"), (128, "bf16x2"), (128, "f32x3")])
def test_apex_learner_matches_the_float64_agent(B, precision):
    """Tolerances: those of tests/test_learner_gpu.py for the rescale-off step (priorities 1e-4 / 2e-4, loss 1e-4 / 1e-5,
    gradients 2e-3 / 2e-5 + 1e-3 of the largest entry; bf16x2 from 128 rows: relative L2 error 2e-2 and cosine 0.9998
    per tensor, as its test_learner_fast_mode_within_stated_tolerance).  At 128 rows the bf16x2 step runs its merged
    split-bf16 forward (asserted through the launch census); the f32x3 step keeps the f32 kernels below 512 rows and is
    held to the f32 bounds."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.learner import HipApexLearner
    from test_learner_gpu import ATOL, RTOL, _assert_fast_learner_kernels

    A = 6
    agent, batch, w = _apex_case(B, A, 3, 11)
    assert float(batch.reward.abs().max()) > 100
    loss64, prio64, g64 = _f64_apex(agent, batch, w)
    learner = HipApexLearner.from_agent(agent.to("cuda"), B)
    learner.set_precision(precision)
    with capi.launch_census() as census:
        loss, prio = learner.backward(batch, w)
    torch.cuda.synchronize()
    if precision == "bf16x2":
        _assert_fast_learner_kernels(census.counts, B)
    print("B=%d %s: priority |err| max %.3g (of %.3g), loss |err| %.3g (of %.4g)" % (
        B, precision, np.abs(prio.cpu().numpy() - prio64).max(), prio64.max(), abs(loss.item() - loss64), loss64))
    np.testing.assert_allclose(prio.cpu().numpy(), prio64, rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(loss.item(), loss64, rtol=1e-4, atol=1e-5)
    grads = learner.state_dict("grads")
    for key in HipApexLearner.KEYS:
        gr, rr = grads[key].cpu().double().numpy(), g64[key]
        if precision == "bf16x2":
            d, n0 = np.linalg.norm(gr - rr), np.linalg.norm(rr) + 1e-20
            cos = float((gr * rr).sum()) / (np.linalg.norm(gr) * n0 + 1e-30)
            assert d <= 2e-2 * n0 and cos > 0.9998, (key, d / n0, cos)
        else:
            scale = float(np.abs(rr).max()) + 1e-12
            np.testing.assert_allclose(gr, rr, rtol=RTOL, atol=ATOL + 1e-3 * scale, err_msg=key)
    assert capi.lib.rela_apex_learner_set_value_rescale(learner.h, 0.0) == capi.ESTATE  # 8
    learner.close()


def _r2d2_case(A, B, seq, burn, n, seed):
    from test_r2d2_learner_gpu import _random_batch

    for s in range(seed, seed + 64):  # the first seed whose batch has a padded sequence next to a full one
        rng = np.random.default_rng(s)
        batch, w = _random_batch(rng, A, B, seq, burn, n, "cuda:0")
        if float(batch.seq_len.min()) < burn + seq:
            return scale_rewards(batch, rng), w
    raise AssertionError("no padded sequence")


def test_r2d2_learner_matches_the_float64_agent():
    """A = 6, B = 3, seq 4, burn-in 2, n 2 with a padded sequence, at the tolerances of
    tests/test_r2d2_learner_gpu.py::test_hip_r2d2_learner_matches_reference_golden (the rescale-off test of this shape:
    loss per sequence and priority 1e-4 / 1e-5, total loss 1e-4, gradients 2e-3 of the largest entry)."""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.learner import HipR2D2Learner

    A, B, seq, burn, n = 6, 3, 4, 2, 2
    batch, w = _r2d2_case(A, B, seq, burn, n, 8)
    assert float(batch.reward.abs().max()) > 100
    agent = r2d2_agent(A, n, seq, burn, VR)
    a64 = copy.deepcopy(agent).double()
    per_seq, prio64 = a64.loss(to_f64_cpu(batch))
    loss64 = (per_seq * w.cpu().double()).mean()
    loss64.backward()
    learner = HipR2D2Learner.from_agent(agent.to("cuda:0"), B, grad_clip=1e9)
    loss, prio, loss_seq = learner.backward(batch, w)
    learner.check()
    torch.cuda.synchronize()
    print("r2d2: priority |err| max %.3g (of %.3g), loss per sequence |err| max %.3g (of %.4g)" % (
        np.abs(prio.cpu().numpy() - prio64.numpy()).max(), float(prio64.max()),
        np.abs(loss_seq.cpu().numpy() - per_seq.detach().numpy()).max(), float(per_seq.detach().max())))
    np.testing.assert_allclose(loss_seq.cpu().numpy(), per_seq.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(prio.cpu().numpy(), prio64.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(loss.cpu()[0]), float(loss64.detach()), rtol=1e-4)
    grads = learner.state_dict("grads")
    for key, p in a64.online_net.named_parameters():
        ref = p.grad.numpy()
        scale = float(np.abs(ref).max()) + 1e-12
        err = float(np.abs(grads[key].cpu().double().numpy() - ref).max())
        assert err <= 2e-3 * scale, (key, err, scale)
    assert capi.lib.rela_r2d2_learner_set_value_rescale(learner.h, 0.0) == capi.ESTATE  # 8
    learner.close()


def test_learners_with_eps_zero_equal_untouched_learners_bit_for_bit():
    import torch

    from rela_amd.learner import HipApexLearner, HipR2D2Learner

    A, B = 6, 8
    agent, batch, w = _apex_case(B, A, 3, 11)
    agent = agent.to("cuda")
    out = []
    for eps in (None, 0.0, -1.0, VR):
        learner = HipApexLearner(A, B, agent.multi_step, agent.gamma)  # (not from_agent: the setter is this test's)
        learner.load_state_dicts(agent.online_net.state_dict(), agent.target_net.state_dict())
        if eps is not None:
            learner.set_value_rescale(eps)
        loss, prio = learner.backward(batch, w)
        out.append((loss.clone(), prio.clone(), learner.flat()[1].clone()))
        learner.close()
    for other in out[1:3]:
        for x, y in zip(out[0], other):
            assert torch.equal(x, y)
    assert not torch.equal(out[0][1], out[3][1])
    A, B, seq, burn, n = 6, 3, 4, 2, 2
    batch, w = _r2d2_case(A, B, seq, burn, n, 8)
    agent = r2d2_agent(A, n, seq, burn, VR, "cuda:0")
    out = []
    for eps in (None, 0.0, VR):
        learner = HipR2D2Learner(A, B, n, agent.gamma, seq, burn, agent.eta, grad_clip=1e9)
        learner.load_state_dicts(agent.online_net.state_dict(), agent.target_net.state_dict())
        if eps is not None:
            learner.set_value_rescale(eps)
        loss, prio, loss_seq = learner.backward(batch, w)
        learner.check()
        out.append((loss.clone(), prio.clone(), loss_seq.clone(), learner.flat()[1].clone()))
        learner.close()
    for x, y in zip(out[0], out[1]):
        assert torch.equal(x, y)
    assert not torch.equal(out[0][1], out[2][1])


# ---- 7 ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mods():
    sys.path.insert(0, os.path.join(ROOT, "rela_amd", "pybind"))
    import torch  # noqa: F401
    import rela
    import synth_atari

    assert "rela_amd/pybind" in rela.__file__
    return rela, synth_atari


def _lockstep_with_learners(rela, synth_atari, value_rescale, writeback):
    """tests/e2e_lockstep.py:run_lockstep's loop for a cohort of 2 threads x 2 envs, with every sampled batch fed to the
    HIP learner and to the torch agent; `writeback` names whose priorities go back into the replay."""
    import torch

    from e2e_lockstep import CFG, _wait, load_agent_params
    from rela_amd.learner import HipApexLearner
    from rela_amd.pyrela.apex import ApexAgent
    from rela_amd.pyrela.net import AtariFFNet

    cfg = dict(CFG, K=2, threads=2)
    agent = load_agent_params(ApexAgent(lambda: AtariFFNet(cfg["num_action"]), cfg["multi_step"], cfg["gamma"],
                                        value_rescale), cfg).to("cuda:0")
    plain_agent = ApexAgent.clone(agent, "cuda:0")  # the same weights, the reference's target
    plain_agent.value_rescale = 0.0
    learner = HipApexLearner.from_agent(agent, cfg["batch"])
    ring = int(1.25 * cfg["capacity"])
    replay = rela.FFPrioritizedReplay(cfg["capacity"], cfg["seed"], cfg["alpha"], cfg["beta"], 0)
    locker = rela.ModelLocker([agent], "cuda:0")
    ctx = rela.Context()
    keep = []
    for t in range(cfg["threads"]):
        actor = rela.DQNActor(locker, cfg["multi_step"], cfg["K"], cfg["gamma"], replay)
        vec = rela.VectorEnv()
        for g in range(cfg["K"]):
            game = synth_atari.SyntheticAtariEnv(cfg["env_seed"] + t * cfg["K"] + g, 0.0, cfg["num_action"],
                                                 cfg["episode_len"])
            keep.append(game)
            vec.append(game)
        keep.append(actor)
        ctx.push_env_thread(rela.BasicThreadLoop(actor, vec, False))
    ctx.start()
    rounds = []
    for r in range(cfg["rounds"]):
        _wait(lambda: replay.size() == ring, "actor never filled the ring")
        batch, w = replay.sample(cfg["batch"], "cuda:0")
        _wait(lambda: replay.size() == ring, "parked block never landed")
        _, hip_prio = learner.loss(batch, w)
        with torch.no_grad():
            _, torch_prio = agent.loss(batch, sync_priority=False)
            _, plain_prio = plain_agent.loss(batch, sync_priority=False)
        s = batch.obs["s"].cpu().numpy().astype(np.int64)
        rounds.append(dict(s_sum=s.reshape(len(s), -1).sum(1).tolist(), a=batch.action["a"].cpu().tolist(),
                           terminal=[int(x) for x in batch.terminal.cpu().tolist()],
                           bootstrap=batch.bootstrap.cpu().tolist(), reward=batch.reward.cpu().tolist(),
                           num_add=replay.num_add(), weight=w.cpu().numpy().copy(),
                           hip=hip_prio.cpu().numpy().copy(), torch=torch_prio.cpu().numpy().copy(),
                           plain=plain_prio.cpu().numpy().copy()))
        replay.update_priority((hip_prio if writeback == "hip" else torch_prio).detach().cpu().clone())
    ctx.terminate()
    ctx.resume()
    t0 = time.time()
    while not ctx.terminated():  # the actors may be parked on the full ring: drain until they exit
        if replay.size() >= cfg["batch"]:
            replay.sample(cfg["batch"], "cuda:0")
            replay.update_priority(torch.ones(cfg["batch"]))
        time.sleep(0.005)
        if time.time() - t0 > 120:
            raise TimeoutError("context did not terminate")
    learner.close()
    return rounds


def test_lockstep_through_the_module_hip_and_torch_learner_agree(mods):
    """The priorities the HIP learner and the torch learner write back agree to the learner tolerance of test 5, the
    runs they steer sample the same rows (integer fields exactly), and the actors took the switch from the agent."""
    rela, synth = mods
    hip = _lockstep_with_learners(rela, synth, VR, "hip")
    tor = _lockstep_with_learners(rela, synth, VR, "torch")
    off = _lockstep_with_learners(rela, synth, 0.0, "hip")
    assert len(hip) == len(tor) == 6
    for r, (a, b) in enumerate(zip(hip, tor)):
        for key in ("s_sum", "a", "terminal", "bootstrap", "reward", "num_add"):
            assert a[key] == b[key], (r, key)
        for run in (a, b):
            np.testing.assert_allclose(run["hip"], run["torch"], rtol=1e-4, atol=2e-4, err_msg="round %d" % r)
        np.testing.assert_allclose(a["hip"], b["torch"], rtol=1e-4, atol=2e-4, err_msg="round %d" % r)
        np.testing.assert_allclose(a["weight"], b["weight"], rtol=1e-3)
    # The actors took the switch from the agent: before the first update_priority every row carries the priority its
    # actor gave it, and with alpha = beta = 1 the IS weight is min_j(p_j) / p_i -- so weight x (the learner's priority
    # of the same transition under the same, never updated, weights) is one constant over the batch exactly when the
    # actors formed the same target as the learner.  The plain learner's priorities do not fit the rescaled run's weights.
    spread = lambda v: float(np.ptp(v) / np.mean(v))
    assert spread(hip[0]["weight"] * hip[0]["hip"]) < 1e-3
    assert spread(off[0]["weight"] * off[0]["hip"]) < 1e-3
    assert spread(hip[0]["weight"] * hip[0]["plain"]) > 0.05


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_training_entry_point_runs_with_value_rescale(mods, capsys, algo):
    """main.py --value_rescale 1e-3 --hip_learner 1: a few steps of each algorithm"""
    from rela_amd.pyrela import main as entry

    argv = ["--algo", algo, "--value_rescale", "1e-3", "--hip_learner", "1", "--num_thread", "2", "--num_game_per_thread", "4",
            "--batchsize", "8", "--epoch_len", "6", "--num_epoch", "1", "--burn_in_frames", "16", "--replay_buffer_size", "64",
            "--episode_len", "30", "--actor_sync_freq", "3"]
    if algo == "r2d2":
        argv += ["--seq_len", "8", "--seq_burn_in", "4"]
    args = entry.parse_args(argv)
    assert args.value_rescale == 1e-3
    hist = entry.train(args)
    out = capsys.readouterr().out
    assert "'value_rescale': 0.001" in out and "Speed: train: " in out
    assert len(hist) == 1 and np.isfinite(hist[0]["loss"]) and hist[0]["act"] > 0
