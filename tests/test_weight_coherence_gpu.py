"""Derived weight copies stay coherent with the flat parameters, whatever an object has been through.

Both learners keep their weights once, in flat f32 buffers, and many times over in the forms the kernels read: the kernel
layouts of the online and target nets (csrc/ffnet_plan.h: B1 .. Bfe, Bl, bl, Wrec, Wx3), the Ape-X learner's own w2p, w3p,
wfcp, frag2, frag3 (csrc/learner.hip) and the R2D2 learner's wihT, whhT, bsum, wihp, wrec, wTrec, wx3
(csrc/learner_r2d2.hip).  They are refreshed in different places: by the re-pack after load / apply / sync_target, on
demand by the next forward that needs them (BfT), or lazily by comparing version counters (wrec / wTrec, wx3), and only
for the precision mode that is set at that moment.  A copy that lags one optimiser step behind moves Q by the order of
the learning rate, far inside every tolerance of the multi-step tests; one that is never refreshed only makes a layer
stop learning.

The rule checked here: an object that has been through ANY sequence of load / step / sync_target / set_precision /
publish computes, bit for bit, what a freshly built object computes after one load of the same flat weights.  Fresh
objects are pinned to the reference, to autograd and to float64 by the other test files; this file carries those
guarantees over to the states training runs in.

  probe    set_precision(mode) + backward(batch, w): changes no weight.  One probe per regime in which another layout
           is read (APEX_PROBES, R2D2_PROBES); each asserts through the launch census that its kernels really ran.
  event    changes weights or state of the long-lived learner (a step in some mode, sync_target, a second load).
After every event the long-lived learner and a fresh learner with the same constructor arguments (the same max_batch:
a net limited to fewer rows legitimately picks other fc kernels) run the whole probe list on the SAME batch tensors,
so that buffer adjacency, and with it the merged forwards, is the same.  The actor-side nets (FFNetHandle,
LSTMNetHandle) receive the learner's weights after every event, through publish and load_net_from_flat in turn.

Teeth (asserted): every tensor moves in every step event; activations stay alive; and for one checkpoint per learner a
probe learner that holds the current weights except for ONE tensor of the previous generation, on the online or the
target side, differs from the coherent one in at least one probe -- for every tensor of KEYS.  No tolerance anywhere:
every comparison is equality of bits."""
import ctypes as C
import functools

import pytest

from kernel_names import (CONV12, CONV12_JOBS, R2D2_BPTT_CHAIN, R2D2_BPTT_STEPS, R2D2_REC_CHAIN, R2D2_REC_STEPS,
                          SPLIT_BF16, X3_FFNET, X3_LSTM)

pytestmark = pytest.mark.gpu

A = 18
DEV = "cuda:0"


def _bits_equal(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _clone_sd(learner, which):
    return {k: v.clone() for k, v in learner.state_dict(which).items()}


def _assert_every_tensor_moved(before, after, what):
    for k in before:
        assert not _bits_equal(before[k], after[k]), "%s: %s did not move" % (what, k)


def _assert_same(got, want, what):
    for name, a, b in zip(got[0], got[1:], want[1:]):
        assert _bits_equal(a, b), "%s: %s of the long-lived object differs from the fresh one's" % (what, name)


def _differs(got, want):
    return any(not _bits_equal(a, b) for a, b in zip(got[1:], want[1:]))


def _assert_alive(prio, what):
    import torch

    assert bool(torch.isfinite(prio).all()) and float(prio.max() - prio.min()) > 0.0, what


# ---- Ape-X ----------------------------------------------------------------------------------------------------------
APEX_MAX_B = 2048  # ("f32", 2048) is the only way to gemm_mfma<GemmFc> and its layout Bf (csrc/ffnet_plan.h: kFcSplitBelow)
APEX_LR = 6.25e-5  # RMSprop's first steps move every weight by up to 10 lr: all tensors move, no layer dies (asserted)
AGENT_SEED, RELOAD_SEED = 41, 43
# (mode, B, s' right behind s): the regime each probe is there for
APEX_PROBES = (
    ("f32", 64, False),       # f32 trunk, f32 split-K fc over BfT
    ("f32", 2048, False),     # gemm_mfma<GemmFc> over Bf
    ("bf16x2", 128, False),   # merged 256-row forward: conv12_i8_jobs, conv3_bf16s_jobs, split-K fc_bf16s
    ("bf16x2", 1024, False),  # not merged: conv12_i8, fc_bf16s; the pass the backward reads stays f32 (BfT again)
    ("f32x3", 512, False),    # conv12_s3, conv3_img_s3, gemm_s3<fc>: three launches per layer
    ("f32x3", 512, True),     # the online net over [s ; s'] as one 1,024-row forward
    ("f32", 64, False),       # BfT on demand after the bf16x2 probes
)
_apex_batches = {}


def _apex_batch(B, adjacent=False):
    """one fixed batch per probe shape, the same tensor objects for every learner"""
    from test_learner_gpu import make_batch

    key = (B, adjacent)
    if key not in _apex_batches:
        _apex_batches[key] = make_batch(B, A, 1000 + B + int(adjacent), adjacent=adjacent)
    return _apex_batches[key]


def _behind(batch):
    so, sn = batch.obs["s"], batch.next_obs["s"]
    lo, ln = batch.obs["legal_move"], batch.next_obs["legal_move"]
    return sn.data_ptr() == so.data_ptr() + so.numel() and ln.data_ptr() == lo.data_ptr() + 4 * lo.numel()


def _assert_apex_census(counts, mode, B, batch, adjacent):
    from test_learner_gpu import _assert_fast_learner_kernels

    ran = set(counts)
    f32_trunk = {"conv1_bf16x3", "conv_mfma<Conv2> (f32)", "conv_mfma<Conv3> (f32)"}
    if mode == "f32":
        assert f32_trunk <= ran and not ((X3_FFNET | SPLIT_BF16) & ran), (mode, B, counts)
        if B >= 2048:
            assert counts.get("gemm_mfma<GemmFc> (f32)") == 3 and "fc_reduce" not in ran, (mode, B, counts)
        else:
            assert counts.get("fc_reduce") == 3 and "gemm_mfma<GemmFc> (f32)" not in ran, (mode, B, counts)
    elif mode == "bf16x2":
        _assert_fast_learner_kernels(counts, B)
        assert not (X3_FFNET & ran), (mode, B, counts)
        if B >= 1024:  # two gradient-free forwards on split-bf16 kernels, the third on the f32 ones
            assert counts.get("fc_bf16s") == 2 and counts.get(CONV12) == 2 and CONV12_JOBS not in ran, (mode, B, counts)
            assert f32_trunk <= ran and counts.get("fc_reduce") == 1, (mode, B, counts)
    else:
        behind = _behind(batch)
        assert behind or not adjacent
        assert X3_FFNET <= ran and not (SPLIT_BF16 & ran), (mode, B, counts)
        assert counts["conv12_s3"] == (2 if behind else 3), (mode, B, counts)


def _apex_probe(learner, probe, census=True):
    """-> (names, loss, priorities, flat gradient), cloned"""
    from rela_amd import _capi as capi

    mode, B, adjacent = probe
    batch, w = _apex_batch(B, adjacent)
    learner.set_precision(mode)
    if census:
        with capi.launch_census() as c:
            loss, prio = learner.backward(batch, w)
        _assert_apex_census(c.counts, mode, B, batch, adjacent)
    else:
        loss, prio = learner.backward(batch, w)
    return ("loss", "priority", "gradient"), loss.clone(), prio.clone(), learner.flat()[1].clone()


def _apex_agent(seed=AGENT_SEED):
    from test_learner_gpu import make_agent

    return make_agent(A, seed)


def _new_apex(agent, opt):
    from rela_amd.learner import HipApexLearner

    learner = HipApexLearner(A, APEX_MAX_B, agent.multi_step, agent.gamma, optimizer=opt, lr=APEX_LR, device=DEV)
    learner.set_value_rescale(getattr(agent, "value_rescale", 0.0))
    return learner


def _apex_step(mode, B):
    def event(live):
        live.set_precision(mode)
        live.step(*_apex_batch(B))

    return event


def _apex_reload(live):
    agent = _apex_agent(RELOAD_SEED)
    live.set_precision("bf16x2")  # the load itself then leaves BfT to the next f32 forward
    live.load_state_dicts(agent.online_net.state_dict(), agent.target_net.state_dict())


APEX_EVENTS = (
    ("step_f32_64", _apex_step("f32", 64), "online"),
    ("step_bf16x2_1024", _apex_step("bf16x2", 1024), "online"),
    ("step_f32x3_512", _apex_step("f32x3", 512), "online"),
    ("sync_target", lambda live: live.sync_target_with_online(), "target"),
    ("second_load", _apex_reload, "both"),
)


def _ffnet_forward(handle, s, legal):
    import torch

    from rela_amd import _capi as capi

    N = s.shape[0]
    q = torch.empty(N, A, device=DEV)
    nb = capi.lib.rela_ffnet_workspace_bytes(handle.h, N)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    capi.check(capi.lib.rela_ffnet_forward(handle.h, N, C.c_void_p(s.data_ptr()), C.c_void_p(legal.data_ptr()),
                                           C.c_void_p(q.data_ptr()), C.c_void_p(ws.data_ptr()), nb,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rela_ffnet_forward")
    torch.cuda.synchronize()
    return q


FFNET_ROWS = (40, 130, 512, 1030, 2050)
LSTM_ROWS = (5, 131, 515, 1030)  # (1,030 rows: the bf16x2 gate GEMM over Wrec, which starts at 1,024)
PRECISIONS = ("f32", "bf16x2", "f32x3")


@functools.lru_cache(maxsize=None)
def _actor_inputs():
    import numpy as np
    import torch

    from synth import synth_obs

    n = max(FFNET_ROWS)
    rng = np.random.default_rng(77)
    legal = (rng.uniform(size=(n, A)) < 0.85).astype(np.float32)
    legal[:, 0] = 1.0
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (to(synth_obs(n, 78)), to(legal), to(rng.normal(0, 0.3, (n, 512)).astype(np.float32)),
            to(rng.normal(0, 0.5, (n, 512)).astype(np.float32)))


def _ffnet_tables(handle):
    s, legal, _, _ = _actor_inputs()
    out = {}
    for mode in PRECISIONS:
        handle.set_precision(mode)
        for N in FFNET_ROWS:
            out[(mode, N)] = _ffnet_forward(handle, s[:N], legal[:N])
    return out


def _assert_ffnet_handle_coherent(live_net, online_sd, what):
    from rela_amd.engine import FFNetHandle

    fresh = FFNetHandle(A, DEV)
    fresh.load_state_dict(online_sd)
    got, want = _ffnet_tables(live_net), _ffnet_tables(fresh)
    fresh.close()
    for key in want:
        assert _bits_equal(got[key], want[key]), "%s: Q of the long-lived FFNetHandle, %s at %d rows" % ((what,) + key)


@pytest.mark.parametrize("opt", ["rmsprop", "adam"])
def test_apex_learner_equals_a_fresh_one_after_every_event(opt):
    """One long-lived HipApexLearner through steps in all three precision modes, sync_target and a second load (made
    while the mode is bf16x2); after each of them a fresh learner with the same weights must give the same bits in
    every probe, and so must the long-lived FFNetHandle the learner publishes to."""
    import torch

    from rela_amd.engine import FFNetHandle
    from rela_amd.learner import HipApexLearner, load_net_from_flat

    agent = _apex_agent()
    live = HipApexLearner.from_agent(agent, APEX_MAX_B, optimizer=opt, lr=APEX_LR)
    actor_net = FFNetHandle(A, DEV)
    for i, (name, event, moves) in enumerate(APEX_EVENTS):
        before = {w: _clone_sd(live, w) for w in ("online", "target")}
        event(live)
        on, tg = _clone_sd(live, "online"), _clone_sd(live, "target")
        for which in ("online", "target"):
            if moves in (which, "both"):
                _assert_every_tensor_moved(before[which], {"online": on, "target": tg}[which], "%s, %s" % (name, which))
        fresh = _new_apex(agent, opt)
        fresh.load_state_dicts(on, tg)
        for probe in APEX_PROBES:
            got, want = _apex_probe(live, probe), _apex_probe(fresh, probe)
            _assert_same(got, want, "after %s, probe %s" % (name, probe))
            _assert_alive(got[2], (name, probe))
            a3 = live.debug_activations()[2]
            assert float((a3 > 0).float().mean()) > 0.05, (name, probe)
        fresh.close()
        # the weights have not changed under the probes
        for k, v in live.state_dict("online").items():
            assert _bits_equal(v, on[k]), k
        if i % 2 == 0:
            live.publish(actor_net)
        else:
            load_net_from_flat(actor_net, live.flat()[0].clone(), A)
        _assert_ffnet_handle_coherent(actor_net, on, "after %s" % name)
    torch.cuda.synchronize()
    actor_net.close()
    live.close()


@pytest.mark.parametrize("opt", ["rmsprop", "adam"])
def test_apex_load_resets_the_optimiser_state(opt):
    """load after several steps, then one step: the same parameters as a fresh learner's load and step (a load zeroes
    S1 / S2 and Adam's step count, csrc/learner_common.h)."""
    agent = _apex_agent()
    from rela_amd.learner import HipApexLearner

    live = HipApexLearner.from_agent(agent, APEX_MAX_B, optimizer=opt, lr=APEX_LR)
    for _, event, _ in APEX_EVENTS[:3]:
        event(live)
    other = _apex_agent(RELOAD_SEED)
    W = (other.online_net.state_dict(), other.target_net.state_dict())
    fresh = _new_apex(agent, opt)
    out = []
    for learner in (live, fresh):
        learner.load_state_dicts(*W)
        learner.set_precision("f32")
        before = _clone_sd(learner, "online")
        learner.step(*_apex_batch(64))
        _assert_every_tensor_moved(before, learner.state_dict("online"), "step after load")
        out.append(learner.flat()[0].clone())
    assert _bits_equal(out[0], out[1])
    live.close()
    fresh.close()


@functools.lru_cache(maxsize=None)
def _apex_generations():
    """-> (online, target) of the long-lived learner after sync_target, and the generation before of either side: the
    online net one optimiser step earlier, the target net one sync earlier"""
    from rela_amd.learner import HipApexLearner

    live = HipApexLearner.from_agent(_apex_agent(), APEX_MAX_B, lr=APEX_LR)
    for _, event, _ in APEX_EVENTS[:2]:
        event(live)
    old_on = _clone_sd(live, "online")
    APEX_EVENTS[2][1](live)
    old_tg = _clone_sd(live, "target")
    APEX_EVENTS[3][1](live)
    cur = _clone_sd(live, "online"), _clone_sd(live, "target")
    live.close()
    return cur, (old_on, old_tg)


@pytest.mark.parametrize("side", ["online", "target"])
def test_apex_probes_see_one_stale_tensor(side):
    """The control of the test above: with ONE tensor of one net a generation behind -- every tensor of KEYS in turn --
    at least one probe gives other bits than with coherent weights."""
    from rela_amd.learner import HipApexLearner

    (on, tg), (old_on, old_tg) = _apex_generations()
    agent = _apex_agent()
    probe_learner = _new_apex(agent, "rmsprop")
    probe_learner.load_state_dicts(on, tg)
    coherent = [_apex_probe(probe_learner, p, census=False) for p in APEX_PROBES]
    cur, old = (on, old_on) if side == "online" else (tg, old_tg)
    for key in HipApexLearner.KEYS:
        assert not _bits_equal(cur[key], old[key]), key
        mixed = dict(cur)
        mixed[key] = old[key]
        probe_learner.load_state_dicts(mixed if side == "online" else on, mixed if side == "target" else tg)
        seen = [p for p, ref in zip(APEX_PROBES, coherent) if _differs(_apex_probe(probe_learner, p, census=False), ref)]
        print("stale %s %s: seen by %d of %d probes" % (side, key, len(seen), len(APEX_PROBES)))
        assert seen, "a stale %s %s passes every probe" % (side, key)
    probe_learner.close()


# ---- R2D2 -----------------------------------------------------------------------------------------------------------
SEQ, BURN, NSTEP = 3, 2, 2  # T = 7, as tests/r2d2_paths.py
R2D2_MAX_B = 129
R2D2_LR = 2.5e-4  # Adam moves every weight by about lr per step
R2D2_MODES = ("f32", "bf16x2", "f32x3", "f32x3_bwd")
# B = 5: 35 frames, the f32 trunk in every mode | 20: 140 frames, bf16x2's online trunk on records | 74: 518 frames, the
# split3 records and the three-part gate GEMM of f32x3 | 129 (once): the per-step BPTT
R2D2_PROBES = tuple((m, B) for B in (5, 20, 74) for m in R2D2_MODES) + (("f32x3_bwd", 129),)
STEP_B = 74  # the steps run where both rec_ver and x3_ver have a stale generation to lose
_r2d2_batches = {}


def _r2d2_batch(B):
    import r2d2_paths as P

    if B not in _r2d2_batches:
        _r2d2_batches[B] = P.make_batch(A, B, SEQ, BURN, NSTEP, 300 + B, DEV)
    return _r2d2_batches[B]


def _assert_r2d2_probe_census(counts, mode, B):
    from test_r2d2_learner_gpu import R2D2_FAST_KERNELS, R2D2_X3_MIN_FRAMES

    ran, frames = set(counts), (BURN + SEQ + NSTEP) * B
    if mode == "bf16x2":
        assert "gemm_rec64_nt" in ran and not (X3_LSTM & ran), (mode, B, counts)
        if frames >= 128:
            assert R2D2_FAST_KERNELS <= ran, (mode, B, counts)
        else:
            assert "conv1_bf16x3" in ran and not ({CONV12, CONV12_JOBS} & ran), (mode, B, counts)
    else:
        assert not (SPLIT_BF16 & ran), (mode, B, counts)
        x3 = mode != "f32" and frames >= R2D2_X3_MIN_FRAMES
        assert (X3_LSTM <= ran) if x3 else not (X3_LSTM & ran), (mode, B, counts)
        assert ("gemm_bf16x3" in ran) == (mode == "f32x3_bwd"), (mode, B, counts)
    # the recurrence: forward chains up to 64 rows, BPTT chains up to 128 (tests/r2d2_paths.py has the table)
    fwd = (R2D2_REC_CHAIN, R2D2_REC_STEPS) if B <= 64 else (R2D2_REC_STEPS, R2D2_REC_CHAIN)
    bptt = (R2D2_BPTT_CHAIN, R2D2_BPTT_STEPS) if B <= 128 else (R2D2_BPTT_STEPS, R2D2_BPTT_CHAIN)
    for runs, absent in (fwd, bptt):
        assert runs <= ran and not (absent & ran), (B, counts)


def _r2d2_probe(learner, probe, census=True):
    """-> (names, loss, priorities, loss per sequence, flat gradient), cloned; then check()"""
    from rela_amd import _capi as capi

    mode, B = probe
    batch, w = _r2d2_batch(B)
    learner.set_precision(mode)
    if census:
        with capi.launch_census() as c:
            loss, prio, loss_seq = learner.backward(batch, w)
        _assert_r2d2_probe_census(c.counts, mode, B)
    else:
        loss, prio, loss_seq = learner.backward(batch, w)
    names = ("loss", "priority", "loss_seq", "gradient")
    out = names, loss.clone(), prio.clone(), loss_seq.clone(), learner.flat()[1].clone()
    learner.check()
    return out


def _r2d2_agent():
    import r2d2_paths as P

    return P.case_agent("B129", DEV)


def _new_r2d2(agent):
    from rela_amd.learner import HipR2D2Learner

    learner = HipR2D2Learner(A, R2D2_MAX_B, agent.multi_step, agent.gamma, agent.seq_len, agent.burn_in, agent.eta,
                             lr=R2D2_LR, device=DEV)
    learner.set_value_rescale(getattr(agent, "value_rescale", 0.0))
    return learner


def _r2d2_step(mode):
    def event(live):
        live.set_precision(mode)
        live.step(*_r2d2_batch(STEP_B))
        live.check()

    return event


def _r2d2_reload(live):
    import torch

    from synth import synth_lstm_params

    sd = lambda seed: {k: torch.from_numpy(v) for k, v in synth_lstm_params(A, seed).items()}
    live.load_state_dicts(sd(73), sd(74))


R2D2_EVENTS = tuple(("step_" + m, _r2d2_step(m), "online") for m in R2D2_MODES) + (
    ("sync_target", lambda live: live.sync_target_with_online(), "target"),
    ("second_load", _r2d2_reload, "both"),
)


def _lstm_step(handle, N):
    import torch

    from rela_amd import _capi as capi

    s, legal, h_in, c_in = (x[:N] for x in _actor_inputs())
    out = [torch.empty((N, 512), device=DEV), torch.empty((N, 512), device=DEV), torch.empty((N, A), device=DEV),
           torch.empty((N, A), device=DEV)]
    nb = capi.lib.rela_lstmnet_workspace_bytes(handle.h, N)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    capi.check(capi.lib.rela_lstmnet_step(handle.h, N, p(s), p(legal), p(h_in), p(c_in), p(out[0]), p(out[1]), p(out[2]),
                                          p(out[3]), p(ws), nb, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "rela_lstmnet_step")
    torch.cuda.synchronize()
    return out  # h, c, q, advantages


def _lstm_tables(handle):
    out = {}
    for mode in PRECISIONS:
        handle.set_precision(mode)
        for N in LSTM_ROWS:
            out[(mode, N)] = _lstm_step(handle, N)
    return out


def _assert_lstm_handle_coherent(live_net, online_sd, what):
    from rela_amd.engine import LSTMNetHandle

    fresh = LSTMNetHandle(A, DEV)
    fresh.load_state_dict(online_sd)
    got, want = _lstm_tables(live_net), _lstm_tables(fresh)
    fresh.close()
    for key in want:
        for name, a, b in zip(("h", "c", "q", "adv"), got[key], want[key]):
            assert _bits_equal(a, b), "%s: %s of the long-lived LSTMNetHandle, %s at %d rows" % ((what, name) + key)


def test_r2d2_learner_equals_a_fresh_one_after_every_event():
    """One long-lived HipR2D2Learner through an Adam step in each of its four precision modes (at 518 frames, where the
    rec64 and three-part copies of W_ih are both in use), sync_target and a second load; after each of them a fresh
    learner with the same weights must give the same bits in every probe, and so must the long-lived LSTMNetHandle."""
    import torch

    from rela_amd.engine import LSTMNetHandle
    from rela_amd.learner import HipR2D2Learner

    agent = _r2d2_agent()
    live = HipR2D2Learner.from_agent(agent, R2D2_MAX_B, lr=R2D2_LR)
    actor_net = LSTMNetHandle(A, DEV)
    for name, event, moves in R2D2_EVENTS:
        before = {w: _clone_sd(live, w) for w in ("online", "target")}
        event(live)
        on, tg = _clone_sd(live, "online"), _clone_sd(live, "target")
        for which in ("online", "target"):
            if moves in (which, "both"):
                _assert_every_tensor_moved(before[which], {"online": on, "target": tg}[which], "%s, %s" % (name, which))
        fresh = _new_r2d2(agent)
        fresh.load_state_dicts(on, tg)
        for probe in R2D2_PROBES:
            got, want = _r2d2_probe(live, probe), _r2d2_probe(fresh, probe)
            _assert_same(got, want, "after %s, probe %s" % (name, probe))
            _assert_alive(got[2], (name, probe))
        fresh.close()
        for k, v in live.state_dict("online").items():
            assert _bits_equal(v, on[k]), k
        live.publish(actor_net)
        _assert_lstm_handle_coherent(actor_net, on, "after %s" % name)
    torch.cuda.synchronize()
    actor_net.close()
    live.close()


@functools.lru_cache(maxsize=None)
def _r2d2_generations():
    """as _apex_generations: the state after sync_target, the online net one Adam step and the target net one sync earlier"""
    from rela_amd.learner import HipR2D2Learner

    live = HipR2D2Learner.from_agent(_r2d2_agent(), R2D2_MAX_B, lr=R2D2_LR)
    for _, event, _ in R2D2_EVENTS[:3]:
        event(live)
    old_on = _clone_sd(live, "online")
    R2D2_EVENTS[3][1](live)
    old_tg = _clone_sd(live, "target")
    R2D2_EVENTS[4][1](live)
    cur = _clone_sd(live, "online"), _clone_sd(live, "target")
    live.close()
    return cur, (old_on, old_tg)


@pytest.mark.parametrize("side", ["online", "target"])
def test_r2d2_probes_see_one_stale_tensor(side):
    """The control of the test above, as test_apex_probes_see_one_stale_tensor."""
    from rela_amd.learner import HipR2D2Learner

    (on, tg), (old_on, old_tg) = _r2d2_generations()
    probe_learner = _new_r2d2(_r2d2_agent())
    probe_learner.load_state_dicts(on, tg)
    coherent = [_r2d2_probe(probe_learner, p, census=False) for p in R2D2_PROBES]
    cur, old = (on, old_on) if side == "online" else (tg, old_tg)
    for key in HipR2D2Learner.KEYS:
        assert not _bits_equal(cur[key], old[key]), key
        mixed = dict(cur)
        mixed[key] = old[key]
        probe_learner.load_state_dicts(mixed if side == "online" else on, mixed if side == "target" else tg)
        seen = [p for p, ref in zip(R2D2_PROBES, coherent) if _differs(_r2d2_probe(probe_learner, p, census=False), ref)]
        print("stale %s %s: seen by %d of %d probes" % (side, key, len(seen), len(R2D2_PROBES)))
        assert seen, "a stale %s %s passes every probe" % (side, key)
    probe_learner.close()
