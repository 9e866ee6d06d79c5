"""The learners' configurable update rules on the GPU (include/rela_amd.h, csrc/learner_common.h and .hip):
  rela_debug_optimizer_apply_opts   optimizer_apply with alpha / centered / betas: rmsprop_centered_update, and the two
                                    existing update kernels with other constants
  rela_debug_target_lerp            target_lerp, the kernel of the soft target update
  rela_*_learner_set_lr / _lr / _set_rmsprop / _set_adam_betas / _soft_update_target, through rela_amd/learner.py
  pyrela/main.py                    --rmsprop_* / --adam_beta* / --lr_* / --target_* through one short train() per algorithm
against tests/optim_rules_ref.py: the float32 restatements in the kernels' order BIT FOR BIT.  Every buffer of a tap call
sits in front of a guard float4 and every tap call's launch census is asserted.  tests/test_optim_rules_ref_cpu.py pins the
references, their bounds against float64 and torch, and the defects these tables catch."""
import ctypes as C

import numpy as np
import pytest

import optim_ref as R
import optim_rules_ref as Q
from test_optimizer_gpu import (A, GUARD, OPTS, WORKLOAD, _stream, assert_bits, bits, make_learner, pad_mask, ptr,
                                table_gradients, zeros)

pytestmark = pytest.mark.gpu

HP = R.hp32(R.TEST_HP)
CENTRED = {alpha: dict(Q.DEFAULTS, alpha=alpha, centered=True) for alpha in (0.99, 0.95)}
LERP_CENSUS = {"target_lerp": 1}


def census_of(opt, o):
    kernel = "adam_update" if opt == "adam" else "rmsprop_centered_update" if o["centered"] else "rmsprop_update"
    return {"sumsq_partial": 1, "clip_coef": 1, kernel: 1}


def tap(opt, p, g, s1, s2, stats, t, hp, o, abort=0):
    """rela_debug_optimizer_apply_opts on device tensors, in place; the census is asserted.  -> skip counter"""
    from rela_amd import _capi as capi

    skipped = C.c_uint(12345)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_optimizer_apply_opts(
            OPTS.index(opt), hp["lr"], hp["eps"], hp["clip"], t, p.numel(), ptr(p), ptr(g), ptr(s1), ptr(s2), ptr(stats), abort,
            C.byref(skipped), o["alpha"], int(o["centered"]), o["b1"], o["b2"], _stream()), "rela_debug_optimizer_apply_opts")
    assert census.counts == census_of(opt, o), census.counts
    return skipped.value


def guarded(arrays):
    """device copies of float32 arrays, each in front of one guard float4 of 2^60 -> (rooms, views)"""
    import torch

    rooms = [torch.full((np.asarray(x).size + 4,), GUARD, dtype=torch.float32, device="cuda") for x in arrays]
    views = [r[:r.numel() - 4] for r in rooms]
    for d, x in zip(views, arrays):
        d.copy_(torch.from_numpy(np.array(x, dtype=np.float32)))
    return rooms, views


def assert_guards(rooms):
    for r in rooms:
        assert bool((r[r.numel() - 4:] == GUARD).all()), "a kernel wrote past the end of a buffer"


def apply(opt, p, g, s1, s2, t, hp, o, abort=0, old_tap=False):
    """one apply of numpy float32 arrays on the device (old_tap: through rela_debug_optimizer_apply, whose census and
    signature stay as they were).  -> dict(p, s1, s2, norm, coef, skipped) of numpy values"""
    import torch

    from test_optimizer_gpu import CENSUS, tap as tap_defaults

    rooms, dev = guarded((p, g, s1, s2))
    stats = torch.full((2,), float("nan"), device="cuda")
    if old_tap:
        skipped, counts = tap_defaults(opt, dev[0], dev[1], dev[2], dev[3], stats, t, hp, abort)
        assert counts == CENSUS[opt], counts
    else:
        skipped = tap(opt, dev[0], dev[1], dev[2], dev[3], stats, t, hp, o, abort)
    assert np.array_equal(dev[1].cpu().numpy().view(np.int32), np.asarray(g, dtype=np.float32).view(np.int32))  # g is read only
    assert_guards(rooms)
    st = stats.cpu().numpy()
    return dict(p=dev[0].cpu().numpy(), s1=dev[2].cpu().numpy(), s2=dev[3].cpu().numpy(), norm=st[0], coef=st[1],
                skipped=skipped)


def dense_start(opt, n, seed):
    g = R.dense_grads(n, seed)
    return R.dense_params(opt, g, zeros(n), zeros(n), 0, HP["lr"], HP["eps"], HP["clip"], seed)


# ---- the centred kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", sorted(CENTRED))
@pytest.mark.parametrize("n4", Q.LENGTHS4)
def test_centred_tap_bit_for_bit(n4, alpha):
    """from the zero state, then 12 applies carrying the device's own state next to the float32 form's"""
    import torch

    o, n, seed = CENTRED[alpha], 4 * n4, R.dense_seed(n4)
    p = dense_start("rmsprop", n, seed)
    g = R.dense_grads(n, seed)
    got = apply("rmsprop", p, g, zeros(n), zeros(n), 0, HP, o)
    assert_bits(got, Q.step_f32("rmsprop", p, g, zeros(n), zeros(n), 0, **HP, **o), "n4 %d alpha %g zero state" % (n4, alpha))
    assert got["s2"].any()  # the centred form does keep its gradient average in S2
    ref = dict(p=p, s1=zeros(n), s2=zeros(n))
    rooms, (dp, dg, ds1, ds2) = guarded((p, g, ref["s1"], ref["s2"]))
    stats = torch.zeros(2, device="cuda")
    for k in range(12):
        g = R.dense_grads(n, seed, k)
        dg.copy_(torch.from_numpy(g))
        assert tap("rmsprop", dp, dg, ds1, ds2, stats, 0, HP, o) == 0
        ref = Q.step_f32("rmsprop", ref["p"], g, ref["s1"], ref["s2"], 0, **HP, **o)
        st = stats.cpu().numpy()
        got = dict(p=dp.cpu().numpy(), s1=ds1.cpu().numpy(), s2=ds2.cpu().numpy(), norm=st[0], coef=st[1])
        assert_bits(got, ref, "n4 %d alpha %g apply %d" % (n4, alpha, k))
    assert_guards(rooms)


def test_constant_gradients_stay_finite_for_600_applies():
    """1,024 gradients that never change, alpha 0.95: s - m * m goes negative on the way (the float32 form shows where) and
    the clamp keeps every weight finite; the device equals the float32 form at every apply"""
    import torch

    n, o = 1024, dict(Q.DEFAULTS, **Q.PUBLISHED)
    g = Q.constant_grads(n)
    p = dense_start("rmsprop", n, 8)
    ref = dict(p=p, s1=zeros(n), s2=zeros(n))
    rooms, (dp, dg, ds1, ds2) = guarded((p, g, ref["s1"], ref["s2"]))
    stats = torch.zeros(2, device="cuda")
    clamped = np.zeros(n, dtype=bool)
    for k in range(600):
        assert tap("rmsprop", dp, dg, ds1, ds2, stats, 0, HP, o) == 0
        ref = Q.step_f32("rmsprop", ref["p"], g, ref["s1"], ref["s2"], 0, **HP, **o)
        clamped |= (ref["s1"] - ref["s2"] * ref["s2"]) < 0
        st = stats.cpu().numpy()
        got = dict(p=dp.cpu().numpy(), s1=ds1.cpu().numpy(), s2=ds2.cpu().numpy(), norm=st[0], coef=st[1])
        assert np.isfinite(got["p"]).all() and np.isfinite(got["s1"]).all() and np.isfinite(got["s2"]).all(), k
        assert_bits(got, ref, "constant gradients, apply %d" % k)
    assert_guards(rooms)
    assert clamped.sum() >= 1, "the table does not reach the hazard it is there for"
    print("the clamp held in %d of %d elements" % (int(clamped.sum()), n))


# ---- old and new taps ------------------------------------------------------------------------------------------------------------
N4_SMALL = 257


def test_plain_rmsprop_with_another_alpha():
    n, o = 4 * N4_SMALL, dict(Q.DEFAULTS, alpha=0.95)
    p = dense_start("rmsprop", n, 31)
    s1, s2 = zeros(n), zeros(n)
    for k in range(2):
        g = R.dense_grads(n, 31, k)
        got = apply("rmsprop", p, g, s1, s2, 0, HP, o)
        assert_bits(got, Q.step_f32("rmsprop", p, g, s1, s2, 0, **HP, **o), "alpha 0.95 apply %d" % k)
        assert not got["s2"].any()  # plain RMSprop never touches S2
        p, s1 = got["p"], got["s1"]
    assert not R.same_bits(got["p"], apply("rmsprop", p, g, s1, s2, 0, HP, Q.DEFAULTS)["p"])  # (alpha does take part)


@pytest.mark.parametrize("opt,t", [("rmsprop", 0), ("adam", 0), ("adam", 9)])
def test_new_tap_with_the_defaults_is_the_old_tap(opt, t):
    n = 4 * N4_SMALL
    p = dense_start(opt, n, 32)
    s1, s2 = zeros(n), zeros(n)
    for k in range(2):
        g = R.dense_grads(n, 32, k)
        new = apply(opt, p, g, s1, s2, t + k, HP, Q.DEFAULTS)
        old = apply(opt, p, g, s1, s2, t + k, HP, None, old_tap=True)
        assert_bits(new, old, "%s t %d apply %d" % (opt, t, k))
        assert new["skipped"] == old["skipped"] == 0
        p, s1, s2 = new["p"], new["s1"], new["s2"]


@pytest.mark.parametrize("t", [0, 9])
def test_adam_with_other_betas(t):
    n, o = 4 * N4_SMALL, dict(Q.DEFAULTS, b1=0.5, b2=0.9)
    p = dense_start("adam", n, 33)
    s1, s2 = zeros(n), zeros(n)
    for k in range(2):
        g = R.dense_grads(n, 33, k)
        got = apply("adam", p, g, s1, s2, t + k, HP, o)
        assert_bits(got, Q.step_f32("adam", p, g, s1, s2, t + k, **HP, **o), "betas 0.5 / 0.9, t %d apply %d" % (t, k))
        p, s1, s2 = got["p"], got["s1"], got["s2"]
    assert not R.same_bits(got["p"], apply("adam", p, g, s1, s2, t + 1, HP, Q.DEFAULTS)["p"])


# ---- abort, NaN, arguments -------------------------------------------------------------------------------------------------------
def test_abort_word_and_nan_gradient_in_the_centred_kernel():
    n, o = 4 * N4_SMALL, CENTRED[0.95]
    p = dense_start("rmsprop", n, 34)
    first = apply("rmsprop", p, R.dense_grads(n, 34), zeros(n), zeros(n), 0, HP, o)
    g1 = R.dense_grads(n, 34, 1)
    got = apply("rmsprop", first["p"], g1, first["s1"], first["s2"], 0, HP, o, abort=1)
    assert got["coef"] == -1.0 and got["skipped"] == 1 and first["skipped"] == 0
    assert R.same_bits(got["norm"], R.clip_f32(g1, HP["clip"])[0])
    for k in ("p", "s1", "s2"):
        assert R.same_bits(got[k], first[k]), k
    # a NaN gradient: the norm and the coefficient are NaN and so is every weight -- its own included
    g1[6] = np.nan
    got = apply("rmsprop", first["p"], g1, first["s1"], first["s2"], 0, HP, o)
    assert np.isnan(got["norm"]) and np.isnan(got["coef"]) and np.isnan(got["p"]).all()
    # a NaN that sits in the element's own state while the coefficient is finite: the clamp (a comparison) lets it through
    s2 = first["s2"].copy()
    s2[6] = np.nan
    g1[6] = 1.0
    got = apply("rmsprop", first["p"], g1, first["s1"], s2, 0, HP, o)
    assert np.isnan(got["p"][6]) and np.isfinite(np.delete(got["p"], 6)).all()
    assert_bits(got, Q.step_f32("rmsprop", first["p"], g1, first["s1"], s2, 0, **HP, **o), "NaN state")


def test_bad_options_are_refused_before_anything_is_launched():
    import torch

    from rela_amd import _capi as capi

    lib = capi.lib
    buf = [torch.zeros(64, device="cuda") for _ in range(5)]
    buf[1].fill_(1.0)  # gradients that would move every weight
    nan = float("nan")

    def call(alpha=0.99, centered=0, b1=0.9, b2=0.999, optimizer=0, n=32):
        with capi.launch_census() as census:
            rc = lib.rela_debug_optimizer_apply_opts(optimizer, 1e-3, 1.5e-4, 40.0, 0, n, *[ptr(b) for b in buf], 0, None, alpha,
                                                     centered, b1, b2, None)
        return rc, census.counts

    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=-0.5), dict(alpha=nan), dict(centered=2), dict(centered=-1),
               dict(b1=-0.1), dict(b1=1.0), dict(b1=nan), dict(b2=0.0), dict(b2=1.0), dict(b2=nan), dict(n=30),
               dict(optimizer=2)):
        assert call(**kw) == (capi.EINVAL, {}), kw
    assert not bool(buf[0].any()) and not bool(buf[2].any()) and not bool(buf[3].any())
    # (b1 = 0 is in range, and an accepted call does move the n weights it was given)
    assert call(b1=0.0)[0] == capi.OK and bool(buf[0][:32].all()) and not bool(buf[0][32:].any())
    pt, p = torch.zeros(64, device="cuda"), torch.ones(64, device="cuda")
    for n, tau, a, b in ((0, 0.5, pt, p), (30, 0.5, pt, p), (32, 0.0, pt, p), (32, 1.5, pt, p), (32, nan, pt, p),
                         (32, 0.5, None, p), (32, 0.5, pt, None), (32, 0.5, pt[1:], p), (32, 0.5, pt, p[1:])):
        with capi.launch_census() as census:
            rc = lib.rela_debug_target_lerp(n, tau, None if a is None else ptr(a), None if b is None else ptr(b), None)
        assert (rc, census.counts) == (capi.EINVAL, {}), (n, tau)
    assert not bool(pt.any())
    torch.cuda.synchronize()


# ---- the soft target update's kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n4", Q.LENGTHS4)
def test_lerp_tap_bit_for_bit(n4):
    from rela_amd import _capi as capi

    n = 4 * n4
    pt, p = Q.lerp_tables(n, n4)
    for tau in Q.TAUS:
        rooms, (dpt, dp) = guarded((pt, p))
        with capi.launch_census() as census:
            capi.check(capi.lib.rela_debug_target_lerp(n, tau, ptr(dpt), ptr(dp), _stream()), "rela_debug_target_lerp")
        assert census.counts == LERP_CENSUS, census.counts
        assert_guards(rooms)
        want = Q.lerp_f32(pt, p, tau)
        assert R.same_bits(dpt.cpu().numpy(), want), (n4, tau, float(R.ulps(dpt.cpu().numpy(), want).max()))
        assert np.array_equal(dp.cpu().numpy().view(np.int32), p.view(np.int32))  # p is read only
        assert not R.same_bits(want, pt)


# ---- through the learners --------------------------------------------------------------------------------------------------------
def rc_of(learner, name, *args):
    from rela_amd import _capi as capi

    return getattr(capi.lib, learner._PREFIX + name)(learner.h, *args)


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_options_and_lr_through_the_learner(algo):
    """set_rmsprop(0.95, True), three apply() calls on dense gradient tables against three tap calls on copies; set_lr
    between applies; the setters' timing and refusals"""
    import torch

    from rela_amd import _capi as capi

    learner, layout, total = make_learner(algo, "rmsprop")
    pads = pad_mask(layout, total)
    o = dict(Q.DEFAULTS, **Q.PUBLISHED)
    nan = float("nan")
    assert np.float32(learner.lr) == np.float32(WORKLOAD["lr"])
    for bad in ((0.0, 0), (1.0, 1), (nan, 1), (0.95, 2)):  # refused, and nothing changes
        assert rc_of(learner, "set_rmsprop", *bad) == capi.EINVAL, bad
    assert rc_of(learner, "set_adam_betas", 0.5, 0.9) == capi.EINVAL and b"RMSprop" in capi.lib.rela_last_error()
    for bad in (-1e-3, nan, float("inf")):
        assert rc_of(learner, "set_lr", bad) == capi.EINVAL, bad
    assert rc_of(learner, "lr", None) == capi.EINVAL
    target = learner.flat_target().clone()
    for bad in (0.0, -0.1, 1.5, nan):
        assert rc_of(learner, "soft_update_target", bad, None) == capi.EINVAL, bad
    torch.cuda.synchronize()
    assert torch.equal(bits(learner.flat_target()), bits(target))
    assert np.float32(learner.lr) == np.float32(WORKLOAD["lr"])
    learner.set_rmsprop(0.95, True)
    P, G = learner.flat()
    S1, S2, _ = learner.debug_optim()
    tp, ts1, ts2, stats = P.clone(), S1.clone(), S2.clone(), torch.zeros(2, device="cuda")
    hp = dict(WORKLOAD)
    for k in range(3):
        if k == 2:  # takes effect at the next apply, and touches nothing else
            before = [x.clone() for x in (P, S1, S2)]
            hp["lr"] = float(np.float32(WORKLOAD["lr"] / 3))
            learner.set_lr(hp["lr"])
            torch.cuda.synchronize()
            assert np.float32(learner.lr) == np.float32(hp["lr"])
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip((P, S1, S2), before))
        g = table_gradients(total, pads, 70, k)
        G.copy_(g)
        learner.apply()
        assert tap("rmsprop", tp, g, ts1, ts2, stats, 0, hp, o) == 0
        torch.cuda.synchronize()
        for name, own, mine in (("P", P, tp), ("S1", S1, ts1), ("S2", S2, ts2), ("stats", learner.stats(), stats)):
            assert torch.equal(bits(own), bits(mine)), (k, name)
    assert bool(S2.any()) and float(stats[1]) < 1
    for name, buf in (("P", P), ("S1", S1), ("S2", S2)):
        assert not bool(buf[torch.from_numpy(pads).cuda()].any()), name
    # after the first apply the options are fixed ...
    assert rc_of(learner, "set_rmsprop", 0.9, 0) == capi.ESTATE and b"before the first apply" in capi.lib.rela_last_error()
    learner.set_lr(WORKLOAD["lr"])  # (the learning rate is not)
    # ... until a load, which resets the state and keeps options and learning rate
    learner.load_state_dicts({k: v.clone() for k, v in learner.state_dict("online").items()})
    assert not bool(S1.any()) and not bool(S2.any()) and np.float32(learner.lr) == np.float32(WORKLOAD["lr"])
    tp, ts1, ts2 = P.clone(), S1.clone(), S2.clone()
    g = table_gradients(total, pads, 70, 3)
    G.copy_(g)
    learner.apply()
    assert tap("rmsprop", tp, g, ts1, ts2, stats, 0, WORKLOAD, o) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(P), bits(tp)) and torch.equal(bits(S2), bits(ts2))  # still centred with alpha 0.95
    learner.load_state_dicts({k: v.clone() for k, v in learner.state_dict("online").items()})
    learner.set_rmsprop(0.99, False)  # accepted again
    G.copy_(g)
    learner.apply()
    torch.cuda.synchronize()
    assert not bool(S2.any())
    learner.close()


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_adam_betas_through_the_learner(algo):
    import torch

    from rela_amd import _capi as capi

    learner, layout, total = make_learner(algo, "adam")
    pads = pad_mask(layout, total)
    o = dict(Q.DEFAULTS, b1=0.5, b2=0.9)
    assert rc_of(learner, "set_rmsprop", 0.95, 1) == capi.EINVAL and b"Adam" in capi.lib.rela_last_error()
    for bad in ((1.0, 0.9), (-0.1, 0.9), (0.5, 0.0), (0.5, 1.0), (float("nan"), 0.9), (0.5, float("nan"))):
        assert rc_of(learner, "set_adam_betas", *bad) == capi.EINVAL, bad
    learner.set_adam_betas(0.5, 0.9)
    P, G = learner.flat()
    S1, S2, _ = learner.debug_optim()
    tp, ts1, ts2, stats = P.clone(), S1.clone(), S2.clone(), torch.zeros(2, device="cuda")
    for k in range(3):
        g = table_gradients(total, pads, 71, k)
        G.copy_(g)
        learner.apply()
        assert tap("adam", tp, g, ts1, ts2, stats, k, WORKLOAD, o) == 0
        torch.cuda.synchronize()
        for name, own, mine in (("P", P, tp), ("S1", S1, ts1), ("S2", S2, ts2), ("stats", learner.stats(), stats)):
            assert torch.equal(bits(own), bits(mine)), (k, name)
    assert learner.debug_optim()[2] == 3
    assert rc_of(learner, "set_adam_betas", 0.9, 0.999) == capi.ESTATE
    learner.close()


def fresh_learner(algo):
    """an unloaded learner of make_learner's shapes"""
    from rela_amd.learner import HipApexLearner, HipR2D2Learner

    return HipApexLearner(A, 4, 3, 0.99) if algo == "apex" else HipR2D2Learner(A, 4, 2, 0.997, 7, 0, 0.9)


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_soft_target_update_is_the_lerp_of_the_flat_buffers(algo):
    """two applies move the online net off the target; soft_update_target(tau) then leaves lerp_f32(target, online) in the
    target, tensor by tensor and pads included, and the online net alone"""
    import torch

    from rela_amd import _capi as capi

    unloaded = fresh_learner(algo)
    assert rc_of(unloaded, "soft_update_target", 0.5, None) == capi.ESTATE
    unloaded.close()
    learner, layout, total = make_learner(algo, "rmsprop" if algo == "apex" else "adam", hp=HP)
    pads = torch.from_numpy(pad_mask(layout, total)).cuda()
    P, G = learner.flat()
    PT = learner.flat_target()
    # gradients of one magnitude (0.5 .. 2, either sign) in every element, so that two applies move every weight by about
    # 10 lr (RMSprop) / lr (Adam) each and a 2^-10 th of that distance is still tens of ulps of any weight below 1,
    # the one-element tensors included (the dense tables hold zeros and 1e-12s: a tensor of one element could stay put)
    rng = np.random.default_rng(72)
    for k in range(2):
        g = torch.from_numpy((rng.uniform(0.5, 2.0, total) * rng.choice([-1.0, 1.0], total)).astype(np.float32)).cuda()
        g[pads] = 0
        G.copy_(g)
        learner.apply()
    for tau in (0.005, 2.0 ** -10):
        torch.cuda.synchronize()
        online = {k: v.clone() for k, v in learner.state_dict("online").items()}
        before = {k: v.clone() for k, v in learner.state_dict("target").items()}
        flat_before, p_before = PT.clone(), P.clone()
        learner.soft_update_target(tau)
        torch.cuda.synchronize()
        after = learner.state_dict("target")
        for key in before:
            want = Q.lerp_f32(before[key].cpu().numpy(), online[key].cpu().numpy(), tau)
            assert R.same_bits(after[key].cpu().numpy(), want), (tau, key)
            assert not torch.equal(bits(after[key]), bits(before[key])), (tau, key, "did not move")
            assert torch.equal(bits(learner.state_dict("online")[key]), bits(online[key])), (tau, key)
        assert R.same_bits(PT.cpu().numpy(), Q.lerp_f32(flat_before.cpu().numpy(), p_before.cpu().numpy(), tau))
        assert torch.equal(bits(P), bits(p_before))
        assert int(pads.sum()) > 0 and not bool(bits(PT)[pads].any()) and not bool(bits(P)[pads].any())  # +0, bit for bit
    learner.soft_update_target(1.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(PT), bits(P))
    learner.close()


# ---- the target's derived copies after a soft update -----------------------------------------------------------------------------
def _pair(algo):
    """-> (make: () -> a learner with fixed constructor arguments, not loaded; agent; batch; weights; precision modes)"""
    import torch

    from rela_amd.learner import HipApexLearner, HipR2D2Learner

    with torch.random.fork_rng(devices=[0]):
        torch.manual_seed(7007)
        if algo == "apex":
            from test_learner_gpu import make_agent, make_batch

            B = 32
            agent = make_agent(A, 5)
            batch, w = make_batch(B, A, 4)
            make = lambda: HipApexLearner(A, B, agent.multi_step, agent.gamma, optimizer="rmsprop", lr=1e-4)
            modes = ("f32", "bf16x2", "f32x3")
        else:
            from test_r2d2_learner_gpu import _agent, _random_batch

            B, seq, burn, n = 5, 7, 0, 2
            agent = _agent(A, n, 0.997, 0.9, seq, burn, 71, 72, "cuda:0")
            batch, w = _random_batch(np.random.default_rng(7007), A, B, seq, burn, n, "cuda:0")
            make = lambda: HipR2D2Learner(A, B, n, 0.997, seq, burn, 0.9, optimizer="adam", lr=1e-4)
            modes = ("f32", "bf16x2", "f32x3", "f32x3_bwd")
    return make, agent, batch, w, modes


def _probe(learner, batch, w):
    import torch

    out = learner.backward(batch, w)
    if hasattr(learner, "check"):
        learner.check()
    torch.cuda.synchronize()
    return out[0].clone(), out[1].clone(), learner.flat()[1].clone()


@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_derived_copies_follow_a_soft_update(algo):
    """two steps, one soft update: the long-lived learner then computes, in every precision mode, what a fresh learner
    loaded with its online and target tensors computes -- so the target's kernel-layout copies were re-packed from the
    moved target -- and its priorities are no longer the ones from before the update"""
    import torch

    make, agent, batch, w, modes = _pair(algo)
    for mode in modes:
        live = make()
        live.load_state_dicts(agent.online_net.state_dict(), agent.target_net.state_dict())
        live.set_precision(mode)
        for _ in range(2):
            live.step(batch, w)
        prio_before = _probe(live, batch, w)[1]
        live.soft_update_target(0.25)
        got = _probe(live, batch, w)
        fresh = make()
        fresh.load_state_dicts({k: v.clone() for k, v in live.state_dict("online").items()},
                               {k: v.clone() for k, v in live.state_dict("target").items()})
        fresh.set_precision(mode)
        want = _probe(fresh, batch, w)
        for name, a, b in zip(("loss", "priority", "gradient"), got, want):
            assert torch.equal(bits(a), bits(b)), "%s %s: %s of the long-lived learner differs from the fresh one's" % (
                algo, mode, name)
        assert bool(torch.isfinite(got[1]).all()) and not torch.equal(bits(got[1]), bits(prio_before)), (algo, mode)
        live.close()
        fresh.close()


# ---- the training entry point ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["apex", "r2d2"])
def test_training_entry_point_with_the_new_rules(algo, monkeypatch, capsys):
    """one short train() in the shape of tests/test_e2e_gpu.py's entry-point tests with the new flags: after every epoch the
    learner's learning rate is lr_at of the epoch's last update; the target net is a soft copy: it equals neither the
    online net nor what it was"""
    import os
    import sys

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rela_amd", "pybind"))
    from rela_amd import learner as learner_mod
    from rela_amd.pyrela import main as entry
    from rela_amd.pyrela.utils import lr_at

    lr, epoch_len, epochs = 6.25e-5, 3, 3
    common = ["--lr", str(lr), "--target_tau", "0.01", "--lr_warmup_updates", "2", "--lr_decay_updates", "4", "--lr_final",
              repr(lr / 4), "--epoch_len", str(epoch_len), "--num_epoch", str(epochs), "--num_thread", "2"]
    if algo == "apex":
        cls = learner_mod.HipApexLearner
        argv = ["--num_game_per_thread", "8", "--batchsize", "32", "--burn_in_frames", "64", "--replay_buffer_size", "512",
                "--episode_len", "25", "--actor_sync_freq", "5", "--rmsprop_centered", "1", "--rmsprop_alpha", "0.95"]
    else:
        cls = learner_mod.HipR2D2Learner
        argv = ["--algo", "r2d2", "--num_game_per_thread", "4", "--batchsize", "8", "--burn_in_frames", "16",
                "--replay_buffer_size", "64", "--episode_len", "30", "--actor_sync_freq", "3", "--seq_len", "8",
                "--seq_burn_in", "4", "--priority_exponent", "0.9", "--importance_exponent", "0.6", "--adam_beta1", "0.5"]
    args = entry.parse_args(argv + common)
    seen = {}
    original = cls.from_agent.__func__

    def from_agent(klass, agent, *a, **kw):
        seen["kw"] = dict(kw)
        seen["learner"] = original(klass, agent, *a, **kw)
        seen["start"] = {which: {k: v.clone() for k, v in seen["learner"].state_dict(which).items()}
                         for which in ("online", "target")}
        return seen["learner"]

    monkeypatch.setattr(cls, "from_agent", classmethod(from_agent))
    rates = []

    def on_epoch(entry_):
        last = (entry_["epoch"] + 1) * epoch_len - 1
        want = lr_at(last, lr, 2, lr / 4, 4)
        assert entry_["lr"] == want and np.float32(seen["learner"].lr) == np.float32(want), (last, entry_["lr"], want)
        rates.append(want)

    # (train() seeds torch's global generators: forked, so that the tests after this one see the streams they would see
    # without it)
    with torch.random.fork_rng(devices=[0]):
        hist = entry.train(args, on_epoch=on_epoch)
    out = capsys.readouterr().out
    assert out.count("--num_update_between_sync 2500 is ignored") == 1
    assert len(hist) == epochs and all(np.isfinite(h["loss"]) for h in hist)
    assert rates[0] == lr and lr / 4 < rates[1] < lr and rates[2] == lr / 4  # updates 2, 5 and 8 of the schedule
    if algo == "apex":
        assert seen["kw"]["alpha"] == 0.95 and seen["kw"]["centered"] is True
        assert bool(seen["learner"].debug_optim()[1].any())  # the gradient average of the centred form
    else:
        assert seen["kw"]["betas"] == (0.5, 0.999)
    torch.cuda.synchronize()
    online, target = (seen["learner"].state_dict(which) for which in ("online", "target"))
    for key in online:
        assert not torch.equal(bits(target[key]), bits(online[key])), key
        assert not torch.equal(bits(target[key]), bits(seen["start"]["target"][key])), key
        assert not torch.equal(bits(target[key]), bits(seen["start"]["online"][key])), key  # (the whole copy of update 0)
