"""tests/optim_rules_ref.py on the CPU: the references of tests/test_optim_rules_gpu.py.
  a. generalisation: with alpha 0.99, not centred and betas 0.9 / 0.999 the restatements and bounds are optim_ref's;
  b. the float32 form stays within the bound counted from its roundings (centred RMSprop at alpha 0.99 and 0.95, Adam with
     betas 0.5 / 0.9, the soft target update);
  c. the float64 form against torch.optim.RMSprop(centered=True) / Adam(betas) in float64 within the bound at u = 2^-53,
     counted for both sides (two_forms_bound);
  d. the constant-gradient table: s - m * m does go negative in float32, and the clamped form stays finite;
  e. every restated defect changes bits on some table;
  f. lr_at."""
import numpy as np
import pytest
import torch

import optim_ref as R
import optim_rules_ref as Q

N = 4096
STEPS = 12
HP = R.hp32(R.TEST_HP)
CASES = [("rmsprop", dict(alpha=0.99, centered=True)), ("rmsprop", dict(alpha=0.95, centered=True)),
         ("adam", dict(b1=0.5, b2=0.9))]
IDS = ["centred-0.99", "centred-0.95", "adam-0.5-0.9"]


def zeros32(n=N):
    return np.zeros(n, dtype=np.float32)


def options(opts):
    o = dict(Q.DEFAULTS, **opts)
    return o, Q.kernel_consts(o["alpha"], o["b1"], o["b2"])


def averaged_state(opt, o, consts, s1, s2):
    """(the state that averages gradients, its decay, one minus it), or Nones for plain RMSprop"""
    if opt == "adam":
        return s1, consts["b1"], consts["one_m_b1"]
    return (s2, consts["alpha"], consts["one_m_alpha"]) if o["centered"] else (None, None, None)


# ---- a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["rmsprop", "adam"])
def test_defaults_are_optim_ref_bit_for_bit(opt):
    """12 applies on optim_ref's dense tables, state carried: the new float32 form with the default options IS optim_ref's,
    and so are the constants and the bound"""
    assert Q.kernel_consts() == R.KERNEL_CONSTS and Q.torch_consts() == R.TORCH_CONSTS
    for clip in (HP["clip"], 1e9):
        g0 = R.dense_grads(N, 3)
        p, s1, s2 = R.dense_params(opt, g0, zeros32(), zeros32(), 0, HP["lr"], HP["eps"], clip, 3), zeros32(), zeros32()
        for k in range(STEPS):
            g = R.dense_grads(N, 3, k)
            old = R.step_f32(opt, p, g, s1, s2, k, HP["lr"], HP["eps"], clip)
            new = Q.step_f32(opt, p, g, s1, s2, k, HP["lr"], HP["eps"], clip, **Q.DEFAULTS)
            for key in ("p", "s1", "s2", "norm", "coef"):
                assert R.same_bits(old[key], new[key]), (opt, clip, k, key)
            ref = R.step_f64(opt, p, g, s1, s2, k, HP["lr"], HP["eps"], clip, R.KERNEL_CONSTS)
            a_abs = Q.a_abs_of(s1, g, ref["coef"], R.KERNEL_CONSTS["b1"], R.KERNEL_CONSTS["one_m_b1"])
            theirs = R.f32_bound(opt, ref, a_abs, R.sq_avg_roundings(0, k == 0), R.adam_a_roundings(0, k == 0), k + 1, HP["lr"],
                                 HP["eps"])
            mine = Q.rules_bound(opt, False, ref, a_abs, k + 1, HP["lr"], HP["eps"], R.KERNEL_CONSTS)
            for key in theirs:
                assert np.allclose(theirs[key], mine[key], rtol=1e-12, atol=0), (opt, key)
            p, s1, s2 = new["p"], new["s1"], new["s2"]


# ---- b ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,opts", CASES, ids=IDS)
def test_float32_form_within_the_counted_roundings(opt, opts, record_property):
    """12 applies of the float32 form carrying its own state; every apply against the float64 form FROM THE SAME INPUTS, as
    tests/test_optim_ref_cpu.py does for the defaults.  No element is left out."""
    o, consts = options(opts)
    for clip in (HP["clip"], 1e9):
        g0 = R.dense_grads(N, 4)
        p = R.dense_params(opt, g0, zeros32(), zeros32(), 0, HP["lr"], HP["eps"], clip, 4)
        s1, s2 = zeros32(), zeros32()
        worst = {}
        for k in range(STEPS):
            g = R.dense_grads(N, 4, k)
            got = Q.step_f32(opt, p, g, s1, s2, k, HP["lr"], HP["eps"], clip, **o)
            ref = Q.step_f64(opt, p, g, s1, s2, k, HP["lr"], HP["eps"], clip, consts, o["centered"])
            avg, c, omc = averaged_state(opt, o, consts, s1, s2)
            a_abs = None if avg is None else Q.a_abs_of(avg, g, ref["coef"], c, omc)
            bound = Q.rules_bound(opt, o["centered"], ref, a_abs, k + 1, HP["lr"], HP["eps"], consts)
            for key in ("p", "s1", "s2", "norm", "coef"):
                err = np.abs(np.asarray(got[key], dtype=np.float64) - ref[key])
                units = float(np.max(err / np.maximum(bound[key], 1e-300)))
                assert bool(np.all(err <= bound[key])), (opt, opts, key, k, units)
                worst[key] = max(worst.get(key, 0.0), units)
            assert np.isfinite(got["p"]).all()
            p, s1, s2 = got["p"], got["s1"], got["s2"]
        for key, v in worst.items():
            print("%s %s clip %g: %s at %.3g of its bound" % (opt, opts, clip, key, v))
            record_property("%s_clip%g" % (key, clip), v)


@pytest.mark.parametrize("tau", Q.TAUS)
def test_lerp_float32_form_within_its_bound(tau):
    pt, p = Q.lerp_tables(N, 5)
    got, ref = Q.lerp_f32(pt, p, tau), Q.lerp_f64(pt, p, tau)
    assert bool(np.all(np.abs(got.astype(np.float64) - ref) <= Q.lerp_bound(pt, p, tau)))
    same = pt == p
    assert same.sum() > N // 20 and R.same_bits(got[same & (pt != 0)], pt[same & (pt != 0)])  # nothing to move: nothing moves


# ---- c ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,opts", CASES, ids=IDS)
def test_float64_form_against_torch(opt, opts, record_property):
    """torch.optim.RMSprop(alpha, centered=True) / Adam(betas) with clip_grad_norm_, float64 on the CPU, 50 applies.  Every
    apply compares the float64 form from torch's own state before it -- identical inputs, the premise of the bound -- with
    u = 2^-53.  Both sides round, each in its own order (torch's norm, its lerps), so the distance is held to
    two_forms_bound: rules_bound counted once for torch's form and once for the restatement's own roundings (its norm,
    coefficient, averages and the u |p| of its final difference).  Centred: torch does not clamp, and in float64 on these
    tables (gradients that change by up to 4x from apply to apply) the variance never comes near zero.  The worst distance
    in steps is printed (3e-12 of a step): it is the norm's summation order and the cancellation in s - m * m, both of
    which the bound carries, not a disagreement."""
    o = dict(Q.DEFAULTS, **opts)
    consts = Q.torch_consts(o["alpha"], o["b1"], o["b2"])
    lr, eps, clip, u = HP["lr"], HP["eps"], HP["clip"], 2.0 ** -53
    g0 = R.dense_grads(N, 6).astype(np.float64)
    z = np.zeros(N)
    p = R.dense_params(opt, g0, z, z, 0, lr, eps, clip, 6).astype(np.float64)
    w = torch.nn.Parameter(torch.from_numpy(p.copy()))
    optim = (torch.optim.RMSprop([w], lr=lr, alpha=o["alpha"], eps=eps, centered=True) if opt == "rmsprop" else
             torch.optim.Adam([w], lr=lr, betas=(o["b1"], o["b2"]), eps=eps))
    names = ("square_avg", "grad_avg") if opt == "rmsprop" else ("exp_avg", "exp_avg_sq")
    worst, worst_step = {}, 0.0
    for k in range(50):
        g = R.dense_grads(N, 6, k).astype(np.float64)
        st = optim.state[w]
        p_in = w.detach().numpy().copy()
        s1, s2 = (st[nm].numpy().copy() if nm in st else z for nm in names)
        w.grad = torch.from_numpy(g.copy())
        norm = float(torch.nn.utils.clip_grad_norm_([w], clip))
        optim.step()
        ref = Q.step_f64(opt, p_in, g, s1, s2, k, lr, eps, clip, consts, o["centered"])
        avg, c, omc = (s1, consts["b1"], consts["one_m_b1"]) if opt == "adam" else (s2, consts["alpha"], consts["one_m_alpha"])
        bound = Q.two_forms_bound(opt, o["centered"], ref, Q.a_abs_of(avg, g, ref["coef"], c, omc), k + 1, lr, eps, consts, u, N)
        got = dict(p=w.detach().numpy(), s1=optim.state[w][names[0]].numpy(), s2=optim.state[w][names[1]].numpy(), norm=norm)
        for key in ("p", "s1", "s2", "norm"):
            err = np.abs(got[key] - ref[key])
            units = float(np.max(err / np.maximum(bound[key], 1e-300)))
            assert bool(np.all(err <= bound[key])), (opt, opts, key, k, units)
            worst[key] = max(worst.get(key, 0.0), units)
        moving = ref["step"] != 0
        worst_step = max(worst_step, float(np.max(np.abs(got["p"] - ref["p"])[moving] / np.abs(ref["step"][moving]))))
        if o["centered"]:
            assert float(ref["var"].min()) >= 0.0
    print("%s %s against torch: worst %.3g of a step; in units of the bound %s" % (opt, opts, worst_step, worst))
    record_property("worst_of_a_step", worst_step)


# ---- d ---------------------------------------------------------------------------------------------------------------------------
def test_constant_gradients_need_the_clamp():
    """4,096 gradients that never change, alpha 0.95, 600 applies: without the clamp s - m * m goes negative and the weight
    NaN; the clamped form is finite everywhere, and its variance is exactly 0 where the unclamped one went negative"""
    g = Q.constant_grads(N)
    hp = dict(lr=HP["lr"], eps=HP["eps"], clip=HP["clip"])
    run = {d: dict(p=R.dense_params("rmsprop", g, zeros32(), zeros32(), 0, hp["lr"], hp["eps"], hp["clip"], 8), s1=zeros32(),
                   s2=zeros32()) for d in (None, "no_clamp")}
    negative = np.zeros(N, dtype=bool)
    for k in range(600):
        for d, st in run.items():
            out = Q.step_f32("rmsprop", st["p"], g, st["s1"], st["s2"], 0, defect=d, **hp, **Q.PUBLISHED)
            run[d] = {key: out[key] for key in ("p", "s1", "s2")}
        st = run[None]
        negative |= (st["s1"] - st["s2"] * st["s2"]) < 0
        assert np.isfinite(st["p"]).all() and np.isfinite(st["s1"]).all() and np.isfinite(st["s2"]).all(), k
    print("s - m * m negative at some apply in %d of %d elements; %d weights NaN without the clamp" % (
        int(negative.sum()), N, int(np.isnan(run["no_clamp"]["p"]).sum())))
    assert negative.sum() >= 1 and np.isnan(run["no_clamp"]["p"]).sum() >= 1


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_restated_defects_change_bits_on_their_tables():
    """the dense table (two applies carrying state, clip engaged), the constant-gradient table for the clamp, the lerp table"""
    seen = set()
    g0 = R.dense_grads(N, 9)
    p0 = R.dense_params("rmsprop", g0, zeros32(), zeros32(), 0, HP["lr"], HP["eps"], HP["clip"], 9)
    for d in Q.STEP_DEFECTS:
        good = bad = dict(p=p0, s1=zeros32(), s2=zeros32())
        for k in range(2):
            g = R.dense_grads(N, 9, k)
            good = Q.step_f32("rmsprop", good["p"], g, good["s1"], good["s2"], 0, **HP, **Q.PUBLISHED)
            bad = Q.step_f32("rmsprop", bad["p"], g, bad["s1"], bad["s2"], 0, defect=d, **HP, **Q.PUBLISHED)
        assert float(good["coef"]) < 1
        if any(not R.same_bits(good[key], bad[key]) for key in ("p", "s1", "s2")):
            seen.add(d)
    assert set(Q.STEP_DEFECTS) - seen == {"no_clamp"}, seen  # the dense table's variance never goes negative ...
    g = Q.constant_grads(N)
    good = bad = dict(p=p0, s1=zeros32(), s2=zeros32())
    for k in range(600):  # ... the constant-gradient table's does (test_constant_gradients_need_the_clamp)
        good = Q.step_f32("rmsprop", good["p"], g, good["s1"], good["s2"], 0, **HP, **Q.PUBLISHED)
        bad = Q.step_f32("rmsprop", bad["p"], g, bad["s1"], bad["s2"], 0, defect="no_clamp", **HP, **Q.PUBLISHED)
    assert not R.same_bits(good["p"], bad["p"])
    pt, p = Q.lerp_tables(N, 5)
    for d in Q.LERP_DEFECTS:
        for tau in Q.TAUS:
            if tau != 0.5:  # (at 0.5 `1 - tau` IS tau: that value alone could not show it)
                assert not R.same_bits(Q.lerp_f32(pt, p, tau), Q.lerp_f32(pt, p, tau, defect=d)), (d, tau)
    assert not R.same_bits(Q.lerp_f32(pt, p, 0.5), Q.lerp_f32(pt, p, 0.5, defect="lerp_from_the_online_side"))
    assert set(Q.DEFECTS) == set(Q.STEP_DEFECTS) | set(Q.LERP_DEFECTS)


def test_nan_gradient_is_not_swallowed_by_the_clamp():
    g = R.dense_grads(N, 10)
    p = R.dense_params("rmsprop", g, zeros32(), zeros32(), 0, HP["lr"], HP["eps"], 1e9, 10)
    g[5] = np.nan
    out = Q.step_f32("rmsprop", p, g, zeros32(), zeros32(), 0, **HP, **Q.PUBLISHED)
    assert np.isnan(out["p"]).all()  # (the norm is NaN: clip_grad_norm_ spreads it)
    # with the coefficient out of the way (a state that already holds the NaN): the element's own variance is NaN and stays
    s2 = zeros32()
    s2[5] = np.nan
    g[5] = 1.0
    out = Q.step_f32("rmsprop", p, g, zeros32(), s2, 0, **HP, **Q.PUBLISHED)
    assert np.isnan(out["p"][5]) and np.isfinite(np.delete(out["p"], 5)).all()


# ---- f ---------------------------------------------------------------------------------------------------------------------------
def test_lr_at():
    from rela_amd.pyrela.utils import lr_at

    for (lr, warmup, lr_final, decay), rows in Q.LR_AT_TABLES:
        for update, want in rows:
            assert lr_at(update, lr, warmup, lr_final, decay) == want, (lr, warmup, lr_final, decay, update)
    lr = 6.25e-5
    for update in (0, 1, 7, 10 ** 9):  # the defaults: lr itself, bit for bit, whatever lr_final says
        assert lr_at(update, lr) == lr and lr_at(update, lr, 0, lr, 0) == lr and lr_at(update, lr, 0, lr / 4, 0) == lr
    # both ramps with a learning rate that is no power of two: the end points exactly, the rest monotone and linear
    warmup, decay, final = 7, 13, lr / 4
    vals = [lr_at(k, lr, warmup, final, decay) for k in range(warmup + decay + 5)]
    assert vals[warmup - 1] == lr and vals[warmup] == lr and abs(vals[0] - lr / warmup) <= 1e-15 * lr
    assert all(a < b for a, b in zip(vals[:warmup - 1], vals[1:warmup]))
    assert all(a > b for a, b in zip(vals[warmup:warmup + decay], vals[warmup + 1:warmup + decay + 1]))
    assert vals[warmup + decay:] == [final] * 5
    for k in range(warmup):
        assert abs(vals[k] - lr * (k + 1) / warmup) <= 1e-15 * lr
    for k in range(decay):
        assert abs(vals[warmup + k] - (lr + (final - lr) * k / decay)) <= 1e-15 * lr
