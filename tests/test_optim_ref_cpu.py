"""tests/optim_ref.py on the CPU: the references of tests/test_optimizer_gpu.py and what its tables can tell apart.
  a. the float64 form with torch's constants IS torch: clip_grad_norm_ + torch.optim.RMSprop / Adam in float64, 12 steps;
  b. the float64 form with the kernels' float32 constants lies where the constants' representation errors put it;
  c. the float32 form in the kernels' order stays within the bound counted from its roundings;
  d. NaN and inf gradients go where torch's clip_grad_norm_ sends them;
  e. every restated defect changes bits on the table that is there for it, or is invisible for a stated reason;
  f. the tables' preconditions: dense tables move every weight with a non-zero gradient, sentinel sums are exact."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R

N = 4096
STEPS = 12
OPTS = ("rmsprop", "adam")
HP = R.hp32(R.TEST_HP)
EPS64 = 2.0 ** -52


def zeros(n=N):
    return np.zeros(n, dtype=np.float64)


def adam_abs(a_abs, gi, consts=R.KERNEL_CONSTS):
    """Adam's first-moment recurrence over |g * coef|: the scale of its rounding and representation errors"""
    return consts["b1"] * a_abs + consts["one_m_b1"] * np.abs(gi)


# ---- a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [40.0, 1e9])
@pytest.mark.parametrize("opt", OPTS)
def test_float64_form_is_torch(opt, clip):
    """clip 40 is always engaged on these gradients, 1e9 never.  A few ulps of float64: measured 2e-16 / 4e-16 relative;
    the bound is 64 ulps of the element's scale (12 steps of a handful of operations)."""
    lr, eps = HP["lr"], HP["eps"]
    g0 = R.dense_grads(N, 1).astype(np.float64)
    p = R.dense_params(opt, g0, zeros(), zeros(), 0, lr, eps, clip, 1).astype(np.float64)
    w = torch.nn.Parameter(torch.from_numpy(p.copy()))
    optim = (torch.optim.RMSprop([w], lr=lr, alpha=0.99, eps=eps) if opt == "rmsprop" else
             torch.optim.Adam([w], lr=lr, betas=(0.9, 0.999), eps=eps))
    s1, s2, a_abs = zeros(), zeros(), zeros()
    worst = 0.0
    for k in range(STEPS):
        g = R.dense_grads(N, 1, k).astype(np.float64)
        w.grad = torch.from_numpy(g.copy())
        norm = float(torch.nn.utils.clip_grad_norm_([w], clip))
        optim.step()
        out = R.step_f64(opt, p, g, s1, s2, k, lr, eps, clip, R.TORCH_CONSTS)
        a_abs = adam_abs(a_abs, g * out["coef"], R.TORCH_CONSTS)
        walked = np.abs(p) + np.abs(out["step"]) if k == 0 else walked + np.abs(out["step"])  # the scale of p's roundings
        p, s1, s2 = out["p"], out["s1"], out["s2"]
        assert (out["coef"] < 1) == (clip == 40.0)
        assert abs(norm - out["norm"]) <= 64 * EPS64 * norm
        st = optim.state[w]
        pairs = ([(st["square_avg"].numpy(), s1, s1)] if opt == "rmsprop" else
                 [(st["exp_avg"].numpy(), s1, a_abs), (st["exp_avg_sq"].numpy(), s2, s2)])
        for got, want, scale in pairs + [(w.detach().numpy(), p, walked)]:
            assert bool((np.abs(got - want) <= 64 * EPS64 * scale).all())
            worst = max(worst, float((np.abs(got - want) / np.maximum(scale, 1e-300)).max()))
    print("%s clip %g: float64 form against torch, worst %.3g relative" % (opt, clip, worst))


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def test_the_constants_representation_errors():
    """what item 3 of the issue states: 1.0f - 0.99f is 9.5e-7 off 0.01, 1.0f - 0.9f three ulps off 0.1f"""
    assert 9.4e-7 < R.const_rel("one_m_alpha") < 9.6e-7
    assert R.KERNEL_CONSTS["one_m_alpha"] == 0.009999990463256836
    ulp = float(np.spacing(np.float32(0.1)))
    assert abs(R.KERNEL_CONSTS["one_m_b1"] - float(np.float32(0.1))) == 3 * ulp
    for name in ("alpha", "b1", "b2"):
        assert R.const_rel(name) <= R.U_F32  # the constants themselves: one rounding
    assert R.const_rel("one_m_b2") < 5e-5  # 1.0f - 0.999f: the difference of two floats near 1 keeps 2^-24 / 1e-3


@pytest.mark.parametrize("clip", [40.0, 1e9])
@pytest.mark.parametrize("opt", OPTS)
def test_kernel_constants_against_torch_constants(opt, clip, record_property):
    """12 steps from a zero state with either set of constants, both in float64: the distance is within consts_bound,
    which is derived from the constants' representation errors alone; after ONE RMSprop step the square average is off
    by exactly the error of 1 - alpha (the state was zero: alpha took no part)."""
    lr, eps = HP["lr"], HP["eps"]
    g0 = R.dense_grads(N, 2).astype(np.float64)
    p0 = R.dense_params(opt, g0, zeros(), zeros(), 0, lr, eps, clip, 2).astype(np.float64)
    state = {c: dict(p=p0, s1=zeros(), s2=zeros()) for c in ("torch", "kernel")}
    a_abs, p_bound = zeros(), zeros()
    worst = {}
    for k in range(STEPS):
        g = R.dense_grads(N, 2, k).astype(np.float64)
        out = {}
        for c, consts in (("torch", R.TORCH_CONSTS), ("kernel", R.KERNEL_CONSTS)):
            st = state[c]
            out[c] = R.step_f64(opt, st["p"], g, st["s1"], st["s2"], k, lr, eps, clip, consts)
            state[c] = {key: out[c][key] for key in ("p", "s1", "s2")}
        ref = out["torch"]
        a_abs = adam_abs(a_abs, g * ref["coef"], R.TORCH_CONSTS)
        bound = R.consts_bound(opt, ref, a_abs, k + 1, k + 1, lr, eps)
        p_bound = p_bound + bound["step"]
        walked = np.abs(ref["step"]) if k == 0 else walked + np.abs(ref["step"])
        for key, b in (("s1", bound["s1"]), ("s2", bound.get("s2")), ("p", p_bound)):
            if b is None:
                continue
            err = np.abs(out["kernel"][key] - ref[key])
            assert bool((err <= b + 1e-300).all()), (key, k, float((err / np.maximum(b, 1e-300)).max()))
            # in units of: the distance walked (p), the sum of |terms| (Adam's first moment), the value itself
            scale = np.maximum(walked if key == "p" else a_abs if key == "s1" and opt == "adam" else np.abs(ref[key]), 1e-300)
            worst[key] = max(worst.get(key, 0.0), float((err / scale).max()))
        if opt == "rmsprop" and k == 0:
            nz = ref["s1"] > 0
            rel = np.abs(out["kernel"]["s1"] - ref["s1"])[nz] / ref["s1"][nz]
            assert bool((np.abs(rel - R.const_rel("one_m_alpha")) <= 1e-3 * R.const_rel("one_m_alpha")).all())
    for key, v in worst.items():
        print("%s clip %g: kernel constants against torch's, %s off by %.3g relative" % (opt, clip, key, v))
        record_property("consts_%s" % key, v)
    assert worst["s1" if opt == "rmsprop" else "s2"] > 1e-7  # the deviation is there: it is not a rounding of float64


# ---- c ---------------------------------------------------------------------------------------------------------------------------
def run_f32_against_f64(opt, hp, clip, seed, n=N, steps=STEPS, t0=0):
    """`steps` applies of the float32 form carrying its own state; every apply against the float64 form FROM THE SAME
    INPUTS (the float32 state is data of that apply: its earlier roundings are no part of the comparison).
    -> worst |error| / bound per output"""
    lr, eps = hp["lr"], hp["eps"]
    g0 = R.dense_grads(n, seed)
    z = np.zeros(n, dtype=np.float32)
    p, s1, s2 = R.dense_params(opt, g0, z, z, t0, lr, eps, clip, seed), z, z
    worst = {}
    for k in range(steps):
        g = R.dense_grads(n, seed, k)
        got = R.step_f32(opt, p, g, s1, s2, t0 + k, lr, eps, clip)
        ref = R.step_f64(opt, p, g, s1, s2, t0 + k, lr, eps, clip, R.KERNEL_CONSTS)
        a_abs = adam_abs(np.abs(s1.astype(np.float64)), g.astype(np.float64) * ref["coef"])
        zero = k == 0
        bound = R.f32_bound(opt, ref, a_abs, R.sq_avg_roundings(0, zero), R.adam_a_roundings(0, zero), t0 + k + 1, lr, eps)
        for key in ("p", "s1", "s2", "norm", "coef"):
            err = np.abs(np.asarray(got[key], dtype=np.float64) - ref[key])
            assert bool(np.all(err <= bound[key])), (opt, key, k, float(np.max(err / np.maximum(bound[key], 1e-300))))
            worst[key] = max(worst.get(key, 0.0), float(np.max(err / np.maximum(bound[key], 1e-300))))
        moved = R.moved_ulps(p, got["p"])[g != 0]
        assert moved.size and float(moved.min()) >= 8, (opt, k, float(moved.min()))  # (f: every apply of the run is visible)
        p, s1, s2 = got["p"], got["s1"], got["s2"]
    return worst


@pytest.mark.parametrize("hp", [R.TEST_HP, R.WORKLOAD_HP], ids=["lr1e-3", "workload"])
@pytest.mark.parametrize("opt", OPTS)
def test_float32_form_within_the_counted_roundings(opt, hp, record_property):
    """the derivation stands next to f32_bound (optim_ref.py); the measured maxima, as fractions of the bound, go into
    profiles/optimizer_error_units.md"""
    for clip in (R.hp32(hp)["clip"], 1e9):
        worst = run_f32_against_f64(opt, R.hp32(hp), clip, 3)
        for key, v in worst.items():
            print("%s lr %g clip %g: %s at %.3g of its bound" % (opt, hp["lr"], clip, key, v))
            record_property("%s_clip%g" % (key, clip), v)


@pytest.mark.parametrize("t0", R.ADAM_STEPS_DONE)
def test_adam_far_from_step_one(t0):
    run_f32_against_f64("adam", HP, HP["clip"], 4, steps=2, t0=t0)
    if t0 == 10 ** 6:
        assert R.bias_corrections_f32(t0 + 1)[0] == np.float32(1.0)  # 0.9^t underflowed: bc1 is exactly 1


# ---- d ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", OPTS)
def test_nan_and_inf_gradients_as_clip_grad_norm(opt):
    """torch: a NaN gradient makes every gradient NaN (the clamp of the coefficient propagates it), an inf gradient gives
    coefficient 0 and NaN (inf * 0) in its own element only; both forms follow."""
    lr, eps, clip = HP["lr"], HP["eps"], HP["clip"]
    n, at = 64, 17
    g0 = R.dense_grads(n, 5)
    z = np.zeros(n, dtype=np.float32)
    p0 = R.dense_params(opt, g0, z, z, 0, lr, eps, clip, 5)
    for bad in (np.nan, np.inf, -np.inf):
        g = g0.copy()
        g[at] = bad
        w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        w.grad = torch.from_numpy(g.copy())
        norm = float(torch.nn.utils.clip_grad_norm_([w], clip))
        clipped = w.grad.numpy()
        others = np.arange(n) != at
        f32 = R.step_f32(opt, p0, g, z, z, 0, lr, eps, clip)
        f64 = R.step_f64(opt, p0, g, z, z, 0, lr, eps, clip, R.KERNEL_CONSTS)
        if bad != bad:
            assert norm != norm and np.isnan(clipped).all()
            for out in (f32, f64):
                assert out["norm"] != out["norm"] and out["coef"] != out["coef"] and np.isnan(out["p"]).all()
        else:
            assert norm == np.inf and np.isnan(clipped[at]) and not clipped[others].any()
            zero_g = R.step_f32(opt, p0, z, z, z, 0, lr, eps, clip)
            for out in (f32, f64):
                assert out["norm"] == np.inf and out["coef"] == 0 and np.isnan(out["p"][at])
            assert R.same_bits(f32["p"][others], zero_g["p"][others]) and R.same_bits(f32["p"][others], p0[others])


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def _tables():
    """name -> f(defect) -> outputs of the float32 form: the roles of test_optimizer_gpu.py's tables at small sizes (the
    norm's structure at the GPU test's own lengths: it is cheap)"""
    lr, eps, clip = HP["lr"], HP["eps"], HP["clip"]
    z = np.zeros(N, dtype=np.float32)
    g = R.dense_grads(N, 6)
    tables = {}
    for n4 in R.LENGTHS4:  # the three rotations of a length are one table
        sgs = [R.sentinel_grads(n4, rot)[0] for rot in R.SENTINEL_ROTATIONS]
        tables["sentinel_%d" % n4] = lambda d, sgs=sgs: {"norm%d" % i: R.clip_f32(sg, clip, d)[0] for i, sg in enumerate(sgs)}
    for opt in OPTS:
        p = R.dense_params(opt, g, z, z, 0, lr, eps, clip, 6)
        prev = R.step_f32(opt, p, g, z, z, 0, lr, eps, clip)
        g1 = R.dense_grads(N, 6, 1)
        tables["dense_%s" % opt] = lambda d, opt=opt, p=p: R.step_f32(opt, p, g, z, z, 0, lr, eps, clip, d)
        tables["dense_%s_carried" % opt] = lambda d, opt=opt, prev=prev: R.step_f32(opt, prev["p"], g1, prev["s1"], prev["s2"], 1, lr, eps, clip, d)
        small = (g * np.float32(2.0 ** -30)).astype(np.float32)  # norm far below clip
        tables["unclipped_%s" % opt] = lambda d, opt=opt, p=p: R.step_f32(opt, p, small, z, z, 0, lr, eps, clip, d)
        eq = np.zeros(8, dtype=np.float32)
        eq[1], eq[6] = 0.375, -0.5  # norm = 0.625 = clip
        tables["norm_is_clip_%s" % opt] = lambda d, opt=opt, eq=eq: R.step_f32(opt, p[:8], eq, z[:8], z[:8], 0, lr, eps, 0.625, d)
    norms = [R.dense_grads(4 * n4, R.dense_seed(n4)) for n4 in R.LENGTHS4]  # the dense tables of the GPU test, their norms
    tables["dense_norms"] = lambda d: {"norm%d" % i: R.clip_f32(gg, clip, d)[0] for i, gg in enumerate(norms)}
    tables["adam_t1e6"] = lambda d: R.step_f32("adam", p, g, z, z, 10 ** 6, lr, eps, clip, d)
    return tables


def _differs(a, b):
    return any(not R.same_bits(a[k], b[k]) for k in a)


# defect -> the tables that must tell it from the true form
CAUGHT_BY = {
    "eps_inside_sqrt": ["dense_rmsprop", "dense_adam"],
    "state_from_unclipped": ["dense_rmsprop", "dense_adam"],
    "coef_on_step_only": ["dense_rmsprop", "dense_adam"],
    "coef_not_clamped": ["unclipped_rmsprop", "unclipped_adam"],
    "no_norm_eps": ["norm_is_clip_rmsprop", "norm_is_clip_adam"],
    "bc2_without_sqrt": ["dense_adam", "dense_adam_carried"],
    "bc1_dropped": ["dense_adam", "dense_adam_carried"],
    "step_not_advancing": ["dense_adam", "dense_adam_carried"],
    "last_float4_not_summed": ["sentinel_%d" % n4 for n4 in R.LENGTHS4],
    "one_block_not_summed": ["sentinel_65536", "sentinel_%d" % (8 * 65536)],
    # (nearly invisible by nature: the tree keeps a float32 sum within an ulp or so, and the square root halves that before
    # the float32 norm rounds it; 2 of the 13 dense norms differ, no sentinel table does)
    "f32_accumulation": ["dense_norms"],
    "remainder_tail_skipped": ["sentinel_%d" % n4 for n4 in R.LENGTHS4 if n4 != 8 * 65536],
}
# ... and where it cannot show, with the reason
INVISIBLE = {
    ("bc1_dropped", "adam_t1e6"): "0.9^t underflowed: bc1 is exactly 1",
    ("coef_not_clamped", "dense_rmsprop"): "the coefficient is below 1: the clamp takes no part",
    ("no_norm_eps", "unclipped_rmsprop"): "the clamp hides the coefficient",
    ("remainder_tail_skipped", "sentinel_%d" % (8 * 65536)): "two unrolled passes cover the buffer: no remainder",
    ("state_from_unclipped", "unclipped_rmsprop"): "the coefficient is 1",
    ("f32_accumulation", "sentinel_1"): "four adjacent sentinels: their squares add exactly in float32 too",
}


def test_restated_defects_change_bits_on_their_tables():
    assert set(CAUGHT_BY) == set(R.DEFECTS)
    tables = _tables()
    true = {name: f(None) for name, f in tables.items()}
    for defect, names in CAUGHT_BY.items():
        for name in names:
            assert _differs(tables[name](defect), true[name]), (defect, name)
    for (defect, name), why in INVISIBLE.items():
        assert not _differs(tables[name](defect), true[name]), (defect, name, why)
    # the clip regimes are what their names say
    assert float(true["dense_rmsprop"]["coef"]) < 1e-2 and float(true["unclipped_rmsprop"]["coef"]) == 1.0
    c = true["norm_is_clip_rmsprop"]
    assert float(c["norm"]) == 0.625 and c["coef"] == np.float32(0.625) / (np.float32(0.625) + np.float32(1e-6)) < 1


# ---- f ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n4", R.LENGTHS4)
def test_sentinel_tables_are_exact(n4):
    seen = set()
    for rot in R.SENTINEL_ROTATIONS:
        g, total, pos = R.sentinel_grads(n4, rot)
        assert len(pos) == len(set(pos)) == min(26, 4 * n4) and max(pos) < 4 * n4
        assert 4 * (n4 - 1) + 3 in pos and 0 in pos
        assert int(np.count_nonzero(g)) == len(pos)
        # every square is a multiple of 2^-24 and the sum stays below 2^53 of them: float64 holds any partial sum exactly
        assert total < 1 << 53 and total == sum(int(round(float(x) ** 2 * 2 ** 24)) for x in g[g != 0])
        assert float(R.sumsq_f32_order(g)) * 2 ** 24 == total
        assert R.clip_f32(g, 40.0)[0] == R.sentinel_norm(total)
        for at in R.sentinel_visible(n4, rot):  # dropped or doubled, the float32 norm changes
            for factor in (0.0, 2.0 ** 0.5):
                h = g.astype(np.float64)
                h[at] *= factor
                assert np.float32(np.sqrt(np.sum(h * h))) != R.sentinel_norm(total), (rot, at, factor)
            seen.add(at)
    assert seen == set(pos)  # every position is visible in one of the rotations
    rem = R.remainder_float4(n4)
    assert rem.size == n4 - 4 * R.STRIDE4 * ((max(0, n4 - 3 * R.STRIDE4) + 4 * R.STRIDE4 - 1) // (4 * R.STRIDE4)) or n4 % R.STRIDE4


def test_remainder_loop_indices_by_simulation():
    """remainder_float4 against a literal walk of sumsq_partial's two loops, at a stride of 8 instead of 65,536"""
    stride = 8
    for n4 in range(1, 80):
        seen = []
        for i0 in range(stride):
            i = i0
            while i + 3 * stride < n4:
                i += 4 * stride
            while i < n4:
                seen.append(i)
                i += stride
        j = np.arange(n4)
        passes = np.maximum(0, (n4 - j % stride - 3 * stride + 4 * stride - 1) // (4 * stride))
        assert sorted(seen) == list(j[j // stride >= 4 * passes]), n4


@pytest.mark.parametrize("hp", [R.TEST_HP, R.WORKLOAD_HP], ids=["lr1e-3", "workload"])
@pytest.mark.parametrize("opt", OPTS)
def test_dense_tables_move_every_weight(opt, hp):
    h = R.hp32(hp)
    z = np.zeros(N, dtype=np.float32)
    for clip in (h["clip"], 1e30):
        g = R.dense_grads(N, 7)
        p = R.dense_params(opt, g, z, z, 0, h["lr"], h["eps"], clip, 7)
        assert float(np.abs(p).max()) <= 1.0 and 0.05 < float(np.mean(g == 0)) < 0.15
        sq = g.astype(np.float64) ** 2
        assert np.any((sq > 0) & (sq < 2.0 ** -126)) and np.any((sq > 0) & (sq < 2.0 ** -150))  # denormal, underflowing
        out = R.step_f32(opt, p, g, z, z, 0, h["lr"], h["eps"], clip)
        assert float(R.moved_ulps(p, out["p"])[g != 0].min()) >= 8
        assert R.same_bits(out["p"][g == 0], p[g == 0])
    assert math.isclose(float(np.abs(g).max()), 1e4, rel_tol=1.0)
