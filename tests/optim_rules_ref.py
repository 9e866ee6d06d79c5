"""The learners' configurable update rules (csrc/learner_common.hip: optimizer_apply with OptimState's alpha / centered / b1 / b2,
rmsprop_centered_update, target_lerp; pyrela/utils.py: lr_at) restated twice, the way tests/optim_ref.py restates the defaults:
  step_f64    clip_grad_norm_ + RMSprop (any alpha, centred or not) / Adam (any betas) in float64, parameterised by the
              constants: torch_consts(...), or kernel_consts(...), the float32 values the kernels compute with;
  step_f32    the kernels' own float32 arithmetic in the kernels' own order, meant to match the device bit for bit; `defect`
              names a one-line change for tests/test_optim_rules_ref_cpu.py;
  lerp_f32 / lerp_f64    the soft target update pt + tau * (p - pt);
  rules_bound / lerp_bound    step_f32 against step_f64(kernel_consts) per element, counted from the roundings (below);
  two_forms_bound    torch's float64 optimiser against step_f64(torch_consts): both sides' roundings, counted side by side;
  LR_AT_TABLES    lr_at's values written out by hand.
With alpha 0.99, not centred and betas 0.9 / 0.999 all of it is optim_ref's (tests/test_optim_rules_ref_cpu.py holds the two
together)."""
import math

import numpy as np

import optim_ref as R

F32, F64 = np.float32, np.float64
DEFAULTS = dict(alpha=0.99, centered=False, b1=0.9, b2=0.999)
PUBLISHED = dict(alpha=0.95, centered=True)  # Ape-X as published
TAUS = (2.0 ** -10, 0.005, 0.5)
LENGTHS4 = (1, 255, 256, 257, 65537)  # the edges of a 256-thread float4 kernel; one past a full grid stride of the norm


def torch_consts(alpha=0.99, b1=0.9, b2=0.999):
    return dict(alpha=alpha, one_m_alpha=1 - alpha, b1=b1, one_m_b1=1 - b1, b2=b2, one_m_b2=1 - b2, norm_eps=1e-6)


def kernel_consts(alpha=0.99, b1=0.9, b2=0.999):
    """what the kernels multiply with: the float arguments and 1.0f - them"""
    a, x, y = F32(alpha), F32(b1), F32(b2)
    return dict(alpha=float(a), one_m_alpha=float(F32(1) - a), b1=float(x), one_m_b1=float(F32(1) - x), b2=float(y),
                one_m_b2=float(F32(1) - y), norm_eps=float(F32(1e-6)))


# ---- float64 form ----------------------------------------------------------------------------------------------------------------
def step_f64(opt, p, g, s1, s2, t, lr, eps, clip, consts, centered=False, clamp=True):
    """one apply; t: Adam steps done before it.  -> dict(p, s1, s2, norm, coef, step), and for centred RMSprop var (s - m * m
    before the clamp) and gi (g * coef).  clamp=False is torch.optim.RMSprop(centered=True) itself"""
    if not (opt == "rmsprop" and centered):
        return R.step_f64(opt, p, g, s1, s2, t, lr, eps, clip, consts)
    p, g, s1, s2 = (np.asarray(x, dtype=F64) for x in (p, g, s1, s2))
    norm, cf = R.clip_f64(g, clip, consts["norm_eps"])
    with np.errstate(all="ignore"):
        gi = g * cf
        s1 = consts["alpha"] * s1 + consts["one_m_alpha"] * gi * gi
        s2 = consts["alpha"] * s2 + consts["one_m_alpha"] * gi
        var = s1 - s2 * s2
        v = np.where(var < 0, 0.0, var) if clamp else var
        step = lr * (gi / (np.sqrt(v) + eps))
    return dict(p=p - step, s1=s1, s2=s2, norm=norm, coef=cf, step=step, var=var, gi=gi)


# ---- float32 form, in the kernels' order -------------------------------------------------------------------------------------------
def bias_corrections_f32(t, b1, b2):
    """the host's formulas with the configured betas: pow and sqrt in double on the float values, the results cast to float"""
    x, y = float(F32(b1)), float(F32(b2))
    return F32(1.0) - F32(math.pow(x, float(t))), F32(math.sqrt(1.0 - math.pow(y, float(t))))


def step_f32(opt, p, g, s1, s2, t, lr, eps, clip, alpha=0.99, centered=False, b1=0.9, b2=0.999, defect=None, abort=False):
    """one apply as the device runs it; all arrays float32.  -> dict(p, s1, s2, norm, coef)"""
    p, g, s1, s2 = (np.array(x, dtype=F32) for x in (p, g, s1, s2))
    lr, eps = F32(lr), F32(eps)
    norm, cf = R.clip_f32(g, clip)
    if abort:
        return dict(p=p, s1=s1, s2=s2, norm=norm, coef=F32(-1.0))
    one = F32(1.0)
    with np.errstate(all="ignore"):
        gi = g * cf
        if opt == "rmsprop":
            a = F32(alpha)
            s1 = a * s1 + (one - a) * gi * gi
            if centered:
                gm = g if defect == "average_from_unclipped" else gi  # the gradient the average sees
                s2 = (one - a) * s2 + a * gm if defect == "alpha_on_the_gradient" else a * s2 + (one - a) * gm
                v = s1 - s2 * s2
                if defect != "no_clamp":
                    v = np.where(v < F32(0), F32(0), v)  # (a NaN compares false and stays)
                den = np.sqrt(v + eps) if defect == "eps_inside_sqrt" else np.sqrt(v) + eps
            else:
                den = np.sqrt(s1) + eps
            p = p - lr * (gi / den)
        else:
            x, y = F32(b1), F32(b2)
            bc1, bc2s = bias_corrections_f32(t + 1, b1, b2)
            s1 = x * s1 + (one - x) * gi
            s2 = y * s2 + (one - y) * gi * gi
            p = p - (lr / bc1) * (s1 / (np.sqrt(s2) / bc2s + eps))
    return dict(p=p, s1=s1, s2=s2, norm=norm, coef=cf)


def lerp_f32(pt, p, tau, defect=None):
    """target_lerp: pt + tau * (p - pt) in float32, in that order"""
    pt, p, tau = np.array(pt, dtype=F32), np.array(p, dtype=F32), F32(tau)
    with np.errstate(all="ignore"):
        if defect == "lerp_from_the_online_side":
            return p + tau * (pt - p)
        if defect == "one_minus_tau":
            return pt + (F32(1.0) - tau) * (p - pt)
        return pt + tau * (p - pt)


def lerp_f64(pt, p, tau):
    """the same with the float32 tau the kernel receives"""
    pt, p = np.asarray(pt, dtype=F64), np.asarray(p, dtype=F64)
    return pt + float(F32(tau)) * (p - pt)


STEP_DEFECTS = ("average_from_unclipped", "no_clamp", "eps_inside_sqrt", "alpha_on_the_gradient")
LERP_DEFECTS = ("lerp_from_the_online_side", "one_minus_tau")
DEFECTS = STEP_DEFECTS + LERP_DEFECTS


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# One apply from identical inputs, the float32 form against the float64 form with the SAME constants, in roundings u of the
# working precision (u = 2^-24: the float32 form; u = 2^-53: another float64 implementation, such as torch's).  The counts are
# optim_ref.f32_bound's, with the gradient's count GI left open:
#   norm    NORM roundings.  float32 form: the sum of squares is accumulated in double, the square root cast once: 1.  A float64
#           sum of n non-negative squares in ANY order is within (n - 1) u of the exact sum, its root within half of that, + 1.
#   coef    NORM + 2 (+ 1e-6, divide);   gi = g * coef: GI = NORM + 3
#   s       square average, all terms >= 0, relative: the new term (c * gi) * gi carries 2 GI + 2, the old one (an input) 1, the
#           sum 1: E = 2 GI + 3 (from a zero state c * 0 is exact; optim_ref.sq_avg_roundings with GI = 4 gives 11 either way)
#   m       gradient average / Adam's first moment, mixed signs, in units of A = c |m_in| + (1 - c) |gi|: the new term GI + 1,
#           the old one 1, the sum 1 more: Ea = GI + 2
#   centred RMSprop, with ds = E u s and dm = Ea u A (each + ABS_FLOOR: denormal products are exact to 2^-150 instead):
#     m * m   off by 2 |m| dm + dm^2, + u m^2 for the product
#     var     s - m * m: dv = ds + d(m * m) + u |var| for the difference.  THE CANCELLATION: dv is measured against s and m^2, not
#             against var, so it is any multiple of var once the gradient barely changes.  The clamp at 0 moves neither side by more.
#     root    |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) and <= sqrt(|a - b|): with v = max(var, 0) of the float64 form
#             droot = min(dv / (sqrt(v) + sqrt(max(v - dv, 0))), sqrt(dv)), which is dv / (2 sqrt(v)) where dv << v; + u for sqrtf
#     den     sqrt + eps: dden = droot + u sqrt(v) + u den; the computed denominator is >= eps whatever happened above, so
#             |1 / den~ - 1 / den| <= dden / (den * max(den - dden, eps))
#     step    lr * (gi / den): gi GI, the quotient 1, the product 1:
#             |error| <= lr |gi| (dden / (den * max(den - dden, eps)) + (GI + 2) u / den)
#   plain RMSprop and Adam: optim_ref.f32_bound's formulas with GI, E, Ea and the configured betas
#   p       the step's error + u |p| for the difference + ABS_FLOOR
SLACK = R.SLACK
ABS_FLOOR = R.ABS_FLOOR


def roundings(n=None, lerp=False):
    """-> dict(norm, coef, gi, sq, a): n None: the float32 form; n: a float64 form that sums n squares in its own order;
    lerp: the averages of gradients are computed as m + w (gi - m), w = 1 - c <= 0.5 (torch's lerp_; for w = 0.5 it takes
    gi - (gi - m)(1 - w), the same count): the difference carries GI |gi| + |gi - m|, the product 1 more, the sum 1 of the
    result: u (w GI |gi| + 2 w |gi - m| + |m_new|) <= u ((GI + 2) w |gi| + 2 (1 - w) |m| + A) <= (GI + 3) u A"""
    norm = 1 if n is None else (n - 1) / 2 + 1
    gi = norm + 3
    return dict(norm=norm, coef=norm + 2, gi=gi, sq=2 * gi + 3, a=gi + 2 + (1 if lerp else 0))


def a_abs_of(s_in, g, coef, c, one_m_c):
    """A = c |m_in| + (1 - c) |g * coef|"""
    return c * np.abs(np.asarray(s_in, dtype=F64)) + one_m_c * np.abs(np.asarray(g, dtype=F64) * coef)


def rules_bound(opt, centered, ref, a_abs, t_next, lr, eps, consts, u=R.U_F32, n=None, lerp=False):
    """per element bounds of |a rounded form - the exact result| for ONE apply, the exact result taken at step_f64(consts)'s
    values.  ref: step_f64's result; a_abs: a_abs_of the state that is an average of gradients (None for plain RMSprop);
    n, lerp: roundings().  -> dict(p, s1, s2, norm, coef)"""
    k = roundings(n, lerp)
    gamma = lambda count: count * u / (1 - count * u)  # optim_ref._k at any u
    out = dict(norm=gamma(k["norm"]) * SLACK * ref["norm"], coef=gamma(k["coef"]) * SLACK * ref["coef"])
    u = u * SLACK
    if opt == "rmsprop" and centered:
        ds = k["sq"] * u * ref["s1"] + ABS_FLOOR
        dm = k["a"] * u * a_abs + ABS_FLOOR
        m = np.abs(ref["s2"])
        dv = ds + 2 * m * dm + dm * dm + u * m * m + u * np.abs(ref["var"]) + ABS_FLOOR
        v = np.maximum(ref["var"], 0.0)
        root = np.sqrt(v)
        droot = np.minimum(dv / np.maximum(root + np.sqrt(np.maximum(v - dv, 0.0)), 1e-300), np.sqrt(dv)) + u * root
        den = root + eps
        dden = (droot + u * den) * SLACK
        step_err = lr * np.abs(ref["gi"]) * (dden / (den * np.maximum(den - dden, eps * (1 - u))) + (k["gi"] + 2) * u / den) * SLACK
        out["s1"], out["s2"] = ds, dm
    elif opt == "rmsprop":
        out["s1"] = k["sq"] * u * ref["s1"] + ABS_FLOOR
        out["s2"] = np.zeros_like(ref["s1"])
        step_err = (k["sq"] / 2 + k["gi"] + 4) * u * np.abs(ref["step"])
    else:
        bc1, bc2s = R.bias_corrections_f64(t_next, consts)
        pw = consts["b1"] ** t_next
        out["s1"] = k["a"] * u * a_abs + ABS_FLOOR
        out["s2"] = k["sq"] * u * ref["s2"] + ABS_FLOOR
        den = np.sqrt(ref["s2"]) / bc2s + eps
        step_err = (lr / bc1) / den * u * (k["a"] * a_abs + np.abs(ref["s1"]) * (k["sq"] / 2 + 8 + pw / bc1))
    out["p"] = step_err + u * np.abs(ref["p"]) + ABS_FLOOR
    return out


def two_forms_bound(opt, centered, ref, a_abs, t_next, lr, eps, consts, u, n):
    """|torch's float64 optimiser - step_f64| per element for ONE apply from identical inputs.  Neither side is exact, so the
    distance is counted side by side, |T - R| <= |T - exact| + |R - exact|, each from its own roundings:
      torch   clip_grad_norm_ sums the n squares in its own order; its averages of gradients are lerps (roundings(n, lerp=True));
              square_avg.mul_(c).addcmul_(g, g, value=1 - c), sqrt, add_(eps), addcdiv_ and Adam's step have the counts of
              rules_bound's derivation, its p one rounding of the final sum;
      step_f64   numpy sums its n squares in another order (roundings(n)); its coefficient, averages, root, quotient and
              product are rules_bound's, its p one rounding of its own final difference.
    The sum is taken at step_f64's values: the difference of the two sides' values under the bounds is second order (SLACK)."""
    sides = [rules_bound(opt, centered, ref, a_abs, t_next, lr, eps, consts, u=u, n=n, lerp=lerp) for lerp in (True, False)]
    return {key: sides[0][key] + sides[1][key] for key in sides[0]}


def lerp_bound(pt, p, tau, u=R.U_F32):
    """|lerp_f32 - lerp_f64| per element: the difference 1 rounding of |p - pt|, the product 1 more, the sum 1 of the result:
    u (2 tau |p - pt| + |result|), second order in SLACK, denormals in ABS_FLOOR"""
    pt, p = np.asarray(pt, dtype=F64), np.asarray(p, dtype=F64)
    return u * SLACK * (2 * float(F32(tau)) * np.abs(p - pt) + np.abs(lerp_f64(pt, p, tau))) + ABS_FLOOR


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def constant_grads(n=4096, seed=7):
    """gradients that never change: log-uniform over 1e-6 .. 1e2 with random signs.  Under alpha^k -> 0 the square average
    tends to g^2 and the gradient average to g: s - m * m is then a difference of two roundings of the same number"""
    rng = np.random.default_rng([seed, 91])
    return (10.0 ** rng.uniform(-6, 2, n) * rng.choice([-1.0, 1.0], n)).astype(F32)


def lerp_tables(n, seed):
    """-> (pt, p): weights in [-1, 1]; a tenth of the online weights equal their target (nothing to move), a tenth differ
    by one ulp, and four are zeros of either sign"""
    rng = np.random.default_rng([seed, 92])
    pt = rng.uniform(-1, 1, n).astype(F32)
    p = rng.uniform(-1, 1, n).astype(F32)
    kind = rng.random(n)
    p = np.where(kind < 0.1, pt, p)
    p = np.where((kind >= 0.1) & (kind < 0.2), np.nextafter(pt, F32(2)), p).astype(F32)
    pt[:2], p[:2] = [0.0, -0.0], [-0.0, 0.0]
    return pt, p


# lr_at(num_update, lr, warmup, lr_final, decay_updates) by hand: (arguments, [(update, value)]); lr = 1.0 keeps them readable
LR_AT_TABLES = (
    ((1.0, 4, 0.25, 3), [(0, 0.25), (1, 0.5), (2, 0.75), (3, 1.0), (4, 1.0), (5, 0.75), (6, 0.5), (7, 0.25), (8, 0.25),
                         (10 ** 9, 0.25)]),
    ((1.0, 0, 0.5, 2), [(0, 1.0), (1, 0.75), (2, 0.5), (3, 0.5)]),
    ((1.0, 2, None, 0), [(0, 0.5), (1, 1.0), (2, 1.0), (10 ** 6, 1.0)]),
    ((1.0, 2, 0.5, 0), [(0, 0.5), (1, 1.0), (2, 1.0), (10 ** 6, 1.0)]),  # no decay length: lr_final takes no part
    ((1.0, 1, 2.0, 4), [(0, 1.0), (1, 1.0), (2, 1.25), (5, 2.0)]),  # (a schedule may also rise)
)
