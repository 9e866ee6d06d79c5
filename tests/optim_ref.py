"""optimizer_apply (csrc/learner_common.hip: sumsq_partial, clip_coef, rmsprop_update / adam_update) restated twice, and the
tables by role that tests/test_optimizer_gpu.py runs through rela_debug_optimizer_apply:
  step_f64    torch's clip_grad_norm_ + RMSprop (alpha 0.99, no momentum, not centred) / Adam (betas 0.9 / 0.999, no
              amsgrad) in float64, parameterised by the constants: TORCH_CONSTS, or KERNEL_CONSTS, the float32 values the
              kernels compute with (1.0f - 0.99f is not 0.01);
  step_f32    the kernels' own float32 arithmetic in the kernels' own order, meant to match the device bit for bit (the
              library is built with -ffp-contract=off; float divide and sqrt are correctly rounded); `defect` names a
              one-line change for tests/test_optim_ref_cpu.py;
  bounds      f32_bound: step_f32 against step_f64(KERNEL_CONSTS) from the count of roundings per output; consts_bound:
              step_f64(KERNEL_CONSTS) against step_f64(TORCH_CONSTS) from the constants' representation errors.
tests/test_optim_ref_cpu.py pins all of it on the CPU."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U_F32 = 2.0 ** -24
THREADS = 256
BLOCKS = 256  # kNormBlocks
STRIDE4 = BLOCKS * THREADS  # float4 per grid-stride visit
# buffer lengths in float4: 3 * STRIDE4 is the last at which the 4x-unrolled loop never runs, 3 * STRIDE4 + 1 makes exactly
# one thread take it; the larger ones mix unrolled passes with a remainder
LENGTHS4 = (1, 2, 255, 256, 257, 65535, 65536, 65537, 196608, 196609, 4 * 65536 + 257, 7 * 65536 + 5, 8 * 65536)
TEST_HP = dict(lr=1e-3, eps=1.5e-4, clip=40.0)
WORKLOAD_HP = dict(lr=6.25e-5, eps=1.5e-4, clip=40.0)
ADAM_STEPS_DONE = (0, 1, 9, 10 ** 4, 10 ** 6)

TORCH_CONSTS = dict(alpha=0.99, one_m_alpha=1 - 0.99, b1=0.9, one_m_b1=1 - 0.9, b2=0.999, one_m_b2=1 - 0.999, norm_eps=1e-6)
KERNEL_CONSTS = dict(alpha=float(F32(0.99)), one_m_alpha=float(F32(1) - F32(0.99)), b1=float(F32(0.9)),
                     one_m_b1=float(F32(1) - F32(0.9)), b2=float(F32(0.999)), one_m_b2=float(F32(1) - F32(0.999)),
                     norm_eps=float(F32(1e-6)))


def hp32(hp):
    """the hyper-parameters as the C ABI's float arguments hold them"""
    return {k: float(F32(v)) for k, v in hp.items()}


def _k(n):
    """n roundings of float32: gamma_n"""
    return n * U_F32 / (1 - n * U_F32)


# ---- float64 form ----------------------------------------------------------------------------------------------------------------
def clip_f64(g, clip, norm_eps):
    """torch.nn.utils.clip_grad_norm_: (norm, coefficient); the clamp at 1 propagates NaN"""
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.sum(np.square(np.asarray(g, dtype=F64)))))
        c = clip / (norm + norm_eps)
    return norm, (c if (c < 1.0 or c != c) else 1.0)


def bias_corrections_f64(t, consts):
    return 1 - consts["b1"] ** t, math.sqrt(1 - consts["b2"] ** t)


def step_f64(opt, p, g, s1, s2, t, lr, eps, clip, consts):
    """one apply; t: Adam steps done before it.  -> dict(p, s1, s2, norm, coef, step)"""
    p, g, s1, s2 = (np.asarray(x, dtype=F64) for x in (p, g, s1, s2))
    norm, cf = clip_f64(g, clip, consts["norm_eps"])
    with np.errstate(all="ignore"):
        gi = g * cf
        if opt == "rmsprop":
            s1 = consts["alpha"] * s1 + consts["one_m_alpha"] * gi * gi
            step = lr * (gi / (np.sqrt(s1) + eps))
        else:
            bc1, bc2s = bias_corrections_f64(t + 1, consts)
            s1 = consts["b1"] * s1 + consts["one_m_b1"] * gi
            s2 = consts["b2"] * s2 + consts["one_m_b2"] * gi * gi
            step = (lr / bc1) * (s1 / (np.sqrt(s2) / bc2s + eps))
    return dict(p=p - step, s1=s1, s2=s2, norm=norm, coef=cf, step=step)


# ---- float32 form, in the kernels' order -------------------------------------------------------------------------------------------
def _tree256(red):
    """the 256-lane shared-memory tree over the last axis (length 256)"""
    red = red.copy()
    o = 128
    while o > 0:
        red[..., :o] = red[..., :o] + red[..., o:2 * o]
        o >>= 1
    return red[..., 0]


def sumsq_f32_order(g, defect=None):
    """sumsq_partial + the tree of clip_coef: float64 partials per thread in grid-stride order (one float4 per visit,
    ((x^2 + y^2) + z^2) + w^2 added to the running sum: the unrolled loop and the remainder loop visit in the same order),
    the 256-lane tree per block, the tree over the 256 block partials"""
    g = np.asarray(g, dtype=F32)
    assert g.size % 4 == 0 and g.size > 0
    acc = F32 if defect == "f32_accumulation" else F64
    v = g.reshape(-1, 4).astype(acc)
    with np.errstate(all="ignore"):
        q = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) + v[:, 3] * v[:, 3]
    n4 = q.size
    if defect == "last_float4_not_summed":
        q[n4 - 1] = 0
    if defect == "remainder_tail_skipped":  # every thread's remainder loop stops one visit early
        rem = remainder_float4(n4)
        q[rem[rem + STRIDE4 >= n4]] = 0
    visits = -(-n4 // STRIDE4)
    q = np.concatenate([q, np.zeros(visits * STRIDE4 - n4, dtype=acc)]).reshape(visits, STRIDE4)
    s = np.zeros(STRIDE4, dtype=acc)
    with np.errstate(all="ignore"):
        for row in q:
            s = s + row
        part = _tree256(s.reshape(BLOCKS, THREADS))
        if defect == "one_block_not_summed":
            part[BLOCKS - 1] = 0
        return F64(_tree256(part))


def remainder_float4(n4):
    """the float4 indices that sumsq_partial's remainder loop reads (ascending); the 4x-unrolled loop reads the others"""
    j = np.arange(n4, dtype=np.int64)
    i = j % STRIDE4
    passes = np.maximum(0, (n4 - i - 3 * STRIDE4 + 4 * STRIDE4 - 1) // (4 * STRIDE4))  # while i + 4*S*c + 3*S < n4
    return j[j // STRIDE4 >= 4 * passes]


def clip_f32(g, clip, defect=None):
    """-> (norm, coefficient) as float32, clip_coef's arithmetic"""
    with np.errstate(all="ignore"):
        norm = F32(np.sqrt(sumsq_f32_order(g, defect)))
        c = F32(clip) / (norm if defect == "no_norm_eps" else norm + F32(1e-6))
    if defect == "coef_not_clamped":
        return norm, c
    return norm, (F32(1.0) if c >= F32(1.0) else c)


def bias_corrections_f32(t):
    """the host's formulas: pow and sqrt in double, the results cast to float"""
    b1, b2 = float(F32(0.9)), float(F32(0.999))
    return F32(1.0) - F32(math.pow(b1, float(t))), F32(math.sqrt(1.0 - math.pow(b2, float(t))))


def step_f32(opt, p, g, s1, s2, t, lr, eps, clip, defect=None, abort=False):
    """one apply as the device runs it; all arrays float32.  -> dict(p, s1, s2, norm, coef)"""
    p, g, s1, s2 = (np.array(x, dtype=F32) for x in (p, g, s1, s2))
    lr, eps = F32(lr), F32(eps)
    norm, cf = clip_f32(g, clip, defect)
    if abort:
        return dict(p=p, s1=s1, s2=s2, norm=norm, coef=F32(-1.0))
    one = F32(1.0)
    with np.errstate(all="ignore"):
        gi = g * cf
        only_step = defect == "coef_on_step_only"  # the update runs on g and the finished step is scaled
        gs = g if defect == "state_from_unclipped" or only_step else gi  # the gradient the state sees
        if opt == "rmsprop":
            alpha = F32(0.99)
            s1 = alpha * s1 + (one - alpha) * gs * gs
            den = np.sqrt(s1 + eps) if defect == "eps_inside_sqrt" else np.sqrt(s1) + eps
            p = p - (lr * (g / den)) * cf if only_step else p - lr * (gi / den)
        else:
            b1, b2 = F32(0.9), F32(0.999)
            bc1, bc2s = bias_corrections_f32(t if defect == "step_not_advancing" else t + 1)
            if defect == "bc2_without_sqrt":
                bc2s = F32(float(bc2s) ** 2)
            if defect == "bc1_dropped":
                bc1 = one
            s1 = b1 * s1 + (one - b1) * gs
            s2 = b2 * s2 + (one - b2) * gs * gs
            den = np.sqrt(s2 / (bc2s * bc2s) + eps) if defect == "eps_inside_sqrt" else np.sqrt(s2) / bc2s + eps
            p = p - ((lr / bc1) * (s1 / den)) * cf if only_step else p - (lr / bc1) * (s1 / den)
    return dict(p=p, s1=s1, s2=s2, norm=norm, coef=cf)


DEFECTS = ("eps_inside_sqrt", "state_from_unclipped", "coef_on_step_only", "coef_not_clamped", "no_norm_eps",
           "bc2_without_sqrt", "bc1_dropped", "step_not_advancing", "last_float4_not_summed", "one_block_not_summed",
           "f32_accumulation", "remainder_tail_skipped")


# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# float32 form against the float64 form with the SAME (kernel) constants, in roundings of float32 (u = 2^-24, gamma_n):
#   norm   the sum of squares is accumulated in double (n * 2^-53, nothing here); sqrt in double, one cast: 1
#   coef   norm (1), + 1e-6f (1), divide (1): 3; the clamp at 1 moves neither value by more
#   gi     = g * cf: 3 + 1 = 4
#   square average (RMSprop's s, Adam's b; all terms >= 0, so relative): the new term (c * gi) * gi carries 2 * 4 + 2
#          = 10, the old one its own E + 1 for the product, the sum 1 more: E_1 = 11 (from a zero state, c * 0 is exact),
#          E_k = max(E_{k-1} + 1, 10) + 1; from a state with E_0 roundings: the same recurrence
#   Adam's a (mixed signs, so in units of A = sum |terms|): the new term (1 - b1) * gi carries 4 + 1 = 5, the old one its
#          own Ea + 1, the sum 1 more of |a| <= A: Ea_k = max(Ea_{k-1} + 1, 5) + 1
#   RMSprop step lr * (gi / (sqrt(s) + eps)): sqrt halves E and adds 1, + eps adds 1 (relative to a LARGER number), the
#          quotient 4 + 1, the product 1: E / 2 + 8
#   Adam step (lr / bc1) * (a / (sqrt(b) / bc2s + eps)): bc1 = 1.0f - (float)pow: the cast errs by u * b1^t, the
#          difference by u * bc1: (1 + b1^t / bc1) roundings, the quotient lr / bc1 one more; bc2s one cast; the denominator
#          Eb / 2 + 1 (sqrt) + 1 (bc2s) + 1 (divide) + 1 (+ eps); the quotient a / den 1, the product 1:
#          |error| <= (lr / bc1) / den * u * (Ea * A + |a| * (Eb / 2 + 8 + b1^t / bc1))
#   p      p - step: one rounding of the new p per apply, on top of the step's error
# Denormal results are exact to 2^-150 instead: ABS_FLOOR covers them in the outputs, and under the square root they move
# the denominator by at most sqrt(64 * 2^-149) = 3e-22 against eps >= 1e-4: 3e-18 of it, inside the slack of SLACK.
COEF_ROUNDINGS, GI_ROUNDINGS = 3, 4
ABS_FLOOR = 64 * 2.0 ** -149
SLACK = 1.0 + 2.0 ** -10  # second-order terms of the products of (1 + u)s, the double roundings under the casts


def sq_avg_roundings(e_prev, zero_state):
    return 11 if zero_state else max(e_prev + 1, 10) + 1


def adam_a_roundings(e_prev, zero_state):
    return 6 if zero_state else max(e_prev + 1, 5) + 1


def f32_bound(opt, ref, a_abs, e_sq, e_a, t_next, lr, eps):
    """per element bounds of |step_f32 - step_f64(KERNEL_CONSTS)| for ONE apply from identical inputs, whose state carried
    e_sq / e_a roundings before (0 and zero_state handled by the caller through sq_avg_roundings / adam_a_roundings):
    ref: step_f64's result; a_abs: the same recurrence as Adam's a over |g * coef| (None for RMSprop); e_sq, e_a: the
    roundings of the NEW state.  -> dict(p, s1, s2, norm, coef)"""
    u = U_F32 * SLACK
    out = dict(norm=_k(1) * SLACK * ref["norm"], coef=_k(COEF_ROUNDINGS) * SLACK * ref["coef"])
    if opt == "rmsprop":
        out["s1"] = e_sq * u * ref["s1"] + ABS_FLOOR
        out["s2"] = np.zeros_like(ref["s1"])
        step_err = (e_sq / 2 + 8) * u * np.abs(ref["step"])
    else:
        bc1, bc2s = bias_corrections_f64(t_next, KERNEL_CONSTS)
        pw = KERNEL_CONSTS["b1"] ** t_next
        out["s1"] = e_a * u * a_abs + ABS_FLOOR
        out["s2"] = e_sq * u * ref["s2"] + ABS_FLOOR
        den = np.sqrt(ref["s2"]) / bc2s + eps
        step_err = (lr / bc1) / den * u * (e_a * a_abs + np.abs(ref["s1"]) * (e_sq / 2 + 8 + pw / bc1))
    out["p"] = step_err + u * np.abs(ref["p"]) + ABS_FLOOR
    return out


# float64 with the kernel's constants against float64 with torch's: relative representation errors of the constants
def const_rel(name):
    return abs(KERNEL_CONSTS[name] - TORCH_CONSTS[name]) / TORCH_CONSTS[name]


def consts_bound(opt, ref, a_abs, k, t_next, lr, eps):
    """per element bound of |step_f64(KERNEL_CONSTS) - step_f64(TORCH_CONSTS)| after k applies from a zero state (p: of the
    k-th step alone; the caller sums).  The constants enter as products, so to first order:
      coef       clip / (norm + e): relative d_c = |e32 - e| / (norm + e), and 0 where the clamp holds on both sides;
      s (>= 0)   sum_j alpha^(k-j) (1 - alpha) gi_j^2: k * d(alpha) + d(1 - alpha) + 2 d_c, relative;
      a          the same with b1 in units of A = sum |terms|: k * d(b1) + d(1 - b1) + d_c;
      bc1        1 - b1^t: t * d(b1) * b1^t / bc1;   bc2 likewise, halved by its square root;
      step       as f32_bound combines them.  SLACK2 covers the second order (the largest factor is 1e-6)."""
    slack2 = 1.001
    d_c = abs(KERNEL_CONSTS["norm_eps"] - TORCH_CONSTS["norm_eps"]) / (ref["norm"] + TORCH_CONSTS["norm_eps"])
    out = {}
    if opt == "rmsprop":
        d_s = (k * const_rel("alpha") + const_rel("one_m_alpha") + 2 * d_c) * slack2
        out["s1"] = d_s * ref["s1"]
        out["step"] = (d_s / 2 + d_c) * slack2 * np.abs(ref["step"])
    else:
        d_a = (k * const_rel("b1") + const_rel("one_m_b1") + d_c) * slack2
        d_b = (k * const_rel("b2") + const_rel("one_m_b2") + 2 * d_c) * slack2
        b1t, b2t = TORCH_CONSTS["b1"] ** t_next, TORCH_CONSTS["b2"] ** t_next
        d_bc1 = t_next * const_rel("b1") * b1t / (1 - b1t)
        d_bc2s = t_next * const_rel("b2") * b2t / (1 - b2t) / 2
        bc1, bc2s = bias_corrections_f64(t_next, TORCH_CONSTS)
        den = np.sqrt(ref["s2"]) / bc2s + eps
        out["s1"] = d_a * a_abs
        out["s2"] = d_b * ref["s2"]
        out["step"] = (lr / bc1) / den * slack2 * (d_a * a_abs + np.abs(ref["s1"]) * (d_b / 2 + d_bc2s + d_bc1))
    return out


# ---- tables by role ---------------------------------------------------------------------------------------------------------------
SENTINEL_EXPONENTS = tuple(range(-12, 14))  # 26 sentinels +-2^k: the squares span 2^-24 .. 2^26, 51 bits: any sum is exact


def sentinel_positions(n4):
    """float indices of the edges of sumsq_partial's structure, each once, then position 0's neighbours for the sentinels
    whose edge does not exist at this length; at most 26 and at most n of them"""
    last = n4 - 1
    edges = [0, 3, 4 * last, 4 * last + 3,  # first and last component of the first and last float4
             4 * 255 + 1, 4 * 256 + 1,  # lanes 255 and 256 of the first visit
             4 * 255 + 2, 4 * 256 + 2]  # = the last float4 of block 0 and the first of block 1
    if n4 > 3 * STRIDE4:  # the four loads of the first unrolled pass: threads 0 .. n4 - 3 * STRIDE4 - 1 take it
        takers = min(STRIDE4, n4 - 3 * STRIDE4)
        for u in range(4):
            edges += [4 * (u * STRIDE4), 4 * (u * STRIDE4 + takers - 1) + 3]
    rem = remainder_float4(n4)
    if rem.size:
        edges += [4 * int(rem[0]) + 1, 4 * int(rem[-1]) + 2]
    pos = []
    for e in edges + [1, 2] + list(range(4, 64)):
        if 0 <= e < 4 * n4 and e not in pos:
            pos.append(e)
    return pos[:len(SENTINEL_EXPONENTS)]


# The norm is all the device shows of the sum, as a float32: a sentinel whose square is below 2^-23 of the sum is invisible
# in it (2^k with k < 2 next to 2^13).  So every length runs three tables, the exponents rotated along the positions by 0, 9
# and 18: each position holds one of the twelve largest sentinels, 2^2 .. 2^13, in at least one of them.
SENTINEL_ROTATIONS = (0, 9, 18)


def sentinel_grads(n4, rot=0):
    """-> (g float32 [4 * n4], exact sum of squares as a Python int scaled by 2^24, positions)"""
    pos = sentinel_positions(n4)
    g = np.zeros(4 * n4, dtype=F32)
    total = 0
    m = len(pos)
    for j, at in enumerate(pos):
        k = SENTINEL_EXPONENTS[(j + rot) % m]
        g[at] = F32((-1.0) ** j * 2.0 ** k)
        total += 1 << (2 * k + 24)
    return g, total, pos


def sentinel_visible(n4, rot):
    """the positions whose sentinel, dropped or doubled, changes float32(sqrt(sum)): its square is 2^-21 of the sum or more"""
    g, total, pos = sentinel_grads(n4, rot)
    return [at for at in pos if float(g[at]) ** 2 * 2.0 ** 24 >= total * 2.0 ** -21]


def sentinel_norm(total):
    """float32(sqrt(exact)): total is the sum of squares * 2^24, below 2^53, so float(total) is exact"""
    assert total < 1 << 53
    return F32(math.sqrt(float(total) * 2.0 ** -24))


def dense_magnitudes(n, seed):
    """per element signed gradient magnitude, fixed over the steps of a run (so that Adam's first moment never cancels and
    every apply of a run moves every weight): log-uniform over 1e-12 .. 1e4, 10 % exact zeros, and a handful whose square
    is denormal (1e-20) or underflows (1e-25, 1e-30)"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-12, 4, n)
    mag[rng.random(n) < 0.1] = 0.0
    small = rng.choice(n, size=min(n, 6), replace=False)
    mag[small] = np.resize([1e-20, 1e-25, 1e-30], small.size)
    return mag * rng.choice([-1.0, 1.0], n)


def dense_seed(n4):
    """the seed of the dense table of a length"""
    return 100 + n4 % 97


def dense_grads(n, seed, step=0):
    """the gradients of apply `step`: the element's signed magnitude times a factor in [0.5, 2) fresh per step"""
    rng = np.random.default_rng([seed, step, 77])
    return (dense_magnitudes(n, seed) * rng.uniform(0.5, 2.0, n)).astype(F32)


def dense_params(opt, g, s1, s2, t, lr, eps, clip, seed):
    """parameters in [-1, 1] on which the first apply is visible: uniform, and where the step of the float64 form would be
    below 2^-14 of the element, a magnitude of 2^4 .. 2^14 steps instead (so every non-zero gradient moves its weight by
    at least 2^-15 of it: 256 ulps)"""
    rng = np.random.default_rng([seed, 78])
    n = g.size
    p = rng.uniform(-1, 1, n)
    step = np.abs(step_f64(opt, p, g, s1, s2, t, lr, eps, clip, KERNEL_CONSTS)["step"])
    small = (step > 0) & (step < np.abs(p) * 2.0 ** -14)
    scaled = step * 2.0 ** rng.integers(4, 15, n) * rng.choice([-1.0, 1.0], n)
    return np.where(small, np.clip(scaled, -1, 1), p).astype(F32)


def moved_ulps(p_before, p_after):
    """|p_after - p_before| in ulps of the larger of the two (float32 arrays)"""
    a, b = np.asarray(p_before, dtype=F32), np.asarray(p_after, dtype=F32)
    big = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(all="ignore"):
        return np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(big).astype(F64)


def ulps(got, want):
    """|got - want| in ulps of want (float32 arrays), 0 where the bits agree"""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)
    return np.where(got.view(np.int32) == want.view(np.int32), 0.0, d)


def same_bits(a, b):
    """the same float32 bits; a NaN equals a NaN (sign and payload of inf * 0 differ between the device and numpy)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=F32)), np.atleast_1d(np.asarray(b, dtype=F32))
    return a.shape == b.shape and bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))
