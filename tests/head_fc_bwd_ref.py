"""Float64 reference of what sits between the Q tables and d_a3 in the Ape-X learner's backward pass, one call at a time:

  rela_debug_loss_grad          loss_reference: batch-global minimum, greedy next action, target, e, Huber, d_ha
  rela_debug_head_fc_backward   reference (csrc/learner.hip: head_fc_backward + the two column sums + head_bias_grad):
      d_h   = [h > 0]  * (d_ha[:, :A] @ fc_a_w + d_ha[:, 31:32] @ fc_v_w)     g_fc_a_w = d_ha[:, :A].T @ h    g_fc_a_b = sum
      d_a3  = [a3 > 0] * (d_h @ Wfc')                                         g_fc_v_w = d_ha[:, 31].T @ h    g_fc_v_b = sum
      g_fc_w = (d_h.T @ a3) in state_dict order                               g_fc_b   = d_h.sum(0)
  with Wfc' the fc weight in a3's channel-last column order (csrc/ffnet_layout.h: column pos * 64 + c <- c * 49 + pos).
  Columns A..30 of d_ha take no part in anything.

Plain torch float64 matmuls, none of the project's kernels; tests/test_head_fc_bwd_ref_cpu.py pins both references to
float64 autograd of tests/f64_ref.py.  The activations are inputs, so the ReLU masks are data.  `device` only says where
the matmuls run.  reference_abs() returns for every output element the SUM OF ABSOLUTE VALUES OF ITS TERMS -- the same
function of the absolute values of the inputs with the masks kept (d_h's own sum of absolute values feeds the fc outputs,
so a term of g_fc_w counts every product behind its d_h) -- the scale of err_units and of the exactness preconditions."""
import functools
import math

import numpy as np
import torch

from trunk_bwd_ref import (BF16X2_SEPARATION, U_BF16X2, U_F32, UNIT_ROUNDOFF, X3_GRAD_SLACK, bf16_hi, err_units,  # noqa: F401
                           needs_lo, rel_fro)

KEYS = ("g_fc_a_w", "g_fc_a_b", "g_fc_v_w", "g_fc_v_b", "g_fc_w", "g_fc_b", "d_h", "d_a3")
MODES = {"f32": 0, "bf16x2": 1, "f32x3": 2}

# ---- bounds of the random-data test (tests/test_head_fc_backward_gpu.py), in units of u * sum|terms| per output element --
# Measured on the MI355X against this reference: per mode, BATCH and output the largest value over the cases of that batch
# in RANDOM_CASES (both gains, both lane forms, A = 31 at 129) and MEASURE_SEEDS (profiles/head_fc_backward_error_units.md).
# Kept per output AND per batch: in these units g_fc_b falls from 2.6 at 5 rows to 0.21 at 1,025 and bf16x2's g_fc_w from
# 2.1 to 0.14, so one bound per output would be the 5-row one and could not fail at 1,025.  bound_units() is 4 x the
# measured value, and never more than the first-order a-priori bound of n_terms units.
MEASURED_UNITS = {
    "f32": {
        5: {"g_fc_a_w": 2.2, "g_fc_a_b": 1.24, "g_fc_v_w": 2.05, "g_fc_v_b": 0.213, "g_fc_w": 3.93,
               "g_fc_b": 2.64, "d_h": 3.05, "d_a3": 1.88},
        129: {"g_fc_a_w": 7.59, "g_fc_a_b": 1.08, "g_fc_v_w": 3.17, "g_fc_v_b": 0.308, "g_fc_w": 4.23,
               "g_fc_b": 0.617, "d_h": 5.99, "d_a3": 2.73},
        257: {"g_fc_a_w": 7.49, "g_fc_a_b": 0.705, "g_fc_v_w": 2.87, "g_fc_v_b": 0.284, "g_fc_w": 4.19,
               "g_fc_b": 0.441, "d_h": 4.26, "d_a3": 2.8},
        1025: {"g_fc_a_w": 7.36, "g_fc_a_b": 0.369, "g_fc_v_w": 3.42, "g_fc_v_b": 0.113, "g_fc_w": 4.04,
               "g_fc_b": 0.212, "d_h": 5.06, "d_a3": 2.96},
    },
    "f32x3": {
        5: {"g_fc_a_w": 2.1, "g_fc_a_b": 1.24, "g_fc_v_w": 2.04, "g_fc_v_b": 0.213, "g_fc_w": 3.45,
               "g_fc_b": 1.67, "d_h": 1.72, "d_a3": 0.843},
        129: {"g_fc_a_w": 3.64, "g_fc_a_b": 1.08, "g_fc_v_w": 1.13, "g_fc_v_b": 0.308, "g_fc_w": 2.49,
               "g_fc_b": 0.546, "d_h": 2.13, "d_a3": 1.16},
        257: {"g_fc_a_w": 3.57, "g_fc_a_b": 0.705, "g_fc_v_w": 0.96, "g_fc_v_b": 0.284, "g_fc_w": 2.32,
               "g_fc_b": 0.413, "d_h": 2.05, "d_a3": 1.12},
        1025: {"g_fc_a_w": 4.04, "g_fc_a_b": 0.369, "g_fc_v_w": 1.24, "g_fc_v_b": 0.113, "g_fc_w": 2.06,
               "g_fc_b": 0.208, "d_h": 2.41, "d_a3": 1.09},
    },
    "bf16x2": {
        5: {"g_fc_a_w": 1.37, "g_fc_a_b": 0.00483, "g_fc_v_w": 1.13, "g_fc_v_b": 0.000832, "g_fc_w": 2.06,
               "g_fc_b": 0.61, "d_h": 0.942, "d_a3": 0.0947},
        129: {"g_fc_a_w": 1.09, "g_fc_a_b": 0.00421, "g_fc_v_w": 0.229, "g_fc_v_b": 0.0012, "g_fc_w": 0.731,
               "g_fc_b": 0.181, "d_h": 0.995, "d_a3": 0.118},
        257: {"g_fc_a_w": 0.6, "g_fc_a_b": 0.00275, "g_fc_v_w": 0.146, "g_fc_v_b": 0.00111, "g_fc_w": 0.308,
               "g_fc_b": 0.0726, "d_h": 1.07, "d_a3": 0.113},
        1025: {"g_fc_a_w": 0.277, "g_fc_a_b": 0.00144, "g_fc_v_w": 0.0669, "g_fc_v_b": 0.000442, "g_fc_w": 0.143,
               "g_fc_b": 0.0391, "d_h": 1.2, "d_a3": 0.12},
    },
}
def n_terms(key, batch, A):
    """the number of products (or summands) behind one element of `key`: a float32 sum of n terms in any order is within
    n * u * sum|terms| of the exact one to first order; d_h's own error reaches the fc outputs through sum|terms|"""
    heads = A + 1
    return {"g_fc_a_w": batch, "g_fc_v_w": batch, "g_fc_a_b": batch, "g_fc_v_b": batch, "d_h": heads,
            "g_fc_b": batch + heads, "g_fc_w": batch + heads, "d_a3": 512 + heads}[key]


def bound_units(mode, key, batch, A):
    return min(4.0 * MEASURED_UNITS[mode][batch][key], float(n_terms(key, batch, A)))


def _perm_fc(w):
    """[512, 3136] state_dict columns c * 49 + pos -> channel-last columns pos * 64 + c"""
    return w.reshape(512, 64, 49).permute(0, 2, 1).reshape(512, 3136)


def _unperm_fc(g):
    return g.reshape(512, 49, 64).permute(0, 2, 1).reshape(512, 3136)


def _evaluate(A, d_ha, hv, hm, a3v, a3m, a_w, v_w, fc_w, d_h_of=None):
    """hv / a3v: the values of h / a3 (weight-gradient operands), hm / a3m: their masks"""
    dA, dV = d_ha[:, :A], d_ha[:, 31:32]
    d_h = hm * (dA @ a_w + dV @ v_w)
    if d_h_of is not None:
        d_h = d_h_of(d_h)
    out = {"g_fc_a_w": dA.t() @ hv, "g_fc_a_b": dA.sum(0), "g_fc_v_w": dV.t() @ hv, "g_fc_v_b": dV.sum(0), "d_h": d_h,
           "d_a3": (a3m * (d_h @ _perm_fc(fc_w))).reshape(-1, 49, 64), "g_fc_w": _unperm_fc(d_h.t() @ a3v).contiguous(),
           "g_fc_b": d_h.sum(0)}
    return out


def _prep(A, d_ha, h, a3, fc_a_w, fc_v_w, fc_w, device):
    f = lambda x: torch.as_tensor(x).detach().to(device).to(torch.float64)
    n = f(d_ha).reshape(-1, 32).shape[0]
    return (f(d_ha).reshape(n, 32), f(h).reshape(n, 512), f(a3).reshape(n, 3136), f(fc_a_w).reshape(A, 512),
            f(fc_v_w).reshape(1, 512), f(fc_w).reshape(512, 3136))


def reference(A, d_ha, h, a3, fc_a_w, fc_v_w, fc_w, device="cpu", rnd=None):
    """-> {key: float64 tensor} for KEYS.  rnd: a function applied to every GEMM operand (the discrimination check)"""
    d, h, a3, aw, vw, fw = _prep(A, d_ha, h, a3, fc_a_w, fc_v_w, fc_w, device)
    r = rnd or (lambda t: t)
    with torch.no_grad():
        hm, a3m = (h > 0).to(h.dtype), (a3 > 0).to(h.dtype)
        if rnd is None:
            return _evaluate(A, d, h, hm, a3, a3m, aw, vw, fw)
        out = _evaluate(A, r(d), r(h), hm, r(a3), a3m, r(aw), r(vw), r(fw), d_h_of=r)
        exact = _evaluate(A, d, h, hm, a3, a3m, aw, vw, fw)
        out["g_fc_a_b"], out["g_fc_v_b"] = exact["g_fc_a_b"], exact["g_fc_v_b"]  # (column sums have no split operands)
        return out


def reference_abs(A, d_ha, h, a3, fc_a_w, fc_v_w, fc_w, device="cpu"):
    d, h, a3, aw, vw, fw = _prep(A, d_ha, h, a3, fc_a_w, fc_v_w, fc_w, device)
    with torch.no_grad():
        return _evaluate(A, d.abs(), h.abs(), (h > 0).to(h.dtype), a3.abs(), (a3 > 0).to(h.dtype), aw.abs(), vw.abs(), fw.abs())


# ---- integer data: every product and every partial sum exactly representable ---------------------------------------------
# d_ha = integers * 2^-6, weights = integers * 2^-4, h / a3 small integers: every term of an output is a whole number of
# UNIT[key], so float32 sums are exact in any order, tiling and precision mode while sum|terms| < 2^24 units.  The bf16x2
# mode multiplies hi + lo operands without lo * lo and the f32x3 mode drops the products of its smallest parts, so a
# product is exact in every mode if ONE operand has at most eight significant bits and the other at most sixteen: d_ha
# carries 257s (needs a lo part) and d_h, an operand of both fc GEMMs, is bounded below 2^16 units; h, a3 and all weights
# have at most two bits.
E_D, E_W = 6, 4
UNIT = {"g_fc_a_w": 2.0 ** -E_D, "g_fc_a_b": 2.0 ** -E_D, "g_fc_v_w": 2.0 ** -E_D, "g_fc_v_b": 2.0 ** -E_D,
        "d_h": 2.0 ** -(E_D + E_W), "g_fc_w": 2.0 ** -(E_D + E_W), "g_fc_b": 2.0 ** -(E_D + E_W), "d_a3": 2.0 ** -(E_D + 2 * E_W)}
EXACT_MAX_BATCH = 1025
DATA_SETS = ("dense", "masked", "last_row")


@functools.lru_cache(maxsize=None)
def _exact_base(name):
    rng = np.random.default_rng({"dense": 311, "masked": 322}[name])
    n = EXACT_MAX_BATCH
    sign = lambda shape: rng.integers(0, 2, shape, dtype=np.int16) * 2 - 1
    small = lambda shape: rng.integers(1, 4, shape, dtype=np.int16)
    d = small((n, 32))
    if name == "dense":  # nothing zero, all masks on; one entry in 16 is 257 (needs a lo part)
        d[rng.integers(0, 16, (n, 32)) == 0] = 257
        d = d * sign((n, 32))
        h, a3 = small((n, 512)), small((n, 3136))
    else:  # about half of h / a3 at or below zero (zeros and negatives); d_ha with zeros and some all-zero rows
        d = d * sign((n, 32)) * (rng.integers(0, 4, (n, 32)) > 0)
        dead = rng.integers(0, 5, n) == 0
        dead[0] = False
        d[dead] = 0
        h, a3 = rng.integers(-2, 4, (n, 512)), rng.integers(-2, 4, (n, 3136))
    w = lambda shape: (small(shape) * sign(shape)).astype(np.float32) * np.float32(2.0 ** -E_W)
    return {"d_ha": d.astype(np.float32) * np.float32(2.0 ** -E_D), "h": h.astype(np.float32), "a3": a3.astype(np.float32),
            "dead": None if name == "dense" else dead, "fc_a_w": w((31, 512)), "fc_v_w": w((1, 512)), "fc_w": w((512, 3136))}


def exact_inputs(name, batch, A):
    """-> dict of numpy arrays in the tap's layouts: the first `batch` rows of the data set and the first A rows of fc_a_w.
    dense: columns A..30 of d_ha keep their non-zero integers (they must not leak); masked: they are zero, and the last
    row is never an all-zero one; last_row: dense with every row of d_ha zero except row batch - 1."""
    b = _exact_base("masked" if name == "masked" else "dense")
    d = b["d_ha"][:batch].copy()
    if name == "masked":
        d[:, A:31] = 0
        if b["dead"][batch - 1]:
            d[batch - 1] = _exact_base("masked")["d_ha"][0]
            d[batch - 1, A:31] = 0
    if name == "last_row":
        d[:batch - 1] = 0
    return {"A": A, "d_ha": d, "h": np.ascontiguousarray(b["h"][:batch]), "a3": np.ascontiguousarray(b["a3"][:batch].reshape(batch, 49, 64)),
            "fc_a_w": np.ascontiguousarray(b["fc_a_w"][:A]), "fc_v_w": b["fc_v_w"], "fc_w": b["fc_w"]}


def exact_preconditions(name, inp, ref, ref_abs):
    """Asserted on the inputs and the REFERENCE of a case, never on a kernel's output: every operand fits the modes' operand
    formats (sixteen significant bits, and of the two operands of every product one has at most eight), and every output's
    sum|terms| stays below 2^24 units with a whole number of units as its value."""
    big = float(ref["d_h"].abs().max()) / UNIT["d_h"]
    assert big < 2 ** 16, "%s: |d_h| reaches %.0f units (>= 2^16)" % (name, big)
    for k in ("d_ha", "h", "a3", "fc_a_w", "fc_v_w", "fc_w"):
        t = torch.as_tensor(inp[k]).double()
        two = t.float() - t.float().to(torch.bfloat16).float()  # what a second bf16 part must hold
        assert bool((two.to(torch.bfloat16).float() == two).all()), "%s: %s does not fit two bf16 parts" % (name, k)
    lo = {k: needs_lo(inp[k]) for k in ("d_ha", "h", "a3", "fc_a_w", "fc_v_w", "fc_w")}
    assert not (lo["h"] or lo["a3"] or lo["fc_a_w"] or lo["fc_v_w"] or lo["fc_w"]), (name, lo)
    for key in KEYS:
        total = float(ref_abs[key].max()) / UNIT[key]
        assert total < 2 ** 24, "%s: sum|terms| of %s reaches %.0f units (>= 2^24)" % (name, key, total)
        val = ref[key] / UNIT[key]
        assert bool((val == val.round()).all()), "%s: %s is not a whole number of units" % (name, key)
    return lo


# (mode, lanes, batch, A).  31 / 33 straddle one K chunk (32) of the weight gradients, 127 / 129 one 128-row tile of the data
# gradients, 257 is an odd chunk count (staging parity) and one row past the 256 column-sum blocks, 1025 is past the
# loss-form switch.  The full A list at 33 and 129, A = 18 elsewhere; every mode and both lane forms everywhere.
EXACT_BATCHES = (1, 31, 33, 127, 129, 257, 1025)
A_LIST = (1, 6, 18, 31)
EXACT_SHAPES = [(n, A) for n in EXACT_BATCHES for A in (A_LIST if n in (33, 129) else (18,))]
EXACT_CASES = [(mode, lanes, n, A) for (n, A) in EXACT_SHAPES for mode in ("f32", "bf16x2", "f32x3") for lanes in (0, 1)]


# ---- random data as in training -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def random_inputs(batch, A, gain, seed=7):
    """h / a3 = relu(normal + 0.126): about 45 % zeros; weights of synth_params at `gain` (1: the default initialisation,
    4.6: the scale of a trained agent); d_ha with the loss kernel's structure: g_b * legal * ([k == a_b] - 1 / A) in
    columns < A, g_b in column 31, zeros in between, g_b = normal / batch, a_b legal"""
    from synth import synth_params

    rng = np.random.default_rng(seed + 1000 * batch + A)
    p = synth_params(A, seed, gain)
    relu = lambda shape: np.maximum(rng.standard_normal(shape, dtype=np.float32) + np.float32(0.126), np.float32(0))
    g = (rng.standard_normal(batch) / batch).astype(np.float32)
    act = rng.integers(0, A, batch)
    legal = (rng.uniform(size=(batch, A)) < 0.7).astype(np.float32)
    legal[np.arange(batch), act] = 1
    d = np.zeros((batch, 32), np.float32)
    ind = np.zeros((batch, A), np.float32)
    ind[np.arange(batch), act] = 1
    d[:, :A] = legal * (g[:, None] * (ind - np.float32(1.0 / A)))
    d[:, 31] = g
    return {"A": A, "d_ha": d, "h": relu((batch, 512)), "a3": relu((batch, 49, 64)), "fc_a_w": p["fc_a.weight"],
            "fc_v_w": p["fc_v.weight"], "fc_w": p["linear.0.weight"]}


# (batch, A, gain, lanes): lanes alternate; A = 31 once at batch 129
RANDOM_CASES = [(5, 18, 1.0, 0), (5, 18, 4.6, 1), (129, 18, 1.0, 1), (129, 18, 4.6, 0), (129, 31, 4.6, 1), (257, 18, 1.0, 0),
                (257, 18, 4.6, 1), (1025, 18, 1.0, 1), (1025, 18, 4.6, 0)]
MEASURE_SEEDS = (7, 21, 22, 23)  # the test runs seed 7; the table's maxima are over all four


# ---- the loss kernels ------------------------------------------------------------------------------------------------------
LOSS_BATCHES = (1, 5, 512, 513, 1024, 1025, 2051)
GAMMA_N = 0.5
GRID = 2.0 ** -5
# rows by index mod 8.  dyadic rows: tables on the 2^-5 grid, gamma_n = 0.5, reward on the 2^-6 grid: e is exact in float32
ROLES = ("small_only_legal_act", "large", "dyadic_plus1", "dyadic_minus1", "dyadic_0", "tie_large", "single_next_legal_small",
         "large_no_bootstrap")


def loss_roles(batch):
    return [ROLES[i % 8] for i in range(batch)]


def _f64(x):
    return torch.as_tensor(x).detach().cpu().to(torch.float64)


def loss_reference(A, q, qno, qnt, nlegal, act, reward, bootstrap, weight, legal, gamma_n=GAMMA_N, e=None, defect=None):
    """float64 from the float32 tables (value rescaling off).  e: the TD errors to continue from (the kernel's own float32
    ones, for the bounds that count the roundings AFTER e); defect: one of the restated defects of the CPU test.
    -> dict: qmin, next_a, target, e, prio, terms (Huber * w per row), loss, g [B], d_ha [B][32]"""
    q, qno, qnt, nlegal, reward, bootstrap, weight, legal = (_f64(t) for t in (q, qno, qnt, nlegal, reward, bootstrap, weight, legal))
    B = q.shape[0]
    q, qno, qnt, nlegal, legal = (t.reshape(B, A) for t in (q, qno, qnt, nlegal, legal))
    act = torch.as_tensor(act).cpu().long()
    rows = torch.arange(B)
    qmin = qno.min()
    lq = (1 + qno - qmin) * nlegal
    next_a = lq.argmax(1)  # (first maximal index)
    if defect == "tie_high":
        next_a = (A - 1) - lq.flip(1).argmax(1)
    target = reward + bootstrap * float(gamma_n) * qnt[rows, next_a]
    if e is None:
        e = target - q[rows, act]
    else:
        e = _f64(e)
    ae = e.abs()
    terms = torch.where(ae < 1, 0.5 * e * e, ae - 0.5) * weight
    clamped = e if defect == "no_clamp" else e.clamp(-1, 1)
    g = -weight * clamped / (1.0 if defect == "no_inv_b" else B)
    mask = nlegal if defect == "next_legal_mask" else legal
    div = mask.sum(1, keepdim=True).clamp(min=1) if defect == "mean_over_legal" else float(A)
    ind = torch.zeros(B, A, dtype=torch.float64)
    ind[rows, act] = 1
    d = torch.zeros(B, 32, dtype=torch.float64)
    d[:, :A] = mask * g[:, None] * (ind - 1.0 / div)
    d[:, 31] = g
    return {"qmin": qmin, "next_a": next_a, "target": target, "e": e, "prio": ae, "terms": terms, "loss": terms.sum() / B,
            "g": g, "d_ha": d}


# Bounds of the loss kernels, DERIVED (u = 2^-24), all counted from the kernel's own float32 e:
#   g_b = -(w * clamp(e)) * fl(1 / B): the product, fl(1 / B) and the second product -- three roundings;
#   column 31 is g_b: within 4 u |g_b| (three roundings, (1 + u)^3 - 1 < 4 u).
#   entry k < A = legal * (g_b * (ind - fl(1 / A))): fl(1 / A), the subtraction and the product -- three more, the factor
#   legal is 0 or 1 and exact; |ind - 1 / A| <= 1: within 8 u |g_b| (six roundings, (1 + u)^6 - 1 < 8 u).
#   loss: a term 0.5 * e * e * w (or (|e| - 0.5) * w) carries three roundings; a lane adds at most ceil(B / 512) terms one
#   after the other, the tree has at most ten levels, then fl(1 / B) and the final product: all terms are >= 0, so the
#   result is within (3 + ceil(B / 512) + 10 + 2) u of sum(terms) / B, to first order; + 1 for the higher orders.
D_HA_UNITS, D_V_UNITS = 8.0, 4.0


def loss_bound_units(batch):
    return 3 + math.ceil(batch / 512) + 10 + 2 + 1


def td_bound(inp, ref):
    """|float32 e - float64 e| per row: target = r + (b * gamma_n) * bq and e = target - q[a] are four float32 roundings of
    quantities no larger than |r| + |b gamma_n bq| + |q[a]|"""
    rows = torch.arange(ref["e"].shape[0])
    A = inp["A"]
    q, qnt = _f64(inp["q"]).reshape(-1, A), _f64(inp["qnt"]).reshape(-1, A)
    mag = _f64(inp["reward"]).abs() + (_f64(inp["bootstrap"]) * GAMMA_N * qnt[rows, ref["next_a"]]).abs() + q[rows, torch.as_tensor(inp["act"]).long()].abs()
    return 4 * U_F32 * mag


@functools.lru_cache(maxsize=4)
def loss_inputs(batch, A, seed=3):
    """float32 tables for rela_debug_loss_grad; check_loss_inputs asserts what the GPU test relies on.  Every table row is a
    permutation of a stretch of the 2^-5 grid (so the entries of a row differ by at least 2^-5) plus, off the dyadic rows,
    noise below 2^-8; the rewards put e into the class of the row's role (ROLES)."""
    rng = np.random.default_rng(seed + 100 * batch + A)
    roles = loss_roles(batch)
    f = np.float32

    def table():
        t = np.stack([rng.permutation(A) for _ in range(batch)]) + rng.integers(-64, 64, (batch, 1))
        t = t.astype(np.float64) * GRID
        for i, r in enumerate(roles):
            if not r.startswith("dyadic"):
                t[i] += rng.uniform(-2.0 ** -8, 2.0 ** -8, A)
        return t.astype(f)

    q, qno, qnt = table(), table(), table()
    nlegal = (rng.uniform(size=(batch, A)) < 0.7).astype(f)
    legal = (rng.uniform(size=(batch, A)) < 0.7).astype(f)
    act = rng.integers(0, A, batch).astype(np.int64)
    legal[np.arange(batch), act] = 1
    boot = np.ones(batch, f)
    for i, r in enumerate(roles):
        if r == "small_only_legal_act":
            legal[i] = 0
            legal[i, act[i]] = 1
        if r == "single_next_legal_small":
            nlegal[i] = 0
            nlegal[i, rng.integers(0, A)] = 1
        if r == "large_no_bootstrap":
            boot[i] = 0
        if nlegal[i].sum() == 0:
            nlegal[i, rng.integers(0, A)] = 1
        if r == "tie_large" and A >= 2:  # two equal maxima among the legal next actions: the lower index must win
            j1, j2 = sorted(rng.choice(A, 2, replace=False))
            nlegal[i, j1] = nlegal[i, j2] = 1
            top = f(qno[i].max() + 4 * GRID)
            qno[i, j1] = qno[i, j2] = top
    base = loss_reference(A, q, qno, qnt, nlegal, act, np.zeros(batch, f), boot, np.ones(batch, f), legal)
    minus = (-base["e"]).numpy()  # e = reward - minus
    want = np.zeros(batch)
    for i, r in enumerate(roles):
        sgn = 1.0 if rng.integers(0, 2) else -1.0
        if "small" in r:
            want[i] = rng.uniform(-0.85, 0.85)
        elif "large" in r:
            want[i] = sgn * rng.uniform(1.15, 3.0)
        else:
            want[i] = {"dyadic_plus1": 1.0, "dyadic_minus1": -1.0, "dyadic_0": 0.0}[r]
    reward = (want + minus).astype(f)
    weight = rng.uniform(0.2, 1.0, batch).astype(f)
    return {"A": A, "q": q, "qno": qno, "qnt": qnt, "nlegal": nlegal, "act": act, "reward": reward, "bootstrap": boot,
            "weight": weight, "legal": legal}


def loss_args(inp):
    return {k: inp[k] for k in ("q", "qno", "qnt", "nlegal", "act", "reward", "bootstrap", "weight", "legal")}


def check_loss_inputs(inp):
    """the properties the GPU test relies on, asserted on the data and its float64 reference; -> the reference"""
    A, batch = inp["A"], inp["q"].shape[0]
    roles = loss_roles(batch)
    ref = loss_reference(A, **loss_args(inp))
    lq = ((1 + _f64(inp["qno"]) - ref["qmin"]) * _f64(inp["nlegal"]))
    nl = _f64(inp["nlegal"])
    assert bool((nl.sum(1) >= 1).all())
    top2 = torch.where(nl > 0, lq, torch.full_like(lq, -1.0)).sort(1, descending=True)[0]
    for i, r in enumerate(roles):
        n_legal = int(nl[i].sum())
        if r == "tie_large" and A >= 2:
            assert float(top2[i, 0]) == float(top2[i, 1]), i
            hi = [j for j in range(A) if float(lq[i, j]) == float(top2[i, 0])]
            assert len(hi) == 2 and int(ref["next_a"][i]) == hi[0]
            assert abs(float(inp["qnt"][i, hi[0]]) - float(inp["qnt"][i, hi[1]])) >= GRID / 2  # the wrong index shows in td
        elif n_legal >= 2:
            assert float(top2[i, 0] - top2[i, 1]) >= 1e-3, (i, float(top2[i, 0] - top2[i, 1]))
        if r == "single_next_legal_small":
            assert n_legal == 1
        e = float(ref["e"][i])
        if "small" in r:
            assert abs(e) <= 0.9, (i, e)
        elif "large" in r:
            assert abs(e) >= 1.1, (i, e)
        else:
            assert e == {"dyadic_plus1": 1.0, "dyadic_minus1": -1.0, "dyadic_0": 0.0}[r], (i, e)
            for k in ("q", "qno", "qnt"):  # dyadic tables; reward on the 2^-6 grid: every float32 operation is exact
                assert bool((inp[k][i] / GRID == np.round(inp[k][i] / GRID)).all())
            assert float(inp["reward"][i]) * 64 == round(float(inp["reward"][i]) * 64)
        assert inp["legal"][i, inp["act"][i]] == 1
        if r == "small_only_legal_act":
            assert inp["legal"][i].sum() == 1
        if r == "large_no_bootstrap":
            assert inp["bootstrap"][i] == 0
    # the entries of a row of qnt differ by more than twice the float32 error of e: td names the greedy next action
    qnt = np.sort(inp["qnt"].astype(np.float64), 1)
    if A >= 2:
        assert float(np.diff(qnt, axis=1).min()) >= GRID - 2.0 ** -7
    return ref


def implied_next_action(inp, td):
    """per row with bootstrap != 0: the index j whose e_j = r + b * gamma_n * qnt[j] - q[a] is nearest the kernel's td (the
    candidates differ by at least gamma_n * (2^-5 - 2^-7), far above float32's error); -1 where bootstrap is 0"""
    A = inp["A"]
    rows = np.arange(inp["q"].shape[0])
    f = np.float64
    cand = inp["reward"].astype(f)[:, None] + inp["bootstrap"].astype(f)[:, None] * GAMMA_N * inp["qnt"].astype(f) - \
        inp["q"].astype(f)[rows, inp["act"]][:, None]
    j = np.abs(cand - np.asarray(td, f)[:, None]).argmin(1)
    return np.where(inp["bootstrap"] != 0, j, -1)
