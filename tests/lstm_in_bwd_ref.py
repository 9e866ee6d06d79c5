"""Float64 reference of ONE call of the LSTM's input-side backward in the R2D2 learner (csrc/learner_r2d2.hip:
lstm_input_backward, reached through rela_debug_lstm_input_backward), between the BPTT and the conv trunk's backward:

  g_w_hh = dg.T @ hprev                                  g_b_ih = g_b_hh = dg.sum(0)
  g_w_ih = (dg.T @ a3) in state_dict order               d_a3 = [a3 > 0] * (dg @ W_ih')
  with a3 channel-last (column pos * 64 + c), weight_ih_l0 and its gradient in state_dict order (column c * 49 + pos) and
  W_ih' the weight in a3's column order.

Plain torch float64 matmuls, none of the project's kernels; tests/test_lstm_in_bwd_ref_cpu.py pins it to float64 autograd.
a3 is an input, so the ReLU mask is data.  `device` only says where the matmuls run.  reference_abs() returns for every
output element the SUM OF ABSOLUTE VALUES OF ITS TERMS (the same function of the absolute values of the inputs with the
mask kept): the scale of err_units and of the exactness preconditions."""
import functools

import numpy as np
import torch

from trunk_bwd_ref import (BF16X2_SEPARATION, U_BF16X2, U_F32, X3_GRAD_SLACK, bf16_hi, bf16_parts, bf16_two,  # noqa: F401
                           err_units, parts_needed, rel_fro)

KEYS = ("g_w_ih", "g_w_hh", "g_b_ih", "g_b_hh", "d_a3")
GEMM_KEYS = ("g_w_ih", "g_w_hh", "d_a3")  # (the bias gradients are one float32 column sum in every mode)
MODES = {"f32": 0, "bf16x2": 1, "f32x3": 2, "f32x3_bwd": 3}  # rela_r2d2_learner_set_precision; f32x3 runs f32's kernels here
UNIT_ROUNDOFF = {"f32": U_F32, "bf16x2": U_BF16X2, "f32x3": U_F32, "f32x3_bwd": U_F32}
GATES, HID, FEAT = 2048, 512, 3136
OUT_SHAPES = {"g_w_ih": (GATES, FEAT), "g_w_hh": (GATES, HID), "g_b_ih": (GATES,), "g_b_hh": (GATES,)}

# Row counts of the GPU test: 1, 2; 31 / 32 / 33 around the K chunk of 32 rows of the weight gradients; 45; 63 / 64 / 65
# around the 64-row M tile of the three-part data gradient and the 64-row record of the rec64 path; 129 = one row past the
# f32 data gradient's 128-row tile; 520; 1,056.
ROWS = (1, 2, 31, 32, 33, 45, 63, 64, 65, 129, 520, 1056)
MAX_ROWS = ROWS[-1]
RANDOM_ROWS = (45, 520, 1056)
GAINS = (1.0, 4.6)

# ---- bounds of the random-data test (tests/test_lstm_input_backward_gpu.py), in units of u * sum|terms| per output element
# The yardstick is not the code under test: float32_evaluation() below -- the same four contractions as torch float32
# matmuls on the CPU -- measured against the float64 reference on random_inputs() at RANDOM_ROWS x GAINS, the largest value
# per output (profiles/lstm_input_backward_error_units.md; tests/test_lstm_in_bwd_ref_cpu.py re-measures all six
# cases and holds the table to them within 1 %).  The bound of a mode with u = 2^-24 is 4 x that value: the project's margin for maxima that move by a factor of two between seeds
# (tests/trunk_bwd_ref.py).  bf16x2 (u = 2^-16: two-part operands, lo * lo dropped, about 2^-16 relative per product) is
# held to the same float32 figures scaled by 2^8, i.e. to the same number of its own units.
# (g_w_ih, g_w_hh and the biases are largest at 45 rows, d_a3 at 520 rows and gain 4.6)
F32_CPU_UNITS = {"g_w_ih": 5.59, "g_w_hh": 4.56, "g_b_ih": 1.15, "g_b_hh": 1.15, "d_a3": 1.56}
BOUND_FACTOR = 4.0


def bound_units(mode, key):
    """in units of UNIT_ROUNDOFF[mode] * sum|terms|"""
    return BOUND_FACTOR * F32_CPU_UNITS[key]


def _to_a3_order(w):
    """[2048, 3136] state_dict columns c * 49 + pos -> channel-last columns pos * 64 + c"""
    return w.reshape(GATES, 64, 49).permute(0, 2, 1).reshape(GATES, FEAT)


def _to_state_dict_order(g):
    return g.reshape(GATES, 49, 64).permute(0, 2, 1).reshape(GATES, FEAT)


def _evaluate(dg, hprev, a3v, a3m, w_ih, unmasked=False, pos_major=False):
    """a3v: the values of a3 (operand of g_w_ih), a3m: its mask"""
    g_ih = dg.t() @ a3v
    d = dg @ _to_a3_order(w_ih)
    bias = dg.sum(0)
    return {"g_w_ih": (g_ih if pos_major else _to_state_dict_order(g_ih)).contiguous(), "g_w_hh": dg.t() @ hprev, "g_b_ih": bias,
            "g_b_hh": bias.clone(), "d_a3": (d if unmasked else a3m * d).reshape(-1, 49, 64)}


def _prep(dg, hprev, a3, w_ih, device, dtype=torch.float64):
    f = lambda x: torch.as_tensor(x).detach().to(device).to(dtype)
    n = f(dg).reshape(-1, GATES).shape[0]
    return f(dg).reshape(n, GATES), f(hprev).reshape(n, HID), f(a3).reshape(n, FEAT), f(w_ih).reshape(GATES, FEAT)


def reference(dg, hprev, a3, w_ih, device="cpu", rnd=None, drop_row=None, unmasked=False, pos_major=False):
    """-> {key: float64 tensor} for KEYS.  The perturbed references of the discrimination checks:
    rnd: a function applied to every GEMM operand (e.g. rounding to one or two bf16 parts); the mask and the column sums
    keep the given data;  drop_row: that row takes no part in any sum and its d_a3 stays zero;  unmasked: d_a3 without
    its ReLU mask;  pos_major: g_w_ih left in a3's column order pos * 64 + c."""
    dg, hprev, a3, w = _prep(dg, hprev, a3, w_ih, device)
    with torch.no_grad():
        mask = (a3 > 0).to(a3.dtype)
        if drop_row is not None:
            dg = dg.clone()
            dg[drop_row] = 0
        r = rnd or (lambda t: t)
        out = _evaluate(r(dg), r(hprev), r(a3), mask, r(w), unmasked, pos_major)
        if rnd is not None:
            out["g_b_ih"] = dg.sum(0)
            out["g_b_hh"] = out["g_b_ih"].clone()
        return out


def reference_abs(dg, hprev, a3, w_ih, device="cpu"):
    dg, hprev, a3, w = _prep(dg, hprev, a3, w_ih, device)
    with torch.no_grad():
        return _evaluate(dg.abs(), hprev.abs(), a3.abs(), (a3 > 0).to(a3.dtype), w.abs())


def float32_evaluation(dg, hprev, a3, w_ih):
    """the same four contractions as float32 torch matmuls on the CPU: the reference-side yardstick of F32_CPU_UNITS"""
    dg, hprev, a3, w = _prep(dg, hprev, a3, w_ih, "cpu", torch.float32)
    with torch.no_grad():
        return _evaluate(dg, hprev, a3, (a3 > 0).to(a3.dtype), w)


# ---- integer data: every product and every partial sum exactly representable ---------------------------------------------
# dg = integers * 2^-6, w_ih = integers * 2^-4, hprev and a3 integers (a3 non-negative, about half of it zero: the mask
# matters): every term of an output is a whole number of UNIT[key], so a float32 sum is exact in any order, tiling and
# precision mode while sum|terms| stays below 2^24 units -- if every PRODUCT is exact.  With three-part operands
# (gemm_bf16x3, PARTS = 3: part i of one operand times part j of the other for i + j <= 2) a product is exact if
# (parts a needs - 1) + (parts b needs - 1) <= 2; with two-part operands and lo * lo dropped (the rec64 path of mode 1) if
# at most one operand needs a lo part and neither needs a third.  Parts are rounded to nearest, so 257 = 256 + 1 needs two
# and WIDE = 2^17 + 2^8 + 1 three.  Both operands of a product share the contraction index, so the data is stratified by it:
#   "by_row"  (f32, f32x3, f32x3_bwd)  the weight gradients contract over rows.  Row r of class r mod 3:
#             0: dg carries WIDE, a3 and hprev one part   1: dg, a3 and hprev carry 257   2: dg one part, a3 and hprev WIDE
#             -- all six part products of dW_ih and dW_hh carry bits.  w_ih has one part (d_a3 meets three-part dg).
#   "by_gate" (f32, f32x3, f32x3_bwd)  d_a3 contracts over gates.  Gate g of class g mod 3:
#             0: dg[:, g] carries WIDE, w_ih[g] one part   1: both carry 257   2: dg[:, g] one part, w_ih[g] carries WIDE
#             -- all six part products of d_a3.  a3 and hprev have one part.
#   "two_part" (every mode)  nothing beyond sixteen bits: dg carries 257 in even rows outside the gates g mod 4 == 3, a3 and
#             hprev carry 257 in odd rows, w_ih carries 257 in the gates g mod 4 == 3 -- the lo part of every operand of the
#             rec64 path is used, and never both in one product.
# A case of n rows uses the first n rows, so sums of absolute values grow with n.
E_D, E_W = 6, 4
UNIT = {"g_w_ih": 2.0 ** -E_D, "g_w_hh": 2.0 ** -E_D, "g_b_ih": 2.0 ** -E_D, "g_b_hh": 2.0 ** -E_D, "d_a3": 2.0 ** -(E_D + E_W)}
WIDE = 2 ** 17 + 2 ** 8 + 1
X3_MODES = ("f32", "f32x3", "f32x3_bwd")
DATA_SETS = {"by_row": X3_MODES, "by_gate": X3_MODES, "two_part": ("f32", "bf16x2", "f32x3", "f32x3_bwd")}


def _small(rng, shape, p_zero16, signed):
    """integers 1..3, zero with probability p_zero16 / 16, random sign if signed; float32"""
    v = rng.integers(1, 4, shape).astype(np.float32)
    if signed:
        v *= (rng.integers(0, 2, shape) * 2 - 1).astype(np.float32)
    v[rng.integers(0, 16, shape) < p_zero16] = 0
    return v


def _widen(rng, t, where, one_in, value):
    """the non-zero entries of t selected by `where` (broadcast against t) become +-value with probability 1 / one_in"""
    hit = (t != 0) & where & (rng.integers(0, one_in, t.shape) == 0)
    t[hit] = np.sign(t[hit]) * np.float32(value)


@functools.lru_cache(maxsize=None)
def exact_data(name):
    rng = np.random.default_rng({"by_row": 411, "by_gate": 422, "two_part": 433}[name])
    n = MAX_ROWS
    dg, hprev = _small(rng, (n, GATES), 4, True), _small(rng, (n, HID), 4, True)
    a3, w = _small(rng, (n, FEAT), 8, False), _small(rng, (GATES, FEAT), 4, True)
    row = np.arange(n)[:, None]
    gate_of_dg, gate_of_w = np.arange(GATES)[None, :], np.arange(GATES)[:, None]
    if name == "by_row":
        _widen(rng, dg, row % 3 == 0, 256, WIDE)
        for t in (a3, hprev):
            _widen(rng, t, row % 3 == 1, 16, 257)
            _widen(rng, t, row % 3 == 2, 128, WIDE)
        _widen(rng, dg, row % 3 == 1, 16, 257)
    elif name == "by_gate":
        _widen(rng, dg, gate_of_dg % 3 == 0, 256, WIDE)
        _widen(rng, dg, gate_of_dg % 3 == 1, 16, 257)
        _widen(rng, w, gate_of_w % 3 == 1, 16, 257)
        _widen(rng, w, gate_of_w % 3 == 2, 256, WIDE)
    else:
        _widen(rng, dg, (row % 2 == 0) & (gate_of_dg % 4 != 3), 16, 257)
        for t in (a3, hprev):
            _widen(rng, t, row % 2 == 1, 16, 257)
        _widen(rng, w, gate_of_w % 4 == 3, 16, 257)
    return {"dg": dg * np.float32(2.0 ** -E_D), "hprev": hprev, "a3": a3.reshape(n, 49, 64), "w_ih": w * np.float32(2.0 ** -E_W)}


def exact_inputs(name, rows):
    d = exact_data(name)
    return {k: (v if k == "w_ih" else np.ascontiguousarray(v[:rows])) for k, v in d.items()}


def _pairs(pa, pb):
    return set(zip(pa.tolist(), pb.tolist()))


def exact_preconditions(name, inp, ref, ref_abs):
    """Asserted on the inputs and the REFERENCE of a case, never on a kernel's output: every product is exact in every mode
    the data set names, and every output's sum|terms| stays below 2^24 units with a whole number of units as its value.
    -> {"rows_a3" | "rows_hprev" | "gates": set of (parts dg needs, parts the other operand needs) over the contraction index}"""
    dg, hprev, a3, w = _prep(inp["dg"], inp["hprev"], inp["a3"], inp["w_ih"], "cpu")
    by_row = lambda t: parts_needed(t, 1)
    dg_row, dg_gate = by_row(dg), parts_needed(dg, 0)
    seen = {"rows_a3": _pairs(dg_row, by_row(a3)), "rows_hprev": _pairs(dg_row, by_row(hprev)), "gates": _pairs(dg_gate, by_row(w))}
    two_part_only = "bf16x2" in DATA_SETS[name]
    for what, pairs in seen.items():
        for pa, pb in pairs:
            assert max(pa - 1, 0) + max(pb - 1, 0) <= 2, "%s, %s: operands of %d and %d parts: gemm_bf16x3 leaves a product out" % (
                name, what, pa, pb)
            if two_part_only:
                assert pa <= 2 and pb <= 2 and not (pa == 2 and pb == 2), "%s, %s: operands of %d and %d parts lose bits in bf16x2" % (
                    name, what, pa, pb)
    for key in KEYS:
        total = float(ref_abs[key].max()) / UNIT[key]
        assert total < 2 ** 24, "%s: sum|terms| of %s reaches %.0f units (>= 2^24)" % (name, key, total)
        val = ref[key] / UNIT[key]
        assert bool((val == val.round()).all()), "%s: %s is not a whole number of units" % (name, key)
    assert bool((a3 == 0).any()) and bool((a3 >= 0).all())  # the mask matters
    return seen


def exact_expected(ref, key):
    return ref[key].cpu().numpy().astype(np.float32)


EXACT_CASES = [(mode, rows) for rows in ROWS for mode in MODES]


# ---- random data as in training -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def random_inputs(rows, gain, seed=7):
    """dg normal, hprev uniform in (-1, 1), a3 = relu(normal), weight_ih_l0 of synth_lstm_params times `gain` (1: the default
    initialisation; 4.6: the scale of a trained agent)"""
    from synth import synth_lstm_params

    rng = np.random.default_rng(seed + 1000 * rows)
    w = synth_lstm_params(6, seed)["lstm.weight_ih_l0"] * np.float32(gain)
    return {"dg": rng.standard_normal((rows, GATES), dtype=np.float32),
            "hprev": rng.uniform(-1, 1, (rows, HID)).astype(np.float32),
            "a3": np.maximum(rng.standard_normal((rows, 49, 64), dtype=np.float32), np.float32(0)), "w_ih": w}


RANDOM_CASES = [(rows, gain) for rows in RANDOM_ROWS for gain in GAINS]
