"""tests/lstm_in_bwd_ref.py on the CPU (no GPU, none of the project's kernels):
  1. the reference equals float64 autograd of x -> W_ih x + b_ih + W_hh h + b_hh with x = relu(z) in state_dict order;
  2. the integer data sets of the GPU test fulfil their exactness preconditions at every row count it uses, and every part
     product of a three-part GEMM is decisive on them;
  3. the checks of the GPU test can fail: a reference that drops a row, rounds its operands to one or two bf16 parts,
     leaves d_a3 unmasked or writes g_w_ih in a3's column order violates the exact expectation and the random-data bounds."""
import numpy as np
import pytest
import torch

import lstm_in_bwd_ref as R


def test_reference_matches_f64_autograd():
    rng = np.random.default_rng(4)
    n, f64 = 3, torch.float64
    z = torch.from_numpy(rng.standard_normal((n, 64, 49))).requires_grad_()  # pre-activation of conv3, [c][pos] as flatten() sees it
    w_ih = torch.from_numpy(rng.standard_normal((R.GATES, R.FEAT)) * 0.05).requires_grad_()
    w_hh = torch.from_numpy(rng.standard_normal((R.GATES, R.HID)) * 0.05).requires_grad_()
    b_ih, b_hh = torch.zeros(R.GATES, dtype=f64, requires_grad=True), torch.zeros(R.GATES, dtype=f64, requires_grad=True)
    h = torch.from_numpy(rng.uniform(-1, 1, (n, R.HID)))
    dg = torch.from_numpy(rng.standard_normal((n, R.GATES)))
    x = torch.relu(z).reshape(n, R.FEAT)  # column c * 49 + pos
    gates = x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
    (gates * dg).sum().backward()
    a3 = torch.relu(z).detach().permute(0, 2, 1).contiguous()  # channel-last [n][49][64]
    assert 0.2 < float((a3 > 0).double().mean()) < 0.8
    ref = R.reference(dg, h, a3, w_ih.detach())
    want = {"g_w_ih": w_ih.grad, "g_w_hh": w_hh.grad, "g_b_ih": b_ih.grad, "g_b_hh": b_hh.grad, "d_a3": z.grad.permute(0, 2, 1)}
    for key in R.KEYS:
        assert ref[key].shape == want[key].shape, key
        scale = float(want[key].abs().max())
        assert scale > 0 and float((ref[key] - want[key]).abs().max()) <= 1e-12 * scale, key
    # the sum of the absolute values of the terms bounds every value, and equals it where nothing has a sign
    ab = R.reference_abs(dg, h, a3, w_ih.detach())
    pos = R.reference(dg.abs(), h.abs(), a3, w_ih.detach().abs())
    for key in R.KEYS:
        assert bool((ab[key] >= ref[key].abs() * (1 - 1e-12)).all()), key
        assert torch.equal(pos[key], ab[key]), key
    # float32_evaluation is the same function in float32
    f32 = R.float32_evaluation(dg, h, a3, w_ih.detach())
    for key in R.KEYS:
        assert f32[key].dtype == torch.float32 and R.rel_fro(f32[key], ref[key]) < 1e-6, key


ALL_PAIRS = {(3, 1), (2, 2), (1, 3)}


@pytest.mark.parametrize("name", sorted(R.DATA_SETS))
def test_integer_data_is_exact_at_every_row_count_of_the_gpu_cases(name):
    for rows in R.ROWS:
        inp = R.exact_inputs(name, rows)
        ref, ab = R.reference(**inp), R.reference_abs(**inp)
        seen = R.exact_preconditions(name, inp, ref, ab)
        for key in R.KEYS:  # the data is not trivial
            assert float((ref[key] != 0).double().mean()) > (0.02 if rows > 2 else 0.0), (key, rows)
        masked = torch.as_tensor(inp["a3"]) == 0
        assert bool(masked.any()) and bool((ref["d_a3"][masked] == 0).all())
        assert bool((R.reference(unmasked=True, **inp)["d_a3"][masked] != 0).any())  # ... and the mask hides something
        if name == "by_row" and rows >= 3:  # every class of rows is there: operands of 3 + 1, 2 + 2 and 1 + 3 parts
            assert ALL_PAIRS <= seen["rows_a3"] and ALL_PAIRS <= seen["rows_hprev"], (rows, seen)
        if name == "by_gate" and rows >= 45:  # (a gate's column of dg needs some rows before it holds a wide entry)
            assert ALL_PAIRS <= seen["gates"], (rows, seen)
        if name == "two_part":
            for what, pairs in seen.items():  # (one row: the even class alone)
                want = {(2, 1)} if rows == 1 and what != "gates" else {(2, 1), (1, 2)}
                assert want <= pairs and (2, 2) not in pairs, (rows, seen)


@pytest.mark.parametrize("rows", [45, 129])
def test_every_part_product_is_decisive(rows):
    """Dropping any one of the six products (part i of dg) * (part j of the other operand), i + j <= 2, from the three-part
    form changes the float32 result: of g_w_ih and g_w_hh on "by_row", of d_a3 on "by_gate"."""
    products = [(i, j) for i in range(3) for j in range(3) if i + j <= 2]
    for name, key in (("by_row", "g_w_ih"), ("by_row", "g_w_hh"), ("by_gate", "d_a3")):
        inp = R.exact_inputs(name, rows)
        ref = R.reference(**inp)
        exp = torch.from_numpy(R.exact_expected(ref, key))
        dg, hprev, a3, w = R._prep(inp["dg"], inp["hprev"], inp["a3"], inp["w_ih"], "cpu")
        pd = R.bf16_parts(dg)
        po = R.bf16_parts({"g_w_ih": a3, "g_w_hh": hprev, "d_a3": R._to_a3_order(w)}[key])
        total = 0
        for i, j in products:
            if key == "d_a3":
                term = ((a3 > 0).double() * (pd[i] @ po[j])).reshape(-1, 49, 64)
            else:
                term = pd[i].t() @ po[j]
                term = R._to_state_dict_order(term) if key == "g_w_ih" else term
            total = total + term
            assert not torch.equal((ref[key] - term).float(), exp), (name, key, i, j)
        assert torch.equal(total, ref[key]), (name, key)  # (the three products left out add nothing)


PERTURBED = {  # name -> (keyword arguments of R.reference, the outputs it touches, the data sets it must show on)
    "last row dropped": (lambda rows: dict(drop_row=rows - 1), R.KEYS, sorted(R.DATA_SETS)),
    "operands rounded to one bf16 part": (lambda rows: dict(rnd=R.bf16_hi), R.GEMM_KEYS, sorted(R.DATA_SETS)),
    "operands rounded to two bf16 parts": (lambda rows: dict(rnd=R.bf16_two), R.GEMM_KEYS, ["by_gate", "by_row"]),
    "d_a3 unmasked": (lambda rows: dict(unmasked=True), ("d_a3",), sorted(R.DATA_SETS)),
    "g_w_ih in a3's column order": (lambda rows: dict(pos_major=True), ("g_w_ih",), sorted(R.DATA_SETS)),
}


@pytest.mark.parametrize("rows", [1, 33, 65])
@pytest.mark.parametrize("what", sorted(PERTURBED))
def test_the_exact_expectation_can_fail(what, rows):
    kwargs, keys, sets = PERTURBED[what]
    for name in sets:
        inp = R.exact_inputs(name, rows)
        ref, bad = R.reference(**inp), R.reference(**inp, **kwargs(rows))
        for key in keys:
            assert not torch.equal(bad[key].float(), ref[key].float()), (what, name, key)


def _violates(bad, ref, ab, key, bound):
    """would the GPU test's check of one output fail?  (err_units itself asserts exact zeros where nothing has a term)"""
    try:
        return R.err_units(bad[key], ref[key], ab[key], 1.0) > bound
    except AssertionError:
        return True


@pytest.mark.parametrize("rows,gain", [(45, 1.0), (1056, 4.6)])
def test_the_random_data_assertions_can_fail(rows, gain):
    """Perturbed references against the exact one, in the units and against the bounds of the GPU test: each exceeds the
    bound of EVERY mode on the outputs it touches.  Two-part operands ARE the bf16x2 mode, so that defect is one of the
    modes with u = 2^-24 only; and since one bound per output (set by the 45-row case) is loose at 1,056 rows, where the
    rounding errors of 1,056 terms average out, it is the other assertion on those modes that must catch it there: the relative
    Frobenius error against X3_GRAD_SLACK x float32's (here the float32 evaluation stands in for the f32 mode)."""
    inp = R.random_inputs(rows, gain)
    ref, ab = R.reference(**inp), R.reference_abs(**inp)
    f32 = R.float32_evaluation(**inp)
    for what, (kwargs, keys, _) in PERTURBED.items():
        bad = R.reference(**inp, **kwargs(rows))
        two = what.endswith("two bf16 parts")
        modes = [m for m in R.MODES if not (two and m == "bf16x2")]
        for key in keys:
            loosest = max(R.bound_units(m, key) * R.UNIT_ROUNDOFF[m] for m in modes)
            caught = _violates(bad, ref, ab, key, loosest)
            if two:
                caught = caught or R.rel_fro(bad[key], ref[key]) > max(R.X3_GRAD_SLACK * R.rel_fro(f32[key], ref[key]), R.U_F32)
            assert caught, "%s on %s passes a bound of %.3g of sum|terms|" % (what, key, loosest)
    # ... and the float32 evaluation the bounds come from passes them with the margin they were given
    for key in R.KEYS:
        assert not _violates(f32, ref, ab, key, R.bound_units("f32", key) * R.U_F32), key


def test_the_bounds_table_is_what_the_float32_evaluation_measures():
    """R.F32_CPU_UNITS, from which every bound of the GPU test comes, IS the largest error of R.float32_evaluation over
    R.RANDOM_CASES (seed 7), to the table's three digits: the bounds cannot drift away from their stated origin.  (The sums
    are torch's float32 matmuls: the figures do not move with the thread count; another BLAS may need the table re-measured.)"""
    worst = {k: 0.0 for k in R.KEYS}
    for rows, gain in R.RANDOM_CASES:
        inp = R.random_inputs(rows, gain)
        ref, ab, f32 = R.reference(**inp), R.reference_abs(**inp), R.float32_evaluation(**inp)
        for k in R.KEYS:
            worst[k] = max(worst[k], R.err_units(f32[k], ref[k], ab[k], R.U_F32))
    for k in R.KEYS:
        assert abs(worst[k] - R.F32_CPU_UNITS[k]) <= 0.01 * R.F32_CPU_UNITS[k], (k, worst[k], R.F32_CPU_UNITS[k])


def test_cases_cover_every_mode_and_row_count():
    assert {m for m, _ in R.EXACT_CASES} == set(R.MODES) and {r for _, r in R.EXACT_CASES} == set(R.ROWS)
    assert set(R.RANDOM_ROWS) <= set(R.ROWS)
    for name, modes in R.DATA_SETS.items():
        assert set(modes) <= set(R.MODES)
    assert all(v > 0 for v in R.F32_CPU_UNITS.values())
