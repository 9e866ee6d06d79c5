"""The LSTM's input-side backward of the R2D2 learner (csrc/learner_r2d2.hip: lstm_input_backward -- dW_hh, dW_ih, the gate
column sum copied into both bias gradients, d_a3 with its ReLU mask) one call at a time, through
rela_debug_lstm_input_backward, against the float64 reference of the same call (tests/lstm_in_bwd_ref.py), in the four
precision modes of the learner: gemm_lds with ProbWhh / ProbWih / ProbIhDgrad (modes 0 and 2), the rec64 path --
split_cols_rec64, split_rows_rec64, gemm_rec64_nt with EpiPlain / EpiReluMask -- (mode 1) and gemm_bf16x3 with three-part
operands on 64 x 64 tiles (mode 3).  a3 is an input of the call, so the mask is data and the only error left is the
kernels' arithmetic:
  a. integer data whose every product and partial sum is exactly representable: all five outputs EQUAL the reference, at
     the row counts where K chunks, M tiles and 64-row records go wrong, on data that makes every part product decisive;
  b. random data: the error of every output element in units of u * sum|terms| stays below 4 x what a float32 evaluation
     on the CPU shows, mode 3 is as accurate as mode 0 and mode 1 is measurably not (else it ran other kernels);
and every case asserts the kernels it launched.  tests/test_lstm_in_bwd_ref_cpu.py pins the reference, proves the
preconditions of (a) and shows that the checks can fail."""
import ctypes as C
import functools

import numpy as np
import pytest

import lstm_in_bwd_ref as R

pytestmark = pytest.mark.gpu

# every counted launch of one call (the launch sites that call note_launch): the three GEMMs; the pack kernels, the rec64
# splits, the column sum and the copy are launched by sites that count nothing
CENSUS = {"f32": {"gemm_lds (f32)": 3}, "f32x3": {"gemm_lds (f32)": 3}, "f32x3_bwd": {"gemm_bf16x3": 3},
          "bf16x2": {"gemm_rec64_nt": 3}}


def out_shapes(rows):
    return dict(R.OUT_SHAPES, d_a3=(rows, 49, 64))


def run_tap(inp, mode):
    """inp: {dg, hprev, a3, w_ih} on the device -> ({key: float32 tensor}, launch census); outputs start as NaN, so an
    element nobody writes cannot pass for a zero"""
    import torch

    from rela_amd import _capi as capi

    rows = inp["dg"].shape[0]
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in out_shapes(rows).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_lstm_input_backward(
            rows, R.MODES[mode], ptr(inp["dg"]), ptr(inp["hprev"]), ptr(inp["a3"]), ptr(inp["w_ih"]), ptr(out["g_w_ih"]),
            ptr(out["g_w_hh"]), ptr(out["g_b_ih"]), ptr(out["g_b_hh"]), ptr(out["d_a3"]),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rela_debug_lstm_input_backward")
    torch.cuda.synchronize()
    return out, census.counts


def to_device(inp):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}


@functools.lru_cache(maxsize=len(R.DATA_SETS))  # (the data sets of the current row count: R.EXACT_CASES keeps its modes together)
def exact_case(name, rows):
    """-> (inputs on the device, {key: expected float32 values on the device}) with the preconditions asserted on the
    float64 reference (evaluated on the device: the same matmuls); shared by the modes"""
    import torch

    inp = R.exact_inputs(name, rows)
    dev = to_device(inp)
    ref, ab = R.reference(device="cuda", **dev), R.reference_abs(device="cuda", **dev)
    R.exact_preconditions(name, inp, ref, ab)
    return dev, {k: torch.from_numpy(R.exact_expected(ref, k)).cuda() for k in R.KEYS}


@pytest.mark.parametrize("mode,rows", R.EXACT_CASES, ids=["%s-%d" % c for c in R.EXACT_CASES])
def test_exact_data_every_term_counted_once(mode, rows):
    """Integer data (tests/lstm_in_bwd_ref.py: exact_data): the result does not depend on summation order, tiling or
    precision mode, so every output element must EQUAL the float64 reference cast to float32 (values: signed zeros may
    differ, NaN equals nothing) in every mode the data set names."""
    import torch

    for name in sorted(R.DATA_SETS):
        if mode not in R.DATA_SETS[name]:
            continue
        inp, want = exact_case(name, rows)
        got, counts = run_tap(inp, mode)
        assert counts == CENSUS[mode], (name, counts)
        for key, exp in want.items():
            g = got[key]
            if not torch.equal(g, exp):
                bad = (g != exp).nonzero()
                first = tuple(int(i) for i in bad[0])
                raise AssertionError("%s, %d rows, data set %s: %s differs in %d of %d elements; first at %s: got %r, "
                                     "expected %r" % (mode, rows, name, key, bad.shape[0], g.numel(), first, float(g[first]),
                                                      float(exp[first])))


def test_reference_on_the_device_equals_the_reference_on_the_cpu():
    """the GPU cases evaluate the float64 matmuls of tests/lstm_in_bwd_ref.py on the device: exactly the CPU's on integer
    data, within 1e-12 relative on random data"""
    import torch

    inp = R.exact_inputs("by_row", 33)
    cpu, dev = R.reference(**inp), R.reference(device="cuda", **to_device(inp))
    for key in R.KEYS:
        assert torch.equal(cpu[key], dev[key].cpu()), key
    rnd = R.random_inputs(45, 4.6)
    cpu, dev = R.reference(**rnd), R.reference(device="cuda", **to_device(rnd))
    for key in R.KEYS:
        assert float((cpu[key] - dev[key].cpu()).abs().max()) <= 1e-12 * float(cpu[key].abs().max()), key


def test_bad_arguments_are_refused():
    import torch

    from rela_amd import _capi as capi

    inp = to_device(R.exact_inputs("two_part", 2))
    p = C.c_void_p(inp["dg"].data_ptr())
    for rows, mode in ((0, 0), (-3, 0), (32769, 0), (2, 4), (2, -1)):
        assert capi.lib.rela_debug_lstm_input_backward(*([rows, mode] + [p] * 9 + [None])) == capi.EINVAL
    for hole in range(9):
        args = [2, 0] + [p] * 9 + [None]
        args[2 + hole] = None
        assert capi.lib.rela_debug_lstm_input_backward(*args) == capi.EINVAL, hole
    # an output that overlaps another buffer of the call is refused before anything is launched: one pointer for
    # everything, and a valid call whose g_b_hh is its g_b_ih
    for mode in R.MODES.values():
        assert capi.lib.rela_debug_lstm_input_backward(*([2, mode] + [p] * 9 + [None])) == capi.EINVAL, mode
        assert b"overlaps" in capi.lib.rela_last_error()
    out = {k: torch.zeros(s, device="cuda") for k, s in out_shapes(2).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = [2, 0] + [ptr(inp[k]) for k in ("dg", "hprev", "a3", "w_ih")] + \
        [ptr(out[k]) for k in ("g_w_ih", "g_w_hh", "g_b_ih", "g_b_ih", "d_a3")] + [None]
    assert capi.lib.rela_debug_lstm_input_backward(*args) == capi.EINVAL


def measure_random_case(rows, gain, seed=7):
    """-> ({mode: {key: err_units}}, {mode: {key: rel_fro}}) of one random case, census asserted"""
    inp = to_device(R.random_inputs(rows, gain, seed))
    ref, ab = R.reference(device="cuda", **inp), R.reference_abs(device="cuda", **inp)
    units, fro = {}, {}
    for mode in R.MODES:
        got, counts = run_tap(inp, mode)
        assert counts == CENSUS[mode], (mode, counts)
        u = R.UNIT_ROUNDOFF[mode]
        units[mode] = {k: R.err_units(got[k], ref[k], ab[k], u) for k in R.KEYS}
        fro[mode] = {k: R.rel_fro(got[k], ref[k]) for k in R.KEYS}
        print("rows %d gain %.1f seed %d %-9s units %s | rel-Frobenius %s" % (
            rows, gain, seed, mode, " ".join("%s=%.3g" % kv for kv in units[mode].items()),
            " ".join("%s=%.3g" % kv for kv in fro[mode].items())))
    return units, fro


@pytest.mark.parametrize("rows,gain", R.RANDOM_CASES)
def test_random_data_error_in_units_of_each_mode(rows, gain, record_property):
    """Inputs as in training with the mask taken from the given a3 (nothing is discontinuous).  Per output element
    |got - ref| / (u * sum|terms|), u = 2^-24 for modes 0, 2 and 3 and 2^-16 for mode 1, against R.bound_units: 4 x what the
    same contractions in float32 on the CPU show against float64 (measured on the reference side, see there).  Whatever is
    measured: mode 3 is no worse than X3_GRAD_SLACK x mode 0 (or below 2^-24), and mode 1 is at least BF16X2_SEPARATION x
    further from float64 than mode 3 on g_w_ih and d_a3; both on the relative Frobenius error of the tensor, as
    tests/test_trunk_backward_gpu.py compares the modes.  Every figure is printed and recorded before anything is asserted."""
    units, fro = measure_random_case(rows, gain)
    for mode in units:
        for k in R.KEYS:
            record_property("err_units_%s_%s" % (mode, k), units[mode][k])
            record_property("rel_fro_%s_%s" % (mode, k), fro[mode][k])
            record_property("bound_units_%s_%s" % (mode, k), R.bound_units(mode, k))
    for k in R.KEYS:
        record_property("f32x3_bwd_over_f32_rel_fro_%s" % k, fro["f32x3_bwd"][k] / max(fro["f32"][k], 1e-300))
        record_property("bf16x2_over_f32x3_bwd_rel_fro_%s" % k, fro["bf16x2"][k] / max(fro["f32x3_bwd"][k], 1e-300))
    for mode in units:
        for k in R.KEYS:
            assert units[mode][k] <= R.bound_units(mode, k), (mode, k, units[mode][k], R.bound_units(mode, k))
    for k in R.KEYS:  # (an error below one unit roundoff of the tensor's norm is below what float32 resolves)
        assert fro["f32x3_bwd"][k] <= max(R.X3_GRAD_SLACK * fro["f32"][k], R.U_F32), (k, fro["f32x3_bwd"][k], fro["f32"][k])
    for k in ("g_w_ih", "d_a3"):
        assert fro["bf16x2"][k] >= R.BF16X2_SEPARATION * fro["f32x3_bwd"][k], (k, fro["bf16x2"][k], fro["f32x3_bwd"][k])
    for k in R.KEYS:  # mode 2 runs mode 0's kernels here: the same bits
        assert units["f32x3"][k] == units["f32"][k] and fro["f32x3"][k] == fro["f32"][k], k
