"""Everything between the Q tables and d_a3 in the Ape-X learner, one call at a time (include/rela_amd.h):
  rela_debug_loss_grad          learner_td_loss_grad, or td_kernel + learner_loss_grad (csrc/learner.hip)
  rela_debug_head_fc_backward   the four head / fc GEMMs of csrc/learner.hip: head_fc_backward in their three tile families
                                (gemm_lds f32, gemm_bf16x3 with two and with three parts), the column sums of d_ha and d_h
                                through the learner's multi-job launcher, head_bias_grad
against the float64 references of tests/head_fc_bwd_ref.py:
  a. integer data whose every product and partial sum is exactly representable: all eight outputs EQUAL the reference in
     every mode and lane form, at the batch sizes where K chunks, row tiles and column-sum blocks end;
  b. random data: every output's error in units of u * sum|terms| below 4 x its measured value, f32x3 as accurate as f32
     and bf16x2 measurably not;
  c. the loss kernels: the two forms bit-identical, priorities bit-identical to the float32 restatement, d_ha and loss
     within DERIVED bounds of the float64 reference, greedy ties, the Huber kink, illegal actions and columns A..30;
  d. the tap runs the learner's code path: bit-identical to one learner step's own buffers;
  e. bad arguments are refused.
Every case asserts the kernels it launched.  tests/test_head_fc_bwd_ref_cpu.py pins the references, proves the
preconditions of (a) and (c) and shows that every bound here can fail."""
import ctypes as C
import functools

import numpy as np
import pytest

import head_fc_bwd_ref as R

pytestmark = pytest.mark.gpu

GEMM_FAMILY = {"f32": "gemm_lds (f32)", "bf16x2": "gemm_bf16x3", "f32x3": "gemm_bf16x3"}


def expected_census(mode):
    """every counted launch of one rela_debug_head_fc_backward call (the launch sites that call note_launch): the four
    GEMMs; permute_weights, the column sums and head_bias_grad are launched by sites that count nothing"""
    return {GEMM_FAMILY[mode]: 4}


def expected_loss_census(form, batch):
    """csrc/learner.hip: launch_loss_grad counts the kernels of the form it ran"""
    fused = batch <= 1024 if form == 0 else form == 1
    return {"learner_td_loss_grad": 1} if fused else {"td_kernel": 1, "learner_loss_grad": 1}


def out_shapes(n, A):
    return {"g_fc_a_w": (A, 512), "g_fc_a_b": (A,), "g_fc_v_w": (1, 512), "g_fc_v_b": (1,), "g_fc_w": (512, 3136),
            "g_fc_b": (512,), "d_h": (n, 512), "d_a3": (n, 49, 64)}


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_tap(inp, mode, lanes):
    """inp: {A, d_ha, h, a3, fc_a_w, fc_v_w, fc_w} on the device -> ({key: float32 tensor}, launch census); outputs start
    as NaN, so an element nobody writes cannot pass for a zero"""
    import torch

    from rela_amd import _capi as capi

    n, A = inp["d_ha"].shape[0], inp["A"]
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in out_shapes(n, A).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_head_fc_backward(
            n, A, R.MODES[mode], lanes, ptr(inp["d_ha"]), ptr(inp["h"]), ptr(inp["a3"]), ptr(inp["fc_a_w"]),
            ptr(inp["fc_v_w"]), ptr(inp["fc_w"]), ptr(out["g_fc_a_w"]), ptr(out["g_fc_a_b"]), ptr(out["g_fc_v_w"]),
            ptr(out["g_fc_v_b"]), ptr(out["g_fc_w"]), ptr(out["g_fc_b"]), ptr(out["d_h"]), ptr(out["d_a3"]), _stream()),
            "rela_debug_head_fc_backward")
    torch.cuda.synchronize()
    return out, census.counts


def to_device(inp):
    import torch

    return {k: (v if isinstance(v, int) else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in inp.items()}


@functools.lru_cache(maxsize=3)  # (the three data sets of the current shape: R.EXACT_CASES keeps a shape's cases together)
def exact_case(name, batch, A):
    """-> (inputs on the device, {key: expected float32 values on the device}) with the preconditions asserted on the
    float64 reference (evaluated on the device: the same matmuls); shared by modes and lanes"""
    inp = R.exact_inputs(name, batch, A)
    dev = to_device(inp)
    ref, ab = R.reference(device="cuda", **dev), R.reference_abs(device="cuda", **dev)
    R.exact_preconditions(name, inp, ref, ab)
    return dev, {k: ref[k].float().reshape(out_shapes(batch, A)[k]) for k in R.KEYS}


@pytest.mark.parametrize("mode,lanes,batch,A", R.EXACT_CASES, ids=["%s-lanes%d-%d-A%d" % c for c in R.EXACT_CASES])
def test_exact_data_every_term_counted_once(mode, lanes, batch, A):
    """Integer data (tests/head_fc_bwd_ref.py: exact_inputs): the result does not depend on summation order, tiling, lane
    form or precision mode, so every output element must EQUAL the float64 reference cast to float32 (values: signed
    zeros may differ, NaN equals nothing)."""
    import torch

    for name in R.DATA_SETS:
        inp, want = exact_case(name, batch, A)
        got, counts = run_tap(inp, mode, lanes)
        assert counts == expected_census(mode), (name, counts)
        for key, exp in want.items():
            g = got[key]
            if not torch.equal(g, exp):
                bad = (g != exp).nonzero()
                first = tuple(int(i) for i in bad[0])
                raise AssertionError("%s, batch %d, A %d, lanes %d, data set %s: %s differs in %d of %d elements; first at %s: "
                                     "got %r, expected %r" % (mode, batch, A, lanes, name, key, bad.shape[0], g.numel(), first,
                                                              float(g[first]), float(exp[first])))


def test_reference_on_the_device_equals_the_reference_on_the_cpu():
    """the GPU cases evaluate the float64 matmuls of tests/head_fc_bwd_ref.py on the device: exactly the CPU's on integer
    data, within 1e-12 relative on random data"""
    import torch

    inp = R.exact_inputs("dense", 33, 6)
    cpu, dev = R.reference(**inp), R.reference(device="cuda", **to_device(inp))
    for key in R.KEYS:
        assert torch.equal(cpu[key], dev[key].cpu()), key
    rnd = R.random_inputs(5, 18, 4.6)
    cpu, dev = R.reference(**rnd), R.reference(device="cuda", **to_device(rnd))
    for key in R.KEYS:
        assert float((cpu[key] - dev[key].cpu()).abs().max()) <= 1e-12 * float(cpu[key].abs().max()), key


def measure_random_case(batch, A, gain, lanes, seed=7):
    """-> ({mode: {key: err_units}}, {mode: {key: rel_fro}}) of one random case, census asserted"""
    inp = to_device(R.random_inputs(batch, A, gain, seed))
    ref, ab = R.reference(device="cuda", **inp), R.reference_abs(device="cuda", **inp)
    units, fro = {}, {}
    for mode in ("f32", "f32x3", "bf16x2"):
        got, counts = run_tap(inp, mode, lanes)
        assert counts == expected_census(mode), (mode, counts)
        u = R.UNIT_ROUNDOFF[mode]
        units[mode] = {k: R.err_units(got[k], ref[k], ab[k], u) for k in R.KEYS}
        fro[mode] = {k: R.rel_fro(got[k], ref[k]) for k in R.KEYS}
        print("batch %d A %d gain %.1f lanes %d seed %d %-7s units %s | rel-Frobenius %s" % (
            batch, A, gain, lanes, seed, mode, " ".join("%s=%.3g" % kv for kv in units[mode].items()),
            " ".join("%s=%.3g" % kv for kv in fro[mode].items())))
    return units, fro


# the outputs on which bf16x2 must be BF16X2_SEPARATION x further from float64 than f32x3: every output a GEMM writes
# (measured: at least 19 x, profiles/head_fc_backward_error_units.md).  The separation does NOT hold on g_fc_a_b and
# g_fc_v_b: they are column sums of the given d_ha, the same float32 kernel in every mode (ratio exactly 1).
SEPARATED = ("g_fc_w", "d_a3", "g_fc_a_w", "g_fc_v_w", "d_h", "g_fc_b")


@pytest.mark.parametrize("batch,A,gain,lanes", R.RANDOM_CASES)
def test_random_data_error_in_units_of_each_mode(batch, A, gain, lanes, record_property):
    """Inputs as in training with the masks taken from the given h / a3 (nothing is discontinuous).  Per output element
    |got - ref| / (u * sum|terms|), u = 2^-24 for f32 and f32x3, 2^-16 for bf16x2, against R.bound_units (4 x the value
    measured per mode, batch and output, at most n_terms).  Whatever is measured: f32x3 is no worse than X3_GRAD_SLACK x f32 (or below 2^-24), and
    bf16x2 is at least BF16X2_SEPARATION x further from float64 than f32x3 on SEPARATED; both on the relative Frobenius
    error of the tensor, as tests/test_trunk_backward_gpu.py compares the modes."""
    units, fro = measure_random_case(batch, A, gain, lanes)
    for mode in units:
        for k in R.KEYS:
            record_property("err_units_%s_%s" % (mode, k), units[mode][k])
            bound = R.bound_units(mode, k, batch, A)
            record_property("bound_units_%s_%s" % (mode, k), bound)
            assert units[mode][k] <= bound, (mode, k, units[mode][k], bound)
    for k in R.KEYS:
        assert fro["f32x3"][k] <= max(R.X3_GRAD_SLACK * fro["f32"][k], R.U_F32), (k, fro["f32x3"][k], fro["f32"][k])
    for k in SEPARATED:
        assert fro["bf16x2"][k] >= R.BF16X2_SEPARATION * fro["f32x3"][k], (k, fro["bf16x2"][k], fro["f32x3"][k])


# ---- c. the loss kernels --------------------------------------------------------------------------------------------------
def run_loss(inp, form, vr_eps):
    """inp: R.loss_inputs on the device -> ({td, prio, d_ha, loss} float32 tensors, census); outputs start as NaN"""
    import torch

    from rela_amd import _capi as capi

    n, A = inp["q"].shape[0], inp["A"]
    out = {"td": (n,), "prio": (n,), "d_ha": (n, 32), "loss": (1,)}
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in out.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_loss_grad(
            n, A, form, ptr(inp["q"]), ptr(inp["qno"]), ptr(inp["qnt"]), ptr(inp["nlegal"]), ptr(inp["act"]),
            ptr(inp["reward"]), ptr(inp["bootstrap"]), R.GAMMA_N, vr_eps, ptr(inp["weight"]), ptr(inp["legal"]),
            ptr(out["td"]), ptr(out["prio"]), ptr(out["d_ha"]), ptr(out["loss"]), _stream()), "rela_debug_loss_grad")
    torch.cuda.synchronize()
    return out, census.counts


@pytest.mark.parametrize("A", R.A_LIST)
@pytest.mark.parametrize("batch", R.LOSS_BATCHES)
def test_loss_kernels_two_forms_and_float64(batch, A):
    """R.loss_inputs (properties asserted by R.check_loss_inputs) through the fused kernel (form 1), td_kernel +
    learner_loss_grad (form 2) and the learner's choice (form 0), without and with value rescaling: the forms agree bit for
    bit (the loss up to 512 rows), priorities are td_priority_f32's bits; at vr_eps = 0 against R.loss_reference: td within
    float32's error of e and naming the reference's greedy next action on every bootstrapped row (tie rows included), then
    -- from the kernel's own e -- d_ha, its zeros and the loss within the bounds DERIVED in tests/head_fc_bwd_ref.py."""
    import torch

    from value_rescale_util import td_priority_f32

    inp = R.loss_inputs(batch, A)
    ref = R.check_loss_inputs(inp)
    dev = to_device(inp)
    roles = R.loss_roles(batch)
    for vr_eps in (0.0, 1e-3):
        runs = {}
        for form in (0, 1, 2):
            runs[form], counts = run_loss(dev, form, vr_eps)
            assert counts == expected_loss_census(form, batch), (form, counts)
        one, two = runs[1], runs[2]
        for k in ("td", "prio", "d_ha"):  # (bit patterns: NaN or a signed zero would show)
            assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), (vr_eps, k)
        if batch <= 512:  # the kernel's own claim about its reduction tree
            assert torch.equal(one["loss"].view(torch.int32), two["loss"].view(torch.int32)), vr_eps
        same = one if batch <= 1024 else two
        for k in ("td", "prio", "d_ha", "loss"):
            assert torch.equal(runs[0][k].view(torch.int32), same[k].view(torch.int32)), (vr_eps, k)
        want = td_priority_f32(inp["q"], inp["qno"], inp["qnt"], inp["nlegal"], inp["act"], inp["reward"], inp["bootstrap"],
                               R.GAMMA_N, vr_eps)
        assert np.array_equal(one["prio"].cpu().numpy().view(np.int32), np.asarray(want, np.float32).view(np.int32)), vr_eps
        if vr_eps > 0:
            continue
        for form, got in ((1, one), (2, two)):
            td = got["td"].cpu().double()
            d = got["d_ha"].cpu().double()
            assert bool(((td - ref["e"]).abs() <= R.td_bound(inp, ref)).all()), form
            implied = R.implied_next_action(inp, td.numpy())
            live = implied >= 0
            assert np.array_equal(implied[live], ref["next_a"].numpy()[live]), form
            assert bool((got["prio"].cpu().double() == td.abs()).all())
            after = R.loss_reference(A, e=td, **R.loss_args(inp))  # the roundings AFTER the kernel's own e
            g = after["g"].abs()[:, None]
            assert bool(((d[:, :A] - after["d_ha"][:, :A]).abs() <= R.D_HA_UNITS * R.U_F32 * g).all()), form
            assert bool(((d[:, 31] - after["d_ha"][:, 31]).abs() <= R.D_V_UNITS * R.U_F32 * g[:, 0]).all()), form
            assert bool((d[:, A:31] == 0).all()), form
            illegal = torch.from_numpy(inp["legal"]).double() == 0
            assert bool((d[:, :A][illegal] == 0).all()), form
            loss_err = abs(float(got["loss"].cpu().double()[0]) - float(after["loss"]))
            unit = R.U_F32 * float(after["terms"].abs().sum()) / batch
            print("batch %d A %d form %d: loss error %.3g units, bound %d" % (batch, A, form, loss_err / unit if unit else 0.0,
                                                                           R.loss_bound_units(batch)))
            assert loss_err <= R.loss_bound_units(batch) * unit, (form, loss_err, unit)
            for i, r in enumerate(roles):  # the dyadic rows: e exact, the clamp on the right side of the kink
                if r.startswith("dyadic"):
                    e = {"dyadic_plus1": 1.0, "dyadic_minus1": -1.0, "dyadic_0": 0.0}[r]
                    assert float(td[i]) == e, (i, r, float(td[i]))
                    if e == 0:
                        assert bool((d[i] == 0).all()), i
                    else:  # g = -(w * e) / B with w * e exact: the two roundings of fl(1 / B) and the product
                        gi = -float(inp["weight"][i]) * e / batch
                        assert abs(float(d[i, 31]) - gi) <= 2 * R.U_F32 * abs(gi) * 1.0000001, (i, float(d[i, 31]), gi)
                elif "large" in r:  # the clamp: |g| = w / B whatever |e| >= 1.1 is
                    gi = float(inp["weight"][i]) / batch
                    assert abs(abs(float(d[i, 31])) - gi) <= R.D_V_UNITS * R.U_F32 * gi, (i, r)
                    assert np.sign(float(d[i, 31])) == -np.sign(float(td[i]))


# ---- d. wiring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16x2", "f32x3"])
def test_the_tap_runs_the_learners_code_path(precision):
    """One learner step at B = 200: the learner's own h, a3 (debug_activations) and d_ha (debug_head_grads) through the tap
    give the learner's own d_h, d_a3 and six gradients, bit for bit."""
    import torch

    from rela_amd.learner import HipApexLearner
    from synth import synth_params
    from test_learner_gpu import make_batch

    A, B = 18, 200
    learner = HipApexLearner(A, B, 3, 0.99)
    sd = {k: torch.from_numpy(v) for k, v in synth_params(A, 41, 4.6).items()}
    tg = {k: torch.from_numpy(v) for k, v in synth_params(A, 42, 4.6).items()}
    learner.load_state_dicts(sd, tg)
    learner.set_precision(precision)
    batch, weight = make_batch(B, A, 5)
    learner.backward(batch, weight)
    torch.cuda.synchronize()
    a3, h = learner.debug_activations()[2:]
    d_ha, d_h, d_a3 = learner.debug_head_grads()
    grads = learner.state_dict("grads")
    on = learner.state_dict("online")
    inp = {"A": A, "d_ha": d_ha, "h": h, "a3": a3, "fc_a_w": on["fc_a.weight"], "fc_v_w": on["fc_v.weight"],
           "fc_w": on["linear.0.weight"]}
    got, counts = run_tap(inp, precision, 1)
    assert counts == expected_census(precision), counts
    own = {"g_fc_a_w": grads["fc_a.weight"], "g_fc_a_b": grads["fc_a.bias"], "g_fc_v_w": grads["fc_v.weight"],
           "g_fc_v_b": grads["fc_v.bias"], "g_fc_w": grads["linear.0.weight"], "g_fc_b": grads["linear.0.bias"], "d_h": d_h,
           "d_a3": d_a3}
    assert float(d_ha.abs().max()) > 0 and float(d_a3.abs().max()) > 0
    for key in R.KEYS:
        assert torch.equal(got[key].view(torch.int32).flatten(), own[key].contiguous().view(torch.int32).flatten()), key
    learner.close()


# ---- e. bad arguments -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    import torch

    from rela_amd import _capi as capi

    buf = torch.zeros(2 * 3136, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    for batch, A, mode, lanes in ((0, 6, 0, 0), (-3, 6, 0, 0), (32769, 6, 0, 0), (2, 0, 0, 0), (2, 32, 0, 0), (2, 6, 3, 0),
                                  (2, 6, -1, 0), (2, 6, 0, 2), (2, 6, 0, -1)):
        assert capi.lib.rela_debug_head_fc_backward(*([batch, A, mode, lanes] + [p] * 14 + [None])) == capi.EINVAL
    for hole in range(14):
        args = [2, 6, 0, 0] + [p] * 14 + [None]
        args[4 + hole] = None
        assert capi.lib.rela_debug_head_fc_backward(*args) == capi.EINVAL, hole
    loss_args = lambda batch, A, form: [batch, A, form] + [p] * 7 + [0.5, 0.0] + [p] * 6 + [None]
    for batch, A, form in ((0, 6, 0), (-1, 6, 0), (32769, 6, 0), (2, 0, 0), (2, 32, 0), (2, 6, 3), (2, 6, -1)):
        assert capi.lib.rela_debug_loss_grad(*loss_args(batch, A, form)) == capi.EINVAL
    for hole in list(range(3, 10)) + list(range(12, 18)):
        args = loss_args(2, 6, 0)
        args[hole] = None
        assert capi.lib.rela_debug_loss_grad(*args) == capi.EINVAL, hole
    out = [C.c_void_p() for _ in range(3)]
    assert capi.lib.rela_apex_learner_debug_head_grads(None, *[C.byref(x) for x in out]) == capi.EINVAL
    from rela_amd.learner import HipApexLearner

    learner = HipApexLearner(6, 4, 3, 0.99)
    assert capi.lib.rela_apex_learner_debug_head_grads(learner.h, None, C.byref(out[1]), C.byref(out[2])) == capi.EINVAL
    assert capi.lib.rela_apex_learner_debug_head_grads(learner.h, *[C.byref(x) for x in out]) == capi.ESTATE  # no loss yet
    learner.close()
