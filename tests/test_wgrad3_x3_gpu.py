"""The learners' wgrad3_x3 option: conv3's weight gradient on three-part bf16 operands (csrc/wgrad_conv3_x3.h), through
rela_debug_trunk_backward_opts3 and through both learners.  Reference, data sets, error units and bounds are those of
tests/trunk_bwd_ref.py; the measured units are in profiles/wgrad3_x3_error_units.md."""
import ctypes as C

import pytest

import trunk_bwd_ref as R
from test_dgrad_x3_gpu import _bits_equal, _global_rng_untouched, _step, census_with_x3  # noqa: F401 (the autouse fixture)
from test_trunk_backward_gpu import FAST_WGRAD_MIN_FRAMES, MODES, OUT_SHAPES, exact_case, expected_census, to_device
from test_wgrad_x3_gpu import census_with_wx3

pytestmark = pytest.mark.gpu

KERNEL = "wgrad_conv3_x3"
DGRAD, WGRAD, WGRAD3 = 1, 2, 4  # bits of `opts`
# frames are strided over min(frames, 256) blocks: one frame, two, the cap - 1, the cap, the cap + 1, 2 x cap + 1; then all
# three options at once, and the bf16x2 mode on either side of the frame count from which it has a conv3 kernel of its own
EXACT_CASES = ([(mode, lanes, n, WGRAD3, 0) for mode in ("f32", "f32x3") for lanes in (0, 1) for n in (1, 2, 255, 256, 257, 513)] +
               [("f32x3", 1, 257, DGRAD | WGRAD | WGRAD3, 0), ("bf16x2", 1, 257, WGRAD3, 0), ("bf16x2", 0, 257, WGRAD3, 256)])
EXACT_CASES.sort(key=lambda c: c[2])  # (cases of one frame count share their inputs and reference)


def run_tap(inp, mode, lanes, opts, min_frames=0):
    """device inputs {obs, a1, a2, d_a3, w2, w3} -> ({key: f32 tensor}, census); outputs start as NaN"""
    import torch

    from rela_amd import _capi as capi

    n = inp["obs"].shape[0]
    shapes = dict(OUT_SHAPES, d_a2=(n, 81, 64), d_a1=(n, 400, 32))
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in shapes.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_trunk_backward_opts3(
            n, MODES[mode], lanes, min_frames, opts, *[ptr(inp[k]) for k in ("obs", "a1", "a2", "d_a3", "w2", "w3")],
            *[ptr(out[k]) for k in R.KEYS], C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "rela_debug_trunk_backward_opts3")
    torch.cuda.synchronize()
    return out, dict(census.counts)


def census_with_w3x3(mode, frames, opts, min_frames=0):
    """the census without bit 2 with conv3's one weight-gradient launch replaced (reduce_splits is not a counted launch)"""
    want = (census_with_wx3(mode, frames, opts & DGRAD) if opts & WGRAD else
            census_with_x3(mode, frames) if opts & DGRAD else expected_census(mode, frames, min_frames))
    fast = mode == "bf16x2" and frames >= (min_frames or FAST_WGRAD_MIN_FRAMES)
    old = "wgrad_conv3_bf16" if fast else {"f32": "gemm_lds (f32)"}.get(mode, "gemm_bf16x3")
    want = dict(want, **{KERNEL: 1, old: want[old] - 1})
    return {k: v for k, v in want.items() if v}


@pytest.mark.parametrize("mode,lanes,frames,opts,min_frames", EXACT_CASES, ids=["%s-lanes%d-%d-opts%d-min%d" % c for c in EXACT_CASES])
def test_exact_data_through_the_new_tap(mode, lanes, frames, opts, min_frames):
    import torch

    for name in ("dense", "sparse"):
        inp, want = exact_case(name, frames)  # (asserts the preconditions on the reference)
        got, counts = run_tap(inp, mode, lanes, opts, min_frames)
        assert counts == census_with_w3x3(mode, frames, opts, min_frames), (name, counts)
        for key in R.DATA_SETS[name]["exact"]:
            assert torch.equal(got[key], want[key]), (name, key, int((got[key] != want[key]).sum()))


@pytest.mark.parametrize("frames,gain,lanes", [(3, 4.6, 1), (257, 1.0, 0), (513, 4.6, 1)])
def test_random_data_error_in_units(frames, gain, lanes, record_property):
    """|got - float64| / (2^-24 * sum|terms|) per output against R.BOUND_UNITS["f32x3"], for g_c3w the bound of the three-part
    GEMM the kernel replaces.  The option moves nothing but g_c3w, and a second run gives the first one's bits."""
    inp = to_device(R.random_inputs(frames, gain))
    ref, ab = R.reference(device="cuda", **inp), R.reference_abs(device="cuda", **inp)
    for mode in ("f32", "f32x3"):
        got, counts = run_tap(inp, mode, lanes, WGRAD3)
        again, _ = run_tap(inp, mode, lanes, WGRAD3)
        off, _ = run_tap(inp, mode, lanes, 0)
        assert counts == census_with_w3x3(mode, frames, WGRAD3), (mode, counts)
        units = {k: R.err_units(got[k], ref[k], ab[k], R.U_F32) for k in R.KEYS}
        for k in R.KEYS:
            record_property("err_units_%s_w3x3_%s" % (mode, k), units[k])
        print(frames, gain, lanes, mode, "units", " ".join("%s=%.3g" % kv for kv in units.items()))
        for k in R.KEYS:
            assert units[k] <= R.BOUND_UNITS["f32x3"][k], (mode, k, units[k])
            assert _bits_equal(got[k], again[k]), (mode, k)
            assert k == "g_c3w" or _bits_equal(got[k], off[k]), (mode, k)


def _only_conv3s_weight_moves(off, on, tap):
    """loss, priorities and every gradient but net.4.weight as with the option off; that one is the tap's; the new kernel
    once, in place of one three-part GEMM"""
    assert on[3].get(KERNEL) == 1 and KERNEL not in off[3], (off[3], on[3])
    assert on[3]["gemm_bf16x3"] == off[3]["gemm_bf16x3"] - 1
    assert _bits_equal(off[0], on[0]) and _bits_equal(off[1], on[1])
    for key in off[2]:
        assert key == "net.4.weight" or _bits_equal(off[2][key], on[2][key]), key
    assert _bits_equal(tap["g_c3w"], on[2]["net.4.weight"]) and float(tap["g_c3w"].abs().max()) > 0


def test_apex_learner_wiring():
    """A = 6, B = 32, f32x3, against the tap (two lanes, bit 2) fed with the learner's own obs, a1, a2, d_a3 and weights"""
    import torch

    from rela_amd.learner import HipApexLearner
    from synth import synth_params
    from test_learner_gpu import make_batch

    A, B = 6, 32
    sd, tg = ({k: torch.from_numpy(v) for k, v in synth_params(A, seed, 4.6).items()} for seed in (41, 42))
    batch, weight = make_batch(B, A, 5)
    res = {}
    for on in (False, True):
        learner = HipApexLearner(A, B, 3, 0.99)
        learner.load_state_dicts(sd, tg)
        learner.set_precision("f32x3")
        learner.set_wgrad3_x3(on)
        res[on] = _step(learner, batch, weight)
        if on:
            w = learner.state_dict("online")
            inp = {"obs": batch.obs["s"], "a1": learner.debug_activations()[0], "a2": learner.debug_activations()[1],
                   "d_a3": learner.debug_head_grads()[2], "w2": w["net.2.weight"], "w3": w["net.4.weight"]}
            tap, _ = run_tap(inp, "f32x3", 1, WGRAD3)
        learner.close()
    _only_conv3s_weight_moves(res[False], res[True], tap)


def test_r2d2_learner_wiring():
    """the smallest shape of tests/test_r2d2_learner_bwd_mode_gpu.py in f32x3_bwd, against the tap (one lane, bit 2) fed with
    the training rows' frames and the learner's own a1, a2, d_a3 and weights"""
    from test_r2d2_learner_bwd_mode_gpu import SMALL, _case, _learner

    _, batch, weight = _case(SMALL)
    res = {}
    for on in (False, True):
        learner = _learner(SMALL, "f32x3_bwd")
        learner.set_wgrad3_x3(on)  # (after the load)
        res[on] = _step(learner, batch, weight)
        learner.check()
        if on:
            w = learner.state_dict("online")
            a1, a2, d_a3 = learner.debug_trunk()
            obs = batch.obs["s"][SMALL[3]:].reshape(-1, 4, 84, 84).contiguous()  # (as many rows as a1 has)
            tap, _ = run_tap({"obs": obs, "a1": a1, "a2": a2, "d_a3": d_a3, "w2": w["net.2.weight"], "w3": w["net.4.weight"]},
                             "f32x3", 0, WGRAD3)
        learner.close()
    _only_conv3s_weight_moves(res[False], res[True], tap)


def test_bad_arguments_are_refused():
    from rela_amd import _capi as capi
    from rela_amd.learner import HipApexLearner, HipR2D2Learner

    for learner, setter in ((HipApexLearner(6, 4, 2, 0.99), capi.lib.rela_apex_learner_set_wgrad3_x3),
                            (HipR2D2Learner(6, 4, 2, 0.99, 7, 0, 0.9), capi.lib.rela_r2d2_learner_set_wgrad3_x3)):
        assert setter(learner.h, 2) == capi.EINVAL and b"_set_wgrad3_x3" in capi.lib.rela_last_error()
        assert setter(None, 1) == capi.EINVAL
        assert setter(learner.h, 1) == capi.OK and setter(learner.h, 0) == capi.OK
        learner.close()
    obs = to_device(R.exact_inputs("dense", 2))["obs"]
    p = C.c_void_p(obs.data_ptr())
    for mode, opts, d_a1 in ((0, 8, p), (0, 12, p), (3, WGRAD3, p), (3, 0, p), (0, WGRAD3, None)):  # (refused before any launch)
        assert capi.lib.rela_debug_trunk_backward_opts3(*([2, mode, 0, 0, opts] + [p] * 13 + [d_a1, None])) == capi.EINVAL
