"""The backward pass of the conv trunk (csrc/learner_common.hip: trunk_backward -- wgrad_conv{1,2,3}_bf16, dgrad_conv{2,3}_bf16,
the f32 / three-part split-K GEMMs with col2im2/3, reduce_splits, the column sums) one call at a time, through
rela_debug_trunk_backward, against the float64 reference of the same call (tests/trunk_bwd_ref.py).  The activations are
inputs of the call, so the ReLU masks are data and the only error left is the kernels' arithmetic:
  a. integer data whose every product and partial sum is exactly representable: all eight outputs EQUAL the reference, in
     every precision mode and lane form, at the frame counts where persistent kernels and split-K GEMMs go wrong;
  b. random data: the error of every output element in units of u * sum|terms| stays below a bound measured per mode,
     f32x3 is as accurate as f32 and bf16x2 is measurably not (else it ran other kernels);
and every case asserts the kernels it launched.  tests/test_trunk_bwd_ref_cpu.py pins the reference, proves the
preconditions of (a) and shows that the bounds of (b) can fail."""
import ctypes as C
import functools

import numpy as np
import pytest

import trunk_bwd_ref as R

pytestmark = pytest.mark.gpu

MODES = {"f32": 0, "bf16x2": 1, "f32x3": 2}
FAST_WGRAD_MIN_FRAMES = 2048  # csrc/learner_plan.h: kFastWgradMinFrames
OUT_SHAPES = {"g_c1w": (32, 4, 8, 8), "g_c1b": (32,), "g_c2w": (64, 32, 4, 4), "g_c2b": (64,), "g_c3w": (64, 64, 3, 3),
              "g_c3b": (64,)}


def expected_census(mode, frames, min_frames):
    """every counted launch of one trunk_backward call (the launch sites that call note_launch)"""
    if mode == "f32":  # three weight-gradient GEMMs, two data-gradient GEMMs
        return {"gemm_lds (f32)": 5}
    if mode == "f32x3":  # the weight gradients with three-part operands, the data gradients (K = 64) in f32
        return {"gemm_bf16x3": 3, "gemm_lds (f32)": 2}
    want = {"wgrad_conv1_bf16": 1, "dgrad_conv2_bf16": 1, "dgrad_conv3_bf16": 1}
    if frames >= (min_frames if min_frames > 0 else FAST_WGRAD_MIN_FRAMES):
        want.update({"wgrad_conv2_bf16": 1, "wgrad_conv3_bf16": 1})
    else:
        want["gemm_bf16x3"] = 2
    return want


def run_tap(inp, mode, lanes, min_frames):
    """inp: {obs, a1, a2, d_a3, w2, w3} on the device -> ({key: float32 tensor}, launch census); outputs start as NaN, so
    an element nobody writes cannot pass for a zero"""
    import torch

    from rela_amd import _capi as capi

    n = inp["obs"].shape[0]
    shapes = dict(OUT_SHAPES, d_a2=(n, 81, 64), d_a1=(n, 400, 32))
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in shapes.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_trunk_backward(
            n, MODES[mode], lanes, min_frames, ptr(inp["obs"]), ptr(inp["a1"]), ptr(inp["a2"]), ptr(inp["d_a3"]),
            ptr(inp["w2"]), ptr(inp["w3"]), ptr(out["g_c1w"]), ptr(out["g_c1b"]), ptr(out["g_c2w"]), ptr(out["g_c2b"]),
            ptr(out["g_c3w"]), ptr(out["g_c3b"]), ptr(out["d_a2"]), ptr(out["d_a1"]),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rela_debug_trunk_backward")
    torch.cuda.synchronize()
    return out, census.counts


def to_device(inp):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}


@functools.lru_cache(maxsize=2)  # (the two data sets of the current frame count: R.EXACT_CASES is sorted by it)
def exact_case(name, frames):
    """-> (inputs on the device, {key: expected float32 values on the device}) with the preconditions asserted on the
    float64 reference (evaluated on the device: the same matmuls, tests/trunk_bwd_ref.py); shared by modes and lanes"""
    import torch

    inp = to_device(R.exact_inputs(name, frames))
    ref, ab = R.reference(device="cuda", **inp), R.reference_abs(device="cuda", **inp)
    R.exact_operand_preconditions(name, inp, ref)
    R.exact_preconditions(name, ref, ab)
    want = {k: torch.from_numpy(R.exact_expected(ref, k)).cuda() for k in R.DATA_SETS[name]["exact"]}
    return inp, want


@pytest.mark.parametrize("mode,lanes,frames,min_frames", R.EXACT_CASES,
                         ids=["%s-lanes%d-%d-min%d" % c for c in R.EXACT_CASES])
def test_exact_data_every_term_counted_once(mode, lanes, frames, min_frames):
    """Integer data (tests/trunk_bwd_ref.py: exact_data): the result does not depend on summation order, split-K, tiling
    or precision mode, so every output element must EQUAL the float64 reference cast to float32 (values: signed zeros
    may differ); g_c1w = float32(S) / float32(255), the one correctly rounded division of reduce_splits."""
    import torch

    for name in sorted(R.DATA_SETS):
        inp, want = exact_case(name, frames)
        got, counts = run_tap(inp, mode, lanes, min_frames)
        assert counts == expected_census(mode, frames, min_frames), (name, counts)
        for key, exp in want.items():
            g = got[key]
            if not torch.equal(g, exp):  # (== on values: -0.0 equals 0.0, NaN equals nothing)
                bad = (g != exp).nonzero()
                first = tuple(int(i) for i in bad[0])
                raise AssertionError("%s, %s, %d frames, lanes %d, data set %s: %s differs in %d of %d elements; first at %s: "
                                     "got %r, expected %r" % (mode, "forced" if min_frames else "default", frames, lanes, name,
                                                              key, bad.shape[0], g.numel(), first, float(g[first]),
                                                              float(exp[first])))


def test_reference_on_the_device_equals_the_reference_on_the_cpu():
    """the GPU cases evaluate tests/trunk_bwd_ref.py's float64 matmuls on the device; on integer data both are exact"""
    import torch

    inp = R.exact_inputs("dense", 5)
    cpu, dev = R.reference(**inp), R.reference(device="cuda", **inp)
    for key in cpu:  # (g_c1w: the device may divide by 255 as a multiplication with its reciprocal)
        if key == "g_c1w":
            assert float((cpu[key] - dev[key].cpu()).abs().max()) <= 2.0 ** -51 * float(cpu[key].abs().max())
        else:
            assert torch.equal(cpu[key], dev[key].cpu()), key
    rnd = R.random_inputs(3, 4.6)
    cpu, dev = R.reference(**rnd), R.reference(device="cuda", **rnd)
    for key in cpu:
        assert float((cpu[key] - dev[key].cpu()).abs().max()) <= 1e-12 * float(cpu[key].abs().max()), key


def test_bad_arguments_are_refused():
    from rela_amd import _capi as capi

    inp = to_device(R.exact_inputs("dense", 2))
    for mode, lanes, frames in ((3, 0, 2), (-1, 0, 2), (0, 2, 2), (0, 0, 0), (0, 0, -5)):
        args = [frames, mode, lanes, 0] + [C.c_void_p(inp["obs"].data_ptr())] * 14 + [None]
        assert capi.lib.rela_debug_trunk_backward(*args) == capi.EINVAL
    args = [2, 0, 0, 0] + [C.c_void_p(inp["obs"].data_ptr())] * 13 + [None, None]  # d_a1 is NULL
    assert capi.lib.rela_debug_trunk_backward(*args) == capi.EINVAL


# (frames, weight gain, lanes): 3 frames = fewer frames than any block count, 257 / 513 = one frame more than one / two rounds
# of 256 blocks, 2,051 = the learners' threshold region; both weight scales and both lane forms at the middle sizes
RANDOM_CASES = [(3, 1.0, 0), (3, 4.6, 1), (257, 1.0, 1), (257, 4.6, 0), (513, 1.0, 0), (513, 4.6, 1), (2051, 4.6, 1)]


@pytest.mark.parametrize("frames,gain,lanes", RANDOM_CASES)
def test_random_data_error_in_units_of_each_mode(frames, gain, lanes, record_property):
    """Inputs as in training with the masks taken from the given a1 / a2 (nothing is discontinuous).  Per output element
    |got - ref| / (u * sum|terms|), u = 2^-24 for f32 and f32x3, 2^-16 for bf16x2 (sixteen significant bits per operand,
    lo * lo dropped), against R.BOUND_UNITS (measured per output, see there); bf16x2 runs with the learners' threshold and -- below it
    -- with conv2's / conv3's weight gradients forced onto their bf16 kernels.  Whatever is measured: f32x3 is no worse
    than X3_GRAD_SLACK x f32, and bf16x2 is at least BF16X2_SEPARATION x further from float64 than f32x3 on g_c2w and
    g_c3w; both on the relative Frobenius error of the tensor, as tests/test_learner_gpu.py compares the modes (the
    largest of 10^5 element errors moves by a factor of two between seeds; a ratio of two such maxima cannot be held to 1.5)."""
    inp = to_device(R.random_inputs(frames, gain))
    ref, ab = R.reference(device="cuda", **inp), R.reference_abs(device="cuda", **inp)
    runs = [("f32", 0), ("f32x3", 0), ("bf16x2", 0)] + ([("bf16x2", 1)] if frames < FAST_WGRAD_MIN_FRAMES else [])
    units, fro = {}, {}
    for mode, min_frames in runs:
        got, counts = run_tap(inp, mode, lanes, min_frames)
        assert counts == expected_census(mode, frames, min_frames), (mode, min_frames, counts)
        tag = mode + ("_forced" if min_frames else "")
        u = R.UNIT_ROUNDOFF[mode]
        units[tag] = {k: R.err_units(got[k], ref[k], ab[k], u) for k in R.KEYS}
        fro[tag] = {k: R.rel_fro(got[k], ref[k]) for k in R.KEYS}
        for k in R.KEYS:
            record_property("err_units_%s_%s" % (tag, k), units[tag][k])
            record_property("rel_fro_%s_%s" % (tag, k), fro[tag][k])
        print("frames %d gain %.1f lanes %d %-13s units %s | rel-Frobenius %s" % (
            frames, gain, lanes, tag, " ".join("%s=%.3g" % kv for kv in units[tag].items()),
            " ".join("%s=%.3g" % kv for kv in fro[tag].items())))
    for tag in units:
        for k in R.KEYS:
            assert units[tag][k] <= R.BOUND_UNITS[tag.split("_")[0]][k], (tag, k, units[tag][k])
            record_property("bound_units_%s_%s" % (tag, k), R.BOUND_UNITS[tag.split("_")[0]][k])
    for k in R.KEYS:  # (an error below one unit roundoff of the tensor's norm is below what float32 resolves)
        assert fro["f32x3"][k] <= max(R.X3_GRAD_SLACK * fro["f32"][k], R.U_F32), (k, fro["f32x3"][k], fro["f32"][k])
    for tag in units:
        if tag.startswith("bf16x2"):
            for k in ("g_c2w", "g_c3w"):
                assert fro[tag][k] >= R.BF16X2_SEPARATION * fro["f32x3"][k], (tag, k, fro[tag][k], fro["f32x3"][k])
