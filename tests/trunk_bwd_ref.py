"""Float64 reference of ONE call of the conv trunk's backward pass (csrc/learner_common.hip: trunk_backward, reached through
rela_debug_trunk_backward), with the forward's activations as inputs, so the ReLU masks are data:

  d_a2  = [a2 > 0] * convT(d_a3, W3)            g_c3w = d_a3 (x) patches(a2)          g_c3b = sum d_a3
  d_a1  = [a1 > 0] * convT_stride2(d_a2, W2)    g_c2w = d_a2 (x) patches(a1)          g_c2b = sum d_a2
                                                g_c1w = d_a1 (x) patches(obs) / 255   g_c1b = sum d_a1

Plain torch: every contraction is a float64 matmul over unfolded patches (F.unfold / F.fold move data only), none of the
project's kernels and no convolution library.  tests/test_trunk_bwd_ref_cpu.py pins it to float64 autograd of
tests/f64_ref.py:trunk.  Inputs and outputs use the tap's layouts (include/rela_amd.h): activations and their gradients
channel-last, weights and weight gradients as in the state_dict.  `device` only says where the matmuls run.

Besides the eight outputs the reference returns "g_c1w_sum", the integer-valued sum behind g_c1w before the 1/255, and
reference_abs() returns for every output element the SUM OF ABSOLUTE VALUES OF ITS TERMS: the same function of the
absolute values of the inputs with the masks kept -- the scale against which a rounding error is measured
(err_units) and the quantity that decides whether float32 sums of integer data are exact (exact_data)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("g_c1w", "g_c1b", "g_c2w", "g_c2b", "g_c3w", "g_c3b", "d_a2", "d_a1")
U_F32, U_BF16X2 = 2.0 ** -24, 2.0 ** -16  # unit roundoff of f32 / f32x3, and of a two-part bf16 operand

# ---- bounds of the random-data test (tests/test_trunk_backward_gpu.py), in units of u * sum|terms| per output element ----
# Measured on the MI355X against this reference: the largest value over frames in {3, 257, 513, 2051}, both lane forms,
# both weight scales and (bf16x2) both thresholds (profiles/trunk_backward_error_units.md).  Over all outputs each mode's
# largest value is d_a2's: f32 4.46, f32x3 4.46, bf16x2 0.483 -- but ONE bound per mode of 4 x that (17.8 / 17.8 / 1.93)
# cannot fail where it matters: the long sums behind the weight and bias gradients sit at 1e-3 .. 1e-1 of such a unit, and
# a reference that drops a frame or the lo parts stays below it on g_c1w, g_c1b, g_c2w and g_c2b
# (test_the_random_data_bounds_can_fail).  So the bound is kept per output, 4 x the measured value of that output:
MEASURED_UNITS = {
    "f32": {"g_c1w": 0.0107, "g_c1b": 0.00392, "g_c2w": 0.266, "g_c2b": 0.067, "g_c3w": 1.74, "g_c3b": 0.385, "d_a2": 4.46,
            "d_a1": 1.10},
    "f32x3": {"g_c1w": 0.0107, "g_c1b": 0.00392, "g_c2w": 0.217, "g_c2b": 0.067, "g_c3w": 1.74, "g_c3b": 0.385, "d_a2": 4.46,
              "d_a1": 1.10},
    "bf16x2": {"g_c1w": 0.00101, "g_c1b": 0.000516, "g_c2w": 0.0369, "g_c2b": 0.00743, "g_c3w": 0.42, "g_c3b": 0.00151,
               "d_a2": 0.483, "d_a1": 0.138},
}
BOUND_UNITS = {mode: {key: 4.0 * v for key, v in per.items()} for mode, per in MEASURED_UNITS.items()}
UNIT_ROUNDOFF = {"f32": U_F32, "f32x3": U_F32, "bf16x2": U_BF16X2}
X3_GRAD_SLACK = 1.5      # f32x3 may be no worse than this x the f32 mode (tests/test_learner_gpu.py)
BF16X2_SEPARATION = 4.0  # bf16x2 must be at least this much further from float64 than f32x3 on g_c2w and g_c3w


def _nchw(x, h, w, c):
    return x.reshape(-1, h, w, c).permute(0, 3, 1, 2)


def _last(x):
    """[n, C, H, W] -> channel-last [n, H * W, C]"""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()


def _wgrad(d, x, k, stride, rnd):
    """d [n, O, oh, ow], x [n, C, H, W] -> [O, C * k * k]: sum over frames and positions of d * patch(x)"""
    p = F.unfold(rnd(x), k, stride=stride)  # [n, C k k, L]
    return rnd(d).flatten(2).permute(1, 0, 2).reshape(d.shape[1], -1) @ p.permute(0, 2, 1).reshape(-1, p.shape[1])


def _dgrad(d, w, hw, k, stride, rnd):
    """transposed convolution: d [n, O, oh, ow], w [O, C, k, k] -> [n, C, H, W]"""
    cols = rnd(w).reshape(w.shape[0], -1).t() @ rnd(d).flatten(2)  # [n, C k k, L]: one product per (tap, position)
    return F.fold(cols, hw, k, stride=stride)


def _without_tap(w, tap):
    w = w.clone()
    w[:, :, tap[0], tap[1]] = 0
    return w


def _evaluate(obs, v1, v2, m1, m2, d3, w2, w3, rnd, drop, chunk):
    """v1 / v2: the values of a1 / a2 (patch operands), m1 / m2: their masks; frames in chunks of `chunk`"""
    ident = lambda t: t
    rnd = rnd or ident
    drop = drop or {}
    n = obs.shape[0]
    dev, f64 = d3.device, torch.float64
    acc = {"g_c1w_sum": torch.zeros(32, 256, dtype=f64, device=dev), "g_c2w": torch.zeros(64, 512, dtype=f64, device=dev),
           "g_c3w": torch.zeros(64, 576, dtype=f64, device=dev), "g_c1b": torch.zeros(32, dtype=f64, device=dev),
           "g_c2b": torch.zeros(64, dtype=f64, device=dev), "g_c3b": torch.zeros(64, dtype=f64, device=dev)}
    w3d = _without_tap(w3, drop["conv3"]) if "conv3" in drop else w3
    w2d = _without_tap(w2, drop["conv2"]) if "conv2" in drop else w2
    d_a2, d_a1 = [], []
    for lo in range(0, n, chunk):
        s = slice(lo, min(n, lo + chunk))
        D3 = _nchw(d3[s], 7, 7, 64)
        A2, M2 = _nchw(v2[s], 9, 9, 64), _nchw(m2[s], 9, 9, 64)
        A1, M1 = _nchw(v1[s], 20, 20, 32), _nchw(m1[s], 20, 20, 32)
        acc["g_c3w"] += _wgrad(D3, A2, 3, 1, rnd)
        acc["g_c3b"] += D3.sum((0, 2, 3))
        D2 = M2 * _dgrad(D3, w3d, (9, 9), 3, 1, rnd)
        acc["g_c2w"] += _wgrad(D2, A1, 4, 2, rnd)
        acc["g_c2b"] += D2.sum((0, 2, 3))
        D1 = M1 * _dgrad(D2, w2d, (20, 20), 4, 2, rnd)
        acc["g_c1w_sum"] += _wgrad(D1, obs[s].to(f64), 8, 4, lambda t: t if t.shape[1] == 4 else rnd(t))
        acc["g_c1b"] += D1.sum((0, 2, 3))
        d_a2.append(_last(D2))
        d_a1.append(_last(D1))
    out = {k: v for k, v in acc.items()}
    out["g_c3w"] = acc["g_c3w"].reshape(64, 64, 3, 3).clone()
    out["g_c2w"] = acc["g_c2w"].reshape(64, 32, 4, 4).clone()
    out["g_c1w_sum"] = acc["g_c1w_sum"].reshape(32, 4, 8, 8).clone()
    for key, layer in (("g_c3w", "conv3"), ("g_c2w", "conv2"), ("g_c1w_sum", "conv1")):
        if layer in drop:
            out[key][:, :, drop[layer][0], drop[layer][1]] = 0
    out["g_c1w"] = out["g_c1w_sum"] / 255.0
    out["d_a2"], out["d_a1"] = torch.cat(d_a2), torch.cat(d_a1)
    return out


def _prep(obs, a1, a2, d_a3, w2, w3, device):
    t = lambda x: torch.as_tensor(x).detach().to(device)
    f = lambda x: t(x).to(torch.float64)
    n = t(obs).shape[0]
    return (t(obs).reshape(n, 4, 84, 84), f(a1).reshape(n, 400, 32), f(a2).reshape(n, 81, 64), f(d_a3).reshape(n, 49, 64),
            f(w2).reshape(64, 32, 4, 4), f(w3).reshape(64, 64, 3, 3))


def reference(obs, a1, a2, d_a3, w2, w3, device="cpu", rnd=None, drop=None, chunk=128):
    """-> {key: float64 tensor} for KEYS + "g_c1w_sum".  The perturbed references of the discrimination check:
    rnd: a function applied to every operand of every contraction but the u8 frames (e.g. rounding to bf16);
    drop: {"conv3" | "conv2" | "conv1": (kh, kw)} -- that kernel tap contributes to neither the layer's weight gradient
    nor its data gradient."""
    obs, a1, a2, d3, w2, w3 = _prep(obs, a1, a2, d_a3, w2, w3, device)
    with torch.no_grad():
        return _evaluate(obs, a1, a2, (a1 > 0).to(a1.dtype), (a2 > 0).to(a2.dtype), d3, w2, w3, rnd, drop, chunk)


def reference_abs(obs, a1, a2, d_a3, w2, w3, device="cpu", chunk=128):
    """-> for every output element the sum of the absolute values of its terms (masks kept)"""
    obs, a1, a2, d3, w2, w3 = _prep(obs, a1, a2, d_a3, w2, w3, device)
    with torch.no_grad():
        return _evaluate(obs, a1.abs(), a2.abs(), (a1 > 0).to(a1.dtype), (a2 > 0).to(a2.dtype), d3.abs(), w2.abs(),
                         w3.abs(), None, None, chunk)


def err_units(got, ref, ref_abs, u):
    """max over the elements of |got - ref| / (u * sum|terms|); an element without terms must be exactly zero"""
    got = torch.as_tensor(got).detach().to(ref.device, torch.float64).reshape(ref.shape)
    live = ref_abs > 0
    assert bool((got[~live] == 0).all()), "an output element without any term is not zero"
    if not bool(live.any()):
        return 0.0
    return float(((got - ref).abs()[live] / (u * ref_abs[live])).max())


def bf16_hi(t):
    """round to nearest-even bfloat16: the `hi` part of the split operands alone"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def bf16_parts(t, n=3):
    """-> the first n bf16 parts of the float32 values of t, as float64 tensors: hi = bf16(x), mid = bf16(x - hi),
    lo = bf16(x - hi - mid), every rounding to nearest-even as the kernels split their operands"""
    rest = torch.as_tensor(t).detach().to(torch.float32)
    parts = []
    for _ in range(n):
        part = rest.to(torch.bfloat16).to(torch.float32)
        parts.append(part.to(torch.float64))
        rest = rest - part
    return parts


def bf16_two(t):
    """hi + mid: an operand rounded to two bf16 parts"""
    hi, mid = bf16_parts(t, 2)
    return hi + mid


def parts_needed(t, dims=None):
    """how many bf16 parts the entries of t need (0 for zero, at most 3 for whatever float32 holds): the largest over the
    whole tensor, or with `dims` the largest over those dimensions"""
    t = torch.as_tensor(t).detach().to(torch.float64)
    hi, mid, lo = bf16_parts(t, 3)
    assert bool((hi + mid + lo == t).all()), "an entry does not fit three bf16 parts"
    need = (hi != 0).to(torch.int64) + (mid != 0).to(torch.int64) + (lo != 0).to(torch.int64)
    return int(need.max()) if dims is None else need.amax(dims)


# ---- integer data: every product and every partial sum exactly representable ------------------------------------
# d_a3 = integers * 2^-6, weights = integers * 2^-4, a1 / a2 small non-negative integers, u8 frames: every term of every
# output is an integer multiple of UNIT[key], so a float32 sum is exact -- whatever its order, split or tiling, and in
# every precision mode -- as long as the sum of the absolute values of the terms stays below 2^24 units and the
# intermediate gradients d_a2 / d_a1, which the bf16x2 mode splits into hi + lo bf16, stay below 2^16 units.
E_D3, E_W = 6, 4
UNIT = {"g_c3w": 2.0 ** -E_D3, "g_c3b": 2.0 ** -E_D3, "d_a2": 2.0 ** -(E_D3 + E_W), "g_c2w": 2.0 ** -(E_D3 + E_W),
        "g_c2b": 2.0 ** -(E_D3 + E_W), "d_a1": 2.0 ** -(E_D3 + 2 * E_W), "g_c1w": 2.0 ** -(E_D3 + 2 * E_W),
        "g_c1b": 2.0 ** -(E_D3 + 2 * E_W)}
# The bf16x2 mode multiplies hi + lo operands without the lo * lo product, so a product is exact there only if at most
# ONE of its operands needs a lo part (more than eight significant bits).
# Two data sets (densities in 1/256; `big`: the share of the non-zero entries that are 257, a value that needs a lo part).
# "dense": conv3's and conv2's kernels see well-filled operands; d_a3 carries 257s, so d_a3, d_a2 and d_a1 need their lo
# parts and everything they are multiplied with (a1, a2, the weights) has at most eight bits.  The sums over frames x 400
# positions behind g_c1w and g_c1b then exceed 2^24 units, so those two are compared in "sparse", whose d_a3 has a few
# small entries per frame, whose frames are mostly small values, and whose a2 and conv3 weights carry the 257s.
EXACT_MAX_FRAMES = 2051
DATA_SETS = {
    "dense": dict(seed=101, p_d3=6, big_d3=16, p_w3=32, big_w3=0, p_w2=64, big_w2=0, p_act=128, big_a1=0, big_a2=0, obs_small=False,
                  exact=("g_c3w", "g_c3b", "d_a2", "g_c2w", "g_c2b", "d_a1")),
    "sparse": dict(seed=202, p_d3=1, big_d3=0, p_w3=12, big_w3=4, p_w2=12, big_w2=0, p_act=128, big_a1=0, big_a2=1, obs_small=True,
                   exact=KEYS),
}


def _ints(rng, shape, p, big, signed):
    """integers: non-zero with probability p / 256, then 1..3 (or 257 with probability big / 256), random sign if signed"""
    v = rng.integers(1, 4, shape, dtype=np.int16)
    if big:
        v[rng.integers(0, 256, shape, dtype=np.uint8) < big] = 257
    if signed:
        v *= rng.integers(0, 2, shape, dtype=np.int16) * 2 - 1
    v[rng.integers(0, 256, shape, dtype=np.uint8) >= p] = 0
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact_data(name):
    """-> dict of numpy arrays for EXACT_MAX_FRAMES frames in the tap's layouts; a case of n frames uses the first n, so the
    sums of absolute values grow with n and a data set that is exact at the largest frame count is exact at every one"""
    cfg = DATA_SETS[name]
    rng = np.random.default_rng(cfg["seed"])
    n = EXACT_MAX_FRAMES
    if cfg["obs_small"]:  # mostly 0..3, one byte in 128 anywhere in 0..255
        obs = rng.integers(0, 4, (n, 4, 84, 84), dtype=np.uint8) * (rng.integers(0, 2, (n, 4, 84, 84), dtype=np.uint8))
        wide = rng.integers(0, 128, obs.shape, dtype=np.uint8) == 0
        obs[wide] = rng.integers(0, 256, int(wide.sum()), dtype=np.uint8)
    else:
        obs = rng.integers(0, 256, (n, 4, 84, 84), dtype=np.uint8)
    return {"obs": obs,
            "a1": _ints(rng, (n, 400, 32), cfg["p_act"], cfg["big_a1"], False),
            "a2": _ints(rng, (n, 81, 64), cfg["p_act"], cfg["big_a2"], False),
            "d_a3": _ints(rng, (n, 49, 64), cfg["p_d3"], cfg["big_d3"], True) * np.float32(2.0 ** -E_D3),
            "w2": _ints(rng, (64, 32, 4, 4), cfg["p_w2"], cfg["big_w2"], True) * np.float32(2.0 ** -E_W),
            "w3": _ints(rng, (64, 64, 3, 3), cfg["p_w3"], cfg["big_w3"], True) * np.float32(2.0 ** -E_W)}


def exact_inputs(name, frames):
    d = exact_data(name)
    return {k: (v if k in ("w2", "w3") else v[:frames]) for k, v in d.items()}


def needs_lo(t):
    """does any entry have more than the eight significant bits of one bf16?"""
    t = torch.as_tensor(t).detach().to(torch.float64)
    return bool((bf16_hi(t) != t).any())


def exact_operand_preconditions(name, inp, ref):
    """Per frame: d_a2 and d_a1 (which the bf16x2 mode splits into hi + lo bf16) stay below 2^16 units, and no contraction
    has operands that BOTH need a lo part.  Asserted on the inputs and the REFERENCE of a case, never on a kernel's output."""
    for key in ("d_a2", "d_a1"):
        big = float(ref[key].abs().max()) / UNIT[key]
        assert big < 2 ** 16, "%s: |%s| reaches %.0f units (>= 2^16)" % (name, key, big)
    lo = {k: needs_lo(v) for k, v in list(inp.items()) + [("d_a2", ref["d_a2"]), ("d_a1", ref["d_a1"])]}
    assert not lo["obs"]
    for a, b in (("d_a3", "a2"), ("d_a3", "w3"), ("d_a2", "a1"), ("d_a2", "w2")):
        assert not (lo[a] and lo[b]), "%s: %s and %s both need a lo part: their products lose lo * lo in bf16x2" % (name, a, b)
    return lo


def exact_preconditions(name, ref, ref_abs):
    """For every output the data set claims: sum|terms| below 2^24 units and the value a whole number of units"""
    for key in DATA_SETS[name]["exact"]:
        total = float(ref_abs[key].max()) / UNIT[key] * (255.0 if key == "g_c1w" else 1.0)
        assert total < 2 ** 24, "%s: sum|terms| of %s reaches %.0f units (>= 2^24)" % (name, key, total)
        val = ref["g_c1w_sum" if key == "g_c1w" else key] / UNIT[key]
        assert bool((val == val.round()).all()), "%s: %s is not a whole number of units" % (name, key)


def exact_expected(ref, key):
    """the float32 value every mode must produce: the reference itself; for g_c1w float32(S) / float32(255), the one
    correctly rounded division reduce_splits performs"""
    if key == "g_c1w":
        s = ref["g_c1w_sum"].cpu().numpy().astype(np.float32)
        return s / np.float32(255.0)
    return ref[key].cpu().numpy().astype(np.float32)


# ---- the cases of tests/test_trunk_backward_gpu.py (the CPU test proves the preconditions for every frame count here) ----
# (mode, lanes, frames, fast_wgrad_min_frames); 0 = the learners' threshold.  All five bf16 kernels stride frames over
# min(frames, 256) persistent blocks, conv1's weight gradient over 128 in the two-lane form: 1 frame, blocks, blocks + 1,
# 2 blocks + 1 for both block counts.  The split-K GEMMs triple their split count up to 1,024 frames.
EXACT_CASES = ([("bf16x2", lanes, n, 1) for lanes in (0, 1) for n in (1, 2, 128, 129, 255, 256, 257, 513)] +
               [(mode, lanes, n, 0) for mode in ("f32", "f32x3") for lanes in (0, 1) for n in (1, 2, 45, 257)] +
               [("f32", 0, 1024, 0), ("f32", 1, 1025, 0), ("f32x3", 1, 1024, 0), ("f32x3", 0, 1025, 0)] +
               [("bf16x2", 1, 2048, 0), ("bf16x2", 0, 2051, 0), ("bf16x2", 0, 2047, 0)])
EXACT_CASES.sort(key=lambda c: c[2])  # (cases of one frame count share their inputs and reference)
EXACT_FRAMES = sorted({c[2] for c in EXACT_CASES})
assert EXACT_FRAMES[-1] == EXACT_MAX_FRAMES


@functools.lru_cache(maxsize=2)
def random_inputs(frames, gain, seed=7):
    """Inputs as in training: u8 frames, a1 / a2 = relu(normal), d_a3 = normal * [random mask], conv2 / conv3 weights of
    synth_params at `gain` (1: the default initialisation; 4.6: the scale of a trained agent)"""
    from synth import synth_params

    rng = np.random.default_rng(seed + 1000 * frames)
    p = synth_params(18, seed, gain)
    relu_normal = lambda shape: np.maximum(rng.standard_normal(shape, dtype=np.float32), np.float32(0))
    d3 = rng.standard_normal((frames, 49, 64), dtype=np.float32) * (rng.integers(0, 2, (frames, 49, 64)) > 0)
    return {"obs": rng.integers(0, 256, (frames, 4, 84, 84), dtype=np.uint8), "a1": relu_normal((frames, 400, 32)),
            "a2": relu_normal((frames, 81, 64)), "d_a3": d3.astype(np.float32), "w2": p["net.2.weight"],
            "w3": p["net.4.weight"]}


def rel_fro(got, ref):
    got = torch.as_tensor(got).detach().to(ref.device, torch.float64).reshape(ref.shape)
    return float((got - ref).norm()) / (float(ref.norm()) + 1e-300)
