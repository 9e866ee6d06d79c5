"""tests/trunk_bwd_ref.py on the CPU (no GPU, none of the project's kernels):
  1. the reference equals float64 autograd of tests/f64_ref.py:trunk with the ReLUs replaced by the given masks;
  2. the integer data sets of the GPU test fulfil their exactness preconditions at every frame count it uses;
  3. the bounds the GPU test asserts on random data can fail: a reference that drops the last frame, one kernel tap, or
     the lo parts of the operands exceeds them on the outputs it touches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trunk_bwd_ref as R
from f64_ref import params_as, trunk
from synth import synth_obs, synth_params


@pytest.mark.parametrize("frames", [2, 3])
def test_reference_matches_f64_autograd_with_the_given_masks(frames):
    f64 = torch.float64
    p = params_as({k: v for k, v in synth_params(18, 5, 4.6).items() if k.startswith("net.")}, f64, True)
    obs = torch.from_numpy(synth_obs(frames, 6))
    x = obs.to(f64) / 255.0
    with torch.no_grad():  # the forward's own activations: their > 0 patterns are the masks
        a1 = F.relu(F.conv2d(x, p["net.0.weight"], p["net.0.bias"], stride=4))
        a2 = F.relu(F.conv2d(a1, p["net.2.weight"], p["net.2.bias"], stride=2))
        a3 = F.relu(F.conv2d(a2, p["net.4.weight"], p["net.4.bias"], stride=1))
        m1, m2, m3 = (a1 > 0).to(f64), (a2 > 0).to(f64), (a3 > 0).to(f64)
        assert 0.2 < float(m1.mean()) < 0.8 and 0.2 < float(m2.mean()) < 0.8
    z1 = F.conv2d(x, p["net.0.weight"], p["net.0.bias"], stride=4)
    z2 = F.conv2d(z1 * m1, p["net.2.weight"], p["net.2.bias"], stride=2)
    z3 = F.conv2d(z2 * m2, p["net.4.weight"], p["net.4.bias"], stride=1)
    out = (z3 * m3).flatten(1)
    assert torch.equal(out.detach(), trunk({k: v.detach() for k, v in p.items()}, obs, f64))  # the same network
    z1.retain_grad(), z2.retain_grad()
    seed = torch.from_numpy(np.random.default_rng(8).standard_normal((frames, 64, 7, 7)))
    (z3 * m3 * seed).sum().backward()
    last = lambda t: t.detach().permute(0, 2, 3, 1).reshape(frames, -1, t.shape[1])
    d_a3 = last(seed * m3)  # already masked, as the tap expects it
    ref = R.reference(obs, last(a1), last(a2), d_a3, p["net.2.weight"].detach(), p["net.4.weight"].detach(), chunk=2)
    want = {"g_c1w": p["net.0.weight"].grad, "g_c1b": p["net.0.bias"].grad, "g_c2w": p["net.2.weight"].grad,
            "g_c2b": p["net.2.bias"].grad, "g_c3w": p["net.4.weight"].grad, "g_c3b": p["net.4.bias"].grad,
            "d_a2": last(z2.grad * m2), "d_a1": last(z1.grad * m1)}
    for key in R.KEYS:
        assert ref[key].shape == want[key].shape, key
        scale = float(want[key].abs().max())
        assert scale > 0 and float((ref[key] - want[key]).abs().max()) <= 1e-12 * scale, key
    assert torch.equal(ref["g_c1w"], ref["g_c1w_sum"] / 255.0)
    # the sum of the absolute values of the terms bounds every value, and equals it where nothing has a sign
    ab = R.reference_abs(obs, last(a1), last(a2), d_a3, p["net.2.weight"].detach(), p["net.4.weight"].detach())
    for key in R.KEYS:
        assert bool((ab[key] >= ref[key].abs() * (1 - 1e-12)).all()), key
    pos = R.reference(obs, last(a1), last(a2), d_a3.abs(), p["net.2.weight"].detach().abs(), p["net.4.weight"].detach().abs())
    for key in R.KEYS:
        assert torch.equal(pos[key], ab[key]), key


@pytest.mark.parametrize("name", sorted(R.DATA_SETS))
def test_integer_data_is_exact_at_every_frame_count_of_the_gpu_cases(name):
    """A case of n frames uses the first n frames of the data set, so the reference of n frames is the reference of the
    previous frame count plus that of the frames in between: one pass over the largest case checks the preconditions of
    every frame count of R.EXACT_CASES."""
    ref, ab, done, lo = None, None, 0, {}
    for n in R.EXACT_FRAMES:
        inp = {k: (v if k in ("w2", "w3") else v[done:n]) for k, v in R.exact_data(name).items()}
        part, part_abs = R.reference(**inp), R.reference_abs(**inp)
        if ref is None:
            ref, ab = part, part_abs
        else:
            for tot, new in ((ref, part), (ab, part_abs)):
                for key in tot:
                    tot[key] = torch.cat([tot[key], new[key]]) if key in ("d_a2", "d_a1") else tot[key] + new[key]
        done = n
        assert ref["d_a1"].shape[0] == n
        for k, v in R.exact_operand_preconditions(name, inp, part).items():
            lo[k] = lo.get(k, False) or v
        R.exact_preconditions(name, ref, ab)
    # the data is not trivial: every output the set claims has entries, and some operand needs the lo part of a split
    for key in R.DATA_SETS[name]["exact"]:
        assert float((ref[key] != 0).double().mean()) > 0.02, key
    # ... and the lo parts are exercised: d_a3 (dense) resp. a2 and conv3's weights (sparse), and d_a2 / d_a1 in both
    assert lo["d_a2"] and lo["d_a1"] and not lo["a1"] and not lo["w2"]
    assert (lo["d_a3"], lo["a2"], lo["w3"]) == ((True, False, False) if name == "dense" else (False, True, True))


def test_exact_cases_cover_every_output_in_some_data_set():
    covered = set()
    for cfg in R.DATA_SETS.values():
        covered |= set(cfg["exact"])
    assert covered == set(R.KEYS)


@pytest.mark.parametrize("frames", [257, 513])
def test_the_random_data_bounds_can_fail(frames):
    """Perturbed references against the exact one, in the units and against the bounds of the GPU test: each must exceed
    the bound of EVERY mode on the outputs it touches (so a kernel with that defect cannot pass in any mode)."""
    inp = R.random_inputs(frames, 1.0)
    ref, ab = R.reference(**inp), R.reference_abs(**inp)

    def exceeds(bad, keys, what):
        for key in keys:
            loosest = max(R.BOUND_UNITS[m][key] * R.UNIT_ROUNDOFF[m] for m in R.BOUND_UNITS)
            worst = R.err_units(bad[key], ref[key], ab[key], 1.0)
            assert worst > loosest, "%s on %s: %.3g of sum|terms|, the bound allows %.3g" % (what, key, worst, loosest)

    grads = ("g_c1w", "g_c1b", "g_c2w", "g_c2b", "g_c3w", "g_c3b")
    exceeds(R.reference(**{k: (v if k in ("w2", "w3") else v[:-1]) for k, v in inp.items()}), grads, "last frame dropped")
    exceeds(R.reference(drop={"conv3": (1, 2), "conv2": (3, 0), "conv1": (5, 6)}, **inp),
            ("g_c3w", "d_a2", "g_c2w", "d_a1", "g_c1w"), "one kernel tap dropped")
    exceeds(R.reference(rnd=R.bf16_hi, **inp), [k for k in R.KEYS if k != "g_c3b"], "operands rounded to their bf16 hi part")
