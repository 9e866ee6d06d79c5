"""tests/head_fc_bwd_ref.py on the CPU (no GPU, none of the project's kernels):
  1. reference and loss_reference equal float64 autograd of the upper half of tests/f64_ref.py:ffnet_forward (a3 as the
     leaf) through the loss of tests/f64_ref.py:apex_loss;
  2. the integer data sets and the loss tables of the GPU test fulfil their preconditions at every case it runs;
  3. every bound of the GPU test can fail: each defect below, restated in float64, breaks exact equality at every exact
     shape and exceeds the bound of EVERY mode at every random case (resp. the derived bounds at every loss case).
Where a defect cannot show, the case is named in DEFECTS / LOSS_DEFECTS with the reason -- it is not skipped silently."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_fc_bwd_ref as R
from f64_ref import dueling, ffnet_forward, params_as
from synth import synth_obs, synth_params

f64 = torch.float64


def _last(a3_sd):
    """[B, 3136] in state_dict column order c * 49 + pos -> the tap's channel-last [B, 49, 64]"""
    return a3_sd.reshape(-1, 64, 49).permute(0, 2, 1).contiguous()


def _upper(p, a3, legal):
    """ffnet_forward from relu(conv3) on: its two lines after trunk(), with the intermediate tensors returned"""
    pre = F.linear(a3, p["linear.0.weight"], p["linear.0.bias"])
    hid = F.relu(pre)
    v, a = F.linear(hid, p["fc_v.weight"], p["fc_v.bias"]), F.linear(hid, p["fc_a.weight"], p["fc_a.bias"])
    return dueling(v, a, legal, 1), pre, hid, v, a


def test_upper_half_is_ffnet_forwards():
    p = params_as(synth_params(6, 5, 4.6), f64)
    obs = torch.from_numpy(synth_obs(2, 6))
    legal = torch.tensor([[1, 0, 1, 1, 0, 1], [1, 1, 1, 0, 1, 1]], dtype=f64)
    from f64_ref import trunk

    assert torch.equal(_upper(p, trunk(p, obs, f64), legal)[0], ffnet_forward(p, obs, legal, f64))


@pytest.mark.parametrize("A", [6, 31])
def test_references_match_f64_autograd(A):
    B = 5
    rng = np.random.default_rng(40 + A)
    p = params_as(synth_params(A, 5, 4.6), f64, True)
    z3 = torch.from_numpy(rng.standard_normal((B, 3136))).requires_grad_(True)
    a3 = F.relu(z3)
    legal = torch.from_numpy((rng.uniform(size=(B, A)) < 0.7).astype(np.float64))
    nlegal = torch.from_numpy((rng.uniform(size=(B, A)) < 0.7).astype(np.float64))
    act = torch.from_numpy(rng.integers(0, A, B))
    legal[torch.arange(B), act] = 1
    nlegal[:, 0] = 1
    q, pre, hid, v, a = _upper(p, a3, legal)
    for t in (pre, v, a):
        t.retain_grad()
    qno, qnt = torch.from_numpy(rng.standard_normal((B, A))), torch.from_numpy(rng.standard_normal((B, A)))
    boot = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0], dtype=f64)
    weight = torch.from_numpy(rng.uniform(0.2, 1.0, B))
    with torch.no_grad():  # apex_loss's lines, on the given tables
        next_a = ((1 + qno - qno.min()) * nlegal).argmax(1)
        boot_q = boot * R.GAMMA_N * qnt.gather(1, next_a.unsqueeze(1)).squeeze(1)
        # rewards that put the errors on both sides of the Huber kink
        reward = torch.tensor([0.3, -2.0, 1.7, -0.6, 0.05], dtype=f64) + q.gather(1, act.unsqueeze(1)).squeeze(1) - boot_q
        target = reward + boot_q
    err = target - q.gather(1, act.unsqueeze(1)).squeeze(1)
    per_sample = F.smooth_l1_loss(err, torch.zeros_like(err), reduction="none")
    loss = (per_sample * weight).mean()
    loss.backward()
    assert float(err.detach().abs().max()) > 1 > float(err.detach().abs().min())

    lref = R.loss_reference(A, q.detach(), qno, qnt, nlegal, act, reward, boot, weight, legal)
    close = lambda x, y: float((x - y).abs().max()) <= 1e-12 * max(float(y.abs().max()), 1e-300)
    assert torch.equal(lref["next_a"], next_a) and close(lref["e"], err.detach()) and close(lref["loss"], loss.detach())
    assert close(lref["d_ha"][:, :A], a.grad) and close(lref["d_ha"][:, 31:32], v.grad)
    assert bool((lref["d_ha"][:, A:31] == 0).all())

    inp = dict(A=A, d_ha=lref["d_ha"], h=hid.detach(), a3=_last(a3.detach()), fc_a_w=p["fc_a.weight"].detach(),
               fc_v_w=p["fc_v.weight"].detach(), fc_w=p["linear.0.weight"].detach())
    ref = R.reference(**inp)
    want = {"g_fc_a_w": p["fc_a.weight"].grad, "g_fc_a_b": p["fc_a.bias"].grad, "g_fc_v_w": p["fc_v.weight"].grad,
            "g_fc_v_b": p["fc_v.bias"].grad, "g_fc_w": p["linear.0.weight"].grad, "g_fc_b": p["linear.0.bias"].grad,
            "d_h": pre.grad, "d_a3": _last(z3.grad)}
    for key in R.KEYS:
        assert ref[key].shape == want[key].shape, key
        assert float(want[key].abs().max()) > 0 and close(ref[key], want[key]), key
    # columns A..30 take no part
    junk = lref["d_ha"].clone()
    junk[:, A:31] = 7.0
    for key, t in R.reference(**dict(inp, d_ha=junk)).items():
        assert torch.equal(t, ref[key]), key
    # the sum of the absolute values of the terms bounds every value, and equals it where nothing has a sign
    ab = R.reference_abs(**inp)
    for key in R.KEYS:
        assert bool((ab[key] >= ref[key].abs() * (1 - 1e-12)).all()), key
    pos = R.reference(**dict(inp, d_ha=inp["d_ha"].abs(), fc_a_w=inp["fc_a_w"].abs(), fc_v_w=inp["fc_v_w"].abs(),
                             fc_w=inp["fc_w"].abs()))
    for key in R.KEYS:
        assert float((pos[key] - ab[key]).abs().max()) <= 1e-12 * float(ab[key].abs().max()), key


# ---- 2. preconditions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,A", R.EXACT_SHAPES)
def test_integer_data_is_exact_at_every_shape_of_the_gpu_cases(batch, A):
    for name in R.DATA_SETS:
        inp = R.exact_inputs(name, batch, A)
        ref, ab = R.reference(**inp), R.reference_abs(**inp)
        lo = R.exact_preconditions(name, inp, ref, ab)
        assert lo["d_ha"] == (name != "masked")  # the 257s: d_ha needs its lo part
        for key in R.KEYS:  # not trivial: every output has entries
            assert float((ref[key] != 0).double().mean()) > (0.02 if name != "last_row" else 0.0), (name, key)
            assert bool((ref[key] != 0).any()), (name, key)
        if name == "dense":
            assert bool((inp["d_ha"] != 0).all()) and bool((inp["h"] > 0).all()) and bool((inp["a3"] > 0).all())
        if name == "masked":
            assert 0.4 < float((inp["h"] <= 0).mean()) < 0.6 and bool((inp["h"] == 0).any()) and bool((inp["h"] < 0).any())
            assert 0.4 < float((inp["a3"] <= 0).mean()) < 0.6
            assert batch < 10 or bool((inp["d_ha"] == 0).all(1).any())
        if name == "last_row":
            assert bool((inp["d_ha"][:-1] == 0).all()) and bool((inp["d_ha"][-1] != 0).all())


@pytest.mark.parametrize("batch", R.LOSS_BATCHES)
def test_loss_tables_have_the_properties_the_gpu_test_relies_on(batch):
    for A in R.A_LIST:
        inp = R.loss_inputs(batch, A)
        R.check_loss_inputs(inp)
        roles = R.loss_roles(batch)
        assert roles[0] == "small_only_legal_act" and (batch < 8 or set(roles) == set(R.ROLES))
    assert R.loss_bound_units(512) == 17 and R.loss_bound_units(2051) == 21


def test_no_bound_exceeds_the_a_priori_one():
    for batch, A, _, _ in R.RANDOM_CASES:
        for mode in R.MEASURED_UNITS:
            for key in R.KEYS:
                assert R.MEASURED_UNITS[mode][batch][key] <= R.n_terms(key, batch, A), (mode, batch, key)
                assert R.bound_units(mode, key, batch, A) <= R.n_terms(key, batch, A)


# ---- 3. the bounds can fail ----------------------------------------------------------------------------------------------
GRADS = ("g_fc_a_w", "g_fc_a_b", "g_fc_v_w", "g_fc_v_b", "g_fc_w", "g_fc_b")
# defect -> (the exact data set that shows it, the outputs it must break on random data)
DEFECTS = {
    "last batch row dropped": ("last_row", GRADS + ("d_h", "d_a3")),
    "last partial K chunk dropped": ("last_row", ("g_fc_a_w", "g_fc_v_w", "g_fc_w")),  # (every batch here has one: none is a multiple of 32)
    "first row counted twice": ("dense", GRADS),
    "row b reads h of row b + 1": ("masked", ("g_fc_a_w", "g_fc_v_w", "d_h")),
    "h > 0 mask replaced by >= 0": ("masked", ("d_h", "g_fc_b", "g_fc_w", "d_a3")),
    # at A = 31 column A IS the value column: there the neighbour, column 30, stands in
    "value column taken from column A": ("dense", ("g_fc_v_w", "g_fc_v_b", "d_h")),
    # needs columns A..30 (none at A = 31) with non-zero entries (the loss kernel writes zeros: exact dense data only)
    "columns A..30 leak into d_h": ("dense", ()),
}


def defective(inp, what):
    """the outputs of a tap with the defect, float64; None where the defect does not exist at this shape"""
    A = inp["A"]
    d, h, a3, aw, vw, fw = R._prep(A, inp["d_ha"], inp["h"], inp["a3"], inp["fc_a_w"], inp["fc_v_w"], inp["fc_w"], "cpu")
    n = d.shape[0]
    hm, a3m = (h > 0).to(f64), (a3 > 0).to(f64)
    ok = R._evaluate(A, d, h, hm, a3, a3m, aw, vw, fw)
    if what == "last batch row dropped":
        d2 = d.clone()
        d2[-1] = 0
        return R._evaluate(A, d2, h, hm, a3, a3m, aw, vw, fw)
    if what == "last partial K chunk dropped":
        d2 = d.clone()
        d2[(n - 1) // 32 * 32:] = 0
        bad = R._evaluate(A, d2, h, hm, a3, a3m, aw, vw, fw)
        return dict(ok, g_fc_a_w=bad["g_fc_a_w"], g_fc_v_w=bad["g_fc_v_w"], g_fc_w=bad["g_fc_w"])
    if what == "first row counted twice":
        one = R._evaluate(A, d[:1], h[:1], hm[:1], a3[:1], a3m[:1], aw, vw, fw)
        return dict(ok, **{k: ok[k] + one[k] for k in GRADS})
    if what == "row b reads h of row b + 1":
        h2 = torch.cat([h[1:], torch.zeros(1, 512, dtype=f64)])
        return R._evaluate(A, d, h2, (h2 > 0).to(f64), a3, a3m, aw, vw, fw)
    if what == "h > 0 mask replaced by >= 0":
        return R._evaluate(A, d, h, (h >= 0).to(f64), a3, a3m, aw, vw, fw)
    if what == "value column taken from column A":
        d2 = d.clone()
        d2[:, 31] = d[:, A if A < 31 else 30]
        return R._evaluate(A, d2, h, hm, a3, a3m, aw, vw, fw)
    if what == "columns A..30 leak into d_h":
        if A == 31 or not bool((d[:, A:31] != 0).any()):
            return None
        rows = aw[torch.arange(A, 31) % A]  # (whatever lies behind fc_a.weight: here its own rows again)
        return R._evaluate(A, d, h, hm, a3, a3m, aw, vw, fw, d_h_of=lambda dh: dh + hm * (d[:, A:31] @ rows))
    raise KeyError(what)


@pytest.mark.parametrize("batch,A", R.EXACT_SHAPES)
def test_every_defect_breaks_exact_equality(batch, A):
    """on the data set named in DEFECTS, after the cast to float32 the GPU test compares"""
    for what, (name, _) in DEFECTS.items():
        inp = R.exact_inputs(name, batch, A)
        bad = defective(inp, what)
        if bad is None:
            assert what == "columns A..30 leak into d_h" and A == 31
            continue
        ref = R.reference(**inp)
        assert any(not torch.equal(bad[k].float(), ref[k].float()) for k in R.KEYS), (what, name, batch, A)


def _f32_autograd_units(inp, ref, ab):
    """the error of pyrela's layers (F.linear, as nn.Linear calls it) under float32 autograd on the same inputs, in units
    of 2^-24 * sum|terms|: the scale a bound must sit above and a defect must clear"""
    A = inp["A"]
    t = lambda x: torch.as_tensor(x).float()
    d, a3 = t(inp["d_ha"]), t(inp["a3"]).reshape(-1, 49, 64).permute(0, 2, 1).reshape(-1, 3136)
    H = t(inp["h"]).clone().requires_grad_(True)
    aw, vw, fw = (t(inp[k]).clone().requires_grad_(True) for k in ("fc_a_w", "fc_v_w", "fc_w"))
    ab_, vb, fb = torch.zeros(A, requires_grad=True), torch.zeros(1, requires_grad=True), torch.zeros(512, requires_grad=True)
    ((F.linear(H, aw, ab_) * d[:, :A]).sum() + (F.linear(H, vw.reshape(1, 512), vb) * d[:, 31:32]).sum()).backward()
    d_h = (H.grad * (H > 0)).detach()
    A3 = a3.clone().requires_grad_(True)
    (F.linear(A3, fw, fb) * d_h).sum().backward()
    got = {"g_fc_a_w": aw.grad, "g_fc_a_b": ab_.grad, "g_fc_v_w": vw.grad.reshape(1, 512), "g_fc_v_b": vb.grad, "g_fc_w": fw.grad,
           "g_fc_b": fb.grad, "d_h": d_h, "d_a3": (A3.grad * (A3 > 0)).reshape(-1, 64, 49).permute(0, 2, 1)}
    return {k: R.err_units(got[k], ref[k], ab[k], R.U_F32) for k in R.KEYS}


def _worst(bad, ref, ab):
    """err_units with u = 1; an element without terms that is not zero fails R.err_units' own assertion: infinitely bad"""
    if bool((bad[ab <= 0] != 0).any()):
        return float("inf")
    return R.err_units(bad, ref, ab, 1.0)


CLEAR_AUTOGRAD_BY = 4.0  # a defect exceeds 4 x pyrela's float32 error by at least this factor


@pytest.mark.parametrize("batch,A", sorted({(b, A) for b, A, _, _ in R.RANDOM_CASES}))
def test_every_defect_exceeds_the_random_data_bounds(batch, A):
    """In the units of the GPU test: the defect's error on each output DEFECTS names exceeds the measured bound of every
    mode (R.bound_units) and, by CLEAR_AUTOGRAD_BY, 4 x the error of pyrela's float32 autograd on the same inputs."""
    inp = R.random_inputs(batch, A, 1.0)
    ref, ab = R.reference(**inp), R.reference_abs(**inp)
    auto = _f32_autograd_units(inp, ref, ab)
    for key in R.KEYS:  # float32 autograd itself passes the bound of the float32 modes' scale: n_terms
        assert auto[key] <= R.n_terms(key, batch, A), (key, auto[key])
    for what, (_, keys) in DEFECTS.items():
        if not keys:
            assert defective(inp, what) is None  # (d_ha of the loss kernel's structure has zeros in columns A..30)
            continue
        bad = defective(inp, what)
        for key in keys:
            worst = _worst(bad[key], ref[key], ab[key])
            loosest = max(R.bound_units(m, key, batch, A) * R.UNIT_ROUNDOFF[m] for m in R.MEASURED_UNITS)
            assert worst > loosest, "%s on %s: %.3g of sum|terms|, the bound allows %.3g" % (what, key, worst, loosest)
            assert worst > CLEAR_AUTOGRAD_BY * 4 * auto[key] * R.U_F32, (what, key, worst, auto[key])
    # ... and operands rounded to one bf16 part exceed them on every output a GEMM writes
    bad = R.reference(rnd=R.bf16_hi, **inp)
    for key in ("g_fc_a_w", "g_fc_v_w", "g_fc_w", "g_fc_b", "d_h", "d_a3"):
        worst = _worst(bad[key], ref[key], ab[key])
        assert worst > max(R.bound_units(m, key, batch, A) * R.UNIT_ROUNDOFF[m] for m in R.MEASURED_UNITS), (key, worst)


# defect of loss_reference -> where it cannot show
LOSS_DEFECTS = {
    "mean_over_legal": lambda batch, A: A == 1,   # one action: it is legal, both divisors are 1
    "next_legal_mask": lambda batch, A: A == 1,   # one action: legal in obs and next_obs
    "no_clamp": lambda batch, A: batch == 1,      # the one row has |e| <= 0.9
    "no_inv_b": lambda batch, A: batch == 1,      # 1 / B = 1
    "tie_high": lambda batch, A: A == 1 or batch < 6,  # the first tie row is row 5
}


@pytest.mark.parametrize("batch", R.LOSS_BATCHES)
def test_every_loss_defect_exceeds_the_derived_bounds(batch):
    for A in R.A_LIST:
        inp = R.loss_inputs(batch, A)
        ref = R.loss_reference(A, **R.loss_args(inp))
        g = ref["g"].abs()[:, None]
        for what, absent in LOSS_DEFECTS.items():
            bad = R.loss_reference(A, defect=what, **R.loss_args(inp))
            if what == "tie_high":
                shows = bool(((bad["e"] - ref["e"]).abs() > 2 * R.td_bound(inp, ref)).any())
            else:  # (twice the bound: a kernel may sit a bound away from the reference on the other side)
                shows = bool(((bad["d_ha"][:, :A] - ref["d_ha"][:, :A]).abs() > 2 * R.D_HA_UNITS * R.U_F32 * g).any()) or \
                    bool(((bad["d_ha"][:, 31] - ref["d_ha"][:, 31]).abs() > 2 * R.D_V_UNITS * R.U_F32 * g[:, 0]).any())
            assert shows == (not absent(batch, A)), (what, batch, A)
