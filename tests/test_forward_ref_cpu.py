"""tests/forward_ref.py on the CPU: the float64 layers against torch, the decoders, the conditions on the bounds, and
the restated defects the per-layer check of tests/test_forward_layers_gpu.py must reject.

A restated defect is applied to the float64 reference of ONE layer; its effect is the largest |y_defect - y| / (u S) over
the layer's elements at the test's own inputs, the figure the GPU test compares with the bound b.  The check rejects the
defect with room to spare when b is below a quarter of that effect (section "the conditions").  Each defect also reports
the change of Q (AtariFFNet) or of h, c (AtariLSTMNet) it causes through the rest of the float64 network -- what the
Q-level comparisons at rtol = atol = 1e-4 (tests/test_ffnet_gpu.py, tests/test_lstmnet_gpu.py) see of it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f64_ref
import forward_ref as fr

F64 = torch.float64
N_CPU = 5  # frames of the test's own inputs; the last one is "the last frame of a ragged tile"
Q_TOL = 1e-4  # the Q-level tolerance of the existing suites (atol = rtol, |Q| <= 0.5 at scale 1)


def tparams(p):
    return {k: torch.from_numpy(v) for k, v in p.items()}


# ---- (b) the float64 layers are torch's -------------------------------------------------------------------------------------
def _nchw(x_last, hw):
    return x_last.reshape(x_last.shape[0], hw, hw, -1).permute(0, 3, 1, 2)


def _last(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])


@pytest.mark.parametrize("scale", fr.SCALES)
def test_layers_equal_torch_in_float64(scale):
    p = f64_ref.params_as(fr.ffnet_params(18, scale), F64)
    obs, legal = fr.all_obs()[:3], fr.all_legal(18)[:3]
    x = torch.from_numpy(obs).to(F64)
    w1 = fr.conv1_weight(p["net.0.weight"])
    a1, S1 = fr.conv1_layer(obs, p["net.0.weight"], p["net.0.bias"])
    want = F.relu(F.conv2d(x, w1, p["net.0.bias"], stride=4))
    torch.testing.assert_close(a1, _last(want), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(S1, _last(F.conv2d(x, w1.abs(), p["net.0.bias"].abs(), stride=4)), rtol=1e-13, atol=1e-13)
    a2, _ = fr.conv2_layer(a1, p["net.2.weight"], p["net.2.bias"])
    want = F.relu(F.conv2d(_nchw(a1, 20), p["net.2.weight"], p["net.2.bias"], stride=2))
    torch.testing.assert_close(a2, _last(want), rtol=1e-13, atol=1e-13)
    a3, S3 = fr.conv3_layer(a2, p["net.4.weight"], p["net.4.bias"])
    want = F.relu(F.conv2d(_nchw(a2, 9), p["net.4.weight"], p["net.4.bias"]))
    torch.testing.assert_close(a3, _last(want), rtol=1e-13, atol=1e-13)
    assert bool((S3 >= a3).all()) and bool((S3 > 0).all())
    h, _ = fr.fc_layer(a3, p["linear.0.weight"], p["linear.0.bias"])
    torch.testing.assert_close(h, F.relu(F.linear(want.flatten(1), p["linear.0.weight"], p["linear.0.bias"])), rtol=1e-13, atol=1e-13)
    ha, _ = fr.heads_layer(h, p["fc_a.weight"], p["fc_a.bias"], p["fc_v.weight"], p["fc_v.bias"])
    q, Sq = fr.duel_layer(ha[:, :18], ha[:, 18:], legal)
    want = f64_ref.dueling(F.linear(h, p["fc_v.weight"], p["fc_v.bias"]), F.linear(h, p["fc_a.weight"], p["fc_a.bias"]),
                           torch.from_numpy(legal).to(F64), 1)
    torch.testing.assert_close(q, want, rtol=1e-13, atol=1e-13)
    assert bool((Sq >= q.abs() - 1e-15).all())
    # the whole chain is the network of pyrela/net.py (f64_ref.ffnet_forward divides the frames by 255 in float64, the
    # kernels' operand is float32(w) / 255.0f: 6e-8 relative per conv1 weight)
    torch.testing.assert_close(q, f64_ref.ffnet_forward(p, obs, legal, F64), rtol=0, atol=1e-6 * scale ** 4)


def test_lstm_layers_equal_torch_nn_lstm_in_float64():
    p = f64_ref.params_as(fr.lstm_params(6, 1.0), F64)
    n = 4
    rng = np.random.default_rng(2)
    a3 = torch.from_numpy(np.maximum(rng.normal(0, 0.5, (n, 49, 64)), 0))
    h0, c0 = (torch.from_numpy(v[:n]).to(F64) for v in fr.all_state())
    lstm = torch.nn.LSTM(3136, 512).double()
    lstm.load_state_dict({k[5:]: v for k, v in p.items() if k.startswith("lstm.")})
    x = a3.permute(0, 2, 1).reshape(n, 3136)  # torch's flatten order c * 49 + pos
    with torch.no_grad():
        _, (h1, c1) = lstm(x.unsqueeze(0), (h0.unsqueeze(0), c0.unsqueeze(0)))
    z, Sz = fr.gates_layer(None, a3, h0, p)
    h, c, _, _ = fr.lstm_cell(z, c0)
    torch.testing.assert_close(h, h1[0], rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(c, c1[0], rtol=1e-13, atol=1e-13)
    # ... and the same through gx: the x part alone (raw sums), then the recurrent part and the bias on top
    gx, _ = fr.gates_x_layer(a3, p["lstm.weight_ih_l0"])
    z2, Sz2 = fr.gates_layer(gx, None, h0, p)
    torch.testing.assert_close(z2, z, rtol=1e-13, atol=1e-13)
    assert bool((Sz2 <= Sz + 1e-12).all())
    _, _, E_h, E_c = fr.lstm_cell(z, c0, 6.0 * fr.U24 * Sz)
    assert bool((E_h > 0).all()) and bool((E_c > 0).all()) and float(E_h.max()) < 1e-4


# ---- (b) decoders -------------------------------------------------------------------------------------------------------------
def test_decoders_round_trip():
    from test_split3_host import _samples, split3

    x = torch.from_numpy(_samples())
    x = x[: x.numel() // 64 * 64].reshape(-1, 64)
    rec = fr.encode_split3(x)
    assert rec.numel() == 384 * x.shape[0]
    assert torch.equal(fr.decode_split3(rec, 0, x.shape[0]), x.to(F64)), "three parts carry an f32 exactly"
    # the same parts as the numpy restatement of csrc/gemm_s3.h's record (tests/test_split3_host.py), in the record's order
    p0, p1, p2 = split3(x.numpy())[:3]
    parts = rec.view(torch.bfloat16).reshape(-1, 3, 64).to(torch.float32).numpy()
    for j, want in enumerate((p0, p1, p2)):
        assert np.array_equal(parts[:, j].view(np.uint32), want.view(np.uint32))
    rec2 = fr.encode_split_bf16(x)
    assert rec2.numel() == 256 * x.shape[0]  # the f32 tensor's bytes
    got = fr.decode_split_bf16(rec2, 0, x.shape[0])
    assert torch.equal(got, fr.round_split_bf16(x))
    live = x != 0
    assert float(((got - x.to(F64)).abs()[live] / x.to(F64).abs()[live]).max()) <= 2.0 ** -16  # two parts: 16 bits and a sign
    # offsets inside a larger buffer, f32
    buf = torch.cat([torch.full((12,), 0xFF, dtype=torch.uint8), x.contiguous().view(torch.uint8).reshape(-1)])
    assert torch.equal(fr.decode_f32(buf, 12, tuple(x.shape)), x.to(F64))
    assert bool(torch.isnan(fr.decode_f32(buf, 8, (1,))).all()) and bool(torch.isnan(fr.decode_split3(buf, 0, 1, 2)).all())
    z = torch.arange(3 * 2048, dtype=F64).reshape(3, 2048)
    gx = fr.gates_to_gx(z)
    assert torch.equal(fr.gx_to_gates(gx), z)
    assert float(gx[1, 4 * 7 + 2]) == float(z[1, 2 * 512 + 7])  # column = 4 * unit + gate
    ha = torch.arange(64, dtype=F64).reshape(2, 32)
    adv, v = fr.decode_ha(ha, 6)
    assert adv.shape == (2, 6) and float(v[1, 0]) == 63.0 and float(adv[1, 5]) == 37.0


def test_restated_arithmetics_on_exact_data():
    """small integers: every arithmetic gives the exact sum; and on data that needs all 24 bits f32x3 is f32-accurate while
    bf16x2 is not"""
    rng = np.random.default_rng(3)
    X = torch.from_numpy(rng.integers(-3, 4, (7, 40)).astype(np.float32))
    W = torch.from_numpy(rng.integers(-3, 4, (40, 5)).astype(np.float32))
    b = torch.arange(5, dtype=torch.float32)
    for arith in ("f32", "f32x3", "bf16x2"):
        assert torch.equal(fr.restate_gemm(X, W, b, arith), X @ W + b), arith
    X = torch.from_numpy(rng.normal(0, 1, (32, 300)).astype(np.float32))
    W = torch.from_numpy(rng.normal(0, 1, (300, 16)).astype(np.float32))
    y, S = X.to(F64) @ W.to(F64), X.to(F64).abs() @ W.to(F64).abs()
    fig = {a: float(((fr.restate_gemm(X, W, None, a).to(F64) - y).abs() / (fr.U24 * S)).max()) for a in ("f32", "f32x3", "bf16x2")}
    assert fig["f32"] < 302 and fig["f32x3"] < 305 and fig["f32x3"] < 3 * fig["f32"] + 3
    assert 8 * fig["f32x3"] < fig["bf16x2"] < 128 * fr.worst_case_units("bf16x2", 300)


# ---- section 3: the conditions on the bounds ------------------------------------------------------------------------------------
LAYER_K = {"conv1": 256, "conv2": 512, "conv3": 576, "fc": 3136, "heads": 512, "gates": 3648, "gates_h": 513, "gates_x": 3136}


def _all_bounds():
    for scale in fr.SCALES:
        yield "ffnet", scale, fr.ffnet_case_bounds(18, scale)
        yield "lstm", scale, fr.lstm_case_bounds(18, scale)
        yield "ffnet sparse", scale, fr.ffnet_case_bounds(18, scale, True)
        yield "lstm sparse", scale, fr.lstm_case_bounds(18, scale, sparse=True)
    yield "ffnet A=6", 1.0, fr.ffnet_case_bounds(6, 1.0)
    yield "lstm zero state", 1.0, fr.lstm_case_bounds(18, 1.0, True)


def test_bounds_stay_below_the_worst_case_of_the_arithmetic():
    for name, scale, B in _all_bounds():
        for (arith, layer), b in B.items():
            print("BOUND %s scale=%g %s %s b=%.4g" % (name, scale, arith, layer, b))
            assert b > 0, (name, arith, layer)
            if layer == "duel":  # A products (exact: the mask is 0 / 1), A additions, a division, an addition, a subtraction
                assert b < 18 + 3, (name, b)
            else:
                record = arith == "bf16x2" and layer in ("conv1", "conv2", "conv3")
                assert b < fr.worst_case_units(arith, LAYER_K[layer], record), (name, arith, layer, b)


# ---- (c) restated defects -------------------------------------------------------------------------------------------------------
class Case:
    """float64 activations of N_CPU frames of the test's own inputs through both networks, layer by layer"""

    def __init__(self, scale, sparse=False):
        self.scale = scale
        self.p = tparams(fr.ffnet_params(18, scale, sparse))
        self.pl = tparams(fr.lstm_params(18, scale, sparse))
        self.obs, self.legal = fr.all_obs()[:N_CPU], torch.from_numpy(fr.all_legal(18)[:N_CPU])
        self.h0, self.c0 = (torch.from_numpy(v[:N_CPU]) for v in fr.all_state())
        self.B, self.BL = fr.ffnet_case_bounds(18, scale, sparse), fr.lstm_case_bounds(18, scale, sparse=sparse)
        self.clean = self.ffnet()
        self.clean_l = self.lstm()

    def ffnet(self, hooks=None, norelu=(), duel_legal_mean=False, inputs=None):
        """-> dict of (y, S) per layer and q; hooks: {layer: defect}; inputs: {layer: replacement input (float64)}"""
        hooks, p, inputs = hooks or {}, self.p, inputs or {}
        out = {}
        out["conv1"] = fr.conv1_layer(self.obs, p["net.0.weight"], p["net.0.bias"], defect=hooks.get("conv1"))
        out["conv2"] = fr.conv_layer(inputs.get("conv2", out["conv1"][0]), p["net.2.weight"], p["net.2.bias"], 20, 4, 2,
                                     "conv2" not in norelu, defect=hooks.get("conv2"))
        out["conv3"] = fr.conv_layer(inputs.get("conv3", out["conv2"][0]), p["net.4.weight"], p["net.4.bias"], 9, 3, 1,
                                     "conv3" not in norelu, defect=hooks.get("conv3"))
        a3 = inputs.get("fc", out["conv3"][0]).reshape(-1, 3136)
        out["fc"] = fr.linear_layer(a3, fr.fc_weight_last(p["linear.0.weight"].to(F64)), p["linear.0.bias"], "fc" not in norelu,
                                    defect=hooks.get("fc"))
        out["heads"] = fr.heads_layer(out["fc"][0], p["fc_a.weight"], p["fc_a.bias"], p["fc_v.weight"], p["fc_v.bias"],
                                      defect=hooks.get("heads"))
        ha = out["heads"][0]
        out["duel"] = fr.duel_layer(ha[:, :18], ha[:, 18:], self.legal, legal_mean=duel_legal_mean)
        return out

    def lstm(self, hooks=None, order=(0, 1, 2, 3), via_gx=False):
        hooks, p = hooks or {}, self.pl
        a1, _ = fr.conv1_layer(self.obs, p["net.0.weight"], p["net.0.bias"])
        a2, _ = fr.conv2_layer(a1, p["net.2.weight"], p["net.2.bias"])
        a3, _ = fr.conv3_layer(a2, p["net.4.weight"], p["net.4.bias"])
        out = {"a3": a3}
        if via_gx:
            out["gates_x"] = fr.gates_x_layer(a3, p["lstm.weight_ih_l0"], defect=hooks.get("gates_x"))
            out["gates"] = fr.gates_layer(out["gates_x"][0], None, self.h0, p, defect=hooks.get("gates"))
            bz = self.BL["f32", "gates_h"]
        else:
            out["gates"] = fr.gates_layer(None, a3, self.h0, p, defect=hooks.get("gates"))
            bz = self.BL["f32", "gates"]
        z, Sz = out["gates"]
        out["cell"] = fr.lstm_cell(z, self.c0, bz * fr.U24 * Sz, order)
        return out


@pytest.fixture(scope="module", params=fr.SCALES)
def case(request):
    return Case(request.param)


@pytest.fixture(scope="module")
def sparse_cases():
    """the sparse inputs (forward_ref.sparse_a3): one value of a3 in sixteen is non-zero"""
    return {scale: Case(scale, sparse=True) for scale in fr.SCALES}


def _effect(got, want, u):
    (y1, _), (y, S) = got, want
    return float(((y1 - y).abs() / (u * S)).max())


def _worst_bound_in_u24(B, layer):
    """the loosest bound any arithmetic gives the layer, in units of 2^-24"""
    return max(b * fr.UNIT[a] / fr.U24 for (a, lay), b in B.items() if lay == layer)


def _reject(case, name, layer, effect_u24, bound_u24, dq=None):
    """the layer check rejects the defect with a factor 4 to spare; dq: what the defect does to the network's output"""
    q_max = max(1.0, float(case.clean["duel"][0].abs().max()))  # (the existing suites: atol = 1e-4 x max(1, max|Q|))
    caught = "" if dq is None else "; Q moves by %.3g of max(1, max|Q|): the Q-level tolerance %s it" % (
        dq / q_max, "also catches" if dq > Q_TOL * q_max else "does NOT catch")
    print("DEFECT scale=%g %-58s layer=%-8s effect=%.4g x 2^-24, bound=%.4g%s" % (case.scale, name, layer, effect_u24, bound_u24, caught))
    assert bound_u24 < effect_u24 / 4, (name, layer, effect_u24, bound_u24)


def _dq(case, out):
    return float((out["duel"][0] - case.clean["duel"][0]).abs().max())


def test_defect_fc_without_its_last_k_chunk(case):
    def drop(y, c):
        return y - c["x"][:, -32:] @ c["w"][:, -32:].t()

    out = case.ffnet({"fc": drop})
    _reject(case, "fc without its last k-chunk (32 of 3,136 terms)", "fc", _effect(out["fc"], case.clean["fc"], fr.U24),
            _worst_bound_in_u24(case.B, "fc"), _dq(case, out))

    def drop_one(y, c):  # per row the last term whose activation is not zero (a dropped zero changes nothing, rightly)
        k = torch.stack([torch.nonzero(r)[-1, 0] for r in c["x"]])
        return y - c["x"].gather(1, k[:, None]) * c["w"][:, k].t()

    out = case.ffnet({"fc": drop_one})
    _reject(case, "fc without its last non-zero term (1 of 3,136)", "fc", _effect(out["fc"], case.clean["fc"], fr.U24),
            _worst_bound_in_u24(case.B, "fc"), _dq(case, out))


def test_defect_conv2_without_pixel_80(case):
    def drop(y, c):
        y = y.clone()
        y[:, 80] = c["b"]
        return y

    out = case.ffnet({"conv2": drop})
    _reject(case, "conv2 without pixel 80 (bias only)", "conv2", _effect(out["conv2"], case.clean["conv2"], fr.U24),
            _worst_bound_in_u24(case.B, "conv2"), _dq(case, out))


def test_defect_conv3_without_one_tap_at_the_last_row(case):
    def drop(y, c):
        w = torch.zeros_like(c["w"])
        w[:, :, 2, 1] = c["w"][:, :, 2, 1]
        tap, _ = fr.conv_layer(c["x"], w, torch.zeros_like(c["b"]), 9, 3, 1, False)
        y = y.clone()
        y[:, 42:] -= tap[:, 42:]  # output row 6 reads the image's last row through kh = 2
        return y

    out = case.ffnet({"conv3": drop})
    _reject(case, "conv3 without tap (2, 1) at the image's last row", "conv3", _effect(out["conv3"], case.clean["conv3"], fr.U24),
            _worst_bound_in_u24(case.B, "conv3"), _dq(case, out))

    def drop_one(y, c):  # one term: one channel of that tap at one pixel
        y = y.clone()
        x = c["x"].reshape(-1, 9, 9, 64)
        y[:, 48] -= x[:, 8, 7, 5:6] * c["w"][:, 5, 2, 1]
        return y

    out = case.ffnet({"conv3": drop_one})
    _reject(case, "conv3 without one term (1 of 576) at pixel 48", "conv3", _effect(out["conv3"], case.clean["conv3"], fr.U24),
            _worst_bound_in_u24(case.B, "conv3"), _dq(case, out))


@pytest.mark.parametrize("layer", ["conv2", "conv3", "fc"])
def test_defect_last_frame_from_the_previous_frames_input(case, layer):
    src = {"conv2": "conv1", "conv3": "conv2", "fc": "conv3"}[layer]
    x = case.clean[src][0].clone()
    x[-1] = x[-2]
    out = case.ffnet(inputs={layer: x})
    _reject(case, "last frame of a ragged tile from the previous frame's input", layer,
            _effect(out[layer], case.clean[layer], fr.U24), _worst_bound_in_u24(case.B, layer), _dq(case, out))


@pytest.mark.parametrize("layer", ["conv2", "conv3", "fc", "heads"])
@pytest.mark.parametrize("times", [2, 0])
def test_defect_bias_twice_or_not_at_all(case, layer, times):
    def bias(y, c):
        return y + (times - 1) * c["b"]

    out = case.ffnet({layer: bias})
    _reject(case, "bias added %s" % ("twice" if times == 2 else "not at all"), layer, _effect(out[layer], case.clean[layer], fr.U24),
            _worst_bound_in_u24(case.B, layer), _dq(case, out))


@pytest.mark.parametrize("layer", ["conv2", "conv3", "fc"])
def test_defect_missing_relu(case, layer):
    out = case.ffnet(norelu=(layer,))
    _reject(case, "missing ReLU", layer, _effect(out[layer], case.clean[layer], fr.U24), _worst_bound_in_u24(case.B, layer),
            _dq(case, out))


def _layer_operands(case, layer):
    """(x [M, K] f32 as the layer of a record trunk is given it, w [O, K] f32, clean (y, S) pre-activation) of conv3 / fc /
    gates_x"""
    if layer == "conv2":  # (on the bit-exact a1 of the record trunks, as the GPU test checks it there)
        a1 = fr.conv1_i8_exact(case.obs, case.p["net.0.weight"], case.p["net.0.bias"])
        x = fr.patches(a1.to(F64), 20, 4, 2).reshape(-1, 512)
        w = case.p["net.2.weight"].reshape(64, 512)
        b = case.p["net.2.bias"]
    elif layer == "conv3":
        x = fr.patches(case.clean["conv2"][0], 9, 3, 1).reshape(-1, 576)
        w = case.p["net.4.weight"].reshape(64, 576)
        b = case.p["net.4.bias"]
    elif layer == "fc":
        x, w, b = case.clean["conv3"][0].reshape(-1, 3136), fr.fc_weight_last(case.p["linear.0.weight"]), case.p["linear.0.bias"]
    else:
        x, w, b = case.clean_l["a3"].reshape(-1, 3136), fr.fc_weight_last(case.pl["lstm.weight_ih_l0"]), None
    return x, w, b


@pytest.mark.parametrize("layer", ["conv2", "conv3", "fc", "gates_x"])
def test_defect_lo_x_hi_dropped_in_bf16x2(case, layer):
    x, w, b = _layer_operands(case, layer)
    x = fr.round_split_bf16(x.to(torch.float32))  # what the records hold
    y, S = fr.linear_layer(x, w, b)
    x_lo, w_hi = fr.bf16_parts(x, 2)[1].to(F64), fr.bf16_parts(w, 2)[0].to(F64)
    B = case.BL if layer == "gates_x" else case.B
    _reject(case, "a_lo x b_hi dropped (bf16x2)", layer, _effect((y - x_lo @ w_hi.t(), S), (y, S), fr.U24),
            B["bf16x2", layer] * fr.U17 / fr.U24)


def _i_plus_j_2_dropped(case, layer):
    """-> (effect, bound) in units of 2^-24"""
    x, w, b = _layer_operands(case, layer)
    x = x.to(torch.float32)
    y, S = fr.linear_layer(x, w, b)
    xp, wp = [t.to(F64) for t in fr.bf16_parts(x, 3)], [t.to(F64) for t in fr.bf16_parts(w, 3)]
    kept = sum(xp[i] @ wp[j].t() for i in range(3) for j in range(3) if i + j <= 1)
    if b is not None:
        kept = kept + b.to(F64)
    B = case.BL if layer == "gates_x" else case.B
    return _effect((kept, S), (y, S), fr.U24), B["f32x3", layer]


@pytest.mark.parametrize("layer", ["conv2", "conv3"])
def test_defect_products_with_i_plus_j_2_dropped_in_f32x3_convs(case, layer):
    _reject(case, "the products with i + j = 2 dropped (f32x3)", layer, *_i_plus_j_2_dropped(case, layer))
    if layer == "conv2":
        # the propagated obs -> a2 bound, which the record trunks are ALSO held to, cannot see this defect (E(a2) is ten
        # times b2 u S2: conv1's fixed-point weights): conv2's own check on the bit-exact a1 is the one that rejects it
        a2, E = fr.conv12_span(case.obs, case.p, case.B["f32x3", "conv1"], case.B["f32x3", "conv2"], fr.U24)
        print("DEFECT scale=%g conv2: the propagated bound is %.3g .. %.3g x 2^-24 of S2 (b2 = %.3g)"
              % (case.scale, float((E / (fr.U24 * case.clean["conv2"][1])).min()),
                 float((E / (fr.U24 * case.clean["conv2"][1])).max()), case.B["f32x3", "conv2"]))


def test_conv1_i8_exact_is_the_bit_exact_restatement():
    p, obs = fr.ffnet_params(18, 4.6), fr.all_obs()[:3]
    want = fr.conv1_i8_restated(obs, p["net.0.weight"], p["net.0.bias"])
    got = fr.conv1_i8_exact(obs, p["net.0.weight"], p["net.0.bias"], chunk=2)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("layer", ["fc", "gates_x"])
def test_defect_products_with_i_plus_j_2_dropped_in_f32x3_long_sums(case, sparse_cases, layer):
    """Over the ~1,600 non-zero terms of an fc or gate element the dropped products (2^-16 of a term, random sign) average
    out: the check still fails on them, but by a factor 2..3, not 4.  With the sparse inputs (forward_ref.SPARSE_CASES, run
    by the GPU test for every f32x3 case, at both scales) the factor is there."""
    effect, bound = _i_plus_j_2_dropped(case, layer)
    print("DEFECT scale=%g the products with i + j = 2 dropped (f32x3), dense inputs: layer=%s effect=%.4g x 2^-24, bound=%.4g"
          % (case.scale, layer, effect, bound))
    assert bound < effect, (layer, effect, bound)
    sparse_case = sparse_cases[case.scale]
    _reject(sparse_case, "the products with i + j = 2 dropped (f32x3), sparse inputs", layer, *_i_plus_j_2_dropped(sparse_case, layer))


def _cell_effect(case, out, clean):
    h, c, E_h, E_c = clean["cell"]
    h1, c1 = out["cell"][:2]
    return float(((h1 - h).abs() / E_h).max()), float(((c1 - c).abs() / E_c).max()), float(max((h1 - h).abs().max(), (c1 - c).abs().max()))


@pytest.mark.parametrize("via_gx", [False, True])
def test_defect_w_hh_last_4_columns_dropped(case, via_gx):
    def drop(y, c):
        k = c["x"].shape[1]
        return y - c["x"][:, k - 4:] @ c["w"][:, k - 4:].t()

    clean = case.lstm(via_gx=via_gx)
    out = case.lstm({"gates": drop}, via_gx=via_gx)
    eh, ec, d = _cell_effect(case, out, clean)
    print("DEFECT scale=%g W_hh's last 4 columns dropped (gx=%d): h at %.4g and c at %.4g of the propagated bound; h, c move by %.3g"
          % (case.scale, via_gx, eh, ec, d))
    assert eh > 4 and ec > 4


def test_defect_gate_order_i_g_f_o(case):
    clean = case.clean_l
    eh, ec, d = _cell_effect(case, case.lstm(order=(0, 2, 1, 3)), clean)
    print("DEFECT scale=%g gate order i, g, f, o: h at %.4g and c at %.4g of the propagated bound; h, c move by %.3g"
          % (case.scale, eh, ec, d))
    assert eh > 4 and ec > 4


def test_defect_duel_mean_over_the_legal_actions(case):
    out = case.ffnet(duel_legal_mean=True)
    _reject(case, "the duel's mean over the legal actions only", "duel", _effect(out["duel"], case.clean["duel"], fr.U24),
            case.B["f32", "duel"], _dq(case, out))
    # the row with a single legal action is where the two means differ most: q = v there with the defect
    assert float((out["duel"][0][0] - case.clean["duel"][0][0]).abs().max()) > 0
