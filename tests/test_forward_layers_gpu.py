"""Every layer of the forward pass against float64, one layer at a time, through the caller's workspace.

One ordinary rela_ffnet_forward / rela_lstmnet_step runs with the workspace pre-filled with 0xFF bytes (NaN in f32 and in
bf16: an element nobody wrote cannot pass).  rela_ffnet_debug_workspace / rela_lstmnet_debug_workspace say where each
layer's output lies and in which format; the plan they report is asserted against the launch census.  Each layer's device
output is then compared with the float64 evaluation of that layer alone on the device's own input to it
(tests/forward_ref.py), every element, in units of u x the sum of the element's absolute terms.  The bounds are 2 x what a
plain CPU restatement of the layer's arithmetic reaches against float64 on the case's own first rows -- never a device
figure; tests/test_forward_ref_cpu.py shows they stay below the worst-case bound of the arithmetic and a quarter of every
restated defect.  The measured figures are in profiles/forward_layers_error_units.md.

Shapes are the smallest at which each path can go wrong (forward_ref.CASES_FFNET / CASES_LSTM): partial tiles, ragged
128- and 112-row blocks, the thresholds of the persistent convolutions (512 / 1,536), of the split-K fcs (128, 1,024,
2,048), of the record trunks (128, 512) and of the gate GEMM's x part (1,024 / 512).  90 cases take 45 s on the MI355X:
4-5 s for the first case of each net, scale and input set (the CPU restatements behind its bounds, cached), 0.1-0.3 s
for the others."""
import ctypes as C

import pytest

import forward_ref as fr
from kernel_names import CONV12, SPLIT_BF16, X3_FFNET, X3_LSTM

pytestmark = pytest.mark.gpu
MODE = {"f32": 0, "bf16x2": 1, "f32x3": 2}
TRUNK_KERNELS = {fr.TRUNK_F32: {"conv1_bf16x3", "conv_mfma<Conv2> (f32)", "conv_mfma<Conv3> (f32)"},
                 fr.TRUNK_BF16: {CONV12, "conv_bf16s<Conv3F>"},
                 fr.TRUNK_S3: {"conv12_s3", "conv3_img_s3"}}
FC_KERNELS = {fr.FC_F32_SPLITK: {"fc_reduce"}, fr.FC_F32_GEMM: {"gemm_mfma<GemmFc> (f32)"}, fr.FC_BF16: {"fc_bf16s"},
              fr.FC_BF16_SPLITK: {"fc_bf16s (split-K)", "fc_reduce"}, fr.FC_S3: {"gemm_s3<fc>"}, fr.FC_S3_SPLITK: {"gemm_s3<fc>"}}


def _cases(table):
    out = []
    for mode, sizes in table.items():
        for i, N in enumerate(sizes):
            for scale in fr.SCALES:
                out.append((mode, N, 18, scale))
                if i == 0:
                    out.append((mode, N, 6, scale))
    return out


def expected_ffnet_plan(mode, N):
    """(trunk, fc) of the issue's table, from the thresholds alone (csrc/ffnet_plan.h)"""
    if mode == "bf16x2" and N >= 128:
        return fr.TRUNK_BF16, (fr.FC_BF16 if N >= 1024 else fr.FC_BF16_SPLITK)
    if mode == "f32x3" and N >= 512:
        return fr.TRUNK_S3, (fr.FC_S3_SPLITK if N <= 1024 else fr.FC_S3)
    return fr.TRUNK_F32, (fr.FC_F32_SPLITK if N < 2048 else fr.FC_F32_GEMM)


class Report:
    """collects (layer, bound, figure) of a case, prints them, then asserts"""

    def __init__(self, tag, record_property):
        self.tag, self.rows, self.record = tag, [], record_property

    def add(self, layer, arith, bound, figure, index):
        self.rows.append((layer, arith, bound, figure, index))

    def finish(self):
        for layer, arith, bound, figure, index in self.rows:
            print("FIGURE %s layer=%s arith=%s bound=%.4g measured=%.4g" % (self.tag, layer, arith, bound, figure))
            self.record("%s_%s" % (layer, arith), figure)
        bad = [(layer, arith, bound, figure, index) for layer, arith, bound, figure, index in self.rows if not figure <= bound]
        assert not bad, "%s: (layer, arithmetic, bound, figure, flat index of the worst element) %s" % (self.tag, bad)


def untouched(ws, lo, hi):
    return bool((ws[lo:hi] == 0xFF).all())


def check_trunk(ws, view, N, obs, p, B, rep):
    """conv1 / conv2 / conv3 from the workspace; -> a3 [N, 49, 64] as the next kernel reads it (float64, on the device)"""
    w = lambda k: p[k]
    arith = fr.TRUNK_ARITH[view.trunk]
    u = fr.UNIT[arith]
    if view.trunk == fr.TRUNK_F32:
        assert (view.a1_format, view.a2_format, view.a3_format) == (fr.FMT_F32,) * 3
        a1 = fr.decode_f32(ws, view.a1, (N, 400, 32))
        a2 = fr.decode_f32(ws, view.a2, (N, 81, 64))
        a3 = fr.decode_f32(ws, view.a3, (N, 49, 64))
        y, S = fr.conv1_layer(obs, w("net.0.weight"), w("net.0.bias"), "cuda")
        rep.add("conv1", arith, B[arith, "conv1"], *fr.err_units(a1, y, S, u))
        y, S = fr.conv2_layer(a1, w("net.2.weight"), w("net.2.bias"), "cuda")
        rep.add("conv2", arith, B[arith, "conv2"], *fr.err_units(a2, y, S, u))
    else:
        # the record trunks do not store a1: obs -> a2 with the propagated bound, and a1's bytes stay as they were
        assert view.a1_format == fr.NOT_WRITTEN and untouched(ws, view.a1, view.a2), "a1 was written"
        if view.trunk == fr.TRUNK_BF16:
            assert view.a2_format == fr.FMT_SPLIT_BF16
            a2 = fr.decode_split_bf16(ws, view.a2, N * 81).reshape(N, 81, 64)
            a3 = (fr.decode_f32(ws, view.a3, (N, 49, 64)) if view.a3_format == fr.FMT_F32 else
                  fr.decode_split_bf16(ws, view.a3, N * 49).reshape(N, 49, 64))
        else:
            assert (view.a2_format, view.a3_format) == (fr.FMT_SPLIT3, fr.FMT_SPLIT3)
            assert untouched(ws, view.a2, view.a3 + 4 * 3136 * N), "the f32 places of a2 / a3 were written"
            a2 = fr.decode_split3(ws, view.rec2, N * 81).reshape(N, 81, 64)
            a3 = fr.decode_split3(ws, view.rec3, N * 49).reshape(N, 49, 64)
        y, E = fr.conv12_span(obs, p, B[arith, "conv1"], B[arith, "conv2"], u, "cuda")
        rep.add("conv1+conv2 (of the propagated bound)", arith, 1.0, *fr.err_vs_bound(a2, y, E))
        # ... and conv2 on its own at its own bound: conv1 on the int8 matrix cores is integer arithmetic up to one fixed
        # sequence of float32 operations, so the a1 the kernel hands to conv2 is known bit for bit without being stored
        a1 = fr.conv1_i8_exact(obs, w("net.0.weight"), w("net.0.bias"), "cuda")
        a1 = fr.round_split_bf16(a1) if view.trunk == fr.TRUNK_BF16 else a1
        y, S = fr.conv2_layer(a1, w("net.2.weight"), w("net.2.bias"), "cuda")
        rep.add("conv2", arith, B[arith, "conv2"], *fr.err_units(a2, y, S, u))
    y, S = fr.conv3_layer(a2, w("net.4.weight"), w("net.4.bias"), "cuda")
    rep.add("conv3", arith, B[arith, "conv3"], *fr.err_units(a3, y, S, u))
    return a3


def check_heads(ha, q, h, legal, p, A, B, rep):
    import torch

    assert not bool(torch.isnan(ha).any()), "a column of ha was not written"
    y, S = fr.heads_layer(h, p["fc_a.weight"], p["fc_a.bias"], p["fc_v.weight"], p["fc_v.bias"], "cuda")
    adv, v = fr.decode_ha(ha, A)
    rep.add("heads", "f32", B["f32", "heads"], *fr.err_units(torch.cat([adv, v], 1), y, S, fr.U24))
    y, S = fr.duel_layer(adv, v, legal, "cuda")
    rep.add("duel", "f32", B["f32", "duel"], *fr.err_units(q, y, S, fr.U24))


def filled(nbytes):
    import torch

    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")


def nans(*shape):
    import torch

    return torch.full(shape, float("nan"), device="cuda")


def _sparse(table):
    """every case of the f32x3 kernels again on the sparse inputs (forward_ref.sparse_a3), at which the check rejects the
    f32x3 defect of tests/test_forward_ref_cpu.py on the long sums of fc and the gates with its full margin"""
    return [("f32x3", N, 18, scale) for N in table["f32x3"] if N >= 512 for scale in fr.SCALES]


FFNET_CASES = [c + (False,) for c in _cases(fr.CASES_FFNET)] + [c + (True,) for c in _sparse(fr.CASES_FFNET)]


@pytest.mark.parametrize("mode,N,A,scale,sparse", FFNET_CASES)
def test_ffnet_layers(mode, N, A, scale, sparse, record_property):
    import torch

    from gpu_util import cur_stream, dev, ptr
    from rela_amd import _capi as capi
    from test_ffnet_gpu import GpuNet

    p = fr.ffnet_params(A, scale, sparse)
    B = fr.ffnet_case_bounds(A, scale, sparse)
    obs, legal = dev(fr.all_obs()[:N]), dev(fr.all_legal(A)[:N])
    net = GpuNet(p, A)
    net.set_precision(mode)
    view = capi.DebugWorkspaceView()
    capi.check(capi.lib.rela_ffnet_debug_workspace(net.h, N, C.byref(view)), "rela_ffnet_debug_workspace")
    nbytes = capi.lib.rela_ffnet_workspace_bytes(net.h, N)
    ws, q = filled(nbytes), nans(N, A)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_ffnet_forward(net.h, N, ptr(obs), ptr(legal), ptr(q), ptr(ws), nbytes, cur_stream()), "forward")
        torch.cuda.synchronize()
    net.close()
    # the plan: the issue's table, the tap and the kernels that really ran agree
    assert (view.trunk, view.fc) == expected_ffnet_plan(mode, N) and view.precision == MODE[mode]
    ran = set(census.counts)
    want = TRUNK_KERNELS[view.trunk] | FC_KERNELS[view.fc] | {"heads_duel"}
    others = set().union(*TRUNK_KERNELS.values(), *FC_KERNELS.values()) - want
    if view.fc_slices > 1:
        want |= {"fc_reduce"}
    assert want <= ran and not (others - {"fc_reduce"}) & ran, (sorted(ran), sorted(want))
    assert ("fc_reduce" in ran) == (view.fc_slices > 1)
    assert mode == "bf16x2" or not SPLIT_BF16 & ran, sorted(ran)
    assert (X3_FFNET <= ran) if view.trunk == fr.TRUNK_S3 else not X3_FFNET & ran, sorted(ran)
    assert 0 <= view.a1 < view.a2 < view.a3 < view.h < view.ha < view.fc_part < view.rec2 < view.rec3 < nbytes
    if view.fc == fr.FC_BF16_SPLITK:  # slices of fc_per positions of a3 cover its 49, the last one ragged
        assert (view.fc_slices - 1) * view.fc_per < 49 <= view.fc_slices * view.fc_per

    rep = Report("ffnet mode=%s N=%d A=%d scale=%g sparse=%d" % (mode, N, A, scale, sparse), record_property)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    a3 = check_trunk(ws, view, N, obs, pt, B, rep)
    h = fr.decode_f32(ws, view.h, (N, 512))
    arith = fr.FC_ARITH[view.fc]
    y, S = fr.fc_layer(a3, pt["linear.0.weight"], pt["linear.0.bias"], "cuda")
    rep.add("fc", arith, B[arith, "fc"], *fr.err_units(h, y, S, fr.UNIT[arith]))
    if view.fc_slices > 1:
        # the partial tiles: all written, and h = relu(bias + their sum) within one rounding per addition
        part = fr.decode_f32(ws, view.fc_part, (view.fc_slices, N, 512))
        assert not bool(torch.isnan(part).any()), "a partial tile of the split-K fc was not written"
        b = pt["linear.0.bias"].to("cuda", torch.float64)
        rep.add("fc_reduce", "f32", float(view.fc_slices + 1),
                *fr.err_units(h, torch.relu(part.sum(0) + b), part.abs().sum(0) + b.abs(), fr.U24))
    check_heads(fr.decode_f32(ws, view.ha, (N, 32)), q, h, legal, pt, A, B, rep)
    rep.finish()


# (+ h_in = c_in = 0 in both gate paths, + the sparse inputs)
LSTM_CASES = ([c + (False, False) for c in _cases(fr.CASES_LSTM)] +
              [("f32x3", 515, 18, 1.0, True, False), ("f32", 131, 18, 1.0, True, False)] +
              [c + (False, True) for c in _sparse(fr.CASES_LSTM)])


@pytest.mark.parametrize("mode,N,A,scale,zero_state,sparse", LSTM_CASES)
def test_lstmnet_layers(mode, N, A, scale, zero_state, sparse, record_property):
    import torch

    from gpu_util import cur_stream, dev, ptr
    from rela_amd import _capi as capi
    from test_lstmnet_gpu import GpuLstmNet

    p = fr.lstm_params(A, scale, sparse)
    B = fr.lstm_case_bounds(A, scale, zero_state, sparse)
    h0, c0 = fr.all_state(zero_state)
    obs, legal, h_in, c_in = dev(fr.all_obs()[:N]), dev(fr.all_legal(A)[:N]), dev(h0[:N]), dev(c0[:N])
    net = GpuLstmNet(p, A)
    capi.check(capi.lib.rela_lstmnet_set_precision(net.h, MODE[mode]), "set_precision")
    view = capi.DebugWorkspaceView()
    capi.check(capi.lib.rela_lstmnet_debug_workspace(net.h, N, C.byref(view)), "rela_lstmnet_debug_workspace")
    nbytes = capi.lib.rela_lstmnet_workspace_bytes(net.h, N)
    ws = filled(nbytes)
    h_out, c_out, q, adv = nans(N, 512), nans(N, 512), nans(N, A), nans(N, A)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_lstmnet_step(net.h, N, ptr(obs), ptr(legal), ptr(h_in), ptr(c_in), ptr(h_out), ptr(c_out),
                                              ptr(q), ptr(adv), ptr(ws), nbytes, cur_stream()), "step")
        torch.cuda.synchronize()
    net.close()
    trunk = fr.TRUNK_BF16 if mode == "bf16x2" and N >= 128 else (fr.TRUNK_S3 if mode == "f32x3" and N >= 512 else fr.TRUNK_F32)
    x_in_gx = (mode == "bf16x2" and N >= 1024) or trunk == fr.TRUNK_S3
    assert (view.trunk, bool(view.x_in_gx), view.precision) == (trunk, x_in_gx, MODE[mode])
    assert bool(view.a3_records) == x_in_gx
    ran = set(census.counts)
    gate_x = {fr.TRUNK_S3: "gemm_s3<gates_x>", fr.TRUNK_BF16: "gemm_rec64_nt"}
    want = TRUNK_KERNELS[trunk] | {"gemm_mfma<GemmLstmH> (f32)" if x_in_gx else "gemm_mfma<GemmLstm> (f32)"}
    if x_in_gx:
        want |= {gate_x[trunk]}
    others = (set().union(*TRUNK_KERNELS.values()) | set(gate_x.values()) |
              {"gemm_mfma<GemmLstmH> (f32)", "gemm_mfma<GemmLstm> (f32)"}) - want
    assert want <= ran and not others & ran, (sorted(ran), sorted(want))
    assert mode == "bf16x2" or not SPLIT_BF16 & ran, sorted(ran)
    assert (X3_LSTM <= ran) if trunk == fr.TRUNK_S3 else not X3_LSTM & ran, sorted(ran)
    assert 0 <= view.a1 < view.a2 < view.a3 < view.ha < view.gx < view.rec2 < view.rec3 < nbytes

    rep = Report("lstm mode=%s N=%d A=%d scale=%g zero=%d sparse=%d" % (mode, N, A, scale, zero_state, sparse), record_property)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    a3 = check_trunk(ws, view, N, obs, pt, B, rep)
    if x_in_gx:
        arith = fr.TRUNK_ARITH[trunk]
        gx = fr.gx_to_gates(fr.decode_f32(ws, view.gx, (N, 2048)))
        y, S = fr.gates_x_layer(a3, pt["lstm.weight_ih_l0"], "cuda")
        rep.add("gates_x", arith, B[arith, "gates_x"], *fr.err_units(gx, y, S, fr.UNIT[arith]))
        z, Sz = fr.gates_layer(gx, None, h_in, pt, "cuda")
        bz = B["f32", "gates_h"]
    else:
        assert untouched(ws, view.gx, view.gx + 4 * 2048 * N), "gx was written"
        z, Sz = fr.gates_layer(None, a3, h_in, pt, "cuda")
        bz = B["f32", "gates"]
    h, c, E_h, E_c = fr.lstm_cell(z, c_in, bz * fr.U24 * Sz)
    rep.add("cell c (of the propagated bound)", "f32", 1.0, *fr.err_vs_bound(c_out, c, E_c))
    rep.add("cell h (of the propagated bound)", "f32", 1.0, *fr.err_vs_bound(h_out, h, E_h))
    ha = fr.decode_f32(ws, view.ha, (N, 32))
    check_heads(ha, q, h_out.to(torch.float64), legal, pt, A, B, rep)
    assert torch.equal(adv, ha[:, :A].to(torch.float32)), "adv is not the raw fc_a output"
    rep.finish()
