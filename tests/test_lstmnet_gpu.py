"""GPU parity of the AtariLSTMNet step (conv trunk -> fused LSTM gates/cell GEMM -> heads) against
a plain PyTorch fp32 forward of the same architecture (rela_amd/pyrela/net.py, itself checked to
be identical to the reference's pyrela/net.py).  Tolerance 1e-4 abs+rel."""
import ctypes as C

import numpy as np
import pytest

from kernel_names import CONV12, CONV12_JOBS  # noqa: F401

pytestmark = pytest.mark.gpu

KEYS = ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias",
        "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc_v.weight", "fc_v.bias",
        "fc_a.weight", "fc_a.bias"]


class GpuLstmNet:
    def __init__(self, params, A):
        from rela_amd import _capi as capi

        self.capi, self.A = capi, A
        h = C.c_void_p()
        capi.check(capi.lib.rela_lstmnet_create(C.byref(h), A, 0), "rela_lstmnet_create")
        self.h = h
        p = capi.LSTMNetParams()
        keep = []
        for (field, _), k in zip(capi.LSTMNetParams._fields_, KEYS):
            a = np.ascontiguousarray(params[k], np.float32)
            keep.append(a)
            setattr(p, field, a.ctypes.data_as(C.c_void_p))
        capi.check(capi.lib.rela_lstmnet_load(h, C.byref(p), 0, None), "rela_lstmnet_load")

    def step(self, s, legal, h_in, c_in):
        import torch

        from gpu_util import cur_stream, dev, ptr

        n = s.shape[0]
        d = [dev(x) for x in (s, legal, h_in, c_in)]
        h_out, c_out = torch.empty((n, 512), device="cuda"), torch.empty((n, 512), device="cuda")
        q, adv = torch.empty((n, self.A), device="cuda"), torch.empty((n, self.A), device="cuda")
        nb = self.capi.lib.rela_lstmnet_workspace_bytes(self.h, n)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        self.capi.check(self.capi.lib.rela_lstmnet_step(self.h, n, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(h_out),
                                                        ptr(c_out), ptr(q), ptr(adv), ptr(ws), nb, cur_stream()), "step")
        torch.cuda.synchronize()
        return h_out.cpu().numpy(), c_out.cpu().numpy(), q.cpu().numpy(), adv.cpu().numpy()

    def close(self):
        self.capi.lib.rela_lstmnet_destroy(self.h)


@pytest.mark.parametrize("precision", ["f32", "f32x3", "bf16x2"])
@pytest.mark.parametrize("N,A", [(1, 18), (5, 6), (80, 18), (131, 18), (1537, 18), (3200, 18)])
def test_lstm_step_vs_torch(N, A, precision):
    """All three precision modes against the plain PyTorch fp32 step, with the launched kernels asserted: in bf16x2 mode
    the trunk's split-bf16 kernels from 128 rows and the rec64 gate GEMM (lstm_gates_x_bf16) from 1,024 rows are
    compared with torch-fp32 directly; in f32x3 mode, from 512 rows, the conv trunk and the x part of the gate GEMM run with
    three-part operands on the bf16 matrix cores (csrc/conv12_s3.h, conv_img_s3.h, gemm_s3.h), the rest on the f32 kernels."""
    import torch

    from rela_amd.pyrela.net import AtariLSTMNet, dueling_q
    from synth import synth_lstm_params, synth_obs

    p = synth_lstm_params(A, 40 + A)
    net = GpuLstmNet(p, A)
    rng = np.random.default_rng(N)
    s = synth_obs(N, 500 + N)
    legal = (rng.uniform(size=(N, A)) < 0.85).astype(np.float32)
    h_in = rng.normal(0, 0.3, (N, 512)).astype(np.float32)
    c_in = rng.normal(0, 0.5, (N, 512)).astype(np.float32)
    net.capi.check(net.capi.lib.rela_lstmnet_set_precision(net.h, {"f32": 0, "bf16x2": 1, "f32x3": 2}[precision]), "set_precision")
    with net.capi.launch_census() as census:
        h, c, q, adv = net.step(s, legal, h_in, c_in)
    fast = {CONV12, "conv_bf16s<Conv3F>"} | ({"gemm_rec64_nt"} if N >= 1024 else set())
    # f32x3 from 512 rows (r5): the trunk on split3 records and the x part of the gates as a three-part GEMM
    emu = {"conv12_s3", "conv3_img_s3", "gemm_s3<gates_x>"}
    x3 = precision == "f32x3" and N >= 512
    if precision == "bf16x2" and N >= 128:
        assert fast <= set(census.counts), sorted(census.counts)
    else:
        assert not (fast & set(census.counts)) and (x3 or "conv1_bf16x3" in census.counts), sorted(census.counts)
    assert (emu <= set(census.counts)) if x3 else not (emu & set(census.counts)), sorted(census.counts)
    ref = AtariLSTMNet("cpu", A)
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    with torch.no_grad():
        x = ref._features(torch.from_numpy(s)).unsqueeze(0)
        o, (hr, cr) = ref.lstm(x, (torch.from_numpy(h_in).unsqueeze(0), torch.from_numpy(c_in).unsqueeze(0)))
        adv_r = ref.fc_a(o).squeeze(0)
        q_r = dueling_q(ref.fc_v(o), ref.fc_a(o), torch.from_numpy(legal).unsqueeze(0), 2).squeeze(0)
    tol = dict(rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(h, hr.squeeze(0).numpy(), **tol)
    np.testing.assert_allclose(c, cr.squeeze(0).numpy(), **tol)
    np.testing.assert_allclose(adv, adv_r.numpy(), **tol)
    np.testing.assert_allclose(q, q_r.numpy(), **tol)
    net.close()


@pytest.mark.parametrize("N", [127, 128, 131, 1537, 3200])
def test_lstm_step_fast_trunk_within_stated_tolerance(N):
    """rela_lstmnet_set_precision(1): the conv trunk on split-bf16 MFMA for batches of 128 rows and more (conv1 -> conv2
    fused, conv3); below 1,024 rows a3 goes back to f32 for the f32 gate GEMM, from 1,024 rows up (1537: ragged last
    row block, 3200: the bench's shape) the x part of the gates is one split-bf16 GEMM on a3's records and the f32 MFMA
    kernel adds h x W_hh and runs the cell; the heads stay f32.  h, c, Q and the advantages stay within the fast mode's
    stated tolerance of the exact f32 step (N = 127 takes the f32 kernels: identical)."""
    from synth import synth_lstm_params, synth_obs

    A = 18
    net = GpuLstmNet(synth_lstm_params(A, 51), A)
    rng = np.random.default_rng(N)
    s = synth_obs(N, 900 + N)
    legal = np.ones((N, A), np.float32)
    h_in = rng.normal(0, 0.3, (N, 512)).astype(np.float32)
    c_in = rng.normal(0, 0.5, (N, 512)).astype(np.float32)
    ref = net.step(s, legal, h_in, c_in)
    net.capi.check(net.capi.lib.rela_lstmnet_set_precision(net.h, 1), "set_precision")
    assert net.capi.lib.rela_lstmnet_precision(net.h) == 1
    fast = net.step(s, legal, h_in, c_in)
    for a, b, name in zip(fast, ref, ("h", "c", "q", "adv")):
        err = float(np.abs(a - b).max())
        assert err < 4e-6, (name, err)
        if N < 128:
            assert np.array_equal(a, b), name
    assert float((fast[2].argmax(1) == ref[2].argmax(1)).mean()) >= 0.995
    net.close()


# test_lstm_step_f32x3_is_f32_accurate: how much further from f64 than the f32 mode the f32x3 mode may be (mean / max |error|
# of h, c and Q), and how much further the bf16x2 mode must be than f32x3 (mean |error|) -- so that the test would notice
# f32x3 running two-part arithmetic anywhere in the step.  Measured on the MI355X (f32x3 / f32: mean 0.34-0.97, max
# 0.25-1.22; bf16x2 / f32x3, mean: h 5.8-7.1 and c 6.0-7.4 at a fresh initialisation, 30-37 at x 4.6; Q 2.8-3.5 and 30-37:
# Q's error at a fresh initialisation is half f32 rounding of the heads, which every mode runs in f32)
X3_MEAN_SLACK, X3_MAX_SLACK = 1.25, 1.5
BF16X2_SEPARATION = {"h": 4.0, "c": 4.0, "q": 2.0}


@pytest.mark.parametrize("scale", [1.0, 4.6])
@pytest.mark.parametrize("N", [515, 1537, 3200])
def test_lstm_step_f32x3_is_f32_accurate(N, scale, record_property):
    """h, c and Q of one step in all three precision modes against a float64 evaluation of the same step on the CPU
    (tests/f64_ref.py): the f32x3 mode is as close to f64 as the exact f32 mode (mean and max |error|), and the bf16x2
    mode is several times further away.  N = 515 (ragged, just above kEmuConvMinN), 1,537 (ragged row blocks of the
    gate GEMM) and 3,200 (the R2D2 actor's rows in bench.py); at a fresh initialisation and with every tensor x 4.6 (the
    scale of trained weights).  The launch census shows the three-part kernels (conv12_s3, conv3_img_s3,
    gemm_s3<gates_x>) and no split-bf16 kernel in the f32x3 step.  The measured errors are recorded."""
    import torch

    from f64_ref import err_stats, lstmnet_step
    from kernel_names import SPLIT_BF16, X3_LSTM
    from synth import synth_lstm_params, synth_obs

    A = 18
    p = {k: (v * scale).astype(np.float32) for k, v in synth_lstm_params(A, 61).items()}
    rng = np.random.default_rng(N + 17)
    s = synth_obs(N, 700 + N)
    legal = (rng.uniform(size=(N, A)) < 0.85).astype(np.float32)
    legal[:, 0] = 1.0
    h_in = rng.normal(0, 0.3, (N, 512)).astype(np.float32)
    c_in = rng.normal(0, 0.5, (N, 512)).astype(np.float32)
    ref = lstmnet_step(p, s, legal, h_in, c_in, torch.float64)
    net = GpuLstmNet(p, A)
    err = {}
    for mode in ("f32", "f32x3", "bf16x2"):
        net.capi.check(net.capi.lib.rela_lstmnet_set_precision(net.h, {"f32": 0, "bf16x2": 1, "f32x3": 2}[mode]), mode)
        with net.capi.launch_census() as census:
            out = net.step(s, legal, h_in, c_in)
        ran = set(census.counts)
        if mode == "f32x3":
            assert X3_LSTM <= ran and not (SPLIT_BF16 & ran), sorted(ran)
        elif mode == "bf16x2":
            assert {CONV12, "conv_bf16s<Conv3F>"} | ({"gemm_rec64_nt"} if N >= 1024 else set()) <= ran, sorted(ran)
        else:
            assert not ((X3_LSTM | SPLIT_BF16) & ran), sorted(ran)
        err[mode] = {name: err_stats(got, r) for name, got, r in zip(("h", "c", "q"), out[:3], ref[:3])}
    net.close()
    for mode, e in err.items():
        for name, (mx, mean) in e.items():
            record_property("max_abs_err_vs_f64_%s_%s" % (name, mode), mx)
            record_property("mean_abs_err_vs_f64_%s_%s" % (name, mode), mean)
    print("N=%d x%.1f |err| vs f64 (max / mean): %s" % (N, scale, "; ".join(
        "%s %s" % (m, " ".join("%s %.3g/%.3g" % (k, *v) for k, v in e.items())) for m, e in err.items())))
    for name in ("h", "c", "q"):
        f32, x3, b2 = err["f32"][name], err["f32x3"][name], err["bf16x2"][name]
        record_property("bf16x2_over_f32x3_mean_%s" % name, b2[1] / x3[1])
        assert x3[1] <= X3_MEAN_SLACK * f32[1], (name, err)
        assert x3[0] <= X3_MAX_SLACK * f32[0], (name, err)
        assert b2[1] >= BF16X2_SEPARATION[name] * x3[1], (name, err)
