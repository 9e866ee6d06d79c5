"""Float64 references of the forward pass ONE LAYER AT A TIME, the decoders of the workspace formats, and the plain
restatements of the three arithmetics from which the per-layer error bounds are taken.

The forwards (rela_ffnet_forward, rela_lstmnet_step) leave every layer's output in the caller's workspace
(csrc/ffnet_layout.h; rela_ffnet_debug_workspace / rela_lstmnet_debug_workspace say where and in which format).  A test
reads a layer's device INPUT and device OUTPUT from there and compares the output with a float64 evaluation of that
layer alone on that input, so the only error left is this layer's arithmetic.  It is measured per element against the sum
of the absolute values of the element's terms,

    figure = |got - y| / (u * S),      S = |W| . |x| + |b|,

with u = 2^-24 for the f32 and f32x3 layers and u = 2^-17 for the split-bf16 layers (two bf16 parts: 16 significant bits).

Every layer function returns (y, S) in float64, evaluated with unfold + matmul on `device` (data movement and float64
matmuls only: none of the project's kernels, no convolution library), frames in chunks.  Activations are channel-last
[n, pixels, C] as the kernels store them; weights are state_dict tensors.

WHERE THE BOUNDS COME FROM.  For every (arithmetic, layer) `restate_gemm` computes the same contraction on the CPU in that
arithmetic -- not in any kernel's order, just the arithmetic:
    f32     a float32 fused multiply-add chain over k
    f32x3   three bf16 parts per operand, the six products with i + j <= 2 (exact in f32), f32 accumulation with the
            small products in accumulators of their own (csrc/gemm_f32emu.h)
    bf16x2  hi + lo bf16 operands, a_lo b_hi + a_hi b_lo + a_hi b_hi, f32 accumulation
and the bound b of the layer is BOUND_MARGIN (2) x the largest figure of that restatement against float64 over the first
rows of the test's own inputs (RESTATE_FRAMES frames for the convolutions, RESTATE_ROWS / RESTATE_GATE_ROWS rows for fc
and the gates: 10^5..10^6 elements per layer).  The margin covers the kernels summing in another order and the maximum
over the up to 10^7 elements of a case (for near-normal errors the expected maximum grows with sqrt(2 ln n): 5.7 against
5.0 sigma).  Nothing here is derived from a device's output.

conv1 of the two record trunks runs on the int8 matrix cores with 24-bit fixed-point weights; its restatement is the
bit-exact one of tests/test_conv1_i8_gpu.py (expected_records), imported unchanged.  Those trunks do not store a1, so
their check spans obs -> a2 with the propagated bound  E(a2) = |W2| . E(a1) + b2 u S2,  E(a1) = b1 u S1.

THE LSTM CELL (gemm_mfma's kEpiLstmCell epilogue, csrc/gemm_f32.h).  From the pre-activations z = (i, f, g, o):
    c' = sig(f) * c + sig(i) * tanh(g)         10 float32 operations: 2 x (expf, add, divide), tanhf, 2 multiplies, 1 add
    h' = sig(o) * tanh(c')                      5 float32 operations: expf, add, divide, tanhf, multiply
The bound propagates E(z) through the cell with the derivatives taken in float64 and adds one rounding (u) per float32
operation, the two library functions included (a sigmoid counts 3 u, a tanh 1 u of the term they enter):
    E(c') = |c| sig'(f) E(f) + |tanh g| sig'(i) E(i) + sig(i) tanh'(g) E(g) + u (4 |sig(f) c| + 5 |sig(i) tanh(g)| + |c'|)
    E(h') = |tanh c'| sig'(o) E(o) + sig(o) tanh'(c') E(c') + 5 u |h'|
(No library promises half an ulp for expf and tanhf; the count is the issue's, and the device keeps it: E(z) dominates.)
Both get float32's smallest normal, 2^-126, on top: with trained-scale weights a gate reaches z = -115, where expf(-z)
is past float32's range and the kernel's sigmoid is 0 against a true 1e-50 -- no relative bound holds below the format.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U24, U17 = 2.0 ** -24, 2.0 ** -17
UNIT = {"f32": U24, "f32x3": U24, "bf16x2": U17}
BOUND_MARGIN = 2.0
# the first rows of the case's own inputs the restatements run over: frames for the convolutions, rows of a3 for fc, rows
# of a3 for the (four times as wide) gate GEMMs, rows of h (float64, from the frames) for heads and duel -- what a few
# seconds of one CPU core allow per net
RESTATE_FRAMES, RESTATE_ROWS, RESTATE_GATE_ROWS, RESTATE_HEAD_ROWS = 128, 128, 64, 512
F32_TINY = 2.0 ** -126  # float32's smallest normal: below it a result is not the rounded value (flush to zero, expf -> inf)
F64 = torch.float64

# formats of a1 / a2 / a3 (rela_debug_workspace_view), TrunkKind, FcKind (csrc/ffnet_plan.h)
NOT_WRITTEN, FMT_F32, FMT_SPLIT_BF16, FMT_SPLIT3 = 0, 1, 2, 3
TRUNK_F32, TRUNK_BF16, TRUNK_S3 = 0, 1, 2
FC_F32_SPLITK, FC_F32_GEMM, FC_BF16, FC_BF16_SPLITK, FC_S3, FC_S3_SPLITK = range(6)
TRUNK_ARITH = {TRUNK_F32: "f32", TRUNK_BF16: "bf16x2", TRUNK_S3: "f32x3"}
FC_ARITH = {FC_F32_SPLITK: "f32", FC_F32_GEMM: "f32", FC_BF16: "bf16x2", FC_BF16_SPLITK: "bf16x2", FC_S3: "f32x3",
            FC_S3_SPLITK: "f32x3"}


# ---- decoders: workspace bytes -> float64 values as the next kernel reads them -------------------------------------------
def _bytes(buf, off, nbytes):
    return buf[off:off + nbytes]


def decode_f32(buf, off, shape):
    n = int(np.prod(shape))
    return _bytes(buf, off, 4 * n).view(torch.float32).reshape(shape).to(F64)


def decode_split_bf16(buf, off, pixels, C=64):
    """[pixels][hi C | lo C] bf16 (in the f32 tensor's bytes) -> [pixels, C], value = hi + lo"""
    r = _bytes(buf, off, 4 * C * pixels).view(torch.bfloat16).reshape(pixels, 2, C).to(F64)
    return r[:, 0] + r[:, 1]


def decode_split3(buf, off, pixels, C=64):
    """split3 records (csrc/gemm_s3.h): 6 C bytes per pixel, [part 0 | part 1 | part 2] x C bf16 -> p0 + p1 + p2"""
    r = _bytes(buf, off, 6 * C * pixels).view(torch.bfloat16).reshape(pixels, 3, C).to(F64)
    return r[:, 0] + r[:, 1] + r[:, 2]


def bf16_parts(x, n):
    """the first n bf16 parts of the float32 values of x (round to nearest even, each residual exact), as f32 tensors"""
    rest = torch.as_tensor(x).to(torch.float32)
    parts = []
    for _ in range(n):
        p = rest.to(torch.bfloat16).to(torch.float32)
        parts.append(p)
        rest = rest - p
    return parts


def encode_split_bf16(x):
    """[pixels, C] f32 -> uint8 bytes of the split-bf16 records"""
    hi, lo = bf16_parts(x, 2)
    return torch.stack([hi, lo], 1).to(torch.bfloat16).contiguous().view(torch.uint8).reshape(-1)


def encode_split3(x):
    return torch.stack(bf16_parts(x, 3), 1).to(torch.bfloat16).contiguous().view(torch.uint8).reshape(-1)


def round_split_bf16(x):
    """the value a split-bf16 record holds of the float32 x"""
    hi, lo = bf16_parts(x, 2)
    return hi.to(F64) + lo.to(F64)


def gx_to_gates(gx):
    """gx [n, 2048] with column = 4 * unit + gate -> [n, 2048] in torch's order gate * 512 + unit"""
    return gx.reshape(-1, 512, 4).permute(0, 2, 1).reshape(-1, 2048)


def gates_to_gx(z):
    return z.reshape(-1, 4, 512).permute(0, 2, 1).reshape(-1, 2048)


def decode_ha(ha, A):
    """ha [n, 32]: columns 0..A-1 = fc_a, column 31 = fc_v -> (adv [n, A], v [n, 1])"""
    return ha[:, :A], ha[:, 31:32]


# ---- float64 layers ----------------------------------------------------------------------------------------------------
def _t(x, device):
    return torch.as_tensor(x).detach().to(device)


def _f(x, device):
    return _t(x, device).to(F64)


def conv1_weight(w, device="cpu"):
    """the operand the kernels are given: float32(w) / 255.0f rounded to float32 (csrc/weight_pack.h), as float64"""
    w32 = torch.as_tensor(w).detach().to("cpu", torch.float32)
    return (w32 / torch.tensor(255.0, dtype=torch.float32)).to(device, F64)


def fc_weight_last(w):
    """[O, 3136] in torch's flatten order c * 49 + pos -> the kernels' k = pos * 64 + c (channel-last a3, flattened)"""
    return w.reshape(w.shape[0], 64, 49).permute(0, 2, 1).reshape(w.shape[0], 3136)


def patches(x_last, hw, k, stride):
    """channel-last [n, H * W, C] -> im2col rows [n, L, C k k] (k order c, kh, kw: that of weight.reshape(O, -1))"""
    n, _, C = x_last.shape
    x = x_last.reshape(n, hw, hw, C).permute(0, 3, 1, 2)
    return F.unfold(x, k, stride=stride).permute(0, 2, 1)


def conv_layer(x_last, w, b, hw, k, stride, relu=True, device="cpu", chunk=64, defect=None):
    """one convolution on channel-last input -> (y, S) channel-last [n, L, O]; w [O, C, k, k], b [O]"""
    x_last, w, b = _f(x_last, device), _f(w, device), _f(b, device)
    wm = w.reshape(w.shape[0], -1).t()
    ys, ss = [], []
    with torch.no_grad():
        for lo in range(0, x_last.shape[0], chunk):
            p = patches(x_last[lo:lo + chunk], hw, k, stride)
            ys.append(p @ wm + b)
            ss.append(p.abs() @ wm.abs() + b.abs())
    y, S = torch.cat(ys), torch.cat(ss)
    if defect:
        y = defect(y, dict(x=x_last, w=w, b=b, hw=hw, k=k, stride=stride, S=S))
    return (torch.relu(y) if relu else y), S


def conv1_layer(obs, w, b, device="cpu", chunk=64, defect=None):
    """u8 frames [n, 4, 84, 84] -> relu(conv1) [n, 400, 32]"""
    x = _t(obs, device).reshape(-1, 4, 84 * 84).permute(0, 2, 1).to(F64)
    return conv_layer(x, conv1_weight(w, device), b, 84, 8, 4, True, device, chunk, defect)


def conv2_layer(a1, w, b, device="cpu", chunk=64, defect=None):
    return conv_layer(a1, w, b, 20, 4, 2, True, device, chunk, defect)


def conv3_layer(a2, w, b, device="cpu", chunk=64, defect=None):
    return conv_layer(a2, w, b, 9, 3, 1, True, device, chunk, defect)


def linear_layer(x, w, b, relu=False, device="cpu", defect=None):
    """x [n, K], w [O, K] (the k order of x), b [O] or None -> (y, S)"""
    x, w = _f(x, device), _f(w, device)
    with torch.no_grad():
        y, S = x @ w.t(), x.abs() @ w.abs().t()
        if b is not None:
            y, S = y + _f(b, device), S + _f(b, device).abs()
        if defect:
            y = defect(y, dict(x=x, w=w, b=None if b is None else _f(b, device), S=S))
    return (torch.relu(y) if relu else y), S


def fc_layer(a3, w, b, device="cpu", defect=None):
    """a3 channel-last [n, 49, 64] -> relu(fc) [n, 512]; w = linear.0.weight in the state_dict's order"""
    return linear_layer(_f(a3, device).reshape(-1, 3136), fc_weight_last(_f(w, device)), b, True, device, defect)


def heads_layer(h, a_w, a_b, v_w, v_b, device="cpu", defect=None):
    """-> (ha [n, A + 1], S): columns 0..A-1 = fc_a, the last = fc_v"""
    w = torch.cat([_f(a_w, device), _f(v_w, device)])
    b = torch.cat([_f(a_b, device).reshape(-1), _f(v_b, device).reshape(-1)])
    return linear_layer(h, w, b, False, device, defect)


def duel_layer(adv, v, legal, device="cpu", legal_mean=False):
    """q = v + a * legal - mean_A(a * legal)  (pyrela/net.py: the mean is over A, not over the legal actions);
    S = |v| + |a * legal| + mean_A |a * legal|.  legal_mean: the restated defect (mean over the legal actions)"""
    adv, v, legal = _f(adv, device), _f(v, device).reshape(-1, 1), _f(legal, device)
    la = adv * legal
    den = legal.sum(1, keepdim=True).clamp(min=1) if legal_mean else float(adv.shape[1])
    return v + la - la.sum(1, keepdim=True) / den, v.abs() + la.abs() + la.abs().sum(1, keepdim=True) / adv.shape[1]


def gates_x_layer(a3, w_ih, device="cpu", defect=None):
    """the x part of the gates, raw sums: a3 [n, 49, 64] . W_ih^T -> [n, 2048] in torch's gate order"""
    return linear_layer(_f(a3, device).reshape(-1, 3136), fc_weight_last(_f(w_ih, device)), None, False, device, defect)


def gates_layer(gx, a3, h_in, p, device="cpu", defect=None):
    """pre-activations z [n, 2048] (torch's order i, f, g, o) and S: from the device's gx (torch order, raw sums) where it
    is written, else from a3"""
    b = _f(p["lstm.bias_ih_l0"], device) + _f(p["lstm.bias_hh_l0"], device)
    w_hh = _f(p["lstm.weight_hh_l0"], device)
    if gx is not None:
        y, S = linear_layer(h_in, w_hh, b, False, device, defect)
        gx = _f(gx, device)
        return y + gx, S + gx.abs()
    w = torch.cat([fc_weight_last(_f(p["lstm.weight_ih_l0"], device)), w_hh], 1)
    x = torch.cat([_f(a3, device).reshape(-1, 3136), _f(h_in, device)], 1)
    return linear_layer(x, w, b, False, device, defect)


CELL_U = dict(fc=4.0, ig=5.0, c=1.0, h=5.0)  # roundings per term, in u = 2^-24 (see the module's docstring)


def lstm_cell(z, c_in, E_z=None, order=(0, 1, 2, 3)):
    """-> (h, c, E_h, E_c): torch.nn.LSTM's cell on z (gate order i, f, g, o) in float64 and, with E_z, the bound on the
    kernel's float32 h and c.  order: the restated defect reads the gates in another order"""
    zi, zf, zg, zo = (z.reshape(-1, 4, 512)[:, j] for j in order)
    c_in = c_in.to(z.device, F64)
    i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
    c = f * c_in + i * g
    tc = torch.tanh(c)
    h = o * tc
    if E_z is None:
        return h, c, None, None
    Ei, Ef, Eg, Eo = (E_z.reshape(-1, 4, 512)[:, j] for j in range(4))
    n = CELL_U
    E_c = (c_in.abs() * f * (1 - f) * Ef + g.abs() * i * (1 - i) * Ei + i * (1 - g * g) * Eg +
           U24 * (n["fc"] * (f * c_in).abs() + n["ig"] * (i * g).abs() + n["c"] * c.abs()))
    E_h = tc.abs() * o * (1 - o) * Eo + o * (1 - tc * tc) * E_c + U24 * n["h"] * h.abs()
    return h, c, E_h + F32_TINY, E_c + F32_TINY


def err_units(got, y, S, u):
    """-> (largest |got - y| / (u S) over the elements, its flat index); NaN (an element nobody wrote) counts as inf"""
    got = torch.as_tensor(got).to(y.device, F64).reshape(y.shape)
    fig = (got - y).abs() / (u * S)
    fig = torch.where(torch.isnan(fig), torch.full_like(fig, float("inf")), fig)
    i = int(fig.argmax())
    return float(fig.reshape(-1)[i]), i


def err_vs_bound(got, y, E):
    """largest |got - y| / E for a propagated per-element bound E"""
    got = torch.as_tensor(got).to(y.device, F64).reshape(y.shape)
    fig = (got - y).abs() / E
    fig = torch.where(torch.isnan(fig), torch.full_like(fig, float("inf")), fig)
    i = int(fig.argmax())
    return float(fig.reshape(-1)[i]), i


def conv12_span(obs, p, b1, b2, u, device="cpu", chunk=64, defect2=None):
    """obs -> a2 through a float64 a1 (the record trunks do not store a1): (a2, E(a2)) with the propagated bound
    E(a2) = |W2| . E(a1) + b2 u S2,  E(a1) = b1 u S1  (ReLU is 1-Lipschitz)"""
    a1, S1 = conv1_layer(obs, p["net.0.weight"], p["net.0.bias"], device, chunk)
    a2, S2 = conv2_layer(a1, p["net.2.weight"], p["net.2.bias"], device, chunk, defect2)
    zero = torch.zeros(64, dtype=F64, device=device)
    _, prop = conv_layer(b1 * u * S1, p["net.2.weight"], zero, 20, 4, 2, False, device, chunk)
    return a2, prop + b2 * u * S2


# ---- the arithmetics, restated on the CPU ---------------------------------------------------------------------------------
def restate_gemm(X, Wt, bias, arith, bias_first=False):
    """X [M, K] f32, Wt [K, O] f32, bias [O] f32 or None -> f32 [M, O] computed in `arith` (see the module's docstring).
    bias_first: the (main) accumulator starts from the bias instead of taking it last.  The kernels over records do
    both (gemm_s3 with one slice and the convolutions of conv12_s3 start their accumulator from the bias, the split-K
    forms leave it to fc_reduce), and the two differ where the bias is a large share of S: every rounding of the running
    sum then happens at the bias's magnitude.  The bounds of the f32x3 and bf16x2 layers take the worse of the two; the
    f32 kernels (conv1_bf16x3, conv_mfma, gemm_mfma, heads_duel) all add the bias behind the sum, and so does their
    restatement (_worse_placement).
    f32: the product is exact in float64 and the float64 addition's own rounding is 2^-29 of a float32 rounding, so
    rounding the float64 sum to float32 is the fused multiply-add up to that."""
    X, Wt = torch.as_tensor(X).to(torch.float32), torch.as_tensor(Wt).to(torch.float32)
    M, K = X.shape
    O = Wt.shape[1]
    start = torch.zeros(M, O)
    if bias is not None and bias_first:
        start, bias = start + torch.as_tensor(bias).to(torch.float32), None
    if arith == "f32":
        Xd, Wd = X.to(F64), Wt.to(F64)
        acc = start.to(F64)
        for k in range(K):
            acc = torch.addcmul(acc, Xd[:, k:k + 1], Wd[k:k + 1]).to(torch.float32).to(F64)
        out = acc.to(torch.float32)
    elif arith == "f32x3":
        a, b = bf16_parts(X, 3), bf16_parts(Wt, 3)
        acc = [start, torch.zeros(M, O), torch.zeros(M, O)]
        for k in range(K):
            ak, bk = [t[:, k:k + 1] for t in a], [t[k:k + 1] for t in b]
            for i in range(3):
                for j in range(3 - i):
                    acc[i + j] = acc[i + j] + ak[i] * bk[j]  # (a product of two bf16 values is exact in f32)
        out = acc[0] + (acc[1] + acc[2])
    elif arith == "bf16x2":
        (ah, al), (bh, bl) = bf16_parts(X, 2), bf16_parts(Wt, 2)
        out = start
        for k in range(K):
            out = out + al[:, k:k + 1] * bh[k:k + 1]
            out = out + ah[:, k:k + 1] * bl[k:k + 1]
            out = out + ah[:, k:k + 1] * bh[k:k + 1]
    else:
        raise ValueError(arith)
    return out if bias is None else out + torch.as_tensor(bias).to(torch.float32)


def worst_case_units(arith, K, record=False):
    """the classical worst-case bound of a K-term float32 sum with bias (gamma_{K+1} ~ (K + 1) u), plus the mode's operand
    term, in the mode's unit: f32x3 drops the products with i + j > 2 (3 x 2^-24 of a term); bf16x2 rounds both operands
    to 16 bits (2 units) and drops lo x lo (2^-16: 2 units), its f32 accumulation counts 2^-7 unit per term; a record
    output adds its own rounding (1 unit)"""
    if arith == "f32":
        return K + 2.0
    if arith == "f32x3":
        return K + 2.0 + 3.0
    return (K + 2.0) / 128.0 + 4.0 + (1.0 if record else 0.0)


def _figure(got, y, S, u):
    return float(((got.to(F64) - y).abs() / (u * S)).max())


def _worse_placement(figure, arith):
    """the larger figure of the placements of the bias that the kernels of `arith` use (restate_gemm)"""
    return figure(False) if arith == "f32" else max(figure(False), figure(True))


def _restate_conv(x_last, w, b, hw, k, stride, arith, record):
    """restated relu(conv) on channel-last f32 input against float64 -> figure in the arithmetic's unit"""
    p = patches(x_last.to(F64), hw, k, stride).reshape(-1, w[0].numel()).to(torch.float32)
    y, S = conv_layer(x_last, w, b, hw, k, stride)

    def figure(bias_first):
        got = torch.relu(restate_gemm(p, w.reshape(w.shape[0], -1).t(), b, arith, bias_first))
        got = round_split_bf16(got) if record else got
        return _figure(got.reshape(y.shape), y, S, UNIT[arith])

    return _worse_placement(figure, arith)


def conv1_i8_restated(obs, w, b):
    """conv1 on the int8 matrix cores (24-bit fixed-point weights), bit for bit: tests/test_conv1_i8_gpu.py's
    restatement, unchanged -> relu(conv1) f32 [n, 400, 32]"""
    from test_conv1_i8_gpu import expected_records

    _, y, _ = expected_records(np.ascontiguousarray(obs), np.asarray(w, np.float32), np.asarray(b, np.float32))
    return torch.from_numpy(np.ascontiguousarray(y))


def conv1_i8_exact(obs, w, b, device="cpu", chunk=64):
    """The same arithmetic as conv1_i8_restated with the integer sums as float64 matmuls on `device` (every sum is an
    integer below 2^31: exact), for whole batches: digits, scales and folded bias from test_conv1_i8_gpu.quantise, then
    u = f32(S_hi) * 65536 + f32(S_mid * 256 + S_lo);  y = relu(u * s_c + b'_c), each float32 operation rounded on its own
    -> relu(conv1) f32 [n, 400, 32], the a1 the record trunks hand to conv2 (tests/test_forward_ref_cpu.py: bit for bit
    conv1_i8_restated)"""
    from test_conv1_i8_gpu import quantise

    sc, _, bq, digits = quantise(np.asarray(w, np.float32), np.asarray(b, np.float32))
    D = [torch.from_numpy(d.astype(np.float64)).to(device).t() for d in digits]  # hi, mid, lo: [256, 32]
    sc, bq = torch.from_numpy(sc).to(device), torch.from_numpy(bq).to(device)
    x = _t(obs, device).reshape(-1, 4, 84 * 84).permute(0, 2, 1)
    out = []
    for lo in range(0, x.shape[0], chunk):
        P = patches(x[lo:lo + chunk].to(F64) - 128.0, 84, 8, 4)
        hi, mid, low = (P @ d for d in D)
        u = hi.to(torch.float32) * 65536.0 + (mid * 256.0 + low).to(torch.float32)
        y = u * sc
        out.append(torch.relu(y + bq))
    return torch.cat(out)


def _weights(p):
    return {k: torch.as_tensor(v).detach().to("cpu", torch.float32) for k, v in p.items()}


def _as_input(x, arith):
    """a float64 activation as the next layer of `arith` is given it: float32, or what a split-bf16 record holds"""
    x32 = x.to(torch.float32)
    return round_split_bf16(x32).to(torch.float32) if arith == "bf16x2" else x32


def trunk_bounds(p, obs):
    """{(arith, layer): b} for conv1 / conv2 / conv3 in the three arithmetics, from the first RESTATE_FRAMES frames; also
    returns a3 (float64, all of obs) for the layers behind the trunk"""
    p = _weights(p)
    obs = torch.as_tensor(obs)
    a1, S1 = conv1_layer(obs, p["net.0.weight"], p["net.0.bias"])
    a2, _ = conv2_layer(a1, p["net.2.weight"], p["net.2.bias"])
    a3, _ = conv3_layer(a2, p["net.4.weight"], p["net.4.bias"])
    R = min(RESTATE_FRAMES, obs.shape[0])
    a1, S1, a2 = a1[:R], S1[:R], a2[:R]
    out = {}
    # conv1: the f32 trunk multiplies the u8 frames with the weight's three exact bf16 parts and accumulates in f32
    w1 = conv1_weight(p["net.0.weight"]).to(torch.float32)
    x = obs[:R].reshape(R, 4, 84 * 84).permute(0, 2, 1).to(torch.float32)
    out["f32", "conv1"] = BOUND_MARGIN * _restate_conv(x, w1, p["net.0.bias"], 84, 8, 4, "f32", False)
    i8 = conv1_i8_restated(obs[:R].numpy(), p["net.0.weight"].numpy(), p["net.0.bias"].numpy())
    out["f32x3", "conv1"] = BOUND_MARGIN * _figure(i8, a1[:R], S1[:R], U24)
    out["bf16x2", "conv1"] = BOUND_MARGIN * _figure(round_split_bf16(i8), a1[:R], S1[:R], U17)
    for arith in ("f32", "bf16x2", "f32x3"):
        rec = arith == "bf16x2"
        out[arith, "conv2"] = BOUND_MARGIN * _restate_conv(_as_input(a1[:R], arith), p["net.2.weight"], p["net.2.bias"], 20, 4,
                                                           2, arith, rec)
        out[arith, "conv3"] = BOUND_MARGIN * _restate_conv(_as_input(a2[:R], arith), p["net.4.weight"], p["net.4.bias"], 9, 3,
                                                           1, arith, rec)
    return out, a3


def _restate_linear(x, w, b, arith, relu):
    y, S = linear_layer(x, w, b, relu)

    def figure(bias_first):
        got = restate_gemm(x, w.t(), b, arith, bias_first)
        return _figure(torch.relu(got) if relu else got, y, S, UNIT[arith])

    return figure(False) if b is None else _worse_placement(figure, arith)


def head_bounds(p, h, legal):
    """{("f32", "heads"), ("f32", "duel")}: b from the case's own first RESTATE_HEAD_ROWS rows of h (float64, from its
    frames through the float64 layers) and of its legal masks"""
    p = _weights(p)
    R = min(RESTATE_HEAD_ROWS, h.shape[0])
    h32 = h[:R].to(torch.float32)
    w = torch.cat([p["fc_a.weight"], p["fc_v.weight"]])
    b = torch.cat([p["fc_a.bias"].reshape(-1), p["fc_v.bias"].reshape(-1)])
    out = {("f32", "heads"): BOUND_MARGIN * _restate_linear(h32, w, b, "f32", False)}
    ha = restate_gemm(h32, w.t(), b, "f32")
    adv, v, lg = ha[:, :-1], ha[:, -1:], torch.as_tensor(legal)[:R].to(torch.float32)
    la = adv * lg
    s = torch.zeros(R, 1)
    for j in range(adv.shape[1]):
        s = s + la[:, j:j + 1]
    got = (v + la) - s / torch.tensor(float(adv.shape[1]))
    y, S = duel_layer(adv, v, lg)
    out["f32", "duel"] = BOUND_MARGIN * _figure(got, y, S, U24)
    return out


def ffnet_trunk_fc_bounds(p, obs):
    """the (arith, layer) bounds of conv1 / conv2 / conv3 / fc of an AtariFFNet from its own parameters and frames (CPU
    only; they do not depend on the number of actions); also returns h (float64) of those frames"""
    out, a3_all = trunk_bounds(p, obs[:RESTATE_HEAD_ROWS])
    a3 = a3_all[:RESTATE_ROWS]
    pw = _weights(p)
    wl = fc_weight_last(pw["linear.0.weight"])
    for arith in ("f32", "bf16x2", "f32x3"):
        out[arith, "fc"] = BOUND_MARGIN * _restate_linear(_as_input(a3, arith).reshape(-1, 3136), wl, pw["linear.0.bias"], arith, True)
    return out, fc_layer(a3_all, pw["linear.0.weight"], pw["linear.0.bias"])[0]


def lstm_bounds(p, obs, h_in, c_in, trunk=None):
    """the (arith, layer) bounds of an AtariLSTMNet case but heads and duel: the trunk, the x part of the gates (raw
    sums), the whole gate GEMM (f32, K = 3648), the recurrent part on top of gx (f32, K = 512); also returns h' (float64)
    of the first RESTATE_HEAD_ROWS rows"""
    out, a3_all = trunk or trunk_bounds(p, obs[:RESTATE_HEAD_ROWS])
    out, a3 = dict(out), a3_all[:RESTATE_GATE_ROWS]
    pw = _weights(p)
    R = a3.shape[0]
    wx, whh = fc_weight_last(pw["lstm.weight_ih_l0"]), pw["lstm.weight_hh_l0"]
    bias = pw["lstm.bias_ih_l0"] + pw["lstm.bias_hh_l0"]
    hin = torch.as_tensor(h_in)[:R].to(torch.float32)
    for arith in ("bf16x2", "f32x3"):
        out[arith, "gates_x"] = BOUND_MARGIN * _restate_linear(_as_input(a3, arith).reshape(-1, 3136), wx, None, arith, False)
    x = torch.cat([a3.to(torch.float32).reshape(-1, 3136), hin], 1)
    out["f32", "gates"] = BOUND_MARGIN * _restate_linear(x, torch.cat([wx, whh], 1), bias, "f32", False)
    # the recurrent part on top of gx: the accumulator starts from gx, the bias is added last
    gx = restate_gemm(a3.to(torch.float32).reshape(-1, 3136), wx.t(), None, "f32")
    acc = gx.to(F64)
    for k in range(512):
        acc = torch.addcmul(acc, hin[:, k:k + 1].to(F64), whh.t()[k:k + 1].to(F64)).to(torch.float32).to(F64)
    got = acc.to(torch.float32) + bias
    y, S = gates_layer(gx, None, hin, pw)
    out["f32", "gates_h"] = BOUND_MARGIN * _figure(got, y, S, U24)
    # h' of the case's first rows in float64: the input of heads and duel
    n = a3_all.shape[0]
    z, _ = gates_layer(None, a3_all, torch.as_tensor(h_in)[:n], pw)
    return out, lstm_cell(z, torch.as_tensor(c_in)[:n])[0]


# ---- the cases' inputs (shared by the GPU test and the CPU test of the bounds) --------------------------------------------
OBS_SEED, MAX_ROWS = 9100, 2051
CASES_FFNET = {"f32": (1, 7, 130, 515, 1537, 2051), "bf16x2": (127, 128, 130, 257, 1024, 1025, 1537),
               "f32x3": (511, 512, 515, 1024, 1025, 2051)}
CASES_LSTM = {"f32": (1, 5, 131, 1537), "bf16x2": (128, 1024, 1025, 1537), "f32x3": (512, 515, 1537)}
SCALES = (1.0, 4.6)


@functools.lru_cache(maxsize=1)
def all_obs():
    from synth import synth_obs

    return synth_obs(MAX_ROWS, OBS_SEED)


@functools.lru_cache(maxsize=None)
def all_legal(A):
    """legal masks at 0.8; row 0 has a single legal action (and no row is empty)"""
    rng = np.random.default_rng(100 + A)
    legal = (rng.uniform(size=(MAX_ROWS, A)) < 0.8).astype(np.float32)
    legal[:, 0] = np.maximum(legal[:, 0], (legal.sum(1) == 0))
    legal[0] = 0.0
    legal[0, A // 2] = 1.0
    return legal


@functools.lru_cache(maxsize=None)
def all_state(zero=False):
    rng = np.random.default_rng(321)
    h = rng.normal(0, 0.3, (MAX_ROWS, 512)).astype(np.float32)
    c = rng.normal(0, 0.5, (MAX_ROWS, 512)).astype(np.float32)
    return (np.zeros_like(h), np.zeros_like(c)) if zero else (h, c)


# The "sparse" inputs.  Dropping the f32x3 products with i + j = 2 leaves an error of random sign per term, 2^-16 of the
# term: over the ~1,600 non-zero terms of an fc or gate element it averages out to 10..12 x 2^-24 of S, only 2..3 x the
# bound -- detected, but not with the factor 4 the CPU test asks of every restated defect.  The answer is other inputs,
# not another bound: with conv3's bias lowered by SPARSE_SHIFT standard deviations of conv3's pre-activations about one
# value of a3 in sixteen is non-zero, an element has ~200 terms, and the same defect stands out by more than that factor.
# fc's bias shrinks with its sums (x 1 / 16), so that it keeps its share of S: gemm_s3 starts its accumulator from the
# bias, and a bias that is a third of S puts every rounding of the running sum at its magnitude (restate_gemm).
SPARSE_SHIFT = 1.53


def sparse_a3(p):
    pt = _weights(p)
    a1, _ = conv1_layer(all_obs()[:8], pt["net.0.weight"], pt["net.0.bias"])
    a2, _ = conv2_layer(a1, pt["net.2.weight"], pt["net.2.bias"])
    z, _ = conv_layer(a2, pt["net.4.weight"], pt["net.4.bias"], 9, 3, 1, False)
    out = dict(p)
    out["net.4.bias"] = (p["net.4.bias"] - np.float32(SPARSE_SHIFT * float(z.std()))).astype(np.float32)
    if "linear.0.bias" in p:
        out["linear.0.bias"] = (p["linear.0.bias"] / np.float32(16)).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def ffnet_params(A, scale, sparse=False):
    from synth import synth_params

    p = synth_params(A, 61, scale)
    return sparse_a3(p) if sparse else p


@functools.lru_cache(maxsize=None)
def lstm_params(A, scale, sparse=False):
    """synth_lstm_params with every weight tensor (not the biases) x scale, as synth_params' gain"""
    from synth import synth_lstm_params

    p = synth_lstm_params(A, 62)
    p = {k: (v * np.float32(scale)).astype(np.float32) if v.ndim > 1 else v for k, v in p.items()}
    return sparse_a3(p) if sparse else p


@functools.lru_cache(maxsize=None)
def _ffnet_core(scale, sparse):
    # (synth_params draws the trunk and fc before the heads: they are the same for every A)
    return ffnet_trunk_fc_bounds(ffnet_params(18, scale, sparse), all_obs()[:RESTATE_HEAD_ROWS])


@functools.lru_cache(maxsize=None)
def ffnet_case_bounds(A, scale, sparse=False):
    core, h = _ffnet_core(scale, sparse)
    return {**core, **head_bounds(ffnet_params(A, scale, sparse), h, all_legal(A))}


@functools.lru_cache(maxsize=None)
def _lstm_trunk(scale, sparse):
    return trunk_bounds(lstm_params(18, scale, sparse), all_obs()[:RESTATE_HEAD_ROWS])


@functools.lru_cache(maxsize=None)
def _lstm_core(scale, zero_state, sparse):
    return lstm_bounds(lstm_params(18, scale, sparse), None, *all_state(zero_state), _lstm_trunk(scale, sparse))


@functools.lru_cache(maxsize=None)
def lstm_case_bounds(A, scale, zero_state=False, sparse=False):
    core, h = _lstm_core(scale, zero_state, sparse)
    return {**core, **head_bounds(lstm_params(A, scale, sparse), h, all_legal(A))}
