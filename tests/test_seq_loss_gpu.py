"""The two stages of the R2D2 learner's backward pass between the Q tables and the BPTT, one call at a time (include/
rela_amd.h, csrc/learner_r2d2.hip):
  rela_debug_seq_loss_grad       seq_td_launch: q_min_all, seq_select, seq_td_loss, seq_head_grad
  rela_debug_seq_head_backward   seq_head_backward: d_o, the head weight gradients as one GEMM (below 1,024 rows) or as 32
                                 split-K slices + head_wgrad_reduce, the column sum of d_ha and head_bias_grad
against the float64 references, the inputs by role and the DERIVED bounds of tests/seq_loss_ref.py:
  a. the loss tap on R.loss_inputs: qa_on / qa_tg bit for bit (the greedy action on every row: ties, illegal maxima, padded
     rows, the place of the global minimum), e, dqa, d_ha, loss_seq, priority and loss within their bounds, the zeros of d_ha,
     the dyadic rows on the Huber kink, and every output bit for bit against the float32 restatement in the kernels' order,
     without and with value rescaling;
  b. the head tap: exact data EQUAL to the reference (every row of a weight gradient a distinct power of two), random data
     within the a-priori n_terms bound, the weight-gradient form of the row count in the census;
  c. both taps run the learner's code path: bit-identical to a learner step's own buffers, in every precision mode;
  d. bad arguments are refused.
tests/test_seq_loss_ref_cpu.py pins the references and shows which restated defects these checks catch."""
import ctypes as C

import numpy as np
import pytest

import seq_loss_ref as R

pytestmark = pytest.mark.gpu

LOSS_CENSUS = {"q_min_all": 1, "seq_select": 1, "seq_td_loss": 1, "seq_head_grad": 1}
LOSS_OUT = ("qa_on", "qa_tg", "dqa", "priority", "loss_seq", "loss", "d_ha")


def head_census(rows):
    """the two GEMMs count themselves (gemm_lds); the tap names the weight gradient's form"""
    if rows >= R.SPLIT_ROWS:
        return {"gemm_lds (f32)": 2, "head_wgrad (split-K)": 1, "head_wgrad_reduce": 1}
    return {"gemm_lds (f32)": 2, "head_wgrad (one launch)": 1}


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_device(inp):
    import torch

    return {k: (torch.from_numpy(np.array(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def bits(t):
    import torch

    t = torch.as_tensor(t)
    return t.detach().cpu().contiguous().view(torch.int32).flatten()


def run_loss(dev, vr_eps, gamma_n=R.GAMMA_N, eta=R.ETA):
    """dev: R.loss_inputs on the device -> ({LOSS_OUT: float32 tensors}, census); outputs start as NaN"""
    import torch

    from rela_amd import _capi as capi

    A, B, seq, burn, n = (dev[k] for k in ("A", "batch", "seq", "burn", "n"))
    rows = (seq + n) * B
    shapes = {"qa_on": (rows,), "qa_tg": (rows,), "dqa": (rows,), "priority": (B,), "loss_seq": (B,), "loss": (1,),
              "d_ha": (rows, 32)}
    out = {k: torch.full(shapes[k], float("nan"), dtype=torch.float32, device="cuda") for k in LOSS_OUT}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_seq_loss_grad(
            B, A, seq, burn, n, ptr(dev["q_on"]), ptr(dev["q_tg"]), ptr(dev["legal"]), ptr(dev["act"]), ptr(dev["reward"]),
            ptr(dev["bootstrap"]), ptr(dev["seq_lens"]), ptr(dev["weight"]), gamma_n, vr_eps, eta,
            *[ptr(out[k]) for k in LOSS_OUT], _stream()), "rela_debug_seq_loss_grad")
    torch.cuda.synchronize()
    return out, census.counts


def check_loss_case(shape, A, min_at, record):
    import torch

    inp = R.loss_inputs(shape[0], A, *shape[1:], min_at=min_at)
    ref = R.check_loss_inputs(inp, min_at)
    dev = to_device(inp)
    B, seq, burn, n = shape
    roles = R.row_roles(B, seq, burn, n)
    lens = inp["seq_lens"]
    units = {}
    for vr_eps in R.VR_EPS:
        got, counts = run_loss(dev, vr_eps)
        assert counts == LOSS_CENSUS, counts
        again, _ = run_loss(dev, vr_eps)
        for k in LOSS_OUT:
            assert torch.equal(bits(got[k]), bits(again[k])), (vr_eps, k)
        host = {k: got[k].cpu().numpy() for k in LOSS_OUT}
        # the gathers, bit for bit: the greedy action of every row (a row of q_tg holds distinct values)
        assert np.array_equal(host["qa_on"].view(np.int32), ref["qa_on"].astype(np.float32).view(np.int32)), vr_eps
        assert np.array_equal(host["qa_tg"].view(np.int32), ref["qa_tg"].astype(np.float32).view(np.int32)), vr_eps
        # everything after the gathers against the float32 restatement in the kernels' order (value_rescale_util's host
        # build of the rescaling): the same bits, which pins the kernel's e to e32
        e32 = R.e_f32(inp, ref["greedy"], vr_eps)
        f32 = R.td_loss_f32(inp, e32)
        for k in ("dqa", "loss_seq", "priority", "loss", "d_ha"):
            assert np.array_equal(host[k].view(np.int32), f32[k].view(np.int32)), (vr_eps, k)
        if vr_eps > 0:
            continue
        # ---- against float64, within the derived bounds ----
        err_e = np.abs(e32.astype(np.float64) - ref["e"])
        assert bool((err_e <= R.e_bound(ref)).all())
        units["e"] = float((err_e / np.maximum(R.e_bound(ref), 1e-300)).max())
        after = R.seq_reference(e=e32, **R.loss_args(inp))  # the roundings AFTER the kernel's own e
        d = host["d_ha"].astype(np.float64)

        def within(name, err, bound):
            if np.size(err) == 0:
                return
            assert bool((err <= bound).all()), (name, float((err / np.maximum(bound, 1e-300)).max()))
            units[name] = float((err / np.maximum(bound, 1e-300)).max())

        within("dqa", np.abs(host["dqa"] - after["dqa"]), R.dqa_bound(after))
        within("d_ha", np.abs(d[:, :A] - after["d_ha"][:, :A]), R.d_ha_bound(after))
        assert np.array_equal(host["d_ha"][:, 31].view(np.int32), host["dqa"].view(np.int32))  # column 31 IS dqa
        assert not d[:, A:31].any()
        assert not d[:, :A][inp["legal"] == 0].any()
        padded = np.array([role == "padded" for role in roles])
        assert not d[padded].any() and not host["dqa"][padded].any()
        within("loss_seq", np.abs(host["loss_seq"] - after["loss_seq"]), R._k(R.loss_seq_roundings(seq)) * after["loss_seq"])
        within("priority", np.abs(host["priority"] - after["priority"]), R._k(R.priority_roundings(seq)) * after["priority"])
        within("loss", np.abs(host["loss"][0] - after["loss"]), np.float64(R._k(R.loss_roundings(seq)) * after["loss"]))
        # a sequence of burn_in + 1 steps: max = mean = |e_0|
        one = np.flatnonzero(lens == burn + 1)
        a0 = np.abs(e32[0, one].astype(np.float64))
        within("one_step_priority", np.abs(host["priority"][one] - a0) / R.ONE_STEP_PRIORITY_UNITS, R.U_F32 * a0)
        # the dyadic rows: e exact, the clamp on the right side of the kink
        ef = e32.reshape(-1)
        for r, role in enumerate(roles[:seq * B]):
            b = r % B
            if role.startswith("dyadic"):
                e = {"dyadic_plus1": 1.0, "dyadic_minus1": -1.0, "dyadic_0": 0.0}[role]
                assert float(ef[r]) == e, (r, role, float(ef[r]))
                if e == 0:
                    assert not d[r].any(), r
                else:  # g = -(w * e) / B with w * e exact: the two roundings of fl(1 / B) and the product
                    g = -float(inp["weight"][b]) * e / B
                    assert abs(d[r, 31] - g) <= R._k(2) * abs(g), (r, d[r, 31], g)
            elif role.startswith("large"):  # the clamp: |g| = w / B whatever |e| >= 1.1 is
                g = float(inp["weight"][b]) / B
                assert abs(abs(d[r, 31]) - g) <= R._k(R.DQA_ROUNDINGS) * g and (g == 0 or np.sign(d[r, 31]) == -np.sign(ef[r])), (r, role)
    for k, v in units.items():
        print("B %d seq %d burn %d n %d A %d min at %s: %s %.3g units of its bound" % (*shape, A, min_at, k, v))
        record("units_%s" % k, v)


@pytest.mark.parametrize("shape,A", R.LOSS_CASES, ids=["B%d-seq%d-burn%d-n%d-A%d" % (*s, A) for s, A in R.LOSS_CASES])
def test_seq_loss_kernels_against_float64_and_float32(shape, A, record_property):
    """R.loss_inputs with the global minimum of q_on in the last element of the table, which lies in a padded row."""
    check_loss_case(shape, A, "last", record_property)


@pytest.mark.parametrize("min_at", ["i1023", "i1024"])
@pytest.mark.parametrize("shape,A", [(R.RAGGED, 18), ((1024, 3, 1, 1), 18)])
def test_the_global_minimum_at_element_1023_and_1024(shape, A, min_at, record_property):
    """the last element one 1024-lane pass of q_min_all reads and the first one of the next pass"""
    check_loss_case(shape, A, min_at, record_property)


# ---- b. the head backward ------------------------------------------------------------------------------------------------------
def run_head(dev):
    """dev: {A, d_ha, o, fc_a_w, fc_v_w} on the device -> ({HEAD_KEYS: float32 tensors}, census); outputs start as NaN"""
    import torch

    from rela_amd import _capi as capi

    rows, A = dev["d_ha"].shape[0], dev["A"]
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in R.head_shapes(rows, A).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_debug_seq_head_backward(
            rows, A, ptr(dev["d_ha"]), ptr(dev["o"]), ptr(dev["fc_a_w"]), ptr(dev["fc_v_w"]), *[ptr(out[k]) for k in R.HEAD_KEYS],
            _stream()), "rela_debug_seq_head_backward")
    torch.cuda.synchronize()
    return out, census.counts


@pytest.mark.parametrize("rows,A", R.HEAD_CASES)
def test_head_backward_exact_data_every_row_counted_once(rows, A):
    """Dyadic data whose every sum is exact in float32 (R.head_exact_inputs, preconditions asserted on the reference): all
    five outputs EQUAL the float64 reference cast to float32; in `rows` a dropped or doubled row or slice changes a weight
    gradient whatever else happens.  The census names the weight-gradient form of the row count."""
    import torch

    for name in R.HEAD_DATA_SETS:
        inp = R.head_exact_inputs(name, rows, A)
        dev = to_device(inp)
        ref, ab = R.head_reference(device="cuda", **dev), R.head_reference_abs(device="cuda", **dev)
        R.head_exact_preconditions(name, inp, {k: v.cpu() for k, v in ref.items()}, {k: v.cpu() for k, v in ab.items()})
        got, counts = run_head(dev)
        assert counts == head_census(rows), (name, counts)
        for key in R.HEAD_KEYS:
            want = ref[key].float().reshape(got[key].shape)
            if not torch.equal(got[key], want):
                bad = (got[key] != want).nonzero()
                first = tuple(int(i) for i in bad[0])
                raise AssertionError("%s, rows %d, A %d: %s differs in %d of %d elements; first at %s: got %r, expected %r" % (
                    name, rows, A, key, bad.shape[0], want.numel(), first, float(got[key][first]), float(want[first])))


@pytest.mark.parametrize("rows,A", R.HEAD_CASES)
def test_head_backward_random_data_within_the_n_terms_bound(rows, A, record_property):
    """d_ha with the loss kernel's structure, o in (-1, 1): per output element |got - ref| / (u * sum|terms|) below the
    a-priori bound of n_terms roundings (rows for the four gradients, A + 1 for d_o)."""
    dev = to_device(R.head_random_inputs(rows, A))
    ref, ab = R.head_reference(device="cuda", **dev), R.head_reference_abs(device="cuda", **dev)
    got, counts = run_head(dev)
    assert counts == head_census(rows), counts
    for key in R.HEAD_KEYS:
        units, bound = R.err_units(got[key], ref[key].reshape(got[key].shape), ab[key].reshape(got[key].shape), R.U_F32), R.head_n_terms(key, rows, A)
        print("rows %d A %d %s: %.3g units, bound %g" % (rows, A, key, units, bound))
        record_property("units_%s" % key, units)
        assert units <= bound, (key, units, bound)


# ---- c. wiring -------------------------------------------------------------------------------------------------------------------
SMALL, AT_1024 = (18, 5, 4, 2, 2), (18, 64, 12, 2, 4)  # (A, B, seq, burn, n); the second: 1,024 training rows, 1,152 frames
GAMMA = 0.997
WIRING = [(SMALL, m) for m in ("f32", "bf16x2", "f32x3", "f32x3_bwd")] + [(AT_1024, "f32")]


@pytest.mark.parametrize("shape,mode", WIRING, ids=["B%d-%s" % (s[1], m) for s, m in WIRING])
def test_the_taps_run_the_learners_code_path(shape, mode):
    """One learner step: its own q_on, q_tg and batch fields through the loss tap give its priorities, loss, loss_seq and
    d_ha; its d_ha, LSTM outputs and head weights through the head tap give its d_o and its four head gradients; bit for
    bit, in every precision mode (the modes share these kernels)."""
    import torch

    from rela_amd.learner import HipR2D2Learner
    from test_r2d2_learner_gpu import _agent, _random_batch

    A, B, seq, burn, n = shape
    rows = (seq + n) * B
    with torch.random.fork_rng(devices=[0]):
        torch.manual_seed(A * 1000 + B)
        agent = _agent(A, n, GAMMA, R.ETA, seq, burn, 71, 72, "cuda:0")
        batch, weight = _random_batch(np.random.default_rng(A * 1000 + B), A, B, seq, burn, n, "cuda:0")
    learner = HipR2D2Learner.from_agent(agent, B, grad_clip=1e9)
    learner.set_precision(mode)
    loss, prio, loss_seq = learner.backward(batch, weight)
    learner.check()
    torch.cuda.synchronize()
    q_on, q_tg, d_ha, o_tr, d_o = learner.debug_heads()
    assert q_on.shape == (rows, A) and o_tr.shape == (rows, 512)
    tr = lambda t, dt: t[burn:].to(dt).contiguous()
    dev = {"A": A, "batch": B, "seq": seq, "burn": burn, "n": n, "q_on": q_on, "q_tg": q_tg,
           "legal": tr(batch.obs["legal_move"], torch.float32), "act": tr(batch.action["a"], torch.int64),
           "reward": tr(batch.reward, torch.float32), "bootstrap": tr(batch.bootstrap, torch.float32),
           "seq_lens": batch.seq_len.float().contiguous(), "weight": weight.float().contiguous()}
    # gamma ** n as rela_r2d2_learner_create folds it: the float gamma raised in double, rounded to float
    gamma_n = float(np.float32(float(np.float32(GAMMA)) ** n))
    got, counts = run_loss(dev, 0.0, gamma_n=gamma_n, eta=agent.eta)
    assert counts == LOSS_CENSUS, counts
    assert float(d_ha.abs().max()) > 0 and float(prio.abs().max()) > 0
    for key, own in (("priority", prio), ("loss", loss), ("loss_seq", loss_seq), ("d_ha", d_ha)):
        assert torch.equal(bits(got[key]), bits(own)), key
    on, grads = learner.state_dict("online"), learner.state_dict("grads")
    head, counts = run_head({"A": A, "d_ha": d_ha, "o": o_tr, "fc_a_w": on["fc_a.weight"], "fc_v_w": on["fc_v.weight"]})
    assert counts == head_census(rows), counts
    own = {"d_o": d_o, "g_fc_a_w": grads["fc_a.weight"], "g_fc_a_b": grads["fc_a.bias"], "g_fc_v_w": grads["fc_v.weight"],
           "g_fc_v_b": grads["fc_v.bias"]}
    assert float(d_o.abs().max()) > 0
    for key in R.HEAD_KEYS:
        assert torch.equal(bits(head[key]), bits(own[key])), key
    learner.close()


# ---- d. bad arguments ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    import torch

    from rela_amd import _capi as capi
    from rela_amd.learner import HipR2D2Learner

    lib = capi.lib
    buf = [torch.zeros(4 * 512, device="cuda") for _ in range(15)]
    p = [C.c_void_p(b.data_ptr()) for b in buf]
    act = torch.zeros(64, dtype=torch.int64, device="cuda")
    p[3] = C.c_void_p(act.data_ptr())
    ones = torch.ones(4 * 512, device="cuda")
    p[6] = C.c_void_p(ones.data_ptr())  # seq_lens = 1

    def loss_args(batch=2, A=6, seq=1, burn=0, n=1, ptrs=p):
        return [batch, A, seq, burn, n] + list(ptrs[:8]) + [0.5, 0.0, 0.9] + list(ptrs[8:15]) + [None]

    assert lib.rela_debug_seq_loss_grad(*loss_args()) == capi.OK  # (the refusals below are refusals of their argument)
    for kw in ({"batch": 0}, {"batch": -1}, {"batch": 1025}, {"A": 0}, {"A": 32}, {"seq": 0}, {"burn": -1},
               {"seq": 2, "burn": 3}, {"n": 0}, {"seq": 2, "n": 3}, {"batch": 1024, "seq": 31, "n": 2}):
        assert lib.rela_debug_seq_loss_grad(*loss_args(**kw)) == capi.EINVAL, kw
    for hole in range(15):
        ptrs = list(p)
        ptrs[hole] = None
        assert lib.rela_debug_seq_loss_grad(*loss_args(ptrs=ptrs)) == capi.EINVAL, hole
    for out in range(8, 15):  # an output that is also an input, or another output
        for other in (0, 14 if out != 14 else 13):
            ptrs = list(p)
            ptrs[out] = ptrs[other]
            assert lib.rela_debug_seq_loss_grad(*loss_args(ptrs=ptrs)) == capi.EINVAL, (out, other)
    assert b"overlaps" in lib.rela_last_error()

    h = p[:3] + [p[4]] + p[8:13]  # nine float buffers: d_ha, o, fc_a_w, fc_v_w | d_o .. g_fc_v_b
    head_args = lambda rows=2, A=3, ptrs=h: [rows, A] + list(ptrs) + [None]
    assert lib.rela_debug_seq_head_backward(*head_args()) == capi.OK
    for kw in ({"rows": 0}, {"rows": -3}, {"rows": 32769}, {"A": 0}, {"A": 32}):
        assert lib.rela_debug_seq_head_backward(*head_args(**kw)) == capi.EINVAL, kw
    for hole in range(9):
        ptrs = list(h)
        ptrs[hole] = None
        assert lib.rela_debug_seq_head_backward(*head_args(ptrs=ptrs)) == capi.EINVAL, hole
    for out in range(4, 9):
        ptrs = list(h)
        ptrs[out] = ptrs[0]
        assert lib.rela_debug_seq_head_backward(*head_args(ptrs=ptrs)) == capi.EINVAL, out

    six = [C.c_void_p() for _ in range(5)]
    rows = C.c_int()
    refs = [C.byref(x) for x in six] + [C.byref(rows)]
    assert lib.rela_r2d2_learner_debug_heads(None, *refs) == capi.EINVAL
    learner = HipR2D2Learner(6, 4, 2, GAMMA, 7, 0, R.ETA)
    assert lib.rela_r2d2_learner_debug_heads(learner.h, None, *refs[1:]) == capi.EINVAL
    assert lib.rela_r2d2_learner_debug_heads(learner.h, *refs[:5], None) == capi.EINVAL
    assert lib.rela_r2d2_learner_debug_heads(learner.h, *refs) == capi.ESTATE  # no loss yet
    learner.close()
    torch.cuda.synchronize()
