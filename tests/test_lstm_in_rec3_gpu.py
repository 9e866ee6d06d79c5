"""The R2D2 learner's lstm_in_rec3 option (csrc/gemm_rec3.h) through rela_debug_lstm_input_backward_opts against the float64
reference of the same call (tests/lstm_in_bwd_ref.py), and one learner step against tests/f64_ref.py:r2d2_loss.  dW_ih
always takes the kernel's large form (N = 3136: a half-filled column block), dW_hh the small one, d_a3 (M = rows) the
small one below 1,281 rows, i.e. in every case here: the large form's partial M block is the same template code but is not
reached.  The weight gradients contract over the rows: their tail chunk is zero-padded from `rows` to a multiple of 64."""
import ctypes as C

import pytest

import lstm_in_bwd_ref as R
from test_lstm_input_backward_gpu import exact_case, out_shapes, to_device

pytestmark = pytest.mark.gpu

CENSUS = {"gemm_rec3_nt": 3}


def tap(inp, mode, rec3):
    import torch
    from rela_amd import _capi as capi

    rows = inp["dg"].shape[0]
    out = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in out_shapes(rows).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with capi.launch_census() as census:  # (the outputs start as NaN)
        capi.check(capi.lib.rela_debug_lstm_input_backward_opts(
            rows, R.MODES[mode], rec3, *[ptr(inp[k]) for k in ("dg", "hprev", "a3", "w_ih")], *[ptr(out[k]) for k in R.KEYS],
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rela_debug_lstm_input_backward_opts")
    torch.cuda.synchronize()
    return out, census.counts


# a row count, or (small form?, d): the row tile of that form of gemm_rec3_nt (the kernel's constant, asked at run time) + d
ROWS = [1, 63, 64, 65] + [(small, d) for small in (1, 0) for d in (-1, 0, 1)] + [520, 1056]


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: "%s%+d" % (("BM", "SBM")[r[0]], r[1]) if isinstance(r, tuple) else str(r))
def test_exact_data_equals_the_reference(rows):
    """The stratified integer data of the mode-3 case (every part product carries bits).  exact_case asserts on the reference
    that every sum of absolute terms stays below 2^24 units: any summation order is exact and the outputs must EQUAL it."""
    import torch
    from rela_amd import _capi as capi

    rows = capi.lib.rela_debug_lstm_in_rec3_row_tile(rows[0]) + rows[1] if isinstance(rows, tuple) else rows
    for name in ("by_gate", "by_row"):
        inp, want = exact_case(name, rows)
        got, counts = tap(inp, "f32x3_bwd", 1)
        assert counts == CENSUS, (name, counts)
        for key, exp in want.items():
            assert torch.equal(got[key], exp), (rows, name, key, int((got[key] != exp).sum()))


@pytest.mark.parametrize("rows,gain", R.RANDOM_CASES)
def test_random_data_is_as_accurate_as_mode_0(rows, gain, record_property):
    """relative Frobenius error against float64: option on <= 1.5 x mode 0 (profiles/lstm_in_rec3_error_units.md)"""
    inp = to_device(R.random_inputs(rows, gain))
    ref, (f32, _), (on, counts) = R.reference(device="cuda", **inp), tap(inp, "f32", 0), tap(inp, "f32x3_bwd", 1)
    assert counts == CENSUS, counts
    fro = {k: (R.rel_fro(on[k], ref[k]), R.rel_fro(f32[k], ref[k])) for k in R.KEYS}
    for k, (e_on, e_f32) in fro.items():
        record_property("rel_fro_rec3_f32_ratio_%s" % k, (e_on, e_f32, e_on / max(e_f32, 1e-300)))
        print("rows %d gain %.1f %-7s rec3 %.4g  f32 %.4g  ratio %.3f" % (rows, gain, k, e_on, e_f32, e_on / max(e_f32, 1e-300)))
    assert all(e_on <= 1.5 * e_f32 for e_on, e_f32 in fro.values()), fro


@pytest.mark.parametrize("mode", ["f32", "bf16x2", "f32x3_bwd"])
def test_the_option_overrides_every_mode(mode):
    """three gemm_rec3_nt launches and no other counted one (gemm_lds, gemm_rec64_nt, gemm_bf16x3); off: the existing tap"""
    import torch
    inp, want = exact_case("two_part", 65)
    got, counts = tap(inp, mode, 1)
    assert counts == CENSUS, counts
    assert all(torch.equal(got[k], want[k]) for k in R.KEYS)
    _, off = tap(inp, mode, 0)
    assert "gemm_rec3_nt" not in off and sum(off.values()) == 3, off


def test_bad_arguments_are_refused():
    import torch
    from rela_amd import _capi as capi

    f = capi.lib.rela_debug_lstm_input_backward_opts
    inp = to_device(R.exact_inputs("two_part", 2))
    out = {k: torch.zeros(s, device="cuda") for k, s in out_shapes(2).items()}
    ptr = lambda t: C.c_void_p(t.data_ptr())
    good = [ptr(inp[k]) for k in ("dg", "hprev", "a3", "w_ih")] + [ptr(out[k]) for k in R.KEYS]
    for rows, mode, rec3 in ((2, 3, -1), (2, 3, 2), (0, 3, 1), (32769, 3, 1), (2, 4, 1), (2, -1, 1)):
        assert f(rows, mode, rec3, *good, None) == capi.EINVAL, (rows, mode, rec3)
    for hole in range(9):
        assert f(2, 3, 1, *(good[:hole] + [None] + good[hole + 1:]), None) == capi.EINVAL, hole
    for args in ([good[0]] * 9, good[:6] + [good[6], good[6], good[8]]):  # one pointer for everything; g_b_hh is g_b_ih
        assert f(2, 3, 1, *args, None) == capi.EINVAL
        assert b"overlaps" in capi.lib.rela_last_error()
    assert all(float(t.abs().max()) == 0 for t in out.values())  # nothing was launched
    assert capi.lib.rela_r2d2_learner_set_lstm_in_rec3(None, 1) == capi.EINVAL


def test_one_learner_step_with_the_option():
    """1,056 training rows, mode 3: every gradient tensor within 2e-3 of its largest entry of the float64 gradient; loss and
    priorities the option-off step's bits; the same bits twice; within the bound again after apply() (W_ih^T's records)"""
    import torch
    from f64_ref import r2d2_loss
    from test_r2d2_learner_bwd_mode_gpu import ABOVE_1024, ETA, GAMMA, _case, _learner

    (A, B, seq, burn, n), (agent, batch, weight) = ABOVE_1024, _case(ABOVE_1024)
    cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}

    def within_bound(learner):
        g64 = r2d2_loss(cpu(learner.state_dict("online")), cpu(agent.target_net.state_dict()), batch, weight, GAMMA, n, ETA,
                        seq, burn, torch.float64)[3]
        for k, g in learner.state_dict("grads").items():
            assert float((g.cpu().double() - g64[k]).abs().max()) <= 2e-3 * float(g64[k].abs().max()), k

    with torch.random.fork_rng(devices=[0]):
        learner = _learner(ABOVE_1024, "f32x3_bwd")
        off = [x.clone() for x in learner.backward(batch, weight)]
        learner.set_lstm_in_rec3(True)
        on = [x.clone() for x in learner.backward(batch, weight)]
        g_on = learner.flat()[1].clone()
        assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
        within_bound(learner)
        learner.flat()[1].zero_()
        learner.backward(batch, weight)
        assert torch.equal(learner.flat()[1], g_on)
        learner.apply()
        learner.backward(batch, weight)
        learner.check()
        within_bound(learner)
        learner.close()
