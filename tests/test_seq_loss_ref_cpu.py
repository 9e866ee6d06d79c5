"""tests/seq_loss_ref.py on the CPU: the float64 references of the R2D2 learner's sequence loss and head backward equal float64
autograd of a literal transcription of pyrela; the inputs of tests/test_seq_loss_gpu.py hold their roles at every shape it
runs (with the shapes that are too small for a role listed here); and float64 restatements of fifteen defects show which of
the GPU test's checks each one breaks -- and which it does not: two of them are invisible to every check and say so."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seq_loss_ref as R

CASE_IDS = ["B%d-seq%d-burn%d-n%d-A%d" % (*s, A) for s, A in R.LOSS_CASES]


# ---- the references equal float64 autograd -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,A", [(R.RAGGED, 6), ((5, 7, 0, 2), 18), ((1, 1, 0, 1), 1)])
def test_seq_reference_equals_float64_autograd(shape, A):
    """leaves a, v in float64, q_on = duel(v, a, legal) (net.py:93-99); td_err / loss / aggregate_priority transcribed
    literally (r2d2.py:103-206) with smooth_l1_loss; (loss * w).mean().backward() gives the reference's d_ha columns and dqa,
    and the same loss, loss_seq and priorities, to 1e-12.  eta = 0.875: the reference holds eta and 1 - eta as float32."""
    batch, seq, burn, n = shape
    eta = 0.875
    inp = dict(R.loss_args(R.loss_inputs(batch, A, seq, burn, n)))
    rows = (seq + n) * batch
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(seq + n, batch, A, dtype=torch.float64, generator=gen, requires_grad=True)
    v = torch.randn(seq + n, batch, 1, dtype=torch.float64, generator=gen, requires_grad=True)
    q_tg = torch.randn(seq + n, batch, A, dtype=torch.float64, generator=gen)
    t = lambda k, *sh: torch.from_numpy(np.asarray(inp[k], np.float64)).reshape(*sh)
    legal, reward, boot = t("legal", seq + n, batch, A), t("reward", seq + n, batch), t("bootstrap", seq + n, batch)
    lens, w = t("seq_lens", batch), t("weight", batch)
    act = torch.from_numpy(inp["act"].copy()).reshape(seq + n, batch)
    masked = a * legal
    q_on = v + masked - masked.mean(2, keepdim=True)                                   # net.py:93-99
    online_qa = q_on.gather(2, act.unsqueeze(2)).squeeze(2)                            # :157
    greedy = ((1 + q_on - q_on.min()) * legal).argmax(2).detach()                      # :160-162
    target_qa = q_tg.gather(2, greedy.unsqueeze(2)).squeeze(2)
    errs = []
    for i in range(seq):                                                               # r2d2.py:172-185
        target = reward[i] + boot[i] * (R.GAMMA_N * target_qa[i + n])
        should_padding = i >= (lens - burn)
        errs.append((target.detach() - online_qa[i]) * (1 - should_padding.double()))
    err = torch.stack(errs, 1)
    loss_seq = F.smooth_l1_loss(err, torch.zeros_like(err), reduction="none").sum(1)   # :199-204
    pr = err.detach().abs() * (torch.arange(seq).unsqueeze(0) < lens.unsqueeze(1)).double()  # :113-119
    priority = eta * pr.max(1)[0] + (1.0 - eta) * (pr.sum(1) / (lens - burn))
    loss = (loss_seq * w).mean()
    loss.backward()

    inp.update(q_on=q_on.detach().numpy().reshape(rows, A), q_tg=q_tg.numpy().reshape(rows, A))
    ref = R.seq_reference(eta=eta, **inp)
    assert np.array_equal(ref["greedy"], greedy.reshape(-1).numpy())
    close = lambda got, want: np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    close(ref["e"], err.detach().numpy().T)
    close(ref["loss_seq"], loss_seq.detach().numpy())
    close(ref["priority"], priority.numpy())
    close(ref["loss"], float(loss.detach()))
    close(ref["d_ha"][:, :A], a.grad.reshape(rows, A).numpy())
    close(ref["d_ha"][:, 31], v.grad.reshape(rows).numpy())
    close(ref["dqa"], v.grad.reshape(rows).numpy())
    assert not ref["d_ha"][:, A:31].any()
    assert float(a.grad.abs().max()) > 0 or A == 1  # (A = 1: a - mean(a) is zero whatever a is)


@pytest.mark.parametrize("rows,A", [(5, 18), (33, 1), (33, 31), (129, 6)])
def test_head_reference_equals_float64_autograd(rows, A):
    inp = R.head_random_inputs(rows, A)
    f = lambda k: torch.from_numpy(np.asarray(inp[k], np.float64))
    o, aw, vw = (f(k).requires_grad_() for k in ("o", "fc_a_w", "fc_v_w"))
    ab, vb = torch.zeros(A, dtype=torch.float64, requires_grad=True), torch.zeros(1, dtype=torch.float64, requires_grad=True)
    d = f("d_ha")
    ((F.linear(o, aw, ab) * d[:, :A]).sum() + (F.linear(o, vw, vb) * d[:, 31:]).sum()).backward()
    ref = R.head_reference(**inp)
    for key, t in (("d_o", o), ("g_fc_a_w", aw), ("g_fc_a_b", ab), ("g_fc_v_w", vw), ("g_fc_v_b", vb)):
        want = t.grad.reshape(ref[key].shape)
        assert float((ref[key] - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30), key


# ---- the inputs hold their roles -------------------------------------------------------------------------------------------------
ALL_ROLES = set(R.ROW_ROLES) | set(R.SEQ_ROLES) | {"padded", "deep", "q_tg_below_min"}
# the shapes that are too small for a role.  deep needs a live row that starts beyond flat element 1024; A = 1 has no
# second action to tie with, to be illegal or to hide q_tg's low value in.
TOO_SMALL = {
    ((1, 1, 0, 1), 18): ALL_ROLES - {"dyadic_plus1", "full", "padded", "q_tg_below_min"},  # one sequence, one live row
    ((5, 7, 0, 2), 18): {"big_weight", "deep"},  # five sequences; 45 rows x 18 = 810 elements
    (R.RAGGED, 1): {"deep", "tie", "illegal_best", "q_tg_below_min"},
}


@pytest.mark.parametrize("shape,A", R.LOSS_CASES, ids=CASE_IDS)
def test_loss_inputs_hold_every_role(shape, A):
    inp = R.loss_inputs(shape[0], A, *shape[1:])
    R.check_loss_inputs(inp)
    assert ALL_ROLES - R.roles_present(inp) == TOO_SMALL.get((shape, A), set())


# the other places of the global minimum, at the shapes whose table has those elements (tests/test_seq_loss_gpu.py)
MIN_CASES = [(s, A, at) for s, A in R.LOSS_CASES if (s[1] + s[3]) * s[0] * A > 1025 for at in ("i1023", "i1024")]


@pytest.mark.parametrize("shape,A,min_at", MIN_CASES)
def test_loss_inputs_with_the_minimum_at_element_1023_and_1024(shape, A, min_at):
    R.check_loss_inputs(R.loss_inputs(shape[0], A, *shape[1:], min_at=min_at), min_at)


# ---- discrimination ----------------------------------------------------------------------------------------------------------------
def applies(defect, shape, A, inp):
    """does the restated defect change anything at this shape?  (Where it does, a check MUST catch it.)"""
    batch, seq, burn, n = shape
    short = bool((inp["seq_lens"] - burn < seq).any())  # a padded step inside the first seq steps
    return {
        "pad_mask_gt": short, "pad_mask_seq_len": short and burn > 0, "target_row_n_minus_1": True,
        "mean_over_seq_len": burn > 0,
        # INVISIBLE, by construction of the agent: should_padding already zeroes e where i >= seq_len_b - burn_in, and the
        # priority mask i < seq_len_b holds wherever e is not zero.  No data can show it; it is listed so that this is said.
        "priority_mask_dropped": False,
        "min_first_1024": "deep" in R.roles_present(inp), "min_with_q_tg": A >= 2, "last_max": A >= 2,
        "argmax_ignores_legal": A >= 2, "one_over_num_legal": A >= 2, "value_in_column_A": A < 31,
        "loss_mean_over_1024": batch != 1024,
        # NOT CAUGHT: float32(1) - float32(0.9) is 4 u above float32(0.1), on the (1 - eta) * mean part, a tenth of the
        # priority: 0.4 u of it against a bound of seq + 4 roundings (profiles/seq_loss_head_backward_error_units.md)
        "one_minus_eta_f32": False,
    }[defect]


@pytest.mark.parametrize("shape,A", R.LOSS_CASES, ids=CASE_IDS)
def test_restated_defects_break_a_check(shape, A, record_property):
    inp = R.loss_inputs(shape[0], A, *shape[1:])
    ref = R.check_loss_inputs(inp)
    clean = R.loss_margins(inp, ref, None)
    assert R.caught(clean) == [], clean
    for defect in R.DEFECTS:
        m = R.loss_margins(inp, ref, defect)
        record_property(defect, {k: (v if isinstance(v, bool) else float("%.3g" % v)) for k, v in m.items()})
        assert bool(R.caught(m)) == applies(defect, shape, A, inp), (defect, m)


def test_a_single_missed_element_cannot_move_the_greedy_rule():
    """Why the minimum's place is tested through a `deep` row and not through the minimum alone: a q.min() that misses ONE
    element returns the next smallest, 1 + q - min stays >= 1 on every legal action and the argmax is what it was.  Only a
    minimum that misses a REGION holding both the minimum and a row more than 1 below everything outside it changes sign
    there -- which is what `deep` builds beyond element 1024."""
    inp = R.loss_inputs(*R.RAGGED[:1], 18, *R.RAGGED[1:])
    q = inp["q_on"].copy()
    q.reshape(-1)[-1] = q.reshape(-1)[:-1].min()  # the table a kernel sees that skips the last element
    assert np.array_equal(R.greedy_f32(q, inp["q_tg"], inp["legal"]), R.greedy_f32(inp["q_on"], inp["q_tg"], inp["legal"]))
    assert R.caught(R.loss_margins(inp, R.check_loss_inputs(inp), "min_first_1024")) != []


@pytest.mark.parametrize("rows,A", R.HEAD_CASES)
def test_head_exact_data_and_its_defects(rows, A):
    """the preconditions of the exact data sets (whole units below 2^24; `rows`: distinct powers of two behind every element
    of a weight gradient), and the two restated weight-gradient defects change the float32 result on `rows`"""
    for name in R.HEAD_DATA_SETS:
        inp = R.head_exact_inputs(name, rows, A)
        ref, ab = R.head_reference(**inp), R.head_reference_abs(**inp)
        R.head_exact_preconditions(name, inp, ref, ab)
    defects = ["wgrad_missing_last_row"] + (["wgrad_missing_slice"] if rows >= R.SPLIT_ROWS else [])
    for defect in defects:
        bad = R.head_reference(defect=defect, **R.head_exact_inputs("rows", rows, A))
        good = R.head_reference(**R.head_exact_inputs("rows", rows, A))
        differs = [k for k in R.HEAD_KEYS if not torch.equal(bad[k].float(), good[k].float())]
        assert differs and set(differs) <= {"g_fc_a_w", "g_fc_v_w"}, (defect, differs)


def test_head_defects_exceed_the_random_data_bound():
    """on random data a missing row or slice is far outside the n_terms bound of the weight gradient it belongs to"""
    rows, A = 1025, 18
    inp = R.head_random_inputs(rows, A)
    ref, ab = R.head_reference(**inp), R.head_reference_abs(**inp)
    for defect in ("wgrad_missing_last_row", "wgrad_missing_slice"):
        bad = R.head_reference(defect=defect, **inp)
        worst = max(R.err_units(bad[k].float(), ref[k], ab[k], R.U_F32) / R.head_n_terms(k, rows, A) for k in ("g_fc_a_w", "g_fc_v_w"))
        assert worst > 1.0, (defect, worst)


@pytest.mark.parametrize("shape,A", R.LOSS_CASES, ids=CASE_IDS)
def test_the_float32_restatement_stays_within_every_derived_bound(shape, A, record_property):
    """R.e_f32 + R.td_loss_f32 (numpy float32 in the kernels' operation order -- what tests/test_seq_loss_gpu.py asks the
    kernels' bits to be) against the float64 reference: a correct float32 evaluation passes every bound derived in
    tests/seq_loss_ref.py, on the CPU, before a kernel is involved."""
    inp = R.loss_inputs(shape[0], A, *shape[1:])
    ref = R.check_loss_inputs(inp)
    seq, burn = shape[1], shape[2]
    e32 = R.e_f32(inp, ref["greedy"], 0.0)
    f32 = R.td_loss_f32(inp, e32)
    after = R.seq_reference(e=e32, **R.loss_args(inp))
    tiny = 1e-300
    units = {"e": np.abs(e32 - ref["e"]) / np.maximum(R.e_bound(ref), tiny),
             "dqa": np.abs(f32["dqa"] - after["dqa"]) / np.maximum(R.dqa_bound(after), tiny),
             "d_ha": np.abs(f32["d_ha"] - after["d_ha"])[:, :A] / np.maximum(R.d_ha_bound(after), tiny),
             "loss_seq": np.abs(f32["loss_seq"] - after["loss_seq"]) / np.maximum(R._k(R.loss_seq_roundings(seq)) * after["loss_seq"], tiny),
             "priority": np.abs(f32["priority"] - after["priority"]) / np.maximum(R._k(R.priority_roundings(seq)) * after["priority"], tiny),
             "loss": np.abs(f32["loss"][0] - after["loss"]) / max(R._k(R.loss_roundings(seq)) * after["loss"], tiny)}
    one = np.flatnonzero(inp["seq_lens"] == burn + 1)
    if one.size:
        a0 = np.abs(e32[0, one].astype(np.float64))
        units["one_step_priority"] = np.abs(f32["priority"][one] - a0) / np.maximum(R.ONE_STEP_PRIORITY_UNITS * R.U_F32 * a0, tiny)
    for k, v in units.items():
        record_property("units_%s" % k, float(np.max(v)))
        assert float(np.max(v)) <= 1.0, (k, float(np.max(v)))
    assert not f32["d_ha"][:, A:31].any() and not f32["d_ha"][:, :A][inp["legal"] == 0].any()
