"""The R2D2 learner's LSTM recurrence in both of its forms (csrc/learner_r2d2.hip) against float64.

The recurrence of a learner step runs as persistent chains (lstm_rec_chain, lstm_bptt_chain: one launch for all T
steps) or as per-step launches (zero_hidden_where_terminal, the split-K TileRec GEMMs on ProbRecFwd / ProbRecBwd,
lstm_cell_fwd / lstm_cell_bwd); which one depends on the batch size and on RELA_R2D2_REC at create
(tests/r2d2_paths.py has the table).  Every case names the form that must have run and asserts it from the launch
census, launch counts included, and that the other form's kernels are absent.

Reference: tests/f64_ref.py:r2d2_loss in float64 on the CPU, cached per (case, weight vector).  Bounds: the project's
own for the same quantities (r2d2_paths.SEQ_TOL, GRAD_TOL); tests/test_r2d2_recurrent_paths_ref_cpu.py shows that they
reject a state that is not zeroed, a dropped recurrent term, a misaddressed or dropped edge row and a dropped cell
gradient at these shapes.  The same error figures are computed for pyrela's f32 autograd on the GPU; both columns are
printed (-s) and recorded as properties: profiles/r2d2_recurrent_paths_error.md.

Measured on the MI355X: every figure of the f32 and f32x3 runs <= 1.0e-6 (pyrela f32: 9.2e-7), the largest bf16x2 figure
5.0e-4 against its bound of 1e-2; chains against steps at B = 64 differ by at most 3.5e-7."""
import pytest

from kernel_names import (R2D2_BPTT_CHAIN, R2D2_BPTT_STEPS, R2D2_REC_CHAIN, R2D2_REC_STEPS, R2D2_REC_ZERO)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_pyrela = {}


def _expected(B, forced_steps):
    """-> (forward, BPTT) form of a batch of B rows"""
    if forced_steps:
        return "steps", "steps"
    return ("chain" if B <= 64 else "steps"), ("chain" if B <= 128 else "steps")


def _assert_paths(counts, seq, burn, n, fwd, bptt):
    T, Tt, ran = burn + seq + n, seq + n, set(counts)
    if fwd == "chain":
        assert counts.get("lstm_rec_chain") == 1 and not ((R2D2_REC_STEPS | {R2D2_REC_ZERO}) & ran), counts
    else:
        assert not (R2D2_REC_CHAIN & ran), counts
        for k in R2D2_REC_STEPS:  # both nets, every step
            assert counts.get(k) == 2 * T, (k, counts)
        assert counts.get(R2D2_REC_ZERO, 0) == (2 if burn > 0 else 0), counts
    if bptt == "chain":
        assert counts.get("lstm_bptt_chain") == 1 and not (R2D2_BPTT_STEPS & ran), counts
    else:
        assert not (R2D2_BPTT_CHAIN & ran), counts
        assert counts.get("lstm_cell_bwd") == Tt and counts.get("gemm_lds<TileRec, ProbRecBwd>") == Tt - 1, counts


def _make_learner(agent, max_batch, precision, monkeypatch, forced_steps):
    """RELA_R2D2_REC is read by rela_r2d2_learner_create: set (or cleared) before the learner exists"""
    from rela_amd.learner import HipR2D2Learner

    if forced_steps:
        monkeypatch.setenv("RELA_R2D2_REC", "steps")
    else:
        monkeypatch.delenv("RELA_R2D2_REC", raising=False)
    learner = HipR2D2Learner.from_agent(agent, max_batch, grad_clip=1e9)
    monkeypatch.delenv("RELA_R2D2_REC", raising=False)
    learner.set_precision(precision)
    return learner


def _step(learner, batch, weight, shape, precision, paths):
    """one backward under the census -> as_result; asserts check(), the path and the precision census"""
    import torch

    import r2d2_paths as P
    from rela_amd import _capi as capi
    from test_r2d2_learner_gpu import _assert_r2d2_census

    A, B, seq, burn, n = shape
    with capi.launch_census() as census:
        loss, prio, loss_seq = learner.backward(batch, weight)
    learner.check()
    torch.cuda.synchronize()
    _assert_paths(census.counts, seq, burn, n, *paths)
    # (bf16x2: the online trunk takes the split-bf16 kernels from 128 frames, csrc/learner_r2d2.hip forward_pre; the
    # kernel set _assert_r2d2_census asks for holds from there on)
    if precision != "bf16x2" or (burn + seq + n) * B >= 128:
        _assert_r2d2_census(census.counts, precision, (burn + seq + n) * B)
    return P.as_result(loss, prio, loss_seq, learner.state_dict("grads"))


def _pyrela_f32(name, kind, agent, batch, weight):
    """pyrela's f32 autograd on the GPU (agent.loss + backward), as as_result; once per (case, weight vector)"""
    import torch

    import r2d2_paths as P

    if (name, kind) not in _pyrela:
        torch.backends.cudnn.allow_tf32 = False
        torch.backends.cuda.matmul.allow_tf32 = False
        agent.online_net.zero_grad()
        per_seq, prio = agent.loss(batch, sync_priority=False)
        loss = (per_seq * weight).mean()
        loss.backward()
        _pyrela[(name, kind)] = P.as_result(loss.reshape(1), prio, per_seq,
                                            {k: p.grad.clone() for k, p in agent.online_net.named_parameters()})
    return _pyrela[(name, kind)]


def _report(record_property, tag, got, torch_f32, ref):
    """both columns of profiles/r2d2_recurrent_paths_error.md, per output (losses and priorities: max / mean |error|;
    gradients: max |error| / max |reference| and the relative Frobenius error)"""
    import r2d2_paths as P

    hip, py = P.figures(got, ref), P.figures(torch_f32, ref)
    for key in hip:
        record_property("%s %s hip" % (tag, key), hip[key])
        record_property("%s %s pyrela_f32" % (tag, key), py[key])
        print("R2D2PATHS| %s | %s | %.3g | %.3g | %.3g | %.3g |" % (tag, key, *hip[key], *py[key]))


RUNS = [("B5", "f32", True), ("B64", "f32", True), ("B65", "f32", False), ("B128", "f32", False),
        ("B129", "f32", False), ("B129", "f32x3", False), ("B129", "bf16x2", False)]


@pytest.mark.parametrize("name,precision,forced_steps", RUNS, ids=["%s-%s" % r[:2] for r in RUNS])
def test_recurrent_path_matches_f64(name, precision, forced_steps, monkeypatch, record_property):
    """Loss, priorities, loss per sequence and every gradient tensor of one step on the form of the recurrence the case
    names, within the project's bounds of float64.
      B5    (A = 6, no burn-in) forced steps: M < 64, one partial GEMM tile, no zeroing launch
      B64   forced steps, and the same batch on the chains (a learner created without the variable shows the chains
            again); both within the bounds; the largest chain-vs-steps difference per output is recorded
      B65   steps / chains: one row in tile 1 of TileRec and one row in BPTT chain 4
      B128  steps / chains: all eight BPTT chains full
      B129  steps / steps by itself; two full GEMM tiles plus one row; f32x3 and bf16x2 too: 903 frames, so their
            kernels engage and dW_hh, dW_ih and d_a3 consume what the per-step BPTT left in gxs[0]
    At B = 65 and B = 129 a second backward puts all weight on the last row, which sits alone in its tile and chain: a
    dropped or misaddressed edge row shows as a zero or foreign gradient."""
    import r2d2_paths as P

    shape = P.shape(name)
    A, B, seq, burn, n = shape
    P.check_case(name)
    agent = P.case_agent(name, DEV)
    batch, weight = P.case_batch(name, DEV)
    paths = _expected(B, forced_steps)
    assert paths == {"B5": ("steps", "steps"), "B64": ("steps", "steps"), "B65": ("steps", "chain"),
                     "B128": ("steps", "chain"), "B129": ("steps", "steps")}[name]
    tol = P.GRAD_TOL[precision]
    learner = _make_learner(agent, B, precision, monkeypatch, forced_steps)
    got = _step(learner, batch, weight, shape, precision, paths)
    ref = P.reference(name)
    _report(record_property, "%s %s %s/%s" % (name, precision, *paths), got, _pyrela_f32(name, "batch", agent, batch, weight), ref)
    assert P.beyond(got, ref, tol) == []
    if B in (65, 129):
        w1 = P.one_hot_weight(B, DEV)
        got1, ref1 = _step(learner, batch, w1, shape, precision, paths), P.reference(name, "onehot")
        assert all(float(g.abs().max()) > 0 for g in ref1["grads"].values())
        _report(record_property, "%s %s %s/%s last row only" % (name, precision, *paths), got1,
                _pyrela_f32(name, "onehot", agent, batch, w1), ref1)
        assert P.beyond(got1, ref1, tol) == []
    learner.close()
    if name == "B64":
        chains = _make_learner(agent, B, precision, monkeypatch, False)
        got_c = _step(chains, batch, weight, shape, precision, ("chain", "chain"))
        chains.close()
        _report(record_property, "%s %s chain/chain" % (name, precision), got_c,
                _pyrela_f32(name, "batch", agent, batch, weight), ref)
        assert P.beyond(got_c, ref, tol) == []
        for key, (mx, fro) in P.figures(got_c, got).items():
            record_property("B64 chains vs steps " + key, (mx, fro))
            print("R2D2PATHS-CS| %s | %.3g | %.3g |" % (key, mx, fro))


@pytest.mark.parametrize("precision", ["f32", "f32x3", "bf16x2"])
def test_one_learner_several_batch_sizes(precision, monkeypatch):
    """One learner with max_batch = 129 differentiates B = 129, 65, 5, 65, 129 (the same B is the same batch): the
    census of every call shows the form of its B (steps / steps, steps / chains, chains / chains), check() passes, and
    loss, priorities, loss per sequence and the flat gradient equal, bit for bit, those of a fresh learner created with
    max_batch == B and those of the other visit of the same B: the buffers are sized by max_batch, every stride uses
    the batch, and nothing a call leaves behind reaches the next."""
    import torch

    import r2d2_paths as P

    A, seq, burn, n = 18, 3, 2, 2
    agent = P.case_agent("B129", DEV)
    data = {B: P.make_batch(A, B, seq, burn, n, B, DEV) for B in (129, 65, 5)}

    def run(learner, B):
        batch, weight = data[B]
        out = _step(learner, batch, weight, (A, B, seq, burn, n), precision, _expected(B, False))
        return out, learner.flat()[1].clone()

    fresh = {}
    for B in data:
        lr = _make_learner(agent, B, precision, monkeypatch, False)
        fresh[B] = run(lr, B)
        lr.close()
    learner = _make_learner(agent, 129, precision, monkeypatch, False)
    seen = {}
    for visit, B in enumerate((129, 65, 5, 65, 129)):
        out, flat = run(learner, B)
        for what, (o, f) in (("a fresh learner", fresh[B]), ("the earlier visit", seen.get(B, fresh[B]))):
            for key in ("loss", "priority", "loss_seq"):
                assert torch.equal(out[key], o[key]), "call %d (B = %d): %s differs from %s" % (visit, B, key, what)
            assert torch.equal(flat, f), "call %d (B = %d): gradients differ from %s" % (visit, B, what)
        seen[B] = (out, flat)
    learner.close()
