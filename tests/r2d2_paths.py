"""Cases, batches, float64 references and bounds shared by tests/test_r2d2_recurrent_paths_gpu.py (the R2D2 learner's
two forms of the LSTM recurrence, csrc/learner_r2d2.hip) and tests/test_r2d2_recurrent_paths_ref_cpu.py (the proof, in
float64 on the CPU, that those bounds reject the defects the GPU test is there to find).

Which form runs (the R2D2 learner's table of paths):
    batch rows 1 .. 64      forward chains   BPTT chains
               65 .. 128    forward steps    BPTT chains (row tiles 4 .. 7)
               129 .. 1024  forward steps    BPTT steps
and RELA_R2D2_REC=steps at create: steps for both at any batch size.

Batches are built on the CPU from one seed per case (numpy's generator as _random_batch takes it, torch's for the
frames) and moved to the device, so both test files see the same data.  The seeds were chosen on the CPU so that every
case has a padded sequence and, where there is a burn-in, a dummy one (check_case asserts it)."""
from types import SimpleNamespace

import numpy as np
import torch

import f64_ref

GAMMA, ETA = 0.997, 0.9
ON_SEED, TG_SEED = 71, 72

# name -> (A, B, seq, burn, n, seed); T = burn + seq + n = 7 (6 without burn-in), seq + n BPTT steps
CASES = {
    "B5": (6, 5, 4, 0, 2, 5),       # M < 64: one partial GEMM tile; no burn-in, so no zeroing launch
    "B64": (18, 64, 3, 2, 2, 64),   # the largest batch of the forward chains, on both forms
    "B65": (18, 65, 3, 2, 2, 65),   # one row in tile 1 of TileRec and one row in BPTT chain 4
    "B128": (18, 128, 3, 2, 2, 128),  # all eight BPTT chains full
    "B129": (18, 129, 3, 2, 2, 129),  # the automatic switch of the BPTT: two full GEMM tiles plus one row
}

# Bounds: the project's own for the same quantities (tests/test_r2d2_learner_gpu.py: ..._matches_autograd,
# ..._matches_reference_golden_c4_shape)
SEQ_TOL = 2e-4                                            # loss per sequence, priorities: rtol = atol; loss: rtol
GRAD_TOL = {"f32": 2e-3, "f32x3": 2e-3, "bf16x2": 1e-2}   # max |error| <= tol x max |reference| per gradient tensor

_batches, _refs, _params = {}, {}, {}


def shape(name):
    A, B, seq, burn, n, _ = CASES[name]
    return A, B, seq, burn, n


def _to(x, device):
    if isinstance(x, dict):
        return {k: _to(v, device) for k, v in x.items()}
    return x.to(device)


def make_batch(A, B, seq, burn, n, seed, device="cpu"):
    """-> (batch, weight) on `device`: _random_batch on the CPU from the seed; the same values at every call"""
    from test_r2d2_learner_gpu import _random_batch

    key = (A, B, seq, burn, n, seed)
    if key not in _batches:
        torch.manual_seed(seed)
        _batches[key] = _random_batch(np.random.default_rng(seed), A, B, seq, burn, n, "cpu")
    b, w = _batches[key]
    batch = SimpleNamespace(**{k: _to(v, device) for k, v in vars(b).items()})
    return batch, w.to(device)


def case_batch(name, device="cpu"):
    return make_batch(*CASES[name], device)


def check_case(name):
    """the properties the seeds were chosen for"""
    A, B, seq, burn, n = shape(name)
    batch, _ = case_batch(name)
    lens = batch.seq_len.numpy()
    assert (lens < burn + seq).any(), "no padded sequence in %s" % name
    assert lens[B - 1] >= burn + 2
    if burn > 0:
        dummy = batch.terminal[burn - 1].numpy()
        assert dummy.any() and not dummy.all(), "no dummy burn-in in %s" % name


def one_hot_weight(B, device="cpu"):
    """all of the loss's weight on the last batch row: the row alone in its GEMM tile and its chain at B = 65, 129"""
    w = torch.zeros(B, dtype=torch.float32, device=device)
    w[B - 1] = 1.0
    return w


def case_agent(name, device):
    from test_r2d2_learner_gpu import _agent

    A, B, seq, burn, n = shape(name)
    return _agent(A, n, GAMMA, ETA, seq, burn, ON_SEED, TG_SEED, device)


def case_params(name):
    """-> (online, target) state dicts on the CPU (they depend on A only)"""
    A = CASES[name][0]
    if A not in _params:
        agent = case_agent(name, "cpu")
        sd = lambda net: {k: v.detach().cpu() for k, v in net.state_dict().items()}
        _params[A] = (sd(agent.online_net), sd(agent.target_net))
    return _params[A]


def as_result(loss, prio, loss_seq, grads):
    d = lambda t: torch.as_tensor(t).detach().cpu().double().reshape(-1)
    return {"loss": d(loss), "priority": d(prio), "loss_seq": d(loss_seq),
            "grads": {k: (None if g is None else g.detach().cpu().double()) for k, g in grads.items()}}


def reference(name, weight="batch", hooks=None):
    """float64 r2d2_loss of the case on the CPU, as as_result; weight: "batch" (the case's own) or "onehot".  Cached per
    (case, weight) when no hooks are given -- callers must not modify it."""
    key = (name, weight)
    if hooks is None and key in _refs:
        return _refs[key]
    A, B, seq, burn, n = shape(name)
    batch, w = case_batch(name)
    if weight == "onehot":
        w = one_hot_weight(B)
    on, tg = case_params(name)
    out = as_result(*f64_ref.r2d2_loss(on, tg, batch, w, GAMMA, n, ETA, seq, burn, torch.float64, hooks))
    if hooks is None:
        _refs[key] = out
    return out


def beyond(got, ref, grad_tol):
    """-> [(output, figure, bound)] of the outputs of `got` outside the bounds around `ref` (both as_result); gradient
    tensors that are None on either side are not compared"""
    bad = []
    for name in ("loss_seq", "priority"):
        d = (got[name] - ref[name]).abs()
        lim = SEQ_TOL + SEQ_TOL * ref[name].abs()
        if bool((d > lim).any()):
            i = int((d - lim).argmax())
            bad.append((name, float(d[i]), float(lim[i])))
    d, lim = float((got["loss"] - ref["loss"]).abs()[0]), SEQ_TOL * float(ref["loss"].abs()[0])
    if d > lim:
        bad.append(("loss", d, lim))
    for key, r in ref["grads"].items():
        g = got["grads"].get(key)
        if r is None or g is None:
            continue
        d, lim = float((g - r).abs().max()), grad_tol * float(r.abs().max())
        if not d <= lim:
            bad.append((key, d, lim))
    return bad


def figures(got, ref):
    """-> {output: (max |error|, mean |error|)} for loss, priorities, loss per sequence and {tensor: (max |error| /
    max |reference|, relative Frobenius error)} for the gradients, all against `ref`"""
    out = {k: f64_ref.err_stats(got[k], ref[k]) for k in ("loss", "priority", "loss_seq")}
    for key, r in ref["grads"].items():
        g = got["grads"].get(key)
        if r is not None and g is not None:
            out[key] = (float((g - r).abs().max()) / (float(r.abs().max()) + 1e-300), f64_ref.rel_fro(g, r))
    return out
