"""The bounds of tests/test_r2d2_recurrent_paths_gpu.py can fail: float64 on the CPU, no GPU and none of the project's
kernels.  tests/f64_ref.py:r2d2_loss is evaluated with hooks that restate one defect of a recurrence kernel or of its
launch site each, at every case of tests/r2d2_paths.py, and the result must leave the bounds the GPU test asserts
around the unmodified reference in at least one output:

  1. not_zeroed      the state after a dummy burn-in is not zeroed (zero_hidden_where_terminal / the chains' `zero`)
  2. h_detached      the recurrent gradient term is dropped at one BPTT step (h detached between training steps 1 and 2)
  3. edge_row_state  the last batch row's forward runs from row B - 2's hidden state (a misaddressed edge row of the
                     recurrent GEMM), in the online net only
  4. edge_row_grad   with all weight on the last row, that row's gradient is dropped: a zero gradient
  5. dc_dropped      the cell gradient carried between steps (dc * f) is dropped

The conv trunk is not part of the recurrence: its float64 features are computed once per case and net and handed to
r2d2_loss through the "trunk" hook, so a mutation costs one LSTM unroll.  The conv gradients are then None and take no
part; the defects must show in the LSTM's and the heads' gradients, the losses or the priorities.

Final choice of shapes and seeds (tests/r2d2_paths.py: CASES): seq 3 / burn-in 2 / n 2 and, without burn-in, seq 4 /
n 2, seeds = the batch sizes: the first choice.  With them every mutation leaves the f32 bounds (gradients 2e-3 of the
tensor's largest entry, losses and priorities 2e-4) at every case it applies to -- the gradient-only ones, h_detached
and dc_dropped, by 17 to 220 times the bound in the LSTM's four tensors -- and, at B = 129, the bf16x2 gradient bound
(1e-2) as well; the figures are printed with -s.  No bound had to be tightened.  Mutation 1 does not apply to the case
without a burn-in."""
import pytest
import torch

import f64_ref
import r2d2_paths as P

_feats = {}


def _cached_trunk(name):
    def hook(net, p, frames, dtype):
        key = (name, net, frames.data_ptr(), frames.shape[0])  # (views of the case's one cached frame tensor)
        if key not in _feats:
            with torch.no_grad():
                _feats[key] = f64_ref.trunk({k: v.detach() for k, v in p.items()}, frames, dtype)
        return _feats[key]

    return hook


def _run(name, weight="batch", **hooks):
    hooks["trunk"] = _cached_trunk(name)
    return P.reference(name, weight, hooks)


def _mutations(name):
    A, B, seq, burn, n = P.shape(name)

    def h_detached(net, t, h, c):
        return (h.detach(), c) if net == "online" and t == burn + 2 else (h, c)

    def edge_row_state(net, t, h, c):
        return (torch.cat([h[:-1], h[B - 2:B - 1]]), c) if net == "online" else (h, c)

    def dc_dropped(net, t, h, c):
        return (h, c.detach()) if net == "online" and t > burn else (h, c)

    out = {"h_detached": ("batch", {"state": h_detached}), "edge_row_state": ("batch", {"state": edge_row_state}),
           "edge_row_grad": ("onehot", {"per_seq": lambda ps: torch.cat([ps[:-1], ps[-1:].detach()])}),
           "dc_dropped": ("batch", {"state": dc_dropped})}
    if burn > 0:  # (without a burn-in there is no state to zero and no zeroing launch)
        out["not_zeroed"] = ("batch", {"keep": torch.ones_like})
    return out


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_cases_have_a_padded_sequence_and_a_dummy_burn_in(name):
    P.check_case(name)


def test_hooks_leave_the_reference_alone():
    """identity hooks: bit for bit r2d2_loss without hooks; the cached trunk: the same losses, priorities and LSTM / head
    gradients, and no conv gradients"""
    name = "B5"
    plain = P.reference(name)
    ident = P.reference(name, "batch", {"state": lambda net, t, h, c: (h, c), "keep": lambda k: k,
                                        "per_seq": lambda ps: ps, "trunk": lambda net, p, s, dt: f64_ref.trunk(p, s, dt)})
    cached = _run(name)
    for key in ("loss", "priority", "loss_seq"):
        assert torch.equal(ident[key], plain[key]) and torch.equal(cached[key], plain[key]), key
    for key, g in plain["grads"].items():
        assert torch.equal(ident["grads"][key], g), key
        if key.startswith("net."):
            assert cached["grads"][key] is None, key
        else:
            assert torch.equal(cached["grads"][key], g), key


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_every_mutation_leaves_the_bounds(name):
    refs = {}
    for what, (weight, hooks) in sorted(_mutations(name).items()):
        if weight not in refs:
            refs[weight] = _run(name, weight)
            assert all(float(g.abs().max()) > 0 for g in refs[weight]["grads"].values() if g is not None)
        ref, bad = refs[weight], _run(name, weight, **hooks)
        assert P.beyond(ref, ref, P.GRAD_TOL["f32"]) == []
        out = P.beyond(bad, ref, P.GRAD_TOL["f32"])
        loose = P.beyond(bad, ref, P.GRAD_TOL["bf16x2"])
        print("%s %s: beyond the f32 bounds: %s; beyond the bf16x2 gradient bound: %s" % (
            name, what, ", ".join("%s %.3g > %.3g" % o for o in out), ", ".join(o[0] for o in loose)))
        assert out, "%s at %s stays inside every f32 bound" % (what, name)
        if name == "B129":  # (the case that also runs in bf16x2, with that mode's wider gradient bound)
            assert loose, "%s at %s stays inside every bf16x2 bound" % (what, name)
