"""The R2D2 learner's fourth precision mode, "f32x3_bwd" (rela_r2d2_learner_set_precision(l, 3), csrc/learner_r2d2.hip).

Mode 3 is mode 2 ("f32x3": both trunks and the x part of the gate GEMM on three-part bf16 operands) plus the large backward
GEMMs over all training rows at once on gemm_bf16x3 with three-part operands (csrc/gemm_bf16x3.h, PARTS = 3), with the
Problem functors they have in mode 0:

  dW_hh (ProbWhh), dW_ih (ProbWih), the input-side data gradient with its ReLU mask (ProbIhDgrad) and the conv1 / conv2 /
  conv3 weight gradients (trunk_backward with emu, one lane, twice the split-K slices):  MOVED_GEMMS = 6 launches.
  The heads' data and weight gradients (K = 32, M = 32) were measured slower in three parts and stay on gemm_lds (f32).

Shapes (A, B, seq, burn, n):
  (6, 5, 7, 0, 2)      45 frames, 45 training rows: K = one chunk of 32 rows and a tail of 13, M below one 128-row tile;
                       the forwards stay on the f32 kernels (fewer than 512 frames)
  (18, 33, 12, 6, 3)   693 frames, 495 training rows: ragged, the three-part forwards run too
  (6, 130, 3, 1, 1)    650 frames, 520 training rows: B > 128 takes the per-step recurrence
  (6, 33, 30, 0, 2)    1,056 frames, 1,056 training rows: above 1,024, where conv2's / conv3's weight gradients run at twice
                       mode 0's split-K slices (54 / 56: kX6SplitMul, csrc/learner_plan.h)

Modes 0, 1 and 2 must not move a bit: sha256 of the flat gradient buffer, the loss and the priorities of the first two
shapes are compared with tests/golden/r2d2_learner_parent_bits.json, recorded on an MI355X with this file's `compute()`
from a checkout of the commit named in it (the parent of mode 3), together with mode 2's launch census at 693 frames.

Re-recording (only ever from the commit BEFORE a change to the kernels):
    python tests/test_r2d2_learner_bwd_mode_gpu.py OUT.json COMMIT
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "r2d2_learner_parent_bits.json")

SMALL, RAGGED, PER_STEP, ABOVE_1024 = (6, 5, 7, 0, 2), (18, 33, 12, 6, 3), (6, 130, 3, 1, 1), (6, 33, 30, 0, 2)
SHAPES = [SMALL, RAGGED, PER_STEP, ABOVE_1024]
PARENT_SHAPES = [RAGGED, SMALL]
PARENT_MODES = ("f32", "bf16x2", "f32x3")
# the GEMM launches that leave "gemm_lds (f32)" for "gemm_bf16x3" between mode 2 and mode 3 (DESIGN 4.7 has the table)
MOVED_GEMMS = 6
X3_GRAD_SLACK = 1.5  # the project's constant (tests/trunk_bwd_ref.py, tests/test_r2d2_learner_gpu.py)
GAMMA, ETA = 0.997, 0.9


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """Tests elsewhere draw their frames from the device generator without a seed: this file's draws, its net
    initialisations and the entry point's manual_seed must not move what they see."""
    import torch

    with torch.random.fork_rng(devices=[0]):
        yield


def _frames(shape):
    A, B, seq, burn, n = shape
    return (burn + seq + n) * B


@functools.lru_cache(maxsize=None)
def _case(shape):
    """-> (agent, batch, weight) of a shape, as test_hip_r2d2_learner_matches_autograd builds them; shared, never changed"""
    import torch
    from test_r2d2_learner_gpu import _agent, _random_batch

    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    A, B, seq, burn, n = shape
    rng = np.random.default_rng(A * 1000 + B)
    agent = _agent(A, n, GAMMA, ETA, seq, burn, 71, 72, "cuda:0")
    with torch.random.fork_rng(devices=[0]):  # (_random_batch draws the frames on the device: the recorded bits need a seed)
        torch.manual_seed(A * 1000 + B)
        batch, weight = _random_batch(rng, A, B, seq, burn, n, "cuda:0")
    return agent, batch, weight


def _learner(shape, mode=None):
    from rela_amd.learner import HipR2D2Learner

    learner = HipR2D2Learner.from_agent(_case(shape)[0], shape[1], grad_clip=1e9)
    if mode is not None:
        learner.set_precision(mode)
    return learner


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def step_bits(shape, mode):
    """-> ({output: sha256}, launch census) of one backward() of a fresh learner in `mode`"""
    import torch
    from rela_amd import _capi as capi

    _, batch, weight = _case(shape)
    learner = _learner(shape, mode)
    with capi.launch_census() as census:
        loss, prio, _ = learner.backward(batch, weight)
    learner.check()
    torch.cuda.synchronize()
    out = {"grads": _sha(learner.flat()[1]), "loss": _sha(loss), "priority": _sha(prio)}
    learner.close()
    return out, dict(census.counts)


def _key(shape, mode):
    return "A%d_B%d_seq%d_burn%d_n%d_%s" % (*shape, mode)


def compute():
    out = {}
    for shape in PARENT_SHAPES:
        for mode in PARENT_MODES:
            out[_key(shape, mode)] = step_bits(shape, mode)[0]
    return out


@functools.lru_cache(maxsize=1)
def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


# ---- the mode exists ---------------------------------------------------------------------------------------------------
def test_mode_3_is_accepted_and_4_is_refused():
    """rela_r2d2_learner_set_precision takes 3 and still refuses 4 with RELA_EINVAL and a message that names the range;
    HipR2D2Learner.set_precision("f32x3_bwd") selects it, HipApexLearner refuses the name with ValueError."""
    from rela_amd import _capi as capi
    from rela_amd.learner import HipApexLearner, HipR2D2Learner

    learner = HipR2D2Learner(6, 4, 2, GAMMA, 7, 0, ETA)
    assert capi.lib.rela_r2d2_learner_set_precision(learner.h, 3) == capi.OK
    assert capi.lib.rela_r2d2_learner_set_precision(learner.h, 4) == capi.EINVAL
    assert b"0, 1, 2 or 3" in capi.lib.rela_last_error()
    assert capi.lib.rela_r2d2_learner_set_precision(learner.h, -1) == capi.EINVAL
    learner.set_precision("f32")
    learner.set_precision("f32x3_bwd")
    with pytest.raises(ValueError):
        learner.set_precision("f32x4")
    learner.close()
    apex = HipApexLearner(6, 4, 2, GAMMA)
    with pytest.raises(ValueError):
        apex.set_precision("f32x3_bwd")
    apex.set_precision("f32x3")
    apex.close()


# ---- against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["A%d-B%d-seq%d-burn%d-n%d" % s for s in SHAPES])
def test_mode_3_matches_autograd(shape):
    """The step and the tolerances of test_hip_r2d2_learner_matches_autograd in mode 3: loss, per-sequence loss and
    priorities to rtol = atol = 2e-4, every gradient tensor within 2e-3 of its largest reference entry, check() clean; the
    census shows gemm_bf16x3, the three-part forwards from 512 frames and the per-step recurrence at B = 130."""
    import torch
    from kernel_names import R2D2_BPTT_CHAIN, R2D2_BPTT_STEPS, SPLIT_BF16, X3_LSTM
    from rela_amd import _capi as capi

    agent, batch, weight = _case(shape)
    learner = _learner(shape, "f32x3_bwd")
    with capi.launch_census() as census:
        loss, prio, loss_seq = learner.backward(batch, weight)
    learner.check()
    torch.cuda.synchronize()
    ran = set(census.counts)
    assert census.counts.get("gemm_bf16x3", 0) >= MOVED_GEMMS and not (SPLIT_BF16 & ran), census.counts
    assert (X3_LSTM <= ran) == (_frames(shape) >= 512), sorted(ran)
    assert (R2D2_BPTT_STEPS <= ran) == (shape[1] > 128) and (R2D2_BPTT_CHAIN <= ran) == (shape[1] <= 128), sorted(ran)
    agent.online_net.zero_grad()
    ref_loss, ref_prio = agent.loss(batch, sync_priority=False)
    (ref_loss * weight).mean().backward()
    np.testing.assert_allclose(loss_seq.cpu().numpy(), ref_loss.detach().cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(prio.cpu().numpy(), ref_prio.cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(float(loss.cpu()[0]), float((ref_loss * weight).mean().detach()), rtol=2e-4)
    grads = learner.state_dict("grads")
    for key, p in agent.online_net.named_parameters():
        ref = p.grad.detach()
        scale = float(ref.abs().max()) + 1e-12
        err = float((grads[key] - ref).abs().max())
        print(key, "max |err| / max |ref| = %.3g" % (err / scale))
        assert err <= 2e-3 * scale, (key, err, scale)
    agent.online_net.zero_grad()
    learner.close()


# ---- the forward of mode 2, the census ------------------------------------------------------------------------------------
def test_mode_3_has_mode_2s_forward_and_moves_six_gemms():
    """693 frames: loss, per-sequence loss and priorities of mode 3 are the bits of mode 2; from mode 2 to mode 3 the
    count of "gemm_lds (f32)" falls by MOVED_GEMMS, the count of "gemm_bf16x3" rises by as many, and every other kernel is
    launched as often as before; mode 2's own census is the one recorded from the parent commit."""
    import torch
    from rela_amd import _capi as capi

    _, batch, weight = _case(RAGGED)
    learner = _learner(RAGGED)
    res, counts = {}, {}
    for mode in ("f32x3", "f32x3_bwd"):
        learner.set_precision(mode)
        with capi.launch_census() as census:
            out = learner.backward(batch, weight)
        learner.check()
        torch.cuda.synchronize()
        res[mode] = [x.clone() for x in out]
        counts[mode] = dict(census.counts)
    learner.close()
    for a, b, name in zip(res["f32x3"], res["f32x3_bwd"], ("loss", "priority", "loss_seq")):
        assert torch.equal(a, b), name
    c2, c3 = counts["f32x3"], counts["f32x3_bwd"]
    print("mode 2:", c2, "\nmode 3:", c3)
    assert c2 == _golden()["census_f32x3_693_frames"], c2
    assert c2["gemm_lds (f32)"] - c3["gemm_lds (f32)"] == MOVED_GEMMS
    assert c3.get("gemm_bf16x3", 0) - c2.get("gemm_bf16x3", 0) == MOVED_GEMMS
    rest = lambda c: {k: v for k, v in c.items() if k not in ("gemm_lds (f32)", "gemm_bf16x3")}
    assert rest(c2) == rest(c3)


# ---- f32 accuracy -----------------------------------------------------------------------------------------------------
def test_mode_3_gradients_are_f32_accurate(record_property):
    """693 frames against tests/f64_ref.py:r2d2_loss in float64: per gradient tensor the relative Frobenius error of mode 3
    is at most X3_GRAD_SLACK x that of mode 0, both measured here; every ratio is recorded."""
    import torch
    from f64_ref import r2d2_loss, rel_fro
    from rela_amd.learner import HipR2D2Learner

    A, B, seq, burn, n = RAGGED
    agent, batch, weight = _case(RAGGED)
    sd = lambda net: {k: v.detach().cpu() for k, v in net.state_dict().items()}
    _, _, _, g64 = r2d2_loss(sd(agent.online_net), sd(agent.target_net), batch, weight, GAMMA, n, ETA, seq, burn, torch.float64)
    learner = _learner(RAGGED)
    gerr = {}
    for mode in ("f32", "f32x3_bwd"):
        learner.set_precision(mode)
        learner.backward(batch, weight)
        learner.check()
        grads = learner.state_dict("grads")
        gerr[mode] = {k: rel_fro(grads[k], g64[k]) for k in HipR2D2Learner.KEYS}
    learner.close()
    for k in HipR2D2Learner.KEYS:
        ratio = gerr["f32x3_bwd"][k] / max(gerr["f32"][k], 1e-300)
        record_property("rel_fro_grad_err_vs_f64_%s_f32" % k, gerr["f32"][k])
        record_property("rel_fro_grad_err_vs_f64_%s_f32x3_bwd" % k, gerr["f32x3_bwd"][k])
        record_property("f32x3_bwd_over_f32_%s" % k, ratio)
        print("%-22s f32 %.3g  f32x3_bwd %.3g  ratio %.3f" % (k, gerr["f32"][k], gerr["f32x3_bwd"][k], ratio))
    for k in HipR2D2Learner.KEYS:
        assert gerr["f32x3_bwd"][k] <= X3_GRAD_SLACK * gerr["f32"][k], (k, gerr["f32x3_bwd"][k], gerr["f32"][k])


# ---- modes 0, 1 and 2 keep their bits -----------------------------------------------------------------------------------
PARENT_CASES = [(s, m) for s in PARENT_SHAPES for m in PARENT_MODES]


def test_fixture_covers_every_case():
    g = _golden()
    assert set(g["sha256"]) == {_key(s, m) for s, m in PARENT_CASES}
    for v in g["sha256"].values():
        assert set(v) == {"grads", "loss", "priority"} and all(len(x) == 64 for x in v.values())
    assert g["census_f32x3_693_frames"]["gemm_lds (f32)"] >= MOVED_GEMMS


@pytest.mark.parametrize("shape,mode", PARENT_CASES, ids=[_key(s, m) for s, m in PARENT_CASES])
def test_existing_modes_keep_the_parents_bits(shape, mode):
    got, _ = step_bits(shape, mode)
    want = _golden()["sha256"][_key(shape, mode)]
    bad = sorted(k for k in want if got[k] != want[k])
    assert not bad, "%s: outputs whose bits differ from the parent commit's: %s" % (_key(shape, mode), bad)


# ---- determinism, the split entry points, the update -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, RAGGED, ABOVE_1024], ids=["45-frames", "693-frames", "1056-frames"])
def test_mode_3_is_reproducible_and_loss_plus_grad_equals_backward(shape):
    """two backward() calls on one batch leave the same gradient bits (any split-K reduces in a fixed order), and
    loss() + grad() leave the bits of backward()"""
    import torch

    _, batch, weight = _case(shape)
    learner = _learner(shape, "f32x3_bwd")
    first = [x.clone() for x in learner.backward(batch, weight)]
    g0 = learner.flat()[1].clone()
    learner.flat()[1].zero_()
    second = learner.backward(batch, weight)
    learner.check()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(learner.flat()[1], g0)
    learner.flat()[1].zero_()
    halves = learner.loss(batch, weight)
    assert all(torch.equal(a, b) for a, b in zip(first, halves))
    learner.grad()
    learner.check()
    assert torch.equal(learner.flat()[1], g0)
    learner.close()


def test_mode_3_adam_step():
    """one step() in mode 3 at the shape, the learning rate and the clip of test_hip_r2d2_learner_adam_step_and_trajectory,
    against clip_grad_norm_ + torch.optim.Adam driven by autograd, at that test's tolerances"""
    import torch
    from rela_amd.learner import HipR2D2Learner
    from test_r2d2_learner_gpu import _agent, _random_batch

    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    A, B, seq, burn, n = 6, 8, 10, 4, 3
    rng = np.random.default_rng(5)
    agent = _agent(A, n, GAMMA, ETA, seq, burn, 81, 82, "cuda:0")
    lr, eps, clip = 1e-3, 1.5e-4, 0.5
    learner = HipR2D2Learner.from_agent(agent, B, lr=lr, eps=eps, grad_clip=clip)
    learner.set_precision("f32x3_bwd")
    optim = torch.optim.Adam(agent.online_net.parameters(), lr=lr, eps=eps)
    batch, weight = _random_batch(rng, A, B, seq, burn, n, "cuda:0")
    learner.step(batch, weight)
    learner.check()
    loss, _ = agent.loss(batch, sync_priority=False)
    (loss * weight).mean().backward()
    norm = torch.nn.utils.clip_grad_norm_(agent.online_net.parameters(), clip)
    optim.step()
    torch.cuda.synchronize()
    st = learner.stats().cpu().numpy()
    np.testing.assert_allclose(st[0], float(norm), rtol=2e-3)
    assert st[1] < 1.0
    sd = learner.state_dict("online")
    for key, p in agent.online_net.named_parameters():
        np.testing.assert_allclose(sd[key].cpu().numpy(), p.detach().cpu().numpy(), rtol=0, atol=0.05 * lr, err_msg=key)
    learner.close()


# ---- the training entry point -------------------------------------------------------------------------------------------
def test_r2d2_entry_point_trains_in_mode_3(capsys):
    """main.py --algo r2d2 --learner_precision f32x3_bwd at the size of test_training_entry_point_runs_with_value_rescale
    (2 threads x 4 envs, six updates): the learner the entry point builds is in mode 3 (gemm_bf16x3 runs in its steps) and
    reports a finite loss."""
    sys.path.insert(0, os.path.join(ROOT, "rela_amd", "pybind"))
    from rela_amd import _capi as capi
    from rela_amd.pyrela import main as entry

    args = entry.parse_args(["--algo", "r2d2", "--hip_learner", "1", "--learner_precision", "f32x3_bwd", "--num_thread", "2",
                             "--num_game_per_thread", "4", "--batchsize", "8", "--epoch_len", "6", "--num_epoch", "1",
                             "--burn_in_frames", "16", "--replay_buffer_size", "64", "--episode_len", "30",
                             "--actor_sync_freq", "3", "--seq_len", "8", "--seq_burn_in", "4"])
    assert args.learner_precision == "f32x3_bwd"
    with capi.launch_census() as census:
        hist = entry.train(args)
    out = capsys.readouterr().out
    assert "'learner_precision': 'f32x3_bwd'" in out and "Speed: train: " in out
    assert len(hist) == 1 and np.isfinite(hist[0]["loss"]) and hist[0]["act"] > 0
    assert census.counts.get("gemm_bf16x3", 0) >= MOVED_GEMMS, census.counts  # (at least one learner step in mode 3)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    assert first == second, "the learner step is not reproducible run to run"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "sha256 of the little-endian f32 flat gradient buffer, loss and priorities after one "
                   "HipR2D2Learner.backward per shape (A, B, seq, burn, n) and precision mode, and the launch census of the "
                   "f32x3 step at 693 frames (tests/test_r2d2_learner_bwd_mode_gpu.py)",
           "sha256": first,
           "census_f32x3_693_frames": step_bits(RAGGED, "f32x3")[1]}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(first), "cases")
