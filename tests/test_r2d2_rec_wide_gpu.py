"""The R2D2 learner's set_rec_wide option: lstm_rec_chain32 (csrc/learner_r2d2.hip), the forward recurrence of both nets
at 65 .. 128 batch rows as one persistent launch, against float64.  Cases, references and bounds are those of
tests/r2d2_paths.py; B = 97 is built here, its seed chosen on the CPU for check_case's properties.  Every step asserts its
form of the recurrence from the launch census.  Without a GPU: the compiler's account of the kernel, and --learner_rec."""
import pytest

import r2d2_paths as P
from kernel_names import R2D2_REC_CHAIN, R2D2_REC_STEPS, R2D2_REC_ZERO, X3_LSTM

DEV = "cuda:0"
B97 = (18, 97, 3, 2, 2, 97)  # (A, B, seq, burn, n, seed): three full tiles plus one row


def _case(name):
    """-> ((A, B, seq, burn, n), batch, weight) on the device; the seeds' properties are asserted"""
    if name != "B97":
        P.check_case(name)
        return (P.shape(name),) + P.case_batch(name, DEV)
    B, burn, cpu = B97[1], B97[3], P.make_batch(*B97)[0]
    lens, dummy = cpu.seq_len.numpy(), cpu.terminal[burn - 1].numpy()
    assert (lens < burn + B97[2]).any() and lens[B - 1] >= burn + 2 and dummy.any() and not dummy.all()
    return (B97[:5],) + P.make_batch(*B97, DEV)


def _reference(name, kind):
    """float64 r2d2_loss on the CPU as r2d2_paths.as_result; kind: "batch" (the case's weights) or "onehot" (used once each)"""
    if name != "B97":
        return P.reference(name, kind)
    (A, B, seq, burn, n, _), (batch, w) = B97, P.make_batch(*B97)
    w = P.one_hot_weight(B) if kind == "onehot" else w
    return P.as_result(*P.f64_ref.r2d2_loss(*P.case_params("B128"), batch, w, P.GAMMA, n, P.ETA, seq, burn, P.torch.float64, None))


def _learner(B, precision="f32"):
    from rela_amd.learner import HipR2D2Learner

    learner = HipR2D2Learner.from_agent(P.case_agent("B128", DEV), B, grad_clip=1e9)  # (the nets depend on A only)
    learner.set_precision(precision)
    return learner


def _step(learner, batch, weight):  # one backward under the census, check() -> (as_result, flat gradient, counts)
    from rela_amd import _capi as capi

    with capi.launch_census() as census:
        out = learner.backward(batch, weight)
    learner.check()
    return P.as_result(*out, learner.state_dict("grads")), learner.flat()[1].clone(), census.counts


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision", [("B65", "f32"), ("B97", "f32"), ("B128", "f32"), ("B128", "f32x3")])
def test_wide_chain_matches_f64(name, precision):
    """B65: tiles 0-1 full, one row in tile 2, tile 3's chains leave; B97: one row in tile 3; B128: all eight chains full,
    in f32x3 on the mode's x-part.  At 65 and 97 a second backward puts all weight on the last row, alone in its tile."""
    (A, B, seq, burn, n), batch, weight = _case(name)
    learner = _learner(B, precision)
    learner.set_rec_wide(True)
    for kind, w in (("batch", weight), ("onehot", P.one_hot_weight(B, DEV)))[:2 if B in (65, 97) else 1]:
        got, _, counts = _step(learner, batch, w)
        assert counts.get("lstm_rec_chain32") == 1 and counts.get("lstm_bptt_chain") == 1, counts
        assert not ((R2D2_REC_CHAIN | R2D2_REC_STEPS | {R2D2_REC_ZERO}) & set(counts)), counts
        assert precision != "f32x3" or X3_LSTM <= set(counts), counts
        ref = _reference(name, kind)
        assert all(float(g.abs().max()) > 0 for g in ref["grads"].values())
        assert P.beyond(got, ref, P.GRAD_TOL[precision]) == []
    learner.close()


@pytest.mark.gpu
def test_off_is_off_64_rows_keep_their_chain_and_refusals():
    """On then off at B = 128: the per-step forward, and a fresh learner's bits.  On at B = 64: lstm_rec_chain."""
    import torch
    from rela_amd import _capi as capi

    (A, B, seq, burn, n), batch, weight = _case("B128")
    fresh = _learner(B)
    want, want_flat, _ = _step(fresh, batch, weight)
    fresh.close()
    learner = _learner(B)
    assert capi.lib.rela_r2d2_learner_set_rec_wide(None, 1) == capi.EINVAL
    assert capi.lib.rela_r2d2_learner_set_rec_wide(learner.h, 2) == capi.EINVAL
    learner.set_rec_wide(True)
    learner.set_rec_wide(False)
    got, flat, counts = _step(learner, batch, weight)
    assert "lstm_rec_chain32" not in counts and not (R2D2_REC_CHAIN & set(counts)), counts
    assert all(counts.get(k) == 2 * (burn + seq + n) for k in R2D2_REC_STEPS) and counts.get(R2D2_REC_ZERO) == 2, counts
    assert all(torch.equal(got[k], want[k]) for k in ("loss", "priority", "loss_seq")) and torch.equal(flat, want_flat)
    learner.set_rec_wide(True)
    counts = _step(learner, *_case("B64")[1:])[2]
    assert counts.get("lstm_rec_chain") == 1 and "lstm_rec_chain32" not in counts, counts
    learner.close()


def test_lstm_rec_chain32_no_scratch_no_spills(tmp_path):
    """one block of 8 waves per CU needs 2 waves per SIMD; the partial tiles are dynamic LDS"""
    from kernel_resources import kernel_resources

    (name, v), = [kv for kv in kernel_resources("learner_r2d2.hip", tmp_path).items() if "16lstm_rec_chain32E" in kv[0]]
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    assert v["Occupancy [waves/SIMD]"] >= 2 and v["LDS Size [bytes/block]"] < 1024, (name, v)


@pytest.mark.parametrize("argv", [["--algo", "apex"], ["--algo", "r2d2", "--hip_learner", "0"]])
def test_learner_rec_flag_and_its_refusals(argv):
    from rela_amd.pyrela import main as entry

    assert entry.learner_rec_wide(entry.parse_args(["--algo", "r2d2"])) is False  # default: mode
    assert entry.learner_rec_wide(entry.parse_args(["--algo", "r2d2", "--learner_rec", "wide"])) is True
    with pytest.raises(SystemExit):
        entry.train(entry.parse_args(argv + ["--learner_rec", "wide"]))
