"""The R2D2 learner's set_rec_wide256 option: lstm_rec_chain64 (csrc/learner_r2d2.hip), the forward recurrence of both
nets at 129 .. 256 batch rows as one persistent launch, against float64.  References, helpers and bounds are those of
tests/r2d2_paths.py and tests/test_r2d2_rec_wide_gpu.py (the arithmetic per row is the same); B = 129 is r2d2_paths' case,
the other batches are built here from seed = B, checked on the CPU for check_case's properties.  Every step asserts its
form of the recurrence from the launch census.  Without a GPU: the compiler's account of the kernel, and --learner_rec."""
import pytest

import r2d2_paths as P
from kernel_names import R2D2_BPTT_STEPS, R2D2_REC_CHAIN, R2D2_REC_STEPS, R2D2_REC_ZERO, X3_LSTM
from test_r2d2_rec_wide_gpu import DEV, _learner, _step

_refs = {}


def _case(B):
    """-> ((A, B, seq, burn, n, seed), batch, weight) on the device; the seed's properties are asserted"""  # (as check_case)
    case = (18, B, 3, 2, 2, B)
    burn, cpu = case[3], P.make_batch(*case)[0]
    lens, dummy = cpu.seq_len.numpy(), cpu.terminal[burn - 1].numpy()
    assert (lens < burn + case[2]).any() and lens[B - 1] >= burn + 2 and dummy.any() and not dummy.all()
    return (case,) + P.make_batch(*case, DEV)


def _reference(case, kind):
    """float64 r2d2_loss on the CPU as r2d2_paths.as_result, once per batch; not to be modified"""
    A, B, seq, burn, n, _ = case
    if B == 129:
        return P.reference("B129", kind)
    assert kind == "batch"  # (the one-hot weights run at 129 only)
    if B not in _refs:
        _refs[B] = P.as_result(*P.f64_ref.r2d2_loss(*P.case_params("B128"), *P.make_batch(*case), P.GAMMA, n, P.ETA, seq,
                                                    burn, P.torch.float64, None))
    return _refs[B]


@pytest.mark.gpu
@pytest.mark.parametrize("B,precision", [(129, "f32"), (177, "f32"), (193, "f32"), (256, "f32"), (256, "f32x3")])
def test_chain64_matches_f64(B, precision):
    """129: tiles 0-1 full, one row in tile 2, tile 3's chains leave; 177: tile 2 ends inside its fourth sub-tile (49
    rows); 193: one row in tile 3, in its first sub-tile; 256: all eight chains full, in f32x3 on the mode's x-part.  At
    129 a second backward puts all weight on the last row, alone in its tile.  The BPTT above 128 rows runs per step."""
    case, batch, weight = _case(B)
    learner = _learner(B, precision)
    learner.set_rec_wide256(True)
    for kind, w in (("batch", weight), ("onehot", P.one_hot_weight(B, DEV)))[:2 if B == 129 else 1]:
        got, _, counts = _step(learner, batch, w)
        assert counts.get("lstm_rec_chain64") == 1 and R2D2_BPTT_STEPS <= set(counts), counts
        assert not ((R2D2_REC_CHAIN | R2D2_REC_STEPS | {R2D2_REC_ZERO, "lstm_rec_chain32"}) & set(counts)), counts
        assert precision != "f32x3" or X3_LSTM <= set(counts), counts
        ref = _reference(case, kind)
        assert all(float(g.abs().max()) > 0 for g in ref["grads"].values())
        assert P.beyond(got, ref, P.GRAD_TOL[precision]) == []
    learner.close()


@pytest.mark.gpu
def test_off_is_off_other_batches_keep_their_paths_and_refusals():
    """On then off at B = 129: the census and the bits of a learner whose option was never touched.  On, with rec_wide
    on: B = 128 runs lstm_rec_chain32 and B = 257 runs per step."""
    import torch
    from rela_amd import _capi as capi

    case, batch, weight = _case(129)
    T = case[3] + case[2] + case[4]  # burn + seq + n
    fresh = _learner(257)
    want, want_flat, want_counts = _step(fresh, batch, weight)
    fresh.close()
    learner = _learner(257)
    for l, on in ((None, 1), (learner.h, 2), (learner.h, -1)):
        assert capi.lib.rela_r2d2_learner_set_rec_wide256(l, on) == capi.EINVAL
    learner.set_rec_wide256(True)
    learner.set_rec_wide256(False)
    got, flat, counts = _step(learner, batch, weight)
    assert counts == want_counts and "lstm_rec_chain64" not in counts, (counts, want_counts)
    assert all(counts.get(k) == 2 * T for k in R2D2_REC_STEPS) and counts.get(R2D2_REC_ZERO) == 2, counts
    assert all(torch.equal(got[k], want[k]) for k in ("loss", "priority", "loss_seq")) and torch.equal(flat, want_flat)
    learner.set_rec_wide256(True)
    learner.set_rec_wide(True)
    counts = _step(learner, *P.case_batch("B128", DEV))[2]
    assert counts.get("lstm_rec_chain32") == 1 and "lstm_rec_chain64" not in counts, counts
    counts = _step(learner, *_case(257)[1:])[2]
    assert all(counts.get(k) == 2 * T for k in R2D2_REC_STEPS) and "lstm_rec_chain64" not in counts, counts
    learner.close()


def test_lstm_rec_chain64_no_scratch_no_spills(tmp_path):
    """one block of 8 waves per CU needs 2 waves per SIMD, so 256 VGPRs at the most; the partial tiles are dynamic LDS"""
    from kernel_resources import kernel_resources
    (name, v), = [kv for kv in kernel_resources("learner_r2d2.hip", tmp_path).items() if "16lstm_rec_chain64E" in kv[0]]
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    assert v["VGPRs"] + v["AGPRs"] <= 256 and v["Occupancy [waves/SIMD]"] >= 2 and v["LDS Size [bytes/block]"] < 1024, (name, v)


@pytest.mark.parametrize("argv", [["--algo", "apex"], ["--algo", "r2d2", "--hip_learner", "0"]])
def test_learner_rec_wide256_flag_and_its_refusals(argv):
    from rela_amd.pyrela import main as entry
    args = entry.parse_args(["--algo", "r2d2", "--learner_rec", "wide256"])
    assert entry.learner_rec_wide(args) is True and entry.learner_rec_wide256(args) is True  # (both options)
    assert entry.learner_rec_wide256(entry.parse_args(["--algo", "r2d2", "--learner_rec", "wide"])) is False
    with pytest.raises(SystemExit):
        entry.train(entry.parse_args(argv + ["--learner_rec", "wide256"]))
