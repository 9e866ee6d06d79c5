"""Whole learner steps keep the bits and the launches they had before the backward plan (csrc/learner_plan.h).

The backward passes of both learners take every kernel choice -- arithmetic of each GEMM, split-K counts, the bf16 weight
gradient kernels, the block cap of conv1 -- from one plan.  The per-call tests pin the taps; tests/test_r2d2_learner_bwd_mode_gpu.py
pins whole R2D2 steps in modes 0 - 2.  This file pins what those leave open:

  R2D2, mode "f32x3_bwd", shapes (A, B, seq, burn, n):
    (6, 5, 7, 0, 2)      45 training rows
    (18, 33, 12, 6, 3)   495 training rows: below 1,024, the head weight gradient in one GEMM, conv2 / conv3 at 3 x the splits
    (6, 33, 30, 0, 2)    1,056 training rows: the head weight gradient split-K, conv2 / conv3 at twice the splits
  Ape-X, modes "f32", "bf16x2" and "f32x3", default lanes, (A, B) = (6, 33) and (18, 5).

Per case: sha256 of the flat gradient buffer, the loss and the priorities after one backward(), and the launch census.
tests/golden/learner_plan_parent_bits.json was recorded on an MI355X with this file's `compute()` from a checkout of the
commit named in it (the parent of the plan).

Re-recording (only ever from the commit BEFORE a change to the learners' backward passes):
    python tests/test_learner_plan_bits_gpu.py OUT.json COMMIT
"""
import functools
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "learner_plan_parent_bits.json")

R2D2_SHAPES = [(6, 5, 7, 0, 2), (18, 33, 12, 6, 3), (6, 33, 30, 0, 2)]
APEX_SHAPES = [(6, 33), (18, 5)]  # (A, B)
APEX_MODES = ("f32", "bf16x2", "f32x3")
OUTPUTS = {"grads", "loss", "priority"}


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """the net initialisations seed the global generators: tests elsewhere must not see that"""
    import torch

    with torch.random.fork_rng(devices=[0]):
        yield


def _r2d2_key(shape):
    return "r2d2_A%d_B%d_seq%d_burn%d_n%d_f32x3_bwd" % shape


def _apex_key(shape, mode):
    return "apex_A%d_B%d_%s" % (*shape, mode)


def r2d2_bits(shape):
    from test_r2d2_learner_bwd_mode_gpu import step_bits

    out, census = step_bits(shape, "f32x3_bwd")
    return {"sha256": out, "census": census}


@functools.lru_cache(maxsize=None)
def _apex_case(shape):
    """-> (agent, batch, weight) of an Ape-X shape, as tests/test_learner_gpu.py builds them; shared, never changed"""
    import torch
    from test_learner_gpu import make_agent, make_batch

    A, B = shape
    with torch.random.fork_rng(devices=[0]):
        agent = make_agent(A, 100 * A + B)
    batch, weight = make_batch(B, A, 1000 * A + B)
    return agent, batch, weight


def apex_bits(shape, mode):
    """-> {"sha256": {output: sha256}, "census": launches} of one backward() of a fresh Ape-X learner in `mode`"""
    import torch
    from rela_amd import _capi as capi
    from rela_amd.learner import HipApexLearner
    from test_r2d2_learner_bwd_mode_gpu import _sha

    agent, batch, weight = _apex_case(shape)
    learner = HipApexLearner.from_agent(agent, shape[1])
    learner.set_precision(mode)
    with capi.launch_census() as census:
        loss, prio = learner.backward(batch, weight)
    torch.cuda.synchronize()
    out = {"grads": _sha(learner.flat()[1]), "loss": _sha(loss), "priority": _sha(prio)}
    learner.close()
    return {"sha256": out, "census": dict(census.counts)}


def compute():
    out = {_r2d2_key(s): r2d2_bits(s) for s in R2D2_SHAPES}
    for shape in APEX_SHAPES:
        for mode in APEX_MODES:
            out[_apex_key(shape, mode)] = apex_bits(shape, mode)
    return out


@functools.lru_cache(maxsize=1)
def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


def _assert_same(key, got):
    want = _golden()["cases"][key]
    bad = sorted(k for k in want["sha256"] if got["sha256"][k] != want["sha256"][k])
    print(key, got["census"])
    assert not bad, "%s: outputs whose bits differ from the parent commit's: %s" % (key, bad)
    assert got["census"] == want["census"], (key, got["census"], want["census"])


APEX_CASES = [(s, m) for s in APEX_SHAPES for m in APEX_MODES]


def test_fixture_covers_every_case():
    g = _golden()
    assert set(g["cases"]) == {_r2d2_key(s) for s in R2D2_SHAPES} | {_apex_key(s, m) for s, m in APEX_CASES}
    for case in g["cases"].values():
        assert set(case["sha256"]) == OUTPUTS and all(len(x) == 64 for x in case["sha256"].values())
        assert case["census"] and all(isinstance(v, int) and v > 0 for v in case["census"].values())
    # the R2D2 shapes lie on both sides of the 1,024-row rule, and mode 3 and two of Ape-X's modes reach gemm_bf16x3
    assert all(g["cases"][_r2d2_key(s)]["census"].get("gemm_bf16x3", 0) >= 6 for s in R2D2_SHAPES)
    for s in APEX_SHAPES:
        assert "gemm_bf16x3" not in g["cases"][_apex_key(s, "f32")]["census"]
        assert all(g["cases"][_apex_key(s, m)]["census"].get("gemm_bf16x3", 0) > 0 for m in ("bf16x2", "f32x3"))


@pytest.mark.parametrize("shape", R2D2_SHAPES, ids=[_r2d2_key(s) for s in R2D2_SHAPES])
def test_r2d2_mode_3_keeps_the_parents_bits_and_launches(shape):
    _assert_same(_r2d2_key(shape), r2d2_bits(shape))


@pytest.mark.parametrize("shape,mode", APEX_CASES, ids=[_apex_key(s, m) for s, m in APEX_CASES])
def test_apex_step_keeps_the_parents_bits_and_launches(shape, mode):
    _assert_same(_apex_key(shape, mode), apex_bits(shape, mode))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    differ = sorted(k for k in first if first[k] != second[k])
    assert not differ, "not reproducible run to run: %s" % [(k, first[k], second[k]) for k in differ]
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "per case the sha256 of the little-endian f32 flat gradient buffer, loss and priorities after one "
                   "backward() of a fresh learner, and the launch census of that call: HipR2D2Learner in f32x3_bwd per "
                   "shape (A, B, seq, burn, n), HipApexLearner per (A, B) and precision mode "
                   "(tests/test_learner_plan_bits_gpu.py)",
           "cases": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(first), "cases")
