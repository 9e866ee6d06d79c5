"""The learner's GEMMs (csrc/gemm_lds.h, csrc/gemm_bf16x3.h) keep their bits under the branch-free loader contract.

A Problem's loaders fetch from an address that is always valid (row, k and image coordinates clamped into range) and
the zero of an out-of-range element is a select applied when the chunk is stored to LDS; ring refills past a slice's
end re-read its last chunk and are never stored; a block whose K slice is empty stores its zeros without a load.  None
of that may change a value: no split count, chunk order, MFMA order or operand changes, only when a wait happens.  So
every output of the two one-call taps is compared by sha256 with tests/golden/gemm_ring_parent_bits.json: recorded
on an MI355X with this file's `compute()` from a checkout of the commit named in it, the parent of the contract (whose
loaders returned zeros from a branch around the load).

Inputs are random at the scale of a trained agent (`random_inputs(.., gain 4.6)`), so any reassociation flips bits; the
exact-integer tests (tests/test_trunk_backward_gpu.py, tests/test_head_fc_backward_gpu.py) already prove that every term
is counted once whatever the order.  Every case runs the three precision modes' kernel families in both lane forms.

Shapes: the smallest where the new code can go wrong.  A chunk is 32 k, the register ring of gemm_bf16x3 is 4 chunks.
  trunk, K = 400 f (conv1), 81 f (conv2), 49 f (conv3) rows of f frames, split over 64 / 81 / 84 K slices
  (csrc/learner_plan.h: kSplitW1, 3 x kSplitW2, 3 x kSplitW3), slice = ceil(chunks / splits) chunks:
    1, 2    13 and 25 (conv1), 3 and 6 (conv2), 2 and 4 (conv3) chunks: one chunk per slice, most slices empty and
            writing zeros, every ring refill clamps, partial last chunks (400, 81, 49, 162, 98 mod 32 != 0);
    5       63 chunks of conv1 in 64 slices: one empty slice; conv2 / conv3 end on partial chunks (405, 245);
    6       75 chunks of conv1: two per slice, the 38th slice holds one, 26 are empty;
    41      513 chunks of conv1: nine per slice (two rounds of the ring and one step), 57 slices, the last two
            refills of every slice clamp; conv2 two per slice, conv3 one;
    257     3,213 / 651 / 394 chunks: 51 / 9 / 5 per slice, none dividing evenly, a partial last chunk in conv2 / conv3;
            the data gradients run 326 and 402 M tiles, the last one partly past M.
  head / fc, K = batch (weight gradients), M = batch (data gradients):
    1       one partial chunk, 127 clamped rows of the only M tile;
    33      one full chunk and one with a single row;
    129     ring depth + 1 chunks, a second M tile with one row;
    513     seventeen chunks: the ring wraps four times and ends on a one-row chunk.

Re-recording (only ever from the commit BEFORE a change to the kernels):
    python tests/test_learner_gemm_bits_gpu.py OUT.json COMMIT
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
FIXTURE = os.path.join(HERE, "golden", "gemm_ring_parent_bits.json")
GAIN = 4.6
MODES = ("f32", "bf16x2", "f32x3")
LANES = (0, 1)
TRUNK_FRAMES = (1, 2, 5, 6, 41, 257)
HEAD_BATCHES = {1: 6, 33: 18, 129: 31, 513: 18}  # batch -> number of actions
TRUNK_CASES = [(m, l, f) for f in TRUNK_FRAMES for m in MODES for l in LANES]
HEAD_CASES = [(m, l, b) for b in HEAD_BATCHES for m in MODES for l in LANES]


def _sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy().astype("<f4", copy=False))
    return hashlib.sha256(a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=1)
def _trunk_inputs(frames):
    import test_trunk_backward_gpu as T
    import trunk_bwd_ref as R

    return T.to_device(R.random_inputs(frames, GAIN))


@functools.lru_cache(maxsize=1)
def _head_inputs(batch):
    import head_fc_bwd_ref as R
    import test_head_fc_backward_gpu as H

    return H.to_device(R.random_inputs(batch, HEAD_BATCHES[batch], GAIN))


def trunk_bits(mode, lanes, frames):
    """-> ({output: sha256}, launch census) of one rela_debug_trunk_backward call"""
    import test_trunk_backward_gpu as T
    import trunk_bwd_ref as R

    out, ran = T.run_tap(_trunk_inputs(frames), mode, lanes, 0)
    assert set(out) == set(R.KEYS)
    return {k: _sha(out[k]) for k in R.KEYS}, dict(ran)


def head_bits(mode, lanes, batch):
    """-> ({output: sha256}, launch census) of one rela_debug_head_fc_backward call"""
    import head_fc_bwd_ref as R
    import test_head_fc_backward_gpu as H

    out, ran = H.run_tap(_head_inputs(batch), mode, lanes)
    assert set(out) == set(R.KEYS)
    return {k: _sha(out[k]) for k in R.KEYS}, dict(ran)


def _key(tap, mode, lanes, n):
    return "%s_%s_lanes%d_%d" % (tap, mode, lanes, n)


def compute():
    out = {}
    for mode, lanes, frames in TRUNK_CASES:
        out[_key("trunk", mode, lanes, frames)] = trunk_bits(mode, lanes, frames)[0]
    for mode, lanes, batch in HEAD_CASES:
        out[_key("head_fc", mode, lanes, batch)] = head_bits(mode, lanes, batch)[0]
    return out


@functools.lru_cache(maxsize=1)
def _golden():
    with open(FIXTURE) as f:
        return json.load(f)["sha256"]


def test_fixture_covers_every_case():
    want = {_key("trunk", *c) for c in TRUNK_CASES} | {_key("head_fc", *c) for c in HEAD_CASES}
    assert set(_golden()) == want
    assert len(want) == 3 * 2 * (6 + 4)
    for v in _golden().values():
        assert len(v) == 8


def _compare(got, want, what):
    bad = sorted(k for k in want if got[k] != want[k])
    assert not bad, "%s: outputs whose bits differ from the parent commit's: %s" % (what, bad)


@pytest.mark.parametrize("mode,lanes,frames", TRUNK_CASES, ids=["%s-lanes%d-%d" % c for c in TRUNK_CASES])
def test_trunk_backward_bits_equal_parent(mode, lanes, frames):
    import test_trunk_backward_gpu as T

    got, ran = trunk_bits(mode, lanes, frames)
    assert ran == T.expected_census(mode, frames, 0), ran
    _compare(got, _golden()[_key("trunk", mode, lanes, frames)], _key("trunk", mode, lanes, frames))


@pytest.mark.parametrize("mode,lanes,batch", HEAD_CASES, ids=["%s-lanes%d-%d" % c for c in HEAD_CASES])
def test_head_fc_backward_bits_equal_parent(mode, lanes, batch):
    import test_head_fc_backward_gpu as H

    got, ran = head_bits(mode, lanes, batch)
    assert ran == H.expected_census(mode), ran
    _compare(got, _golden()[_key("head_fc", mode, lanes, batch)], _key("head_fc", mode, lanes, batch))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    assert first == second, "the backward taps are not reproducible run to run"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "sha256 of the little-endian f32 outputs of rela_debug_trunk_backward and rela_debug_head_fc_backward "
                   "on random inputs at gain 4.6 (tests/test_learner_gemm_bits_gpu.py)",
           "sha256": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(first), "cases")
