"""A deeper stage of the learner's GEMMs (csrc/gemm_lds.h, csrc/gemm_bf16x3.h: TileCfg's S chunks of 32 k per barrier)
keeps every bit.

A stage of S chunks is fetched, stored and multiplied per barrier; its chunks are multiplied one after the other in k
order, so an accumulator sees the MFMAs of the S = 1 kernel in the same order, and splits, kslice and the fold groups
stay counted in chunks.  What can go wrong is at a slice's end: a slice whose chunk count is no multiple of S ends in a
SHORT stage whose surplus chunks must not be multiplied (they would belong to the next split), a slice shorter than S
is one short stage, an empty slice stores zeros, and the last chunk of a K that is no multiple of 32 is partly zeroed.
So every output of the two one-call taps is compared by sha256 with tests/golden/gemm_stage_parent_bits.json, recorded
on an MI355X with this file's `compute()` from a checkout of the commit named in it: the parent of the stage depth
(S = 1 everywhere).  Inputs are random at the scale of a trained agent (gain 4.6), so any reassociation flips bits.

The instantiation with S > 1 (csrc/learner_common.hip: TileW1, Tile6W32U8) is conv1's weight gradient; the 64 x 64 tiles of
conv2 / conv3 were measured at S = 2 with these same cases (and passed them) but are slower there and stay at S = 1.  The
frame counts cover all three, so that a stage depth given to conv2 / conv3 later meets its slice ends here:
  conv1 (ProbW1),  K = 400 f, kSplitW1 = 64 slices,            S = 4 in f32 (gemm_lds), S = 2 in f32x3 (gemm_bf16x3)
  conv2 (ProbW2),  K =  81 f, 3 x kSplitW2 = 81 (f <= 1,024),  (S = 2)
  conv3 (ProbW3),  K =  49 f, 3 x kSplitW3 = 84 (f <= 1,024),  (S = 2)
With chunks = ceil(K / 32) and kslice = ceil(chunks / splits), slice z holds chunks [z kslice, min(chunks, (z + 1) kslice)):

  frames  conv1: K, chunks, kslice -> slices              conv2: K, chunks, kslice            conv3: K, chunks, kslice
     3    1,200 (37.5) 38, 1 -> 38 of 1 (< S = 2 too),    243 (7.6) 8, 1, 73 empty            147 (4.6) 5, 1, 79 empty
          26 empty
     7    2,800 (87.5) 88, 2 -> 44 of 2 (< S), 20 empty   567 (17.7) 18, 1 (< S), 63 empty    343 (10.7) 11, 1, 73 empty
    25    10,000 (312.5) 313, 5 -> 62 of 5 = 4 + 1,       2,025 (63.3) 64, 1, 17 empty        1,225 (38.3) 39, 1, 45 empty
          one of 3, one empty
    90    36,000 1,125, 18 -> 62 of 18 = 4 x 4 + 2 (five  7,290 (227.8) 228, 3 = 2 + 1        4,410 (137.8) 138, 2 = one full
          stages: one round of the ring), one of 9        -> 76 slices, 5 empty               stage -> 69 slices, 15 empty
          = 2 x 4 + 1, one empty
   113    45,200 (1412.5) 1,413, 23 -> 61 of 23 = 5 x 4   9,153 (286.03) 287, 4 = 2 x 2       5,537 (173.03) 174, 3 = 2 + 1
          + 3, one of 10 = 2 x 4 + 2, 2 empty             -> 71 of 4, one of 3, 9 empty       -> 58 slices, 26 empty

so each of the three has a slice whose chunk count is no multiple of S (25, 90, 113; 90 and 113; 113), a slice shorter
than S (7 for S = 4, 3 for S = 2 and 4), an empty slice (all) and a K that is no multiple of 32 (3, 7, 25, 113; all; all).  The bf16x2 mode runs its
own kernels for conv1 and the data gradients and gemm_bf16x3 for conv2 / conv3 below `fast_wgrad_min_frames` (2,048: all
five frame counts, so the default stays); it is run as well, as are the head / fc taps at two small batches (their
GEMMs stay at S = 1: 3 is one partial chunk, 70 two full chunks and one of six rows).

Re-recording (only ever from the commit BEFORE a change to the kernels):
    python tests/test_learner_gemm_stage_bits_gpu.py OUT.json COMMIT
"""
import functools
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gemm_stage_parent_bits.json")
MODES = ("f32", "bf16x2", "f32x3")
LANES = (0, 1)
TRUNK_FRAMES = (3, 7, 25, 90, 113)
HEAD_BATCHES = {3: 6, 70: 18}  # batch -> number of actions
TRUNK_CASES = [(m, l, f) for f in TRUNK_FRAMES for m in MODES for l in LANES]
HEAD_CASES = [(m, l, b) for b in HEAD_BATCHES for m in MODES for l in LANES]


def _slices(K, splits):
    """-> (chunks, kslice, [chunks of every slice])"""
    chunks = -(-K // 32)
    kslice = -(-chunks // splits)
    return chunks, kslice, [max(0, min(chunks, (z + 1) * kslice) - z * kslice) for z in range(splits)]


def test_frame_counts_reach_every_slice_end():
    """the arithmetic of the docstring: per conv layer and its S, the five frame counts together hold a slice that is no
    multiple of S, a slice shorter than S, an empty slice and a partial last chunk (no GPU work)"""
    for per_frame, splits, S in ((400, 64, 4), (400, 64, 2), (81, 81, 2), (49, 84, 2)):
        seen = set()
        for f in TRUNK_FRAMES:
            K = per_frame * f
            _, _, sl = _slices(K, splits)
            seen |= {"ragged" for n in sl if n > S and n % S}
            seen |= {"short" for n in sl if 0 < n < S}
            seen |= {"empty" for n in sl if n == 0}
            seen |= {"partial chunk"} if K % 32 else set()
        assert seen == {"ragged", "short", "empty", "partial chunk"}, (per_frame, seen)


@functools.lru_cache(maxsize=1)
def _trunk_inputs(frames):
    import test_learner_gemm_bits_gpu as B
    import test_trunk_backward_gpu as T
    import trunk_bwd_ref as R

    return T.to_device(R.random_inputs(frames, B.GAIN))


@functools.lru_cache(maxsize=1)
def _head_inputs(batch):
    import head_fc_bwd_ref as R
    import test_head_fc_backward_gpu as H
    import test_learner_gemm_bits_gpu as B

    return H.to_device(R.random_inputs(batch, HEAD_BATCHES[batch], B.GAIN))


def trunk_bits(mode, lanes, frames):
    """-> ({output: sha256}, launch census) of one rela_debug_trunk_backward call"""
    import test_learner_gemm_bits_gpu as B
    import test_trunk_backward_gpu as T
    import trunk_bwd_ref as R

    out, ran = T.run_tap(_trunk_inputs(frames), mode, lanes, 0)
    assert set(out) == set(R.KEYS)
    return {k: B._sha(out[k]) for k in R.KEYS}, dict(ran)


def head_bits(mode, lanes, batch):
    """-> ({output: sha256}, launch census) of one rela_debug_head_fc_backward call"""
    import head_fc_bwd_ref as R
    import test_head_fc_backward_gpu as H
    import test_learner_gemm_bits_gpu as B

    out, ran = H.run_tap(_head_inputs(batch), mode, lanes)
    assert set(out) == set(R.KEYS)
    return {k: B._sha(out[k]) for k in R.KEYS}, dict(ran)


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
    assert len(want) == 3 * 2 * (5 + 2)
    for v in _golden().values():
        assert len(v) == 8


def _compare(got, want, what):
    assert set(got) == set(want), what
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
                   "on random inputs at gain 4.6 (tests/test_learner_gemm_stage_bits_gpu.py)",
           "sha256": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(first), "cases")
