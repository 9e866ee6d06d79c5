"""conv12_s3's patch ring (csrc/conv12_s3.h): pixel 80 of conv2's 9 x 9 image, batched across frames, keeps the bits.

A frame runs five 16-pixel conv2 tiles (pixels 0 .. 79).  The sixteen a1 records pixel 80 reads go into slot `filled` of
an LDS ring of S = Conv12S::RING_S slots, and one more tile over the ring -- lane li takes slot li and stores pixel 80 of
frame first + li * grid -- runs when the ring is full and once after a block's last frame.  tests/test_conv12_s3_bits_gpu.py
stops at 769 rows: with 256 blocks that is at most four frames per block, so the ring there never fills.  The row counts
here are the smallest at which the ring logic can go wrong (256 blocks, one per CU):

  256 S        every block ends with its ring exactly full: one deferred tile, not two;
  256 S + 1    block 0 gets one more frame: a full tile, then a tile with one slot;
  512 S + 1    two full tiles, then a partial one.

(a) sha256 of Q [n][A] of the f32x3 forward (conv12_s3<false>) at each size, and of a1 / a2 of the keep-f32 learner pass
    (conv12_s3<true>) at 256 S + 1 rows, against tests/golden/conv12_s3_ring_parent_bits.json: recorded on an MI355X with
    this file's `compute()` from a checkout of the commit named in it, the parent of the ring (whose kernel ran a sixth,
    padded tile per frame).  The launch census shows that conv12_s3 really ran.
(b) no fixture: the 512 S + 1 rows in ONE launch against the same rows in consecutive 512-row launches (the remainder
    padded to 512 with repeated rows), `np.array_equal`.  In the one launch a row's patch sits in slot (row / grid) % S of
    a ring that fills to S; in the 512-row launches it sits in slot 0 or 1 of a ring that fills to 2: any mix-up of slot
    and frame shows.  What is compared is a2 [n][81][64], the kernel's own output with pixel 80 in it, from the keep-f32
    learner pass (conv12_s3<true>; (a) covers <false> at the same row counts).  Q cannot serve here: below 2,048 rows fc
    splits its contraction over eight slices that fc_reduce adds (s3::plan, kFcSplitBelow), so Q of a 512-row forward
    and Q of the same rows inside a 2,561-row forward differ in their last bits whatever conv12_s3 does -- measured on
    the parent commit and on this kernel alike: all 2,561 rows of Q differ, no element of a2 does.

Re-recording (only ever from the commit BEFORE a change to the kernel; `compute()` needs no ring in the kernel it runs):
    python tests/test_conv12_s3_ring_bits_gpu.py OUT.json COMMIT
"""
import json
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "conv12_s3_ring_parent_bits.json")
A = 18
S = 5  # Conv12S::RING_S, asserted against the header below
BLOCKS = 256  # persistent blocks: one per CU
ROWS = (BLOCKS * S, BLOCKS * S + 1, 2 * BLOCKS * S + 1)
CHUNK = 512


def kernel_ring_slots():
    with open(os.path.join(os.path.dirname(HERE), "rela_amd", "csrc", "conv12_s3.h")) as f:
        m = re.search(r"constexpr int RING_S = (\d+);", f.read())
    assert m, "Conv12S::RING_S not found in csrc/conv12_s3.h"
    return int(m.group(1))


def test_rows_follow_the_kernels_ring():
    assert kernel_ring_slots() == S
    assert ROWS == (1280, 1281, 2561)


def compute():
    from test_conv12_s3_bits_gpu import ffnet_q, learner_a1_a2

    out = {}
    for n in ROWS:
        out["ffnet_q_%d" % n] = ffnet_q(n)[0]
    out["learner_a1_%d" % ROWS[1]], out["learner_a2_%d" % ROWS[1]] = learner_a1_a2(ROWS[1])[:2]
    return out


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)["sha256"]


@pytest.mark.parametrize("n", ROWS)
def test_ffnet_q_bits_equal_parent(n):
    from kernel_names import X3_FFNET
    from test_conv12_s3_bits_gpu import ffnet_q

    sha, ran = ffnet_q(n)
    assert X3_FFNET <= set(ran), sorted(ran)
    assert ran["conv12_s3"] == 1, ran
    assert sha == _golden()["ffnet_q_%d" % n]


def test_keep_f32_a1_a2_bits_equal_parent():
    from kernel_names import X3_FFNET
    from test_conv12_s3_bits_gpu import learner_a1_a2

    n = ROWS[1]
    a1, a2, ran = learner_a1_a2(n)
    assert X3_FFNET <= set(ran) and ran["conv12_s3"] == 3 and "unsplit_s3" in ran, ran
    assert a1 == _golden()["learner_a1_%d" % n]
    assert a2 == _golden()["learner_a2_%d" % n]


def _chunks(n):
    """[(first row, rows taken, index array of CHUNK rows: the remainder is padded with its last row)]"""
    out = []
    for r0 in range(0, n, CHUNK):
        k = min(CHUNK, n - r0)
        out.append((r0, k, np.minimum(np.arange(r0, r0 + CHUNK), r0 + k - 1)))
    return out


def _keep_f32_a2(learner, s_rows):
    """a2 [n][81][64] of the learner's online(obs) pass (conv12_s3<true>) over the frames s_rows, and the census"""
    import torch
    from types import SimpleNamespace

    from rela_amd import _capi as capi

    dev = "cuda:0"
    n = len(s_rows)
    # [s' ; s] in one tensor: s' is never right behind s, so online(s) stays a launch of its own
    frames = torch.empty((2, n, 4, 84, 84), dtype=torch.uint8, device=dev)
    frames[1].copy_(torch.from_numpy(s_rows))
    frames[0].copy_(frames[1].flip(0))
    moves = torch.ones((2, n, A), device=dev)
    batch = SimpleNamespace(obs={"s": frames[1], "eps": torch.zeros(n, 1, device=dev), "legal_move": moves[1]},
                            next_obs={"s": frames[0], "eps": torch.zeros(n, 1, device=dev), "legal_move": moves[0]},
                            action={"a": torch.zeros(n, dtype=torch.int64, device=dev)},
                            reward=torch.zeros(n, device=dev),
                            terminal=torch.zeros(n, dtype=torch.bool, device=dev), bootstrap=torch.ones(n, device=dev))
    with capi.launch_census() as census:
        learner.loss(batch, torch.ones(n, device=dev))
        torch.cuda.synchronize()
    a2 = learner.debug_activations()[1]
    assert tuple(a2.shape) == (n, 81, 64)
    return a2.cpu().numpy(), dict(census.counts)


def test_one_launch_equals_512_row_launches_a2():
    """a2 of the 512 S + 1 rows in one keep-f32 pass against a2 of the same rows in consecutive 512-row passes."""
    import torch

    from rela_amd.learner import HipApexLearner
    from synth import synth_obs, synth_params

    n = ROWS[2]
    obs = synth_obs(n, 7400 + n)
    sd_on = {k: torch.from_numpy(v) for k, v in synth_params(A, 55).items()}
    sd_tg = {k: torch.from_numpy(v) for k, v in synth_params(A, 56).items()}

    def learner_of(rows):
        learner = HipApexLearner(A, rows, 3, 0.99, device="cuda:0")
        learner.load_state_dicts(sd_on, sd_tg)
        learner.set_precision("f32x3")
        return learner

    big = learner_of(n)
    whole, ran = _keep_f32_a2(big, obs)
    big.close()
    assert ran["conv12_s3"] == 3 and "unsplit_s3" in ran, ran
    assert np.isfinite(whole).all() and (whole > 0).mean() > 0.05
    small = learner_of(CHUNK)
    for r0, k, idx in _chunks(n):
        part, ran = _keep_f32_a2(small, obs[idx])
        assert ran["conv12_s3"] == 3 and "unsplit_s3" in ran, ran
        bad = np.flatnonzero((whole[r0:r0 + k] != part[:k]).any(axis=(1, 2)))
        print("rows from", r0, ": rows whose a2 differs:", len(bad), bad[:16])
        assert np.array_equal(whole[r0:r0 + k], part[:k]), r0
    small.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    assert first == second, "the forward is not reproducible run to run"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "sha256 of the little-endian f32 outputs of the f32x3 forward and of the keep-f32 learner pass "
                   "(tests/test_conv12_s3_ring_bits_gpu.py)",
           "sha256": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc))
