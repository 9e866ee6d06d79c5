"""gemm_s3 with its LDS-DMAs spread over the pair's MFMA groups yields the SAME BITS as the kernel it replaced.

The change to csrc/gemm_s3.h's k-loop moves only WHERE a wave issues its LDS-DMA pieces (and which counted wait covers
them); per output element the operations and their order are what they were.  tests/test_gemm_s3_bits_gpu.py pins the
benchmark's sizes; this file adds row counts around the edges of the f32x3 forward and of s3::plan(), with the sha256 of
the outputs recorded on an MI355X from a checkout of the commit named in tests/golden/gemm_s3_sched_parent_bits.json
(the parent of the change), with this file's `compute()`:

  * AtariFFNet Q in f32x3 mode at 1, 17, 113, 225, 769 and 897 rows.  The forward plan (csrc/ffnet_plan.h) gives a
    batch below kEmuConvMinN = 512 rows to the exact-f32 kernels even in f32x3 mode, so the four small sizes pin what
    that mode computes there (the census must then NOT hold gemm_s3: the plan did not change) and the kernel itself
    runs at 769 rows (the first size s3::plan() does not split: 56 row blocks of one tile or none) and 897 (64 row
    blocks, a ragged last tile);
  * because those sizes reach only one-tile passes, three more that walk the other pass shapes of the k-loop:
    2,049 rows (blocks of 2 and 3 tiles and one ragged row), 4,500 (4 and 5 tiles), and the AtariLSTMNet step at 1,800
    rows (16 row blocks of 7 or 8 tiles: one pass of 7, or two passes of 4 -- a pass boundary inside the pipeline);
  * the AtariLSTMNet step (h, c, Q) at 1, 113 and 769 rows (769: 16 row blocks of 3 and 4 tiles).

Each case asserts through the launch census which fc form ran: `fc_reduce` is present exactly where the contraction is
split (up to 768 rows: s3::plan()'s rule from 512 rows on, the f32 split-K fc below), and gemm_s3<...> from 512 rows on.

Re-recording (only ever from the commit BEFORE a change to the kernel):
    python tests/test_gemm_s3_sched_bits_gpu.py OUT.json COMMIT
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gemm_s3_sched_parent_bits.json")
FF_ROWS = (1, 17, 113, 225, 769, 897)  # the sizes the change was specified with
FF_ROWS_PASSES = (2049, 4500)          # further pass shapes of the k-loop
LSTM_ROWS = (1, 113, 769)
LSTM_ROWS_PASSES = (1800,)
X3_FROM = 512     # csrc/ffnet_plan.h: kEmuConvMinN
SPLIT_UPTO = 768  # s3::plan<ProbFc>(M, true) splits up to 48 row tiles; below X3_FROM the f32 fc splits too


def _fns():
    sys.path.insert(0, HERE)
    from test_gemm_s3_bits_gpu import ffnet_q, lstm_step

    return ffnet_q, lstm_step


def compute():
    ffnet_q, lstm_step = _fns()
    out = {}
    for n in FF_ROWS + FF_ROWS_PASSES:
        out["ffnet_q_%d" % n] = ffnet_q(n)[0]
    for n in LSTM_ROWS + LSTM_ROWS_PASSES:
        out["lstm_step_%d" % n] = lstm_step(n)[0]
    return out


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("n", FF_ROWS + FF_ROWS_PASSES)
def test_ffnet_q_bits_equal_parent(n):
    from kernel_names import X3_FFNET

    ffnet_q, _ = _fns()
    sha, ran = ffnet_q(n)
    if n >= X3_FROM:
        assert X3_FFNET <= ran, sorted(ran)
    else:
        assert not (X3_FFNET & ran), sorted(ran)
    assert ("fc_reduce" in ran) == (n <= SPLIT_UPTO), sorted(ran)
    assert sha == _golden()["sha256"]["ffnet_q_%d" % n]


@pytest.mark.parametrize("n", LSTM_ROWS + LSTM_ROWS_PASSES)
def test_lstm_step_bits_equal_parent(n):
    from kernel_names import X3_LSTM

    _, lstm_step = _fns()
    sha, ran = lstm_step(n)
    if n >= X3_FROM:
        assert X3_LSTM <= ran, sorted(ran)
    else:
        assert not (X3_LSTM & ran), sorted(ran)
    assert sha == _golden()["sha256"]["lstm_step_%d" % n]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    assert first == second, "the forward is not reproducible run to run"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "sha256 of the little-endian f32 outputs of the f32x3 forward (tests/test_gemm_s3_sched_bits_gpu.py)",
           "sha256": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc))
