"""The f32x3 fc / gate GEMM (csrc/gemm_s3.h) yields the SAME BITS as the kernel it replaced.

The eight-wave form of gemm_s3 keeps the sequence of operations per output element (k-steps ascending, the six
products of a k-step in the same order into the same two accumulators, one acc + accs, then the epilogue), plan() and
fc_reduce, so the f32x3 forward must reproduce the outputs of the four-wave kernel bit for bit.  The fixture
tests/golden/gemm_s3_parent_bits.json holds the sha256 of those outputs, recorded on an MI355X from a checkout of the
commit named in it (the parent of the change), with this file's `compute()`:

  * AtariFFNet Q in f32x3 mode at 512 rows (split-K slices + fc_reduce), 1,024 (the learner's merged [s ; s'] rows: one
    slice, one tile per block), 1,537 (a ragged last tile, row blocks of unequal size) and 6,400 rows (the benchmark's
    actor tick: row blocks of 6 and 7 tiles);
  * the AtariLSTMNet step (h, c, Q) in f32x3 mode at 515 and 3,200 rows: the x part of the gates, 3136 -> 2048, raw sums.
    (The bias epilogue of the same kernel body runs in the R2D2 learner's forward: tests/test_r2d2_learner_gpu.py.)

Inputs are seeded (tests/synth.py weights, a CPU torch.Generator for the frames), so they are the same everywhere.
Each case also asserts through the launch census that gemm_s3<...> really ran.

Re-recording (only ever from the commit BEFORE a change to the kernel):  python tests/test_gemm_s3_bits_gpu.py OUT.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gemm_s3_parent_bits.json")
A = 18
FF_ROWS = (512, 1024, 1537, 6400)
LSTM_ROWS = (515, 3200)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, "<f4").tobytes())
    return h.hexdigest()


def _frames(n, seed):
    import torch

    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, 4, 84, 84), dtype=torch.uint8, generator=g)


def ffnet_q(n):
    """(sha256 of Q [n][A] of the f32x3 forward, the launch census)"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import FFNetHandle
    from synth import synth_params

    net = FFNetHandle(A, "cuda:0")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 41).items()})
    net.set_precision("f32x3")
    s = _frames(n, 9000 + n).cuda()
    legal = torch.ones((n, A), device="cuda")
    q = torch.empty((n, A), device="cuda")
    nb = capi.lib.rela_ffnet_workspace_bytes(net.h, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with capi.launch_census() as census:
        capi.check(capi.lib.rela_ffnet_forward(net.h, n, C.c_void_p(s.data_ptr()), C.c_void_p(legal.data_ptr()),
                                               C.c_void_p(q.data_ptr()), C.c_void_p(ws.data_ptr()), nb, stream), "fwd")
        torch.cuda.synchronize()
    out = q.cpu().numpy()
    net.close()
    assert np.isfinite(out).all()
    return _sha(out), set(census.counts)


def lstm_step(n):
    """(sha256 of h, c, Q of one f32x3 step, the launch census)"""
    from rela_amd import _capi as capi
    from synth import synth_lstm_params
    from test_lstmnet_gpu import GpuLstmNet

    net = GpuLstmNet(synth_lstm_params(A, 43), A)
    capi.check(capi.lib.rela_lstmnet_set_precision(net.h, 2), "f32x3")
    rng = np.random.default_rng(n + 5)
    s = _frames(n, 9100 + n).numpy()
    legal = np.ones((n, A), np.float32)
    h_in = rng.normal(0, 0.3, (n, 512)).astype(np.float32)
    c_in = rng.normal(0, 0.5, (n, 512)).astype(np.float32)
    with capi.launch_census() as census:
        h, c, q, _ = net.step(s, legal, h_in, c_in)
    net.close()
    assert np.isfinite(h).all() and np.isfinite(c).all() and np.isfinite(q).all()
    return _sha(h, c, q), set(census.counts)


def compute():
    out = {}
    for n in FF_ROWS:
        out["ffnet_q_%d" % n] = ffnet_q(n)[0]
    for n in LSTM_ROWS:
        out["lstm_step_%d" % n] = lstm_step(n)[0]
    return out


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("n", FF_ROWS)
def test_ffnet_q_bits_equal_parent(n):
    from kernel_names import X3_FFNET

    sha, ran = ffnet_q(n)
    assert X3_FFNET <= ran, sorted(ran)
    assert ("fc_reduce" in ran) == (n == 512), sorted(ran)  # both sides of plan()'s split-K rule (it splits up to 768 rows)
    assert sha == _golden()["sha256"]["ffnet_q_%d" % n]


@pytest.mark.parametrize("n", LSTM_ROWS)
def test_lstm_step_bits_equal_parent(n):
    from kernel_names import X3_LSTM

    sha, ran = lstm_step(n)
    assert X3_LSTM <= ran, sorted(ran)
    assert sha == _golden()["sha256"]["lstm_step_%d" % n]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    assert first == second, "the forward is not reproducible run to run"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "sha256 of the little-endian f32 outputs of the f32x3 forward (tests/test_gemm_s3_bits_gpu.py)",
           "sha256": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc))
