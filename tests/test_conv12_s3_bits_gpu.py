"""conv12_s3 (csrc/conv12_s3.h, conv1 -> conv2 of the f32x3 trunk) yields the SAME BITS as the kernel it replaced.

A rewrite of the kernel's register use, addressing or staging keeps, per output element, the three i8 digit sums, the
two-fma scale and bias, split3_4 and the six-product order of acc / accs with their acc + accs, so a2's records, a1_out
and everything behind them must come out bit for bit.  The fixture tests/golden/conv12_s3_parent_bits.json holds the
sha256 of the outputs below, recorded on an MI355X from a checkout of the commit named in it (the parent of the change),
with this file's `compute()`.

The sizes come from how the kernel can go wrong, not from the workload: a block walks the frames b, b + grid, ... and
its last round re-stages its own frame.  512 rows is the smallest batch that takes this path (kEmuConvMinN); at 513 and
769 rows only some blocks run a second / a third round, so both the clamp of the staged frame and the copy-out of the
previous tile under the next frame's conv1 are exercised on some blocks and not on others.  For each size:

  * Q [n][A] of the f32x3 forward (conv12_s3<false>);
  * a1 [n][400][32] and a2 [n][81][64] of the learner's online(obs) pass, the keep-f32 forward mode
    (kModeF32x3KeepF32: conv12_s3<true> writes a1_out, a2 is its records turned back into f32), read through
    HipApexLearner.debug_activations().  The batch keeps s' in FRONT of s in memory so that the learner never merges the
    two online forwards: the keep-f32 launch has exactly n rows.

Inputs are seeded (tests/synth.py), so they are the same everywhere.  Each case asserts through the launch census that
conv12_s3 really ran.

Re-recording (only ever from the commit BEFORE a change to the kernel):
    python tests/test_conv12_s3_bits_gpu.py OUT.json COMMIT
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
FIXTURE = os.path.join(HERE, "golden", "conv12_s3_parent_bits.json")
A = 18
ROWS = (512, 513, 769)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, "<f4").tobytes()).hexdigest()


def ffnet_q(n):
    """(sha256 of Q [n][A] of the f32x3 forward, the launch census)"""
    import torch

    from rela_amd import _capi as capi
    from rela_amd.engine import FFNetHandle
    from synth import synth_obs, synth_params

    net = FFNetHandle(A, "cuda:0")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_params(A, 51).items()})
    net.set_precision("f32x3")
    s = torch.from_numpy(synth_obs(n, 7000 + n)).cuda()
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
    return _sha(out), dict(census.counts)


def learner_a1_a2(n):
    """(sha256 of a1, sha256 of a2 of the f32x3 learner's online(obs) pass over n rows, the launch census)"""
    import torch
    from types import SimpleNamespace

    from rela_amd import _capi as capi
    from rela_amd.learner import HipApexLearner
    from synth import synth_obs, synth_params

    dev = "cuda:0"
    sd_on = {k: torch.from_numpy(v) for k, v in synth_params(A, 52).items()}
    sd_tg = {k: torch.from_numpy(v) for k, v in synth_params(A, 53).items()}
    learner = HipApexLearner(A, n, 3, 0.99, device=dev)
    learner.load_state_dicts(sd_on, sd_tg)
    learner.set_precision("f32x3")
    # [s' ; s] in one tensor each: s' is never right behind s, so online(s) stays a launch of its own
    frames = torch.from_numpy(synth_obs(2 * n, 7100 + n)).reshape(2, n, 4, 84, 84).to(dev)
    moves = torch.ones((2, n, A), device=dev)
    rng = np.random.default_rng(7200 + n)
    to = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    batch = SimpleNamespace(obs={"s": frames[1], "eps": torch.zeros(n, 1, device=dev), "legal_move": moves[1]},
                            next_obs={"s": frames[0], "eps": torch.zeros(n, 1, device=dev), "legal_move": moves[0]},
                            action={"a": to(rng.integers(0, A, n).astype(np.int64))},
                            reward=to(rng.normal(0, 0.7, n).astype(np.float32)),
                            terminal=torch.zeros(n, dtype=torch.bool, device=dev), bootstrap=torch.ones(n, device=dev))
    w = torch.ones(n, device=dev)
    with capi.launch_census() as census:
        learner.loss(batch, w)
        torch.cuda.synchronize()
    a1, a2 = learner.debug_activations()[:2]
    assert tuple(a1.shape) == (n, 400, 32) and tuple(a2.shape) == (n, 81, 64)
    a1, a2 = a1.cpu().numpy(), a2.cpu().numpy()
    learner.close()
    assert np.isfinite(a1).all() and np.isfinite(a2).all()
    assert (a1 > 0).mean() > 0.05 and (a2 > 0).mean() > 0.05  # (real activations, not a cleared buffer)
    return _sha(a1), _sha(a2), dict(census.counts)


def compute():
    out = {}
    for n in ROWS:
        out["ffnet_q_%d" % n] = ffnet_q(n)[0]
        out["learner_a1_%d" % n], out["learner_a2_%d" % n] = learner_a1_a2(n)[:2]
    return out


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)["sha256"]


@pytest.mark.parametrize("n", ROWS)
def test_ffnet_q_bits_equal_parent(n):
    from kernel_names import X3_FFNET

    sha, ran = ffnet_q(n)
    assert X3_FFNET <= set(ran), sorted(ran)
    assert ran["conv12_s3"] == 1, ran
    assert sha == _golden()["ffnet_q_%d" % n]


@pytest.mark.parametrize("n", ROWS)
def test_keep_f32_a1_a2_bits_equal_parent(n):
    from kernel_names import X3_FFNET

    a1, a2, ran = learner_a1_a2(n)
    # three launches of n rows each: online(s'), target(s'), online(s) keeping f32 -- not one merged 2 n-row launch
    assert X3_FFNET <= set(ran) and ran["conv12_s3"] == 3 and "unsplit_s3" in ran, ran
    assert a1 == _golden()["learner_a1_%d" % n]
    assert a2 == _golden()["learner_a2_%d" % n]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    first, second = compute(), compute()
    assert first == second, "the forward is not reproducible run to run"
    doc = {"recorded_from_commit": sys.argv[2] if len(sys.argv) > 2 else "unknown",
           "what": "sha256 of the little-endian f32 outputs of the f32x3 forward and of the keep-f32 learner pass "
                   "(tests/test_conv12_s3_bits_gpu.py)",
           "sha256": first}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc))
