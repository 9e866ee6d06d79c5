#!/usr/bin/env python3
"""Per-kernel HIP-event timings of the isolated R2D2 learner step at C4's shape (B = 64, seq 80 / burn 40 / n 3).

  ITERS=10 [PRECISION=bf16x2] [DGRAD=x3] [WGRAD=x3|x3_all] [LSTM_IN=rec3] python tools/time_r2d2_learner.py   -> one line: kernel -> ms per step
  LSTM_IN_AB=5 ITERS=20 PRECISION=f32x3_bwd DGRAD=x3 python tools/time_r2d2_learner.py
      -> lstm_in_rec3 off and on alternated in this one process, LSTM_IN_AB pairs: per leg the whole step (device events,
         profiler off) and, from a second window with the profiler on, the LSTM input backward's scopes; then
         median [min .. max] of both per leg (profiles/lstm_in_rec3_ab.md)
  WGRAD3_AB=7 ITERS=4 PRECISION=f32x3_bwd DGRAD=x3 WGRAD=x3 LSTM_IN=rec3 python tools/time_r2d2_learner.py
      -> the same for wgrad3_x3 and the learner_wgrad_conv3 scope (profiles/wgrad3_x3_ab.md)
  REC_WIDE_AB=5 ITERS=10 B=128 python tools/time_r2d2_learner.py
      -> the same for rec_wide and the forward recurrence's scopes (per-step: learner_lstm_rec_fwd + learner_lstm_cell, the
         two zeroing launches have no scope; wide: learner_lstm_rec_wide), after three legs of the same learner at B = 64
         on lstm_rec_chain (profiles/rec_wide_ab.md)
  REC_WIDE256_AB=7 ITERS=10 B=256 python tools/time_r2d2_learner.py
      -> the same for rec_wide256 (on: learner_lstm_rec_wide256), without the legs at B = 64 (profiles/rec_wide256_ab.md)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from rela_amd import _capi as capi
from rela_amd.learner import HipR2D2Learner
from test_r2d2_learner_gpu import _agent, _random_batch

A, B, SEQ, BURN, N = 18, int(os.environ.get("B", "64")), 80, 40, 3
ITERS = int(os.environ.get("ITERS", "10"))
rng = np.random.default_rng(5)
agent = _agent(A, N, 0.997, 0.9, SEQ, BURN, 71, 72, "cuda:0")
batch, weight = _random_batch(rng, A, B, SEQ, BURN, N, "cuda:0")
learner = HipR2D2Learner.from_agent(agent, B)
learner.set_precision(os.environ.get("PRECISION", "f32"))
if os.environ.get("DGRAD") == "x3":
    learner.set_dgrad_x3(True)
if os.environ.get("WGRAD") in ("x3", "x3_all"):
    learner.set_wgrad_x3(True)
if os.environ.get("WGRAD") == "x3_all":
    learner.set_wgrad3_x3(True)
if os.environ.get("LSTM_IN") == "rec3":
    learner.set_lstm_in_rec3(True)

# the scopes of lstm_input_backward's GEMM path, and the W_ih^T record refresh of every step (the weights move every step)
LSTM_IN_SCOPES = ("learner_lstm_split_cols", "learner_wgrad_lstm_ih", "learner_wgrad_lstm_hh", "learner_lstm_split_rows",
                  "learner_dgrad_lstm_ih", "learner_lstm_split_w")


def window(profile):
    """ITERS steps -> (ms per step by device events, {scope: ms per step} if profile)"""
    capi.lib.rela_prof_enable(int(profile))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(ITERS):
        learner.step(batch, weight)
    t1.record()
    learner.check()
    capi.lib.rela_prof_enable(0)
    buf = C.create_string_buffer(1 << 16)
    capi.check(capi.lib.rela_prof_summary_json(buf, len(buf)), "prof")
    return t0.elapsed_time(t1) / ITERS, {k: v["total_ms"] / ITERS for k, v in json.loads(buf.value.decode()).items()}


def alternate(pairs, name, setter, scopes, what):
    """`name` off and on alternated, `pairs` pairs: per leg the whole step and the sum of `scopes`, then the medians"""
    legs = {0: [], 1: []}
    for pair in range(pairs):
        for on in (0, 1):
            setter(bool(on))
            for _ in range(3):
                learner.step(batch, weight)
            learner.check()
            step_ms, _ = window(False)
            _, prof = window(True)
            picked = {k: round(prof.get(k, 0.0), 4) for k in scopes}
            legs[on].append((step_ms, sum(picked.values())))
            print("pair %d %s %d step %.3f ms  %s %.3f ms  %s" % (pair, name, on, step_ms, what, sum(picked.values()), picked),
                  flush=True)
    for on in (0, 1):
        for label, col in (("whole step", 0), (what + " scopes", 1)):
            v = sorted(x[col] for x in legs[on])
            print("%s %d %-27s median %.3f [%.3f .. %.3f] ms" % (name, on, label, v[len(v) // 2], v[0], v[-1]), flush=True)
    sys.exit(0)


if os.environ.get("LSTM_IN_AB"):
    alternate(int(os.environ["LSTM_IN_AB"]), "lstm_in_rec3", learner.set_lstm_in_rec3, LSTM_IN_SCOPES, "lstm input backward")
if os.environ.get("WGRAD3_AB"):
    alternate(int(os.environ["WGRAD3_AB"]), "wgrad3_x3", learner.set_wgrad3_x3, ("learner_wgrad_conv3",), "conv3 weight gradient")

if os.environ.get("REC_WIDE_AB"):  # (B=128: the option concerns 65 .. 128 rows)
    if B > 64:  # for comparison, the same learner's step at 64 rows on lstm_rec_chain
        wide_batch = (batch, weight)
        batch, weight = _random_batch(np.random.default_rng(6), A, 64, SEQ, BURN, N, "cuda:0")
        for _ in range(3):
            learner.step(batch, weight)
        learner.check()
        for leg in range(3):
            step_ms, _ = window(False)
            _, prof = window(True)
            print("B 64 leg %d step %.3f ms  learner_lstm_rec_persist %.3f ms" % (leg, step_ms, prof.get("learner_lstm_rec_persist", 0.0)),
                  flush=True)
        batch, weight = wide_batch
    alternate(int(os.environ["REC_WIDE_AB"]), "rec_wide", learner.set_rec_wide,
              ("learner_lstm_rec_fwd", "learner_lstm_cell", "learner_lstm_rec_wide"), "forward recurrence")
if os.environ.get("REC_WIDE256_AB"):  # (B=256: the option concerns 129 .. 256 rows)
    alternate(int(os.environ["REC_WIDE256_AB"]), "rec_wide256", learner.set_rec_wide256,
              ("learner_lstm_rec_fwd", "learner_lstm_cell", "learner_lstm_rec_wide256"), "forward recurrence")

for _ in range(2):
    learner.step(batch, weight)
learner.check()
torch.cuda.synchronize()
capi.lib.rela_prof_enable(1)
t0 = torch.cuda.Event(enable_timing=True)
t1 = torch.cuda.Event(enable_timing=True)
t0.record()
for _ in range(ITERS):
    learner.step(batch, weight)
t1.record()
learner.check()
capi.lib.rela_prof_enable(0)
buf = C.create_string_buffer(1 << 16)
capi.check(capi.lib.rela_prof_summary_json(buf, len(buf)), "prof")
prof = json.loads(buf.value.decode())
tab = {k: round(v["total_ms"] / ITERS, 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])}
print(os.environ.get("TAG", ""), "ms/step", round(t0.elapsed_time(t1) / ITERS, 3), "kernels", round(sum(tab.values()), 3), tab, flush=True)
