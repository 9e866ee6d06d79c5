#!/usr/bin/env python3
"""What --target_tau costs per step: soft_update_target against sync_target_with_online for both HIP learners at A = 18
(the lerp or the copy over the flat buffer, then the same target re-pack).  A call is a handful of short launches, so one
event pair brackets a batch of CALLS back-to-back calls and the time is divided by CALLS: the stream stays fed and the figure
is the call's time on the stream (device time plus whatever launch gaps remain between its kernels), not the host's
launch latency.  Batches of the two calls alternate, so both see the same clocks and neighbours; medians over the batches.

  REPEATS=100 CALLS=20 python tools/time_target_update.py      -> one JSON line
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from rela_amd.learner import HipApexLearner, HipR2D2Learner
from synth import synth_lstm_params, synth_params

A, TAU = 18, 0.005
REPEATS, CALLS = int(os.environ.get("REPEATS", "100")), int(os.environ.get("CALLS", "20"))


def timed(fn):
    """us per call over one batch"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / CALLS


out = {"A": A, "batches": REPEATS, "calls_per_batch": CALLS, "tau": TAU}
# (neither call depends on the batch or the sequence shape: small ones keep the learners' other buffers small)
for name, learner, params in (("apex", HipApexLearner(A, 32, 3, 0.997), synth_params(A, 1)),
                              ("r2d2", HipR2D2Learner(A, 8, 3, 0.997, 8, 4, 0.9), synth_lstm_params(A, 2))):
    learner.load_state_dicts({k: torch.from_numpy(v).cuda() for k, v in params.items()})
    calls = {"soft_update_target": lambda: learner.soft_update_target(TAU), "sync_target": learner.sync_target_with_online}
    for fn in calls.values():  # warm-up of both
        timed(fn)
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, fn in calls.items():
            us[k].append(timed(fn))
    out[name] = {"floats": int(learner.flat()[0].numel()),
                 **{k + "_us": round(statistics.median(v), 1) for k, v in us.items()},
                 **{k + "_us_p10_p90": [round(sorted(v)[len(v) // 10], 1), round(sorted(v)[len(v) * 9 // 10], 1)]
                    for k, v in us.items()}}
    learner.close()
print(json.dumps(out))
