"""catch_step_render and its two halves alone at 6,400 rows, next to a fill of the same bytes: device events around every
launch and a back-to-back average, one JSON line.  For kernel times run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_catch_env.py
(profiles/catch_env_timing.md)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rela_amd.device_env import DeviceCatchEnv  # noqa: E402

ROWS, A, N = 6400, 18, 300
dev = "cuda:0"
env = DeviceCatchEnv(ROWS, A, 200, 10002, dev)
slot = torch.empty((ROWS, 4, 84, 84), dtype=torch.uint8, device=dev)
g = torch.Generator(device=dev)
g.manual_seed(1)
actions = [torch.randint(0, A, (ROWS,), device=dev, generator=g) for _ in range(16)]
env.reset(slot)


def timed(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(20):
        fn(i)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(n):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return {"median_us": float(np.median(us)), "min_us": float(us.min()), "p90_us": float(np.percentile(us, 90)),
            "back_to_back_us": t0.elapsed_time(t1) * 1e3 / n}


out = {"rows": ROWS, "bytes_per_launch": ROWS * 28224}
out["catch_step_render"] = timed(lambda i: env.step(actions[i % 16], slot), N)
out["catch_step"] = timed(lambda i: env.step(actions[i % 16]), N)
out["catch_render"] = timed(lambda i: env.render(slot), N)
out["memset_same_bytes"] = timed(lambda i: slot.zero_(), N)
for k in ("catch_step_render", "catch_render", "memset_same_bytes"):
    out[k]["TB_per_s_median"] = out["bytes_per_launch"] / out[k]["median_us"] * 1e-6
    out[k]["TB_per_s_back_to_back"] = out["bytes_per_launch"] / out[k]["back_to_back_us"] * 1e-6
st = env.episode_stats()
out["episodes"] = st["episodes"]
print(json.dumps(out))
