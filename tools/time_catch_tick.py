"""The Ape-X actor tick at the benchmark's shapes (6,400 rows, K = 80, A = 18, n = 3, f32x3, replay 2^18 filled first, the
adds non-blocking, no learner): with the device Catch env (act, catch_step, post_step, catch_render) against the same
engine ticking on a resident observation with pooled rewards (bench.py's actor tick), alternated in one process; one
JSON line (profiles/catch_env_timing.md)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rela_amd.device_env import DeviceCatchEnv  # noqa: E402
from rela_amd.engine import ApexActorEngine, FFNetHandle  # noqa: E402
from rela_amd.pyrela.net import AtariFFNet  # noqa: E402
from rela_amd.pyrela.utils import generate_eps  # noqa: E402
from rela_amd.replay import FFReplay  # noqa: E402

ROWS, K, A, n, CAP, SEED = 6400, 80, 18, 3, 1 << 18, 10002
STEPS, PASSES = 300, 3
dev = "cuda:0"
torch.manual_seed(SEED + 2)
net_on, net_tg = AtariFFNet(A).to(dev), AtariFFNet(A).to(dev)
online, target = FFNetHandle(A, dev), FFNetHandle(A, dev)
online.load_state_dict(net_on.state_dict())
target.load_state_dict(net_tg.state_dict())
online.set_precision("f32x3")
target.set_precision("f32x3")


def make(with_env):
    replay = FFReplay(CAP, SEED, 0.6, 0.4, 0, A, dev, guard_units=(n + 8) * ROWS)
    eng = ApexActorEngine(ROWS, K, A, n, 0.997, replay, generate_eps(0.4, 7, ROWS), dev, seed=SEED)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED + 7)
    env = None
    if with_env:
        env = DeviceCatchEnv(ROWS, A, 200, SEED, dev)
        env.reset(eng.next_obs_slot())
    else:
        for h in range(n + 1):
            eng.obs_hist[h].copy_(torch.randint(0, 256, eng.obs_hist[h].shape, dtype=torch.uint8, device=dev, generator=g))
    rew = torch.randint(-1, 2, (16, ROWS), device=dev, generator=g).float()
    term = (torch.rand((16, ROWS), device=dev, generator=g) < 0.005).to(torch.uint8)
    i = [0]

    def tick():
        action = eng.act(online)
        if env is not None:
            r, t = env.step(action)
            eng.post_step(r, t, online, target, nonblocking=True)
            env.render(eng.next_obs_slot())
        else:
            eng.post_step(rew[i[0] % 16], term[i[0] % 16], online, target, nonblocking=True)
        i[0] += 1

    for _ in range(n + 1):
        tick()
    prio = torch.empty(ROWS, device=dev)
    z_a = torch.zeros(ROWS, dtype=torch.int64, device=dev)
    z_f = torch.zeros(ROWS, device=dev)
    z_b = torch.zeros(ROWS, dtype=torch.uint8, device=dev)
    while replay.size() + ROWS <= CAP:  # bulk inserts, as bench.py fills its ring
        prio.uniform_(0.01, 2.0, generator=g)
        a, b = eng.obs_hist[0], eng.obs_hist[1]
        replay.add_rows(ROWS, [a.data_ptr(), b.data_ptr(), eng.eps.data_ptr(), eng.eps.data_ptr(), eng.legal.data_ptr(),
                               eng.legal.data_ptr(), z_a.data_ptr(), z_f.data_ptr(), z_b.data_ptr(), z_f.data_ptr()], prio)
    torch.cuda.synchronize()
    return tick, eng, replay, env


def bracket(tick, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        tick()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


stream = torch.cuda.Stream(device=dev)
with torch.cuda.stream(stream):
    tick_env, eng_e, rp_e, env = make(True)
    tick_res, eng_r, rp_r, _ = make(False)
    for _ in range(60):  # both rings run full here: from now on every block is dropped, as in bench.py's actor-only mode
        tick_env()
        tick_res()
    out = {"rows": ROWS, "steps": STEPS, "with_env_ms": [], "resident_ms": []}
    for _ in range(PASSES):
        out["resident_ms"].append(bracket(tick_res, STEPS))
        out["with_env_ms"].append(bracket(tick_env, STEPS))
out["resident_median_ms"] = float(np.median(out["resident_ms"]))
out["with_env_median_ms"] = float(np.median(out["with_env_ms"]))
out["env_cost_ms"] = out["with_env_median_ms"] - out["resident_median_ms"]
out["with_env_env_steps_per_s"] = ROWS / out["with_env_median_ms"] * 1e3
out["resident_env_steps_per_s"] = ROWS / out["resident_median_ms"] * 1e3
out["catch_episodes"] = env.episode_stats()["episodes"]
print(json.dumps(out))
