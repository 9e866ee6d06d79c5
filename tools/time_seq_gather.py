#!/usr/bin/env python3
"""Sample time of the sequence replay (RNNReplay, BASELINE C4's window: seq 80 / burn-in 40 / n 3, T = 123) with the
stacks stored in full and de-duplicated (rela_replay_set_schema_seq_dedup, "stack" and "plane" units), B = 64.
Three replays of capacity CAP are filled by R2D2 actor shards of 256 envs with the same sliding-stack stream; then
each runs ITERS rounds of sample + update_priority, timed with HIP events around sample().  Run it under
`rocprofv3 --kernel-trace --stats` for the gather kernels alone (replay_gather_big: full storage;
replay_gather_seq_dedup: de-duplicated).

  ITERS=200 python tools/time_seq_gather.py      -> one JSON line
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from rela_amd.engine import LSTMNetHandle, R2D2ActorEngine
from rela_amd.replay import RNNReplay
from synth import synth_lstm_params

ITERS, B = int(os.environ.get("ITERS", "200")), int(os.environ.get("BATCH", "64"))
CAP = int(os.environ.get("CAP", "4096"))
R, K, A, n, seq, burn = 256, 64, 18, 3, 80, 40
T = burn + seq + n
dev = "cuda:0"
nets = []
for seed in (1, 2):
    h = LSTMNetHandle(A, dev)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth_lstm_params(A, seed).items()})
    h.set_precision("bf16x2")
    nets.append(h)
on, tg = nets
modes = (None, "stack", "plane")
reps, engs = [], []
for mode in modes:
    rp = RNNReplay(CAP, 7, 0.6, 0.4, 0, A, T, dev, dedup=mode, guard_units=(2 * T + n + 10) * R, units_per_slot=seq + n)
    reps.append(rp)
    engs.append(R2D2ActorEngine(R, K, A, n, 0.997, seq, burn, 0.9, rp, [0.0] * R, dev))
rows = torch.arange(R, device=dev, dtype=torch.int32)
px = torch.arange(84 * 84, device=dev, dtype=torch.int32)
rng = np.random.default_rng(1)
stack, t = None, 0
zeros_r = np.zeros(R, np.float32)
term = np.zeros(R, np.uint8)
while reps[0].size() < CAP:
    p = ((rows[:, None] * 7919 + t * 104729 + px[None, :] * 31) % 251).to(torch.uint8).reshape(R, 84, 84)
    fresh = p[:, None].expand(R, 4, 84, 84)
    if stack is None:
        stack = fresh.clone()
    else:  # slide by one plane; an episode starts with its first plane four times (atari/game_state.h:53-82)
        restart = torch.from_numpy(term.astype(bool)).to(dev)[:, None, None, None]
        stack = torch.where(restart, fresh, torch.cat([stack[:, 1:], p[:, None]], 1))
    term = (rng.uniform(size=R) < 0.003).astype(np.uint8)
    for eng in engs:
        eng.next_obs_slot().copy_(stack)
        eng.act(on)
        eng.post_step(zeros_r, term, on, tg)
    t += 1
torch.cuda.synchronize()
out = {"batch": B, "T": T, "capacity": CAP, "iters": ITERS, "ticks_filled": t}
ref = None
for mode, rp in zip(modes, reps):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for i in range(10 + ITERS):
        e = evs[i - 10] if i >= 10 else None
        if e:
            e[0].record()
        b, w = rp.sample(B)
        if e:
            e[1].record()
        rp.update_priority(torch.linspace(0.5, 1.5, B, device=dev))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(z) for a, z in evs)
    out["sample_ms_%s" % (mode or "full")] = {"median": ms[len(ms) // 2], "mean": sum(ms) / len(ms), "min": ms[0]}
    s = b.obs["s"].clone()
    if ref is None:
        ref = s
    out["same_last_batch_%s" % (mode or "full")] = bool(torch.equal(ref, s))
print(json.dumps(out))
