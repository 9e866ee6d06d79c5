#!/usr/bin/env python3
"""The end of an Ape-X tick in a rocprofv3 --kernel-trace CSV of the bench: where the insert's row copies run.

Per tick (one td_kernel each), over the ticks of the middle half of the trace:
  * the replay_scatter_rows launches between this tick's td_kernel and the next tick's first conv12_s3 (any variant):
    how many, how long each, how much of each runs with NO other kernel on the GPU (exposed) and how much under others;
  * the interval from td_kernel's end to the next conv12_s3's start, and the GPU-idle time inside it;
  * the kernels that overlap the copies, by name;
  * the per-launch time of conv12_s3<false> and conv12_s3_copy at the tick's grid.
python tools/trace_insert_tail.py <kernel_trace.csv>"""
import csv
import statistics as st
import sys

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
name = lambda r: r[2].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]  # noqa: E731
tds = [i for i, r in enumerate(rows) if "td_kernel" in r[2]]
if len(tds) < 8:
    sys.exit("fewer than 8 td_kernel launches in the trace")
tds = tds[len(tds) // 4:3 * len(tds) // 4]


def union(iv):
    """total length of the union of intervals"""
    tot, end = 0, None
    for s, e in sorted(iv):
        if end is None or s > end:
            tot += e - s
            end = e
        elif e > end:
            tot += e - end
            end = e
    return tot


per_tick = []
overlappers = {}
for i in tds:
    t_end = rows[i][1]
    nxt = next((j for j in range(i + 1, len(rows)) if "conv12_s3" in rows[j][2] and rows[j][0] >= t_end), None)
    if nxt is None:
        break
    c_start = rows[nxt][0]
    win = [r for r in rows if r[1] > t_end and r[0] < c_start]
    sc = [r for r in win if "replay_scatter_rows" in r[2] and r[0] >= t_end]
    exposed, under, dur = [], [], []
    for s in sc:
        others = [(max(o[0], s[0]), min(o[1], s[1])) for o in rows if o is not s and o[1] > s[0] and o[0] < s[1]]
        for o in rows:
            if o is not s and o[1] > s[0] and o[0] < s[1]:
                overlappers[name(o)[:50]] = overlappers.get(name(o)[:50], 0) + min(o[1], s[1]) - max(o[0], s[0])
        u = union(others)
        dur.append(s[1] - s[0])
        under.append(u)
        exposed.append(s[1] - s[0] - u)
    busy = union([(max(r[0], t_end), min(r[1], c_start)) for r in win])
    per_tick.append(dict(n=len(sc), dur=sum(dur), exposed=sum(exposed), under=sum(under), tail=c_start - t_end,
                         idle=c_start - t_end - busy))
us = lambda v: "%.1f" % (v / 1e3)  # noqa: E731
med = lambda k: st.median(t[k] for t in per_tick)  # noqa: E731
print("%d ticks; replay_scatter_rows launches per tick between td_kernel and the next conv12_s3: %s" % (
    len(per_tick), sorted(set(t["n"] for t in per_tick))))
print("per tick, median us: copies %s (exposed %s, under other kernels %s) | td_kernel end -> next conv12_s3 start %s "
      "(GPU idle inside %s)" % (us(med("dur")), us(med("exposed")), us(med("under")), us(med("tail")), us(med("idle"))))
print("per tick, min .. max us: exposed %s .. %s | tail %s .. %s" % (
    us(min(t["exposed"] for t in per_tick)), us(max(t["exposed"] for t in per_tick)), us(min(t["tail"] for t in per_tick)),
    us(max(t["tail"] for t in per_tick))))
print("kernels overlapping the copies, us per tick:")
for k, v in sorted(overlappers.items(), key=lambda kv: -kv[1])[:8]:
    print("  %-50s %s" % (k, us(v / len(per_tick))))
lo, hi = rows[tds[0]][0], rows[tds[-1]][1]
for key in ("conv12_s3<false>", "conv12_s3_copy", "conv12_s3_copies2"):  # (the last: the kernel labelled conv12_s3_copy2)
    d = [r[1] - r[0] for r in rows if key in r[2] and lo <= r[0] <= hi]
    d = [x for x in d if x > 0.5 * max(d)] if d else d  # (the tick's grid, not the learner's smaller batches)
    if d:
        print("%-18s %d launches, median %s us (min %s, max %s)" % (key, len(d), us(st.median(d)), us(min(d)), us(max(d))))
