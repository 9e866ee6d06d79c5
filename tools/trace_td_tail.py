#!/usr/bin/env python3
"""The insert tail of an Ape-X tick in a rocprofv3 --kernel-trace CSV of the bench, by kernel.

Beside tools/trace_insert_tail.py (interval and idle time from the TD kernel's end to the next tick's first conv12_s3),
for the ticks of the middle half of the trace:
  * the TD kernel's own time (td_kernel<false>, or td_kernel<true> where the fused insert's mode 3 runs);
  * the kernels that START inside that interval, by name: launches per tick and median time of a launch.
python tools/trace_td_tail.py <kernel_trace.csv>"""
import csv
import statistics as st
import sys

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
name = lambda r: r[2].replace("(anonymous namespace)::", "").replace("rela_amd::", "").replace("void ", "").split("(")[0]  # noqa: E731
tds = [i for i, r in enumerate(rows) if "td_kernel" in r[2]]
if len(tds) < 8:
    sys.exit("fewer than 8 td_kernel launches in the trace")
tds = tds[len(tds) // 4:3 * len(tds) // 4]
us = lambda v: "%.1f" % (v / 1e3)  # noqa: E731
inside = {}
ticks = 0
for i in tds:
    t_end = rows[i][1]
    nxt = next((j for j in range(i + 1, len(rows)) if "conv12_s3" in rows[j][2] and rows[j][0] >= t_end), None)
    if nxt is None:
        break
    ticks += 1
    for r in rows[i + 1:nxt]:
        if t_end <= r[0] < rows[nxt][0]:
            inside.setdefault(name(r)[:60], []).append(r[1] - r[0])
d = [rows[i][1] - rows[i][0] for i in tds]
print("%s: %d launches, median %s us (min %s, max %s)" % (sorted(set(name(rows[i]) for i in tds)), len(d), us(st.median(d)),
                                                         us(min(d)), us(max(d))))
print("kernels that start between the TD kernel's end and the next conv12_s3, over %d ticks:" % ticks)
for k, v in sorted(inside.items(), key=lambda kv: -len(kv[1])):
    print("  %-60s %.2f per tick, median %s us" % (k, len(v) / ticks, us(st.median(v))))
