"""Times rela_atari_features (csrc/atari_screen.hip) alone: `rows` screen pairs of H x W -> 84x84 features, one launch.

    python tools/time_screen_features.py [--rows 2400,6400] [--height 210] [--width 160] [--iters 50] [--indexed]

--indexed times rela_atari_features_indexed instead: palette indices (a third of the screen bytes) and one 768-byte
palette per row, which counts as traffic.

Prints one JSON line per row count: the median and minimum kernel time (HIP events around `iters` back-to-back launches
on one stream, after warm-up), the bytes the kernel must move (the source rows the 84 output rows interpolate between,
of both screens, plus the 7,056 B written per row) and that traffic over the HBM peak (MI355X: 8 TB/s).
The screens are uniform noise; the kernel does the same work for any content."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rela_amd import _capi as capi  # noqa: E402

HBM_PEAK = 8.0e12  # B/s


def source_rows(H):
    """distinct source rows the 84 output rows read (align_corners bilinear, float32 as csrc/atari_screen.h)"""
    scale = np.float32(H - 1) / np.float32(83)
    src = scale * np.arange(84, dtype=np.float32)
    i0 = np.minimum(src.astype(np.int64), H - 1)
    i1 = np.minimum(i0 + 1, H - 1)
    return len(set(i0.tolist()) | set(i1.tolist()))


def time_rows(rows, H, W, iters, dev="cuda:0", indexed=False):
    g = torch.Generator(device=dev)
    g.manual_seed(rows)
    ch = 1 if indexed else 3
    scr = torch.randint(0, 256, (rows, 2, H, W, ch), dtype=torch.uint8, device=dev, generator=g)
    out = torch.empty((rows, 84, 84), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)
    if indexed:
        pal = torch.randint(0, 256, (rows, 256, 3), dtype=torch.uint8, device=dev, generator=g)
        fn, name = capi.lib.rela_atari_features_indexed, "rela_atari_features_indexed"
        args = (C.c_void_p(scr.data_ptr()), C.c_void_p(pal.data_ptr()), rows, H, W, C.c_void_p(out.data_ptr()), s)
    else:
        fn, name = capi.lib.rela_atari_features, "rela_atari_features"
        args = (C.c_void_p(scr.data_ptr()), rows, H, W, C.c_void_p(out.data_ptr()), s)
    for _ in range(5):
        capi.check(fn(*args), name)
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        capi.check(fn(*args), name)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    nbytes = rows * (2 * source_rows(H) * W * ch + (768 if indexed else 0) + 84 * 84)
    med = float(np.median(ms)) * 1e3
    return dict(kernel="atari_features_indexed" if indexed else "atari_features", rows=rows, height=H, width=W, iters=iters, median_us=round(med, 2), min_us=round(min(ms) * 1e3, 2),
                bytes=nbytes, achieved_GBps=round(nbytes / (med * 1e-6) / 1e9, 1),
                roofline_us=round(nbytes / HBM_PEAK * 1e6, 2), fraction_of_roofline=round(nbytes / HBM_PEAK * 1e6 / med, 3))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="2400,6400")
    p.add_argument("--height", type=int, default=210)
    p.add_argument("--width", type=int, default=160)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--indexed", action="store_true", help="time rela_atari_features_indexed (palette indices)")
    a = p.parse_args()
    for r in (int(v) for v in a.rows.split(",")):
        print(json.dumps(time_rows(r, a.height, a.width, a.iters, indexed=a.indexed)), flush=True)


if __name__ == "__main__":
    main()
