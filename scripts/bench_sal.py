"""Device time of the SAL records (sal.py): plane_records on 100 scenarios of one 256 x 256 day at 4 thresholds, beside
CellStructure.add on the same array and thresholds in the same run -- the cost of label + merge + resolve + reduce, the pass the
SAL kernels sit on -- with their ratio and the split by kernel.  Prints one JSON line.

    python scripts/bench_sal.py [--reps 10] [--warmup 3]

Synthetic seeded spells made on the device (as scripts/bench_extremes.py makes them).  Times are HIP events around the whole call,
allocation of outputs and workspace included, median of 10 after 3 warm-up calls (--reps / --warmup), one process.  The split is
the device time of every kernel of one further call of each, from the profiler's kernel records; null where the profiler gives
none."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import cells as CL, sal as SL

THRESHOLDS = (0.1, 1.0, 5.0, 10.0)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def rain(n, ny, nx, dry, seed):
    """spells: an hour is wet where a noise field smoothed over 4 hours and 3 x 3 pixels is high, so that wet pixels come in areas"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (n, 24, ny, nx)
    u = torch.rand(shape, generator=g, device="cuda")
    u = (u + u.roll(1, 1) + u.roll(2, 1) + u.roll(3, 1)) / 4
    u = torch.nn.functional.avg_pool2d(u.view(n * 24, 1, ny, nx), 3, 1, 1).view(shape)
    wet = u > torch.quantile(u.flatten()[:1 << 20], dry)
    return -4.0 * torch.log1p(-torch.rand(shape, generator=g, device="cuda")) * wet


def kernel_split(fn):
    """{kernel name: ms} of one call, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            if t and ev.key.startswith(("k_", "void k_")):
                out[ev.key.split("(")[0].replace("void ", "")] = t / 1000.0
        return out or None
    except Exception as e:                                           # the numbers above do not depend on the profiler
        print(f"kernel split unavailable: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n, ny, nx = 100, 256, 256
    x = rain(n, ny, nx, 0.8, 1)
    sal_call = lambda: SL.plane_records(x, THRESHOLDS)
    cells_call = lambda: CL.CellStructure(THRESHOLDS).add(x)
    ms_sal, rec = timed(sal_call, a.reps, a.warmup)
    ms_cells, cs = timed(cells_call, a.reps, a.warmup)
    stats = cs.result()
    assert np.array_equal(rec.n_objects.sum(dim=(0, 1)).cpu().numpy(), stats.cells.sum(axis=(1, 2)))       # the same objects
    res = {"scenarios": n, "plane": [ny, nx], "thresholds": list(THRESHOLDS), "read_bytes": 4 * 24 * n * ny * nx,
           "objects_per_threshold": stats.cells.sum(axis=(1, 2)).tolist(), "wet_fraction": (stats.wet_pixels.sum(axis=1) / (24 * n * ny * nx)).tolist(),
           "plane_records_ms": ms_sal, "cells_add_ms": ms_cells, "ratio": ms_sal / ms_cells,
           "plane_records_kernels_ms": kernel_split(sal_call), "cells_add_kernels_ms": kernel_split(cells_call)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
