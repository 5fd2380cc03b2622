"""Device time of the distribution checks (distribution.py): (a) the KS statistic of 20 x 24 columns of 1 000 + 1 000 values in one
launch, against 480 single-column launches and against the host route (copy to the host + the numpy mirror's searchsorted);
(b) the box statistics of 4 x 24 columns of n = 10 000 (the daily cycle); (c) ecdf_on_grid at N = 61 440 000 for T = 512 and 4 096
thresholds as GB/s of the data read, against torch.sort of the same tensor.  Prints one JSON line.  Recorded, not asserted.

    python scripts/bench_distribution.py [--pixels 61440000] [--reps 10] [--warmup 3]

Synthetic seeded data with dry (zero) values.  Times are HIP events around the whole call (host work of the call included), median
of --reps after --warmup calls."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import distribution as D

HBM_ACHIEVABLE_GBS = 6290.0            # float4 copy on an MI355X (8 000 spec)


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


def host_ks(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    out = np.empty(a.shape[0] * a.shape[2])
    k = 0
    for bt in range(a.shape[0]):
        for c in range(a.shape[2]):
            x, y = np.sort(a[bt, :, c]), np.sort(b[bt, :, c])
            pooled = np.concatenate([x, y])
            out[k] = np.abs(np.searchsorted(x, pooled, side="right") / len(x) - np.searchsorted(y, pooled, side="right") / len(y)).max()
            k += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=61440000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)

    def fields(shape, dry=0.45):
        x = torch.empty(shape, dtype=torch.float32, device="cuda").exponential_(0.7, generator=g) ** 2
        x[torch.rand(shape, generator=g, device="cuda") < dry] = 0.0
        return x

    res = {"metric": "distribution", "reps": a.reps, "warmup": a.warmup}
    # (a) KS
    sa, sb = fields((20, 1000, 24)), fields((20, 1000, 24))
    ms_one, (counts, d) = timed(lambda: D.ks_statistic_device(sa, sb), a.reps, a.warmup)
    cols = [(sa[p, :, c].contiguous(), sb[p, :, c].contiguous()) for p in range(20) for c in range(24)]
    ms_480, singles = timed(lambda: [D.ks_statistic_device(x, y)[1] for x, y in cols], a.reps, a.warmup)
    t0 = time.perf_counter()
    dh = host_ks(sa, sb)
    ms_host = (time.perf_counter() - t0) * 1e3
    res["ks_20x24_n1000"] = {"one_launch_ms": round(ms_one, 4), "launches_480_ms": round(ms_480, 3), "host_route_ms": round(ms_host, 2),
                             "equal_to_single_launches": bool(torch.equal(torch.cat(singles).view(-1), d.view(-1))),
                             "max_abs_diff_host": float(np.abs(dh - d.cpu().numpy().ravel()).max())}
    # (b) box statistics
    am = fields((4, 10000, 24), dry=0.1)
    ms_box, _ = timed(lambda: D.boxplot_stats(am), a.reps, a.warmup)
    ms_box_nosort, _ = timed(lambda: D.boxplot_stats(am, keep_sorted=False), a.reps, a.warmup)
    res["box_4x24_n10000"] = {"ms": round(ms_box, 4), "without_sorted_output_ms": round(ms_box_nosort, 4)}
    # (c) ECDF on a grid
    x = fields((a.pixels,), dry=0.5)
    gb = a.pixels * 4 / 1e9
    res["ecdf"] = {"pixels": a.pixels}
    for T in (512, 4096):
        grid = D.log_grid(1e-3, 100.0, T)
        ms, _ = timed(lambda: D.ecdf_counts_device(x, grid)[0], a.reps, a.warmup)
        res["ecdf"][f"T{T}"] = {"ms": round(ms, 3), "GBps": round(gb / ms * 1e3, 1), "of_achievable_hbm": round(gb / ms * 1e3 / HBM_ACHIEVABLE_GBS, 3)}
    ms_sort, _ = timed(lambda: torch.sort(x).values, a.reps, a.warmup)
    res["ecdf"]["torch_sort_ms"] = round(ms_sort, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
