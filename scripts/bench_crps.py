"""Device time of the CRPS experiment's new pieces (crps_experiment.py): (a) one crps_fixed_ensemble_device call for D days against
a fixed n-member ensemble; (b) the same days through D calls of the per-day kernel (ensemble.crps_ensemble_device + the area mean),
the only way to these numbers without the fixed-ensemble kernel; (c) bootstrapped_difference_onesample at n = 240 000, N = 10 000.
Prints one JSON line; exits non-zero if (a) is not faster than (b).

    python scripts/bench_crps.py [--nd 16] [--members 5000] [--days 1000] [--boot-n 240000] [--boot-N 10000] [--skip-bootstrap]

Synthetic seeded fields (gamma with dry pixels), made on the host once.  Times are HIP events around the whole call, median of 10
after 3 warm-up calls (--reps / --warmup)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import crps_experiment as ce
from pr_disagg_radar_gan_amd.ensemble import crps_ensemble_device


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=16)
    ap.add_argument("--members", type=int, default=5000)
    ap.add_argument("--days", type=int, default=1000)
    ap.add_argument("--boot-n", type=int, default=240000)
    ap.add_argument("--boot-N", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-bootstrap", action="store_true")
    a = ap.parse_args()
    nd, n, D = a.nd, a.members, a.days
    rng = np.random.default_rng(nd)

    def fields(count):
        f = rng.gamma(0.5, 1.5, (count, 24, nd, nd)).astype(np.float32)
        f[rng.random(f.shape) < 0.4] = 0.0
        return torch.from_numpy(f).cuda()

    ens, obs = fields(n), fields(D)
    ms_fixed, hourly = timed(lambda: ce.crps_fixed_ensemble_device(ens, obs), a.reps, a.warmup)

    def per_day():
        return torch.stack([crps_ensemble_device(ens, obs[d]).mean(dim=(1, 2)) for d in range(D)])

    ms_days, hourly_days = timed(per_day, a.reps, a.warmup)
    res = {"metric": "crps_experiment", "nd": nd, "members": n, "days": D, "reps": a.reps, "warmup": a.warmup,
           "fixed_ensemble_ms": round(ms_fixed, 3), "per_day_calls_ms": round(ms_days, 3), "ratio": round(ms_days / ms_fixed, 1),
           "max_abs_diff": float((hourly - hourly_days).abs().max()), "mean_crps": round(float(hourly.mean()), 5)}
    if not a.skip_bootstrap:
        x = rng.gamma(0.5, 0.2, a.boot_n) - rng.gamma(0.5, 0.23, a.boot_n)
        xd = torch.from_numpy(x).cuda()
        ms_boot, b = timed(lambda: ce.bootstrapped_difference_onesample(xd, perc=1, N=a.boot_N, seed=0), a.reps, a.warmup)
        res["bootstrap"] = {"n": a.boot_n, "N": a.boot_N, "ms": round(ms_boot, 3), "gdraws_per_s": round(a.boot_n * a.boot_N / ms_boot / 1e6, 1),
                            "result": [float(v) for v in b]}
    print(json.dumps(res))
    if not ms_fixed < ms_days:
        raise SystemExit("the fixed-ensemble call is not faster than the per-day calls")


if __name__ == "__main__":
    main()
