"""Device time of the RainFARM baseline (rainfarm.py): generation in members/s at nd 16 and 64 (counter-RNG phases, one broadcast
daily sum), the slope calibration of one 5 000-sample batch, and one CRPS day (1 000 members generated, then their CRPS against the
real day) at nd 16.  Prints one JSON line.

    python scripts/bench_rainfarm.py [--members 1000] [--nd 16 64] [--calib 5000] [--reps 5]

Synthetic seeded inputs made on the host once.  Times are CUDA events around the whole call (including the copy of small results
to the host), median of --reps after one warm-up call.  fp32_tflops counts the generation's DFT arithmetic only (8 flops per complex
multiply-add of the time sum and the row IDFT, 4 per real-output column step; no sincos, exp or hash), against the MI355X's 157.3
TFLOP/s fp32 vector peak."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import rainfarm

FP32_PEAK_TFLOPS = 157.3


def timed(fn, reps):
    fn()
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


def gen_flops(nd):
    nn = nd * nd
    return 24 * (23 * nn * 8 + nn * nd * 8 + nn * nd * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--nd", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--calib", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    alpha, beta = 2.2, 1.4
    res = {"metric": "rainfarm", "members": a.members, "calib_samples": a.calib}
    for nd in a.nd:
        rng = np.random.default_rng(nd)
        precip = torch.from_numpy((rng.gamma(0.6, 12.0, (nd, nd)) * (rng.random((nd, nd)) > 0.2)).astype(np.float32)).cuda()
        ms, _ = timed(lambda: rainfarm.downscale_device(precip, alpha, beta, n_members=a.members, seed=1), a.reps)
        res[f"gen_nd{nd}"] = {"ms": round(ms, 3), "members_per_s": round(a.members / ms * 1e3),
                              "fp32_tflops": round(gen_flops(nd) * a.members / ms / 1e9, 2),
                              "frac_fp32_peak": round(gen_flops(nd) * a.members / ms / 1e9 / FP32_PEAK_TFLOPS, 3)}
    for nd in a.nd:
        x = rainfarm.downscale_device(torch.full((nd, nd), 20.0, device="cuda"), alpha, beta, n_members=a.calib, seed=2)
        ms, (al, be) = timed(lambda: rainfarm.estimate_slopes(x), a.reps)
        res[f"calib_nd{nd}"] = {"ms": round(ms, 3), "alpha": round(al, 4), "beta": round(be, 4)}
    nd = 16
    rng = np.random.default_rng(3)
    day = rainfarm.downscale_device(torch.from_numpy(rng.gamma(0.6, 12.0, (nd, nd)).astype(np.float32)).cuda(), alpha, beta,
                                    n_members=1, seed=9)[0]
    ms, crps = timed(lambda: rainfarm.crps_for_day(day, alpha, beta, n_members=1000, seed=4), a.reps)
    res["crps_day_nd16"] = {"ms": round(ms, 3), "members": 1000, "crps_mean": round(float(np.mean(crps)), 5)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
