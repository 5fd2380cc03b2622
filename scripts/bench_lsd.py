"""Device time of spectral.lsd_evaluation (radial spectra of real and generated fields, then the three comparisons in histogram
mode) at n = 1000 days, nd 16 and 64: 24 000 fields per side, 3 x 24 000 x 23 999 = 1.73 G pairs.  Prints one JSON line.

    python scripts/bench_lsd.py [--days 1000] [--nd 16 64] [--reps 5]

Synthetic seeded fields (gamma with dry pixels), made on the host once per nd.  Times are CUDA events around the whole call
(including the copy of the small results to the host), median of --reps after one warm-up call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import spectral


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=int, default=1000)
    ap.add_argument("--nd", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = {"metric": "lsd_evaluation_ms", "days": a.days, "fields_per_side": 24 * a.days}
    for nd in a.nd:
        rng = np.random.default_rng(nd)
        f = rng.gamma(0.5, 1.5, (2, a.days, 24, nd, nd)).astype(np.float32)
        f[rng.random(f.shape) < 0.4] = 0.0
        real, gen = (torch.from_numpy(x).cuda() for x in f)
        ms, out = timed(lambda: spectral.lsd_evaluation(real, gen), a.reps)
        flat = real.reshape(-1, nd, nd)
        ms_spec, _ = timed(lambda: spectral.radial_spectra_device(flat, log=True), a.reps)
        s = spectral.radial_spectra_device(flat, log=True)
        ms_pairs, _ = timed(lambda: spectral.log_spectral_distance_device(s), a.reps)
        n = flat.shape[0]
        res[f"nd{nd}"] = {"ms": round(ms, 3), "spectra_ms_per_side": round(ms_spec, 3), "pairs_ms_per_comparison": round(ms_pairs, 3),
                          "gpairs_per_s": round(n * (n - 1) / ms_pairs / 1e6, 1), "K": int(s.shape[1]),
                          "mean_real": round(out["real"].mean, 4), "mean_gen_real": round(out["gen_real"].mean, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
