"""Device time of the random-cascade baseline (cascade.py): (a) the calibration pass over an hourly array -- 200 000 tiles at nd 16 and
20 000 at nd 64 -- against the bytes it reads over the achievable HBM bandwidth, and against the analog library's feature pass
(k_analog_features), which reads the same bytes; (b) the generation of 1 000 queries x 100 members at nd 16 against the bytes it
writes.  Prints one JSON line.

    python scripts/bench_cascade.py [--tiles16 200000] [--tiles64 20000] [--queries 1000] [--members 100] [--dry 0.7]

Synthetic seeded fields made on the device: wet spells of one to three hours, `--dry` of the pixel-hours dry.  Times are HIP events
around the whole call, median of 10 after 3 warm-up calls (--reps / --warmup).  The analog pass takes at most 2^24 - 1 days."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import cascade as cs
from pr_disagg_radar_gan_amd.analog import AnalogLibrary

HBM_BYTES_PER_S = 6.3e12                      # achievable, of 8 TB/s peak


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


def rain(n, nd, dry, seed):
    """(n, 24, nd, nd) float32 on the device, made in slices of at most 2^28 values"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((n, 24, nd, nd), dtype=torch.float32, device="cuda")
    step = max(1, (1 << 28) // (24 * nd * nd))
    p = (1.0 - dry) / 2.1                      # a spell lasts 1 + 0.7 + 0.4 hours on average
    for i in range(0, n, step):
        shape = out[i:i + step].shape
        start = torch.rand(shape, generator=g, device="cuda") < p
        wet = start.clone()
        wet[:, 1:] |= start[:, :-1] & (torch.rand(shape, generator=g, device="cuda")[:, 1:] < 0.7)
        wet[:, 2:] |= start[:, :-2] & (torch.rand(shape, generator=g, device="cuda")[:, 2:] < 0.4)
        out[i:i + step] = -2.0 * torch.log1p(-torch.rand(shape, generator=g, device="cuda")) * wet
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles16", type=int, default=200000)
    ap.add_argument("--tiles64", type=int, default=20000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--members", type=int, default=100)
    ap.add_argument("--dry", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "dry": a.dry}
    model = None
    for nd, n in ((16, a.tiles16), (64, a.tiles64)):
        if n < 1:
            continue
        x = rain(n, nd, a.dry, nd)
        nbytes = x.numel() * 4
        cal = cs.CascadeCalibrator()
        ms, _ = timed(lambda: cal.add(x), a.reps, a.warmup)
        state = cal.state().cpu().numpy()
        r = {"tiles": n, "read_bytes": nbytes, "dry_pixel_days": float(state[-1] / state[-3]), "calibrate_ms": ms,
             "calibrate_bytes_per_s": nbytes / (ms * 1e-3), "calibrate_fraction_of_hbm": nbytes / HBM_BYTES_PER_S / (ms * 1e-3)}
        if nd * nd <= 4096:
            ms_an, _ = timed(lambda: AnalogLibrary(x), a.reps, a.warmup)       # the feature pass and its small second kernel, buffers included
            r["analog_library_ms"] = ms_an
        res[f"nd{nd}"] = r
        if model is None:
            model = cs.CascadeCalibrator().add(x).result()
        del x, cal
        torch.cuda.empty_cache()
    if a.queries >= 1 and model is not None:
        nd = 16
        cond = rain(a.queries, nd, a.dry, 7).sum(1)
        out = torch.empty((a.queries, a.members, 24, nd, nd), dtype=torch.float32, device="cuda")
        nbytes = out.numel() * 4
        g = {"queries": a.queries, "members": a.members, "write_bytes": nbytes}
        for patch in (1, nd):
            ms, _ = timed(lambda: model.generate(cond, a.members, seed=1, patch=patch, out=out), a.reps, a.warmup)
            g[f"patch{patch}_ms"] = ms
            g[f"patch{patch}_fraction_of_hbm"] = nbytes / HBM_BYTES_PER_S / (ms * 1e-3)
        assert torch.equal(out.sum(2, dtype=torch.float64), (torch.round(cond * 1024) / 1024).double()[:, None].expand(-1, a.members, -1, -1))
        res["generate_nd16"] = g
    print(json.dumps(res))


if __name__ == "__main__":
    main()
