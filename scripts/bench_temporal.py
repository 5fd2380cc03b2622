"""Device time of the temporal-structure pass (temporal.py) at the project's field workload: S scenarios of one
256 x 256 day (ndomain 16, overlap 4, a seeded init_generator), T = 4 thresholds, K = 6 lags.

  (a) rdgan_temporal_accumulate on the held ensemble, as a time and as a rate over the bytes it has to read (a rate over the
      bytes needed, not a counter measurement);
  (b) the same in groups of 16 scenarios, as temporal_structure_field feeds it;
  (c) a plain-torch restatement of wet_hours and trans alone on the same tensor -- what a user would write today -- with its time,
      the ratio, and whether its counts equal the kernel's;
  (d) T = 1 against T = 8 at K = 6, and K = 1 against K = 12 at T = 4: does the pass stay memory-bound;
  (e) temporal_structure_field against field.disaggregate run over the same scenario chunks into the same buffer.

    python scripts/bench_temporal.py [--field 256] [--scenarios 100] [--reps 10] [--warmup 3] [--out FILE]

Times are HIP events around the whole call (host work of the call included: the two memsets that zero the state, the C entry's
argument checks and its hipFuncSetAttribute, the launches of the accumulate and final kernels; the state and the workspace are
allocated before): median, min and max of --reps calls after --warmup, one
process.  Appends one JSON line to --out and prints it.  Recorded, not asserted; the equalities it reports are asserted by the tests."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import models
from pr_disagg_radar_gan_amd import field as F
from pr_disagg_radar_gan_amd import temporal as TS
from pr_disagg_radar_gan_amd import weights as W

THR8 = (0.0, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0)


def timed(fn, reps, warmup):
    """-> ({median, min, max} in ms, the last result)"""
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
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}, out


def torch_counts(x, thr):
    """wet_hours (T, 25) and trans (T, 23, 2, 2) of x (S, 24, ny, nx) over the series without a NaN or an inf"""
    ok = torch.isfinite(x).all(dim=1)
    wh, tr = [], []
    for t in thr:
        w = x > t
        wh.append(torch.bincount(w.sum(dim=1)[ok], minlength=25))
        code = (w[:, :-1].to(torch.int64) * 2 + w[:, 1:]).movedim(1, -1)[ok]                   # (series, 23)
        tr.append(torch.stack([(code == c).sum(dim=0) for c in range(4)], dim=1).view(23, 2, 2))
    return torch.stack(wh), torch.stack(tr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_bench_temporal.jsonl"))
    a = ap.parse_args()
    nd, n, S = 16, a.field, a.scenarios
    thr, K = (0.1, 1.0, 5.0, 10.0), 6
    rng = np.random.default_rng(0)
    gen = models.Generator(W.init_generator(rng, nd), nd)
    obs = (rng.gamma(0.5, 2.0, (W.NHOURS, n, n)) * (rng.random((W.NHOURS, n, n)) < 0.5)).astype(np.float32)
    daily = torch.from_numpy(obs).cuda().sum(0)
    z = rng.normal(size=(S, 1, W.LATENT_DIM)).astype(np.float32)
    ens, _ = F.disaggregate(gen, daily, S, overlap=a.overlap, latent=z)
    nbytes = ens.numel() * 4
    res = {"field": [n, n], "ndomain": nd, "overlap": a.overlap, "scenarios": S, "thresholds": list(thr), "max_lag": K, "bytes": nbytes,
           "reps": a.reps, "warmup": a.warmup, "wet_fraction": [float(f) for f in TS.temporal_structure(ens, thr, K).wet_fraction()]}

    states = {}

    def accumulate(thresholds, max_lag, step=None):
        """the state and its workspace are made once per (thresholds, max_lag), outside the timed calls, and zeroed inside"""
        key = (tuple(thresholds), max_lag)
        if key not in states:
            states[key] = TS.TemporalStructure(thresholds, max_lag).add(ens)
        ts = states[key]
        for t in ts.state():
            t.zero_()
        for s0 in range(0, S, step or S):
            ts.add(ens[s0:s0 + (step or S)])
        return ts

    def row(t):
        return dict(t, gbs=nbytes / t["median_ms"] / 1e6)

    t_once, ts = timed(lambda: accumulate(thr, K), a.reps, a.warmup)
    res["accumulate"] = row(t_once)                                                        # (a)
    res["accumulate_groups_of_16"] = row(timed(lambda: accumulate(thr, K, 16), a.reps, a.warmup)[0])      # (b)
    t_torch, (wh, tr) = timed(lambda: torch_counts(ens, thr), a.reps, a.warmup)            # (c)
    got = ts.result()
    res["torch_wet_hours_and_trans"] = t_torch
    res["torch_over_accumulate"] = t_torch["median_ms"] / t_once["median_ms"]
    res["counts_equal_torch"] = bool(np.array_equal(got.wet_hours, wh.cpu().numpy()) and np.array_equal(got.trans, tr.cpu().numpy()))
    del wh, tr
    for name, (tt, kk) in (("T1_K6", (THR8[2:3], 6)), ("T8_K6", (THR8, 6)), ("T4_K1", (thr, 1)), ("T4_K12", (thr, 12))):      # (d)
        res[name] = row(timed(lambda: accumulate(tt, kk), a.reps, a.warmup)[0])
    del ens
    torch.cuda.empty_cache()

    step = 16                                                                              # (e)
    buf = torch.empty((step, W.NHOURS, n, n), dtype=torch.float32, device="cuda")

    def disaggregate_chunks():
        for s0 in range(0, S, step):
            k = min(step, S - s0)
            F.disaggregate(gen, daily, k, overlap=a.overlap, latent=z[s0:s0 + k], out=buf[:k])

    t_dis, _ = timed(disaggregate_chunks, a.reps, a.warmup)
    t_tf, _ = timed(lambda: TS.temporal_structure_field(gen, daily, S, thr, max_lag=K, latent=z, scenario_chunk=step, overlap=a.overlap),
                    a.reps, a.warmup)
    res["disaggregate_same_chunks"] = t_dis
    res["temporal_structure_field"] = t_tf
    res["temporal_structure_field_over_disaggregate_same_chunks"] = t_tf["median_ms"] / t_dis["median_ms"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
