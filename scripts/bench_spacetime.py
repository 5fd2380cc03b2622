"""Device time of the space-time pass (spacetime.py) at the project's field workload: S scenarios of one 256 x 256
day (ndomain 16, overlap 4, a seeded init_generator), T = 4 thresholds.

  (a) rdgan_spacetime_accumulate on the held ensemble at radius 4 and 8, max_lag 1 and 3, as a time;
  (b) the pack pass beside the bytes it reads: the entry has no pack-only form, so the call at radius 1, max_lag 1 -- the same
      pack pass and the least correlate work -- is reported as an upper bound of the pack pass, with the rate over the bytes the
      pass has to read (a rate over the bytes needed, not a counter measurement); the kernels' own times come from the
      profiler's kernel records, taken in a run of their own;
  (c) a plain-torch restatement of joint[t][k][d] for ONE threshold at radius 4, max_lag 1 (shifted slices and sum) -- what a
      user would write today -- with its time, the ratio, and whether its counts equal the kernel's;
  (d) the same call in groups of 16 scenarios, as spacetime_structure_field feeds it.

    python scripts/bench_spacetime.py [--field 256] [--scenarios 100] [--reps 10] [--warmup 3] [--out FILE]

Times are HIP events around the whole call (host work of the call included: the memset that zeroes the state, the C entry's
argument checks, the two launches per pass; the state and the workspace are allocated before): median, min and max of --reps calls
after --warmup, one process.  Appends one JSON line to --out and prints it.  Recorded, not asserted; the equality it reports is
asserted by the tests."""
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
from pr_disagg_radar_gan_amd import spacetime as ST
from pr_disagg_radar_gan_amd import weights as W


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


def torch_joint(x, thr, R, K):
    """joint (K + 1, 2R + 1, 2R + 1) of x (S, 24, ny, nx) at one threshold: both pixels finite and wet"""
    ny, nx = x.shape[-2:]
    w = torch.isfinite(x) & (x > thr)
    out = torch.zeros((K + 1, 2 * R + 1, 2 * R + 1), dtype=torch.int64, device=x.device)
    for k in range(K + 1):
        a, b = w[:, :24 - k], w[:, k:]
        for dy in range(-R, R + 1):
            ya, yb = slice(max(0, -dy), ny - max(0, dy)), slice(max(0, dy), ny - max(0, -dy))
            for dx in range(-R, R + 1):
                xa, xb = slice(max(0, -dx), nx - max(0, dx)), slice(max(0, dx), nx - max(0, -dx))
                out[k, dy + R, dx + R] = (a[:, :, ya, xa] & b[:, :, yb, xb]).sum()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_bench_spacetime.jsonl"))
    a = ap.parse_args()
    nd, n, S = 16, a.field, a.scenarios
    thr = (0.1, 1.0, 5.0, 10.0)
    rng = np.random.default_rng(0)
    gen = models.Generator(W.init_generator(rng, nd), nd)
    obs = (rng.gamma(0.5, 2.0, (W.NHOURS, n, n)) * (rng.random((W.NHOURS, n, n)) < 0.5)).astype(np.float32)
    daily = torch.from_numpy(obs).cuda().sum(0)
    z = rng.normal(size=(S, 1, W.LATENT_DIM)).astype(np.float32)
    ens, _ = F.disaggregate(gen, daily, S, overlap=a.overlap, latent=z)
    nbytes = ens.numel() * 4
    res = {"field": [n, n], "ndomain": nd, "overlap": a.overlap, "scenarios": S, "thresholds": list(thr), "bytes": nbytes,
           "reps": a.reps, "warmup": a.warmup, "tile_rows_words": {str(R): list(ST.tile_shape(n, n, R)) for R in (1, 4, 8)}}

    states = {}

    def accumulate(thresholds, R, K, step=None):
        """the state and its workspace are made once per (thresholds, R, K), outside the timed calls, and zeroed inside"""
        key = (tuple(thresholds), R, K)
        if key not in states:
            states[key] = ST.SpaceTimeStructure(thresholds, R, K).add(ens)
        st = states[key]
        st.state().zero_()
        for s0 in range(0, S, step or S):
            st.add(ens[s0:s0 + (step or S)])
        return st

    for R in (4, 8):                                                                        # (a)
        for K in (1, 3):
            t, st = timed(lambda: accumulate(thr, R, K), a.reps, a.warmup)
            res[f"accumulate_R{R}_K{K}"] = t
            if (R, K) == (4, 1):
                s = st.result()
                res["wet_fraction"] = [float(f) for f in s.wet_first[:, 0, R, R] / max(1, s.pairs[0, R, R])]
                res["stationary_fraction_R4_K1"] = [float(f) for f in s.stationary_fraction()[:, 0]]
                res["shift_gain_R4_K1"] = [float(f) for f in s.shift_gain()[:, 0]]
                joint_kernel = s.joint[1]
    t_small, _ = timed(lambda: accumulate(thr, 1, 1), a.reps, a.warmup)                     # (b)
    res["accumulate_R1_K1_upper_bound_of_pack"] = dict(t_small, gbs_over_bytes_read=nbytes / t_small["median_ms"] / 1e6)
    res["accumulate_R4_K1_T1"] = timed(lambda: accumulate(thr[1:2], 4, 1), a.reps, a.warmup)[0]
    t_torch, joint = timed(lambda: torch_joint(ens, thr[1], 4, 1), max(2, a.reps // 3), 1)  # (c)
    res["torch_joint_one_threshold_R4_K1"] = t_torch
    res["torch_over_accumulate_R4_K1_T1"] = t_torch["median_ms"] / res["accumulate_R4_K1_T1"]["median_ms"]
    res["torch_over_accumulate_R4_K1_T4"] = t_torch["median_ms"] / res["accumulate_R4_K1"]["median_ms"]
    res["joint_equals_torch"] = bool(np.array_equal(joint.cpu().numpy(), joint_kernel))
    res["accumulate_R4_K1_groups_of_16"] = timed(lambda: accumulate(thr, 4, 1, 16), a.reps, a.warmup)[0]      # (d)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
