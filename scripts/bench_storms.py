"""Device time of the storm pass (storms.py) at the project's field workload: S scenarios of one 256 x 256 day
(ndomain 16, overlap 4, a seeded init_generator), thresholds (0.1, 1, 5, 10) mm/h, 8-connectivity, reach 0, 1 and 4.

  (a) StormStructure.add on the held ensemble at T = 4 for every reach, as a time and as a rate over the bytes it has to read once
      per threshold, and its ratio to CellStructure.add (cells.py, which this pass contains) on the same tensor;
  (b) the same at T = 1 (1 mm/h) with the label map written;
  (c) the same at T = 4 with days_per_pass = 1 (the default holds 10 days of this size);
  (d) the time per kernel of one T = 4 call for every reach, from the profiler's own kernel records (null when the profiler is not
      available);
  (e) a plain-torch baseline that labels the same tensor at 1 mm/h and reach 1 by iterated max-pooling of index maps -- 3 x 3
      inside the hour, (2 reach + 1)^2 towards the hours before and after -- until nothing changes, on the first --torch-scenarios
      scenarios, with its time and whether its labels equal the kernel's.

    python scripts/bench_storms.py [--field 256] [--scenarios 100] [--reps 10] [--warmup 3] [--out FILE]

Times are HIP events around the whole call (host work included: the memset that zeroes the state, the C entry's checks and its
launches; the state and the workspace are allocated before): median, min and max of --reps calls after --warmup, one process.
Appends one JSON line to --out and prints it.  Recorded, not asserted; the equalities it reports are asserted by the tests."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import cells as CL
from pr_disagg_radar_gan_amd import field as F
from pr_disagg_radar_gan_amd import models
from pr_disagg_radar_gan_amd import storms as SM
from pr_disagg_radar_gan_amd import weights as W

REACHES = (0, 1, 4)


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


def torch_labels(x, thr, reach):
    """canonical labels of x (N, 24, ny, nx) at 8-connectivity: every wet voxel starts with its own day-local index and takes the
    smallest index among its wet 3 x 3 neighbourhood and the wet (2 reach + 1)^2 neighbourhoods of the hours before and after,
    until nothing changes"""
    N, H, ny, nx = x.shape
    wet = torch.isfinite(x) & (x > thr)
    big = float(H * ny * nx)
    idx = torch.arange(H * ny * nx, device=x.device, dtype=torch.float32).view(1, H, ny, nx).expand(N, H, ny, nx)  # (exact below 2^24)
    lab = torch.where(wet, idx, torch.full_like(idx, big))
    steps = 0
    while True:
        near = -torch.nn.functional.max_pool2d(-lab, 3, 1, 1)                              # (the hours are the channels)
        wide = -torch.nn.functional.max_pool2d(-lab, 2 * reach + 1, 1, reach) if reach else lab
        new = near.clone()
        new[:, 1:] = torch.minimum(new[:, 1:], wide[:, :-1])
        new[:, :-1] = torch.minimum(new[:, :-1], wide[:, 1:])
        new = torch.where(wet, new, lab)
        steps += 1
        if torch.equal(new, lab):
            break
        lab = new
    return torch.where(wet, lab, torch.full_like(lab, -1.0)).to(torch.int32), steps


def kernel_times(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key.split("(")[0]: [int(e.count), float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))) / 1e3]
            for e in prof.key_averages() if e.key.startswith(("k_cells", "k_storm"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--torch-scenarios", type=int, default=4)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_bench_storms.jsonl"))
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
    res = {"field": [n, n], "ndomain": nd, "overlap": a.overlap, "scenarios": S, "thresholds": list(thr), "connectivity": 8, "bytes": nbytes,
           "reps": a.reps, "warmup": a.warmup}
    labels = torch.empty(ens.shape, dtype=torch.int32, device="cuda")
    states = {}

    def add(thresholds, reach, per_pass=None, with_labels=False):
        key = (tuple(thresholds), reach, per_pass)
        if key not in states:
            states[key] = SM.StormStructure(thresholds, 8, reach, per_pass).add(ens)
        ss = states[key]
        ss.state().zero_()
        return ss.add(ens, labels_out=labels if with_labels else None)

    def row(t, T):
        return dict(t, gbs_per_threshold=T * nbytes / t["median_ms"] / 1e6)

    cells = CL.CellStructure(thr, 8).add(ens)

    def add_cells():
        cells.state().zero_()
        return cells.add(ens)

    t_cells, _ = timed(add_cells, a.reps, a.warmup)
    res["cells_T4"] = row(t_cells, 4)
    for reach in REACHES:
        r = {}
        t4, ss = timed(lambda: add(thr, reach), a.reps, a.warmup)
        st = ss.result()
        r["T4"] = row(t4, 4)                                                                 # (a)
        r["over_cells_T4"] = t4["median_ms"] / t_cells["median_ms"]
        r["mean_storms_per_day"] = [float(v) for v in st.mean_storms_per_day()]
        r["mean_duration"] = [float(v) for v in st.mean_duration()]
        r["one_hour_fraction"] = [float(v) for v in st.one_hour_fraction()]
        r["T1_labels"] = row(timed(lambda: add(thr[1:2], reach, with_labels=True), a.reps, a.warmup)[0], 1)  # (b)
        r["T4_days_per_pass_1"] = row(timed(lambda: add(thr, reach, 1), a.reps, a.warmup)[0], 4)             # (c)
        try:                                                                                 # (d)
            r["kernel_ms"] = kernel_times(lambda: add(thr, reach))
        except Exception as exc:                                                             # noqa: BLE001 -- recorded, not hidden
            r["kernel_ms"] = None
            r["kernel_ms_error"] = repr(exc)[:200]
        res[f"reach{reach}"] = r
    res["wet_fraction"] = [float(v) for v in st.wet_pixels.sum(axis=1) / (st.n_days * W.NHOURS * st.n_pixels)]
    m = min(a.torch_scenarios, S)                                                            # (e)
    t_torch, (lab_t, steps) = timed(lambda: torch_labels(ens[:m], thr[1], 1), 2, 1)
    t_sub, _ = timed(lambda: SM.label_storms(ens[:m], thr[1], 8, 1), a.reps, a.warmup)
    res["torch_maxpool_labels"] = dict(t_torch, scenarios=m, steps=steps, reach=1)
    res["label_storms_same_scenarios"] = t_sub
    res["torch_over_label_storms"] = t_torch["median_ms"] / t_sub["median_ms"]
    res["labels_equal_torch"] = bool(torch.equal(lab_t, SM.label_storms(ens[:m], thr[1], 8, 1)))
    line = json.dumps(res)
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
