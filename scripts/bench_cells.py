"""Device time of the cell pass (cells.py) at the project's field workload: S scenarios of one 256 x 256 day
(ndomain 16, overlap 4, a seeded init_generator), thresholds (0.1, 1, 5, 10) mm/h, 8-connectivity.

  (a) CellStructure.add on the held ensemble at T = 4, as a time and as a rate over the bytes it has to read once per threshold;
  (b) the same at T = 1 (1 mm/h);
  (c) the same at T = 1 with the label map written;
  (d) the same at T = 4 with planes_per_pass = 24 (the default holds 256 planes of this size);
  (e) the time per kernel of one T = 4 call, from the profiler's own kernel records (null when the profiler is not available);
  (f) a plain-torch baseline that labels the same tensor at 1 mm/h by iterated 3 x 3 max-pooling of index maps until nothing
      changes, on the first --torch-scenarios scenarios, with its time and whether its labels equal the kernel's.

    python scripts/bench_cells.py [--field 256] [--scenarios 100] [--reps 10] [--warmup 3] [--out FILE]

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


def torch_labels(x, thr):
    """canonical labels of x (N, ny, nx) at 8-connectivity: every wet pixel starts with its own flat index and takes the smallest
    index of its wet 3 x 3 neighbourhood until nothing changes (one step per pixel of the longest shortest path inside a cell)"""
    N, ny, nx = x.shape
    wet = torch.isfinite(x) & (x > thr)
    big = float(ny * nx)
    idx = torch.arange(ny * nx, device=x.device, dtype=torch.float32).view(1, ny, nx).expand(N, ny, nx)      # (exact below 2^24)
    lab = torch.where(wet, idx, torch.full_like(idx, big))
    steps = 0
    while True:
        new = -torch.nn.functional.max_pool2d(-lab[:, None], 3, 1, 1)[:, 0]
        new = torch.where(wet, new, lab)
        steps += 1
        if torch.equal(new, lab):
            break
        lab = new
    return torch.where(wet, lab, torch.full_like(lab, -1.0)).to(torch.int32), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--torch-scenarios", type=int, default=4)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_bench_cells.jsonl"))
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

    def add(thresholds, per_pass=None, with_labels=False):
        key = (tuple(thresholds), per_pass)
        if key not in states:
            states[key] = CL.CellStructure(thresholds, 8, per_pass).add(ens)
        cs = states[key]
        cs.state().zero_()
        return cs.add(ens, labels_out=labels if with_labels else None)

    def row(t, T):
        return dict(t, gbs_per_threshold=T * nbytes / t["median_ms"] / 1e6)

    t4, cs = timed(lambda: add(thr), a.reps, a.warmup)
    st = cs.result()
    res["mean_cells_per_plane"] = [float(v) for v in st.mean_cells_per_plane()]
    res["wet_fraction"] = [float(v) for v in st.wet_pixels.sum(axis=1) / (st.n_planes * st.n_pixels)]
    res["speckle_fraction"] = [float(v) for v in st.speckle_fraction()]
    res["T4"] = row(t4, 4)                                                                   # (a)
    res["T1"] = row(timed(lambda: add(thr[1:2]), a.reps, a.warmup)[0], 1)                    # (b)
    res["T1_labels"] = row(timed(lambda: add(thr[1:2], with_labels=True), a.reps, a.warmup)[0], 1)      # (c)
    res["T4_planes_per_pass_24"] = row(timed(lambda: add(thr, 24), a.reps, a.warmup)[0], 4)  # (d)
    try:                                                                                     # (e)
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            add(thr)
            torch.cuda.synchronize()
        res["kernel_ms"] = {e.key.split("(")[0]: [int(e.count), float(getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))) / 1e3]
                            for e in prof.key_averages() if e.key.startswith("k_cells")}
    except Exception as exc:                                                                 # noqa: BLE001 -- recorded, not hidden
        res["kernel_ms"] = None
        res["kernel_ms_error"] = repr(exc)[:200]
    m = min(a.torch_scenarios, S)                                                            # (f)
    sub = ens[:m].reshape(-1, n, n)
    t_torch, (lab_t, steps) = timed(lambda: torch_labels(sub, thr[1]), 2, 1)
    t_sub, _ = timed(lambda: CL.label_cells(ens[:m], thr[1]), a.reps, a.warmup)
    res["torch_maxpool_labels"] = dict(t_torch, scenarios=m, steps=steps)
    res["label_cells_same_scenarios"] = t_sub
    res["torch_over_label_cells"] = t_torch["median_ms"] / t_sub["median_ms"]
    res["labels_equal_torch"] = bool(torch.equal(lab_t.view(ens[:m].shape), CL.label_cells(ens[:m], thr[1])))
    line = json.dumps(res)
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
