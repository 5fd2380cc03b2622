"""Device time of the scaling evaluation (scaling.py): 100 scenarios of a 256 x 256 day (629 MB) and 200 016 training tiles of
16 x 16, against the time to read the bytes once at the achievable HBM bandwidth, and against a torch restatement measured in the
same run on the same data: the quantised depths summed over the boxes with avg_pool2d in fp64 (exact below 2^53) and over the
windows with a reshape, then bucketize against the bin edges and bincount, per pair of levels.  Prints one JSON line.

    python scripts/bench_scaling.py [--scenarios 100] [--size 256] [--tiles 200016] [--dry 0.7]

Synthetic seeded fields made on the device, `--dry` of the pixel-hours dry.  Times are HIP events around the whole call, median of 10
after 3 warm-up calls (--reps / --warmup), one process.  The torch route takes the array in pieces of 2^26 values and stops at the
histograms and the first moment, which are asserted equal to the module's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import scaling as sc

HBM_BYTES_PER_S = 6.3e12                      # achievable, of 8 TB/s peak
PIECE = 1 << 26                               # values the torch route holds in fp64 at a time


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


def rain(n, size, dry, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (n, 24, size, size)
    return -2.0 * torch.log1p(-torch.rand(shape, generator=g, device="cuda")) * (torch.rand(shape, generator=g, device="cuda") >= dry)


def by_torch(x, A, edges):
    """-> (hist (A + 1, 5, 288), sum1 (A + 1, 5)) int64; x holds no bad value"""
    n, _, ny, nx = x.shape
    hist = torch.zeros((A + 1, sc.N_TIME, sc.N_BINS), dtype=torch.int64, device=x.device)
    sum1 = torch.zeros((A + 1, sc.N_TIME), dtype=torch.int64, device=x.device)
    step = max(1, PIECE // (24 * ny * nx))
    for d0 in range(0, n, step):
        q = torch.round(x[d0:d0 + step] * 1024.0).to(torch.float64)
        m = q.shape[0]
        for a in range(A + 1):
            s = 1 << a
            boxes = q if a == 0 else torch.nn.functional.avg_pool2d(q.view(m * 24, 1, ny, nx), s).view(m, 24, ny // s, nx // s) * float(s * s)
            for b, T in enumerate(sc.DURATIONS):
                R = boxes.view(m, 24 // T, T, -1).sum(dim=2).to(torch.int64).view(-1)
                hist[a, b] += torch.bincount(torch.bucketize(R, edges, right=True) - 1, minlength=sc.N_BINS)
                sum1[a, b] += R.sum()
    return hist, sum1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--tiles", type=int, default=200016)
    ap.add_argument("--dry", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    edges = torch.from_numpy(sc.bin_edges()).cuda()
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "dry": a.dry}
    for name, n, size in (("field", a.scenarios, a.size), ("tiles", a.tiles, 16)):
        x = rain(n, size, a.dry, 1)
        A = sc.largest_space_levels(size, size)
        acc = sc.ScalingStructure(A)
        ms, _ = timed(lambda: acc.reset().add(x), a.reps, a.warmup)
        stats = acc.result()
        nbytes = x.numel() * 4
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        ms_t, (hist, sum1) = timed(lambda: by_torch(x, A, edges), a.reps, a.warmup)
        assert np.array_equal(hist.cpu().numpy(), stats.hist) and np.array_equal(sum1.cpu().numpy(), stats.sum1), name
        res[name] = {"days": n, "plane": [size, size], "space_levels": A, "read_bytes": nbytes, "read_floor_ms": floor_ms, "hip_ms": ms,
                     "hip_bytes_per_s": nbytes / (ms * 1e-3), "hip_fraction_of_hbm": floor_ms / ms, "torch_ms": ms_t, "torch_over_hip": ms_t / ms}
        del x, hist, sum1, acc
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
