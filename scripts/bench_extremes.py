"""Device time of the extremes evaluation (extremes.py): the block-maxima pass and the L-moment sums, each against the bytes it must
move over the achievable HBM bandwidth and against a torch restatement on the same data.  Prints one JSON line.

    python scripts/bench_extremes.py [--reps 10] [--warmup 3]

 * BlockMaxima.add on 100 scenarios of one 256 x 256 day (one block per scenario, 629 MB) and on 8 blocks x 45 days of a 64 x 64
   plane, 5 windows; the read bound is 4 * 24 * n * plane bytes.  torch: field_products.peaks_device (fp32 peaks, the nearest
   existing route) followed by amax per block through scatter_reduce.
 * lmoment_sums at S = 100, M = 5 * 65536, B = 8 and B = 64; the bound is the table read once and the sums written.  torch:
   torch.sort along the block axis plus the three weighted sums, asserted equal.

Synthetic seeded spells made on the device.  Times are HIP events around the whole call, median of 10 after 3 warm-up calls
(--reps / --warmup), one process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import extremes as ex, field_products as fp

HBM_BYTES_PER_S = 6.3e12                      # achievable, of 8 TB/s peak
WINDOWS = (1, 3, 6, 12, 24)


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


def rain(n, ny, nx, dry, seed):
    """spells: an hour is wet where a noise field smoothed over 4 hours is high, so that wet hours come in runs"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (n, 24, ny, nx)
    u = torch.rand(shape, generator=g, device="cuda")
    u = (u + u.roll(1, 1) + u.roll(2, 1) + u.roll(3, 1)) / 4
    wet = u > torch.quantile(u.flatten()[:1 << 20], dry)
    return -2.0 * torch.log1p(-torch.rand(shape, generator=g, device="cuda")) * wet


def bench_maxima(name, n, ny, nx, block, n_blocks, a):
    x = rain(n, ny, nx, 0.7, 1)
    plane = ny * nx
    bm = ex.BlockMaxima(WINDOWS, n_blocks)
    ms, _ = timed(lambda: bm.add(x, block), a.reps, a.warmup)
    nbytes = 4 * 24 * n * plane
    idx = torch.from_numpy(np.asarray(block, np.int64)).cuda().view(n, 1, 1, 1).expand(n, len(WINDOWS), ny, nx)

    def by_torch():
        peaks, _ = fp.peaks_device(x, WINDOWS)
        return torch.full((n_blocks, len(WINDOWS), ny, nx), -1.0, device="cuda").scatter_reduce_(0, idx, peaks, "amax", include_self=True)

    ms_t, out = timed(by_torch, a.reps, a.warmup)
    # the integer maxima against the fp32 ones: the same maxima up to the rounding of the fp32 sums
    got = ex.BlockMaxima(WINDOWS, n_blocks).add(x, block).result().bmax.to(torch.float64) / 1024.0
    assert float((got - out.to(torch.float64)).abs().max()) < 0.05
    return {"days": n, "plane": [ny, nx], "blocks": n_blocks, "windows": list(WINDOWS), "read_bytes": nbytes, "hip_ms": ms,
            "hip_bytes_per_s": nbytes / (ms * 1e-3), "hip_fraction_of_hbm": nbytes / HBM_BYTES_PER_S / (ms * 1e-3), "bound_ms": nbytes / HBM_BYTES_PER_S * 1e3,
            "torch_peaks_amax_ms": ms_t}


def bench_sums(S, B, M, a):
    g = torch.Generator(device="cuda").manual_seed(2)
    table = torch.randint(0, 1 << 22, (S, B, M), generator=g, device="cuda", dtype=torch.int64)
    table[torch.rand((S, B, M), generator=g, device="cuda") < 0.02] = -1
    ms, (n, A) = timed(lambda: ex.lmoment_sums(table), a.reps, a.warmup)
    rank = torch.arange(B, device="cuda", dtype=torch.int64).view(1, B, 1)

    def by_torch():
        keep = table >= 0
        srt, _ = torch.sort(torch.where(keep, table, torch.full_like(table, 1 << 62)), dim=1)
        srt = torch.where(srt < (1 << 62), srt, torch.zeros_like(srt))
        return keep.sum(dim=1).to(torch.int32), torch.stack([srt.sum(dim=1), (rank * srt).sum(dim=1), (rank * (rank - 1) * srt).sum(dim=1)], dim=2)

    ms_t, (n_t, A_t) = timed(by_torch, a.reps, a.warmup)
    assert torch.equal(n, n_t) and torch.equal(A, A_t)
    nbytes = 8 * S * B * M + 28 * S * M
    return {"series": S, "blocks": B, "positions": M, "bytes": nbytes, "hip_ms": ms, "hip_fraction_of_hbm": nbytes / HBM_BYTES_PER_S / (ms * 1e-3),
            "bound_ms": nbytes / HBM_BYTES_PER_S * 1e3, "torch_sort_sums_ms": ms_t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S}
    res["maxima_100x256x256"] = bench_maxima("ensemble day", 100, 256, 256, np.arange(100), 100, a)
    torch.cuda.empty_cache()
    res["maxima_8x45x64x64"] = bench_maxima("years", 360, 64, 64, np.repeat(np.arange(8), 45), 8, a)
    torch.cuda.empty_cache()
    for B in (8, 64):
        res[f"lmoment_sums_B{B}"] = bench_sums(100, B, 5 * 65536, a)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
