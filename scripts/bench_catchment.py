"""Device time of the catchment-rainfall evaluation (catchments.py): 100 scenarios of a 256 x 256 day for three maps -- 16 square
basins of 64 x 64, about 200 irregular basins over 80 % of the plane (a seeded nearest-centre partition whose outermost pixels lie
in no basin), a nested stack of 8 -- against the bytes the pass must read, 4 * 24 * E * n plus the lists, over the achievable HBM
bandwidth, and against two torch routes to the same hyetographs on the same data: index_add_ over the listed pixels, and the one-hot
(C, plane) @ (plane, n * 24) matmul in fp64 (exact below 2^53).  Prints one JSON line.

    python scripts/bench_catchment.py [--scenarios 100] [--size 256] [--dry 0.7]

Synthetic seeded fields made on the device, `--dry` of the pixel-hours dry.  Times are HIP events around the whole call, median of 10
after 3 warm-up calls (--reps / --warmup), one process.  The module's call also classifies the days of 5 windows and 7 levels and
writes the depths; the torch routes stop at the series, which is asserted equal."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import catchments as ct

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


def maps(size, seed=0):
    """name -> CatchmentMap on a size x size plane"""
    yy, xx = np.mgrid[:size, :size]
    q = size // 4
    squares = ct.CatchmentMap(regions=(yy // q) * 4 + xx // q)
    rng = np.random.default_rng(seed)
    centres = rng.random((200, 2)) * size
    d2 = (yy.ravel()[:, None] + 0.5 - centres[None, :, 0]) ** 2 + (xx.ravel()[:, None] + 0.5 - centres[None, :, 1]) ** 2
    near, dist = d2.argmin(axis=1), d2.min(axis=1)
    near[dist > np.quantile(dist, 0.8)] = -1                                   # the outermost fifth lies in no basin
    _, near = np.unique(near, return_inverse=True)                             # (a centre that owns no pixel leaves no gap)
    irregular = ct.CatchmentMap(regions=near.reshape(size, size) - 1)
    half = size // 2
    nested = ct.CatchmentMap(masks=np.stack([(abs(yy - half + 0.5) < half - c * (half // 9)) & (abs(xx - half + 0.5) < half - c * (half // 9))
                                             for c in range(8)]))
    return {"squares16": squares, "irregular200": irregular, "nested8": nested}


def rain(n, size, dry, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (n, 24, size, size)
    return -2.0 * torch.log1p(-torch.rand(shape, generator=g, device="cuda")) * (torch.rand(shape, generator=g, device="cuda") >= dry)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dry", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n, plane = a.scenarios, a.size * a.size
    x = rain(n, a.size, a.dry, 1)
    res = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "scenarios": n, "plane": [a.size, a.size], "dry": a.dry}
    for name, cmap in maps(a.size).items():
        C, E = cmap.n_catch, cmap.n_entries
        series = torch.empty((n, C, 24), dtype=torch.int64, device="cuda")
        depths = torch.empty((n, C, len(WINDOWS)), dtype=torch.int64, device="cuda")
        cr = ct.CatchmentRainfall(cmap, WINDOWS, ct.DEFAULT_LEVELS)
        ms, _ = timed(lambda: cr.add(x, series_out=series, depths_out=depths), a.reps, a.warmup)
        nbytes = 4 * 24 * E * n + cmap.pixels.nbytes + cmap.chunks.nbytes
        r = {"catchments": C, "entries": E, "covered": float(np.unique(cmap.pixels).size / plane), "chunks": len(cmap.chunks), "read_bytes": nbytes,
             "hip_ms": ms, "hip_bytes_per_s": nbytes / (ms * 1e-3), "hip_fraction_of_hbm": nbytes / HBM_BYTES_PER_S / (ms * 1e-3)}
        pixels = torch.from_numpy(cmap.pixels.astype(np.int64)).cuda()
        owner = torch.from_numpy(np.repeat(np.arange(C), cmap.npix)).cuda()
        onehot = torch.zeros((C, plane), dtype=torch.float64, device="cuda")
        onehot.index_put_((owner, pixels), torch.ones((), dtype=torch.float64, device="cuda"), accumulate=True)

        def by_index_add():
            q = torch.round(x.view(n, 24, plane) * 1024.0).to(torch.int64)
            return torch.zeros((n, 24, C), dtype=torch.int64, device="cuda").index_add_(2, owner, q[:, :, pixels]).transpose(1, 2)

        def by_matmul():
            q = torch.round(x.view(n * 24, plane) * 1024.0).to(torch.float64)
            return (onehot @ q.t()).view(C, n, 24).permute(1, 0, 2).to(torch.int64)

        for key, fn in (("torch_index_add", by_index_add), ("torch_onehot_matmul", by_matmul)):
            ms_t, out = timed(fn, a.reps, a.warmup)
            assert torch.equal(out, series), key
            r[key + "_ms"] = ms_t
            del out
        res[name] = r
        del series, depths, onehot, cr
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
