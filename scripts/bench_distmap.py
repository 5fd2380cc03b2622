"""Device time of the distance-map verification (distmap.py): whole DistanceMapVerifier(obs, thr).add(ens) calls -- the
observation's maps, the members' transforms and the records, allocations included -- at 4 thresholds on 100 scenarios of one
256 x 256 day, on 200 016 tiles of nd 16 (one member of 8334 days), and on 100 scenarios of 256 x 256 with a few wet pixels per
plane, where the outward column scan is at its worst.  Each beside the bound of reading the members once and the observation's maps
once per member at 6.3 TB/s, beside a torch restatement of the same records (a separable min over rows, run in the same process and
giving the same integers), and beside IntensityScaleVerifier.add on the same data in the same run.  Prints one JSON line.

    python scripts/bench_distmap.py [--reps 10] [--warmup 3]

Synthetic seeded spells made on the device (as scripts/bench_sal.py makes them), without bad values.  Times are HIP events around
the whole call, median of 10 after 3 warm-up calls (--reps / --warmup), one process; the torch restatement runs once after one
warm-up.  The split is the device time of every kernel of one further call, from the profiler's kernel records."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import distmap as DM, intensity_scale as IS
from scripts.bench_sal import kernel_split, rain, timed

THRESHOLDS = (0.1, 1.0, 5.0, 10.0)
HBM = 6.3e12
EMPTY = 0xFFFF


def torch_d(mask):
    """(B, ny, nx) bool -> D (B, ny, nx) int64, EMPTY for an empty set: g by rows, then the min over rows, both by brute force"""
    B, ny, nx = mask.shape
    dev = mask.device
    col, row = torch.arange(nx, dtype=torch.int32, device=dev), torch.arange(ny, dtype=torch.int32, device=dev)
    big = torch.tensor(1 << 14, dtype=torch.int32, device=dev)
    g = torch.where(mask[:, :, None, :], (col[:, None] - col[None, :]).abs()[None, None], big).amin(dim=3)
    d2 = (((row[:, None] - row[None, :]) ** 2)[None, :, :, None] + (g * g)[:, None, :, :]).amin(dim=2)
    D = torch.sqrt((d2.to(torch.int64) << 8).to(torch.float64)).floor().to(torch.int64)
    D[~mask.flatten(1).any(dim=1)] = EMPTY
    return D


def torch_records(ens, obs, thresholds, C):
    """records (s, n_days, 24, T, 12) int64 of arrays without bad values"""
    s, ny, nx = ens.shape[0], ens.shape[-2], ens.shape[-1]
    o, e = obs.reshape(-1, ny, nx), ens.reshape(s, -1, ny, nx)
    n = o.shape[0]
    out = torch.zeros((s, n, len(thresholds), 12), dtype=torch.int64, device=ens.device)
    step = max(1, (1 << 27) // (ny * nx * max(ny, nx)))               # 512 MB of int32 at a time
    for t, u in enumerate(thresholds):
        for i in range(0, n, step):
            B = o[i:i + step] > u
            DB = torch_d(B)
            eB = (DB == EMPTY).flatten(1).any(dim=1)
            for m in range(s):
                A = e[m, i:i + step] > u
                DA = torch_d(A)
                eA = (DA == EMPTY).flatten(1).any(dim=1)
                r = out[m, i:i + step, t]
                r[:, 0], r[:, 1], r[:, 2], r[:, 3] = ny * nx, A.flatten(1).sum(1), B.flatten(1).sum(1), (A & B).flatten(1).sum(1)
                ba, ab = (DA * B).flatten(1), (DB * A).flatten(1)
                r[:, 4], r[:, 6] = ba.sum(1) * ~eA, ba.amax(1) * ~eA
                r[:, 5], r[:, 7] = ab.sum(1) * ~eB, ab.amax(1) * ~eB
                d = (DA.clamp(max=C) - DB.clamp(max=C)).abs().flatten(1)
                r[:, 8], r[:, 9], r[:, 10] = d.sum(1), (d * d).sum(1), d.amax(1)
                r[:, 11] = 2 * eA + 4 * eB
    return out.view(s, -1, 24, len(thresholds), 12)


def case(name, ens, obs, reps, warmup):
    call = lambda: DM.DistanceMapVerifier(obs, THRESHOLDS).add(ens)
    ms, ver = timed(call, reps, warmup)
    rec = torch.cat(ver._parts, dim=0)
    ms_torch, ref = timed(lambda: torch_records(ens, obs, THRESHOLDS, ver.cutoff16), 1, 1)
    assert torch.equal(rec, ref), name
    ms_iss, _ = timed(lambda: IS.IntensityScaleVerifier(obs, THRESHOLDS).add(ens), reps, warmup)
    T = len(THRESHOLDS)
    nbytes = 4 * ens.numel() + 2 * T * ens.numel()                    # the members once, the observation's maps once per member
    bound_ms = nbytes / HBM * 1e3
    wet = [float((ens > u).float().mean()) for u in THRESHOLDS]
    return {"case": name, "wet_fraction": wet, "read_bytes": nbytes, "add_ms": ms, "bound_ms": bound_ms, "fraction_of_bound": bound_ms / ms,
            "torch_ms": ms_torch, "torch_over_add": ms_torch / ms, "iss_add_ms": ms_iss, "add_over_iss": ms / ms_iss,
            "kernels_ms": kernel_split(call)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    x = rain(101, 256, 256, 0.8, 1)
    tiles = rain(2 * 8334, 16, 16, 0.8, 2)                           # 8334 days x 24 hours: 200 016 tiles a side
    g = torch.Generator(device="cuda").manual_seed(3)
    sparse = 20.0 * (torch.rand((101, 24, 256, 256), generator=g, device="cuda") < 5.0 / 65536)       # about 5 wet pixels a plane
    res = {"thresholds": list(THRESHOLDS), "cases": [
        case("100 scenarios of 256 x 256", x[1:], x[0], a.reps, a.warmup),
        case("200 016 tiles of nd 16", tiles[None, 8334:], tiles[:8334], a.reps, a.warmup),
        case("100 scenarios of 256 x 256, about 5 wet pixels a plane", sparse[1:], sparse[0], a.reps, a.warmup)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
