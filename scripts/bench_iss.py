"""Device time of the intensity-scale state (intensity_scale.py): IntensityScaleVerifier.add of 100 scenarios of one 256 x 256 day
at 4 thresholds with L = 6 and L = 8, and of 200 000 tiles of nd 16 (one member of 8334 days) at L = 4, each beside a torch
restatement of the same state in the same run (avg_pool2d of the two event fields per level, squared and summed) and beside the
bound of reading the members once and the observation once at 6.3 TB/s.  Prints one JSON line.

    python scripts/bench_iss.py [--reps 10] [--warmup 3]

Synthetic seeded spells made on the device (as scripts/bench_sal.py makes them), without bad values: the torch restatement has no
void rule.  Times are HIP events around the whole call, the state's and the workspace's allocation included, median of 10 after 3
warm-up calls (--reps / --warmup), one process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import intensity_scale as IS
from scripts.bench_sal import rain, timed

THRESHOLDS = (0.1, 1.0, 5.0, 10.0)
HBM = 6.3e12


def torch_state(ens, obs, thresholds, L):
    """counts (T, 24, L + 1, 3) int64 of planes whose sides are multiples of 2^L and hold no bad value"""
    s, ny, nx = ens.shape[0], ens.shape[-2], ens.shape[-1]
    out = torch.zeros((len(thresholds), 24, L + 1, 3), dtype=torch.int64, device=ens.device)
    o = obs.reshape(-1, 24, ny, nx)
    e = ens.reshape(s, -1, 24, ny, nx)
    for t, u in enumerate(thresholds):
        eo = (o > u).to(torch.float32).reshape(-1, 1, ny, nx)
        for m in range(s):                                           # member by member: the pooled fields of one are held
            ex = (e[m] > u).to(torch.float32).reshape(-1, 1, ny, nx)
            for l in range(L + 1):
                k = 1 << l
                sx = torch.nn.functional.avg_pool2d(ex, k, divisor_override=1) if l else ex
                so = torch.nn.functional.avg_pool2d(eo, k, divisor_override=1) if l else eo
                sx, so = sx.to(torch.float64), so.to(torch.float64)             # (a block sum is exact in fp32, its square is not)
                q = torch.stack([sx * sx, so * so, sx * so], dim=-1)
                out[t, :, l] += q.view(-1, 24, q.shape[-3] * q.shape[-2], 3).sum(dim=(0, 2)).to(torch.int64)
    return out


def case(name, ens, obs, L, reps, warmup):
    call = lambda: IS.IntensityScaleVerifier(obs, THRESHOLDS, L).add(ens)
    ms, ver = timed(call, reps, warmup)
    ms_torch, ref = timed(lambda: torch_state(ens, obs, THRESHOLDS, L), max(1, reps // 3), 1)
    assert torch.equal(ver.state()[0], ref), name
    nbytes = 4 * (ens.numel() + obs.numel())
    bound_ms = nbytes / HBM * 1e3
    return {"case": name, "levels": L, "read_bytes": nbytes, "add_ms": ms, "torch_ms": ms_torch, "torch_over_add": ms_torch / ms,
            "bound_ms": bound_ms, "fraction_of_bound": bound_ms / ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    x = rain(101, 256, 256, 0.8, 1)
    tiles = rain(2 * 8334, 16, 16, 0.8, 2)                           # 8334 days x 24 hours: 200 016 tiles a side
    res = {"thresholds": list(THRESHOLDS), "cases": [
        case("100 scenarios of 256 x 256, L = 6", x[1:], x[0], 6, a.reps, a.warmup),
        case("100 scenarios of 256 x 256, L = 8", x[1:], x[0], 8, a.reps, a.warmup),
        case("200 016 tiles of nd 16, L = 4", tiles[None, 8334:], tiles[:8334], 4, a.reps, a.warmup)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
