"""Device time of the multivariate rank histograms (multivariate_ranks.py): (a) prerank_sums of `--days` days of nd x nd against
ensembles of 100 and of 1000 members; (b) one 256 x 256 day against 100 members; (c) mst_leave_one_out at N = 101 and N = 1001.
Each time stands beside a torch restatement on the same device -- for the ranks a double argsort per day (ordinal ranks: the cheapest
torch gets, and not yet the mid-ranks) and the exact restatement by sort and searchsorted, whose sums must equal the kernel's; for the
MST a Prim loop of torch calls for ONE left-out index, times N -- and, for the ranks, beside the compare-issue bound: 2 N^2
lane-operations per valid position that is not constant, at 16 lanes per SIMD and clock.  Prints one JSON line.

    python scripts/bench_mvrank.py [--nd 16] [--days 100] [--field 256] [--skip-field]

Synthetic seeded fields (gamma with dry pixels; one hour in four dry everywhere).  Times are HIP events around the whole call, median
of 10 after 3 warm-up calls (--reps / --warmup); the torch restatements run once after one warm-up."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import multivariate_ranks as mr

VALU_LANES_PER_S = 256 * 4 * 16 * 2.4e9       # 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz: 32-bit vector lane-operations per second


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


def fields(rng, shape):
    f = rng.gamma(0.5, 1.5, shape).astype(np.float32)
    f[rng.random(shape) < 0.6] = 0.0
    f[..., ::4, :, :] = 0.0                                                 # dry hours
    return torch.from_numpy(f).cuda()


def stack(ens, obs):
    """(N, P): index 0 the observation"""
    return torch.cat([obs.reshape(1, -1), ens.reshape(ens.shape[0], -1)])


def torch_argsort(ens, obs):
    """twice the ordinal rank, summed: two argsorts of the (N, P) matrix of one day"""
    z = stack(ens, obs)
    return (2 * z.argsort(dim=0).argsort(dim=0) + 2).sum(dim=1)


def torch_exact(ens, obs):
    """(N, 2): the definitions by sort and searchsorted, every position valid"""
    z = stack(ens, obs).t().contiguous()                                    # (P, N)
    s = z.sort(dim=1).values
    N = z.shape[1]
    lt = torch.searchsorted(s, z, right=False)
    gt = N - torch.searchsorted(s, z, right=True)
    return torch.stack([(lt - gt + N + 1).sum(dim=0), ((N - 1) * (N - 2) - lt * (lt - 1) - gt * (gt - 1)).sum(dim=0)], dim=1)


def ranked_positions(ens, obs):
    z = stack(ens, obs)
    return int((z != z[:1]).any(dim=0).sum())


def bench_ranks(ens, obs, reps, warmup):
    """ens (D, m, 24, ny, nx), obs (D, 24, ny, nx)"""
    D, m = ens.shape[:2]
    N = m + 1
    ms, (sums, n_valid) = timed(lambda: mr.prerank_sums(ens, obs), reps, warmup)
    ms_sort, _ = timed(lambda: [torch_argsort(ens[d], obs[d]) for d in range(D)], 1, 1)
    ms_exact, exact = timed(lambda: torch.stack([torch_exact(ens[d], obs[d]) for d in range(D)]), 1, 1)
    ranked = sum(ranked_positions(ens[d], obs[d]) for d in range(D))
    bound = 2.0 * N * N * ranked / VALU_LANES_PER_S * 1e3
    return {"days": D, "members": m, "plane": list(ens.shape[-2:]), "ms": round(ms, 3), "torch_double_argsort_ms": round(ms_sort, 3),
            "torch_sort_searchsorted_ms": round(ms_exact, 3), "torch_argsort_over_kernel": round(ms_sort / ms, 2),
            "equals_torch_exact": bool(torch.equal(exact, sums)), "valid_positions": int(n_valid.sum()), "ranked_positions": ranked,
            "compare_issue_bound_ms": round(bound, 4), "bound_over_time": round(bound / ms, 3)}


def torch_prim(dist, left):
    """Prim on the device for one left-out index, a torch call per step"""
    n = dist.shape[0]
    keep = torch.ones(n, dtype=torch.bool, device=dist.device)
    keep[left] = False
    d = dist[keep][:, keep]
    big = torch.iinfo(torch.int64).max
    key, inside, total = d[0].clone(), torch.zeros(n - 1, dtype=torch.bool, device=dist.device), torch.zeros((), dtype=torch.int64, device=dist.device)
    inside[0] = True
    for _ in range(n - 2):
        u = torch.where(inside, big, key).argmin()
        total += key[u]
        inside[u] = True
        key = torch.minimum(key, d[u])
    return total


def bench_mst(rng, n, reps, warmup):
    pts = torch.from_numpy(rng.integers(0, 65536, (n, 64))).cuda()
    dist = (pts[:, None] - pts[None, :]).abs().sum(-1)
    ms, out = timed(lambda: mr.mst_leave_one_out(dist, check=False), reps, warmup)
    ms_one, one = timed(lambda: torch_prim(dist, 0), 1, 1)
    return {"n": n, "ms": round(ms, 3), "torch_prim_one_index_ms": round(ms_one, 3), "torch_prim_all_over_kernel": round(ms_one * n / ms, 1),
            "equals_torch_prim": bool(out[0] == one)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=16)
    ap.add_argument("--days", type=int, default=100)
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-field", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(a.nd)
    res = {"metric": "multivariate_ranks", "reps": a.reps, "warmup": a.warmup, "ranks": [], "mst": []}
    for m in (100, 1000):
        ens, obs = fields(rng, (a.days, m, 24, a.nd, a.nd)), fields(rng, (a.days, 24, a.nd, a.nd))
        res["ranks"].append(bench_ranks(ens, obs, a.reps, a.warmup))
        del ens, obs
    if not a.skip_field:
        ens, obs = fields(rng, (1, 100, 24, a.field, a.field)), fields(rng, (1, 24, a.field, a.field))
        res["ranks"].append(bench_ranks(ens, obs, a.reps, a.warmup))
        del ens, obs
    for n in (101, 1001):
        res["mst"].append(bench_mst(rng, n, a.reps, a.warmup))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
