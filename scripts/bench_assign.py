"""Device time of the least-cost assignment (sequence.optimal_matching) at S = 100 members with 29 boundaries
and at S = 1000 with 1 and with 29, each beside greedy_matching on the same costs and beside the host route it replaces --
costs.cpu() and scipy.optimize.linear_sum_assignment per boundary, where scipy imports (host clock, the copy included).  Per case:
the search steps (worked out by the numpy restatement, tests/assign_np.py; the most of any boundary is what one workgroup walks),
time per step, and the matched mean of greedy and optimal in mm/h per valid pixel.  Prints one JSON line.

    python scripts/bench_assign.py [--size 256] [--days 30] [--members 100] [--large 1000]

The costs are seam costs of the synthetic seeded fields of scripts/bench_sequence.py, `--dry` of the pixel-hours dry.  Device times
are HIP events around the whole call, median of 10 after 3 warm-up calls (--reps / --warmup), one process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch

from bench_sequence import edges_of, timed
from pr_disagg_radar_gan_amd import sequence as sq
from tests import assign_np as an

try:
    from scipy.optimize import linear_sum_assignment
except ImportError:
    linear_sum_assignment = None


def host_route(costs, reps, warmup):
    """median wall time, ms, of copying the costs to the host and solving every boundary there; the totals"""
    ts = []
    for n in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        C = costs.cpu().numpy()
        totals = [int(c[linear_sum_assignment(c)].sum()) for c in C]
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[warmup:])), totals


def case(costs, n_valid, reps, warmup):
    B, S = costs.shape[:2]
    ms, (perm, total, u, v) = timed(lambda: sq.optimal_matching(costs, return_duals=True), reps, warmup)
    ms_g, greedy = timed(lambda: sq.greedy_matching(costs), reps, warmup)
    C = costs.cpu().numpy()
    want = an.optimal_matching(C)
    for b in range(B):
        an.check_certificate(C[b], perm[b].cpu().numpy(), u[b].cpu().numpy(), v[b].cpu().numpy())
    assert np.array_equal(perm.cpu().numpy(), want[0]) and np.array_equal(total.cpu().numpy(), want[1])
    steps = want[4]
    per_pixel = lambda q: float((torch.gather(costs, 2, q.long()[..., None]).sum(dim=(1, 2)).double() / (S * sq.UNIT * n_valid.double())).mean())
    out = {"members": S, "boundaries": B, "optimal_ms": ms, "greedy_ms": ms_g, "steps_total": int(steps.sum()), "steps_max": int(steps.max()),
           "us_per_step_of_the_longest_boundary": ms * 1e3 / int(steps.max()), "mm_per_h_greedy": per_pixel(greedy), "mm_per_h_optimal": per_pixel(perm),
           "distinct_costs_share": float(np.unique(C[0]).size / C[0].size)}
    if linear_sum_assignment is not None:
        out["host_scipy_ms"], totals = host_route(costs, reps, warmup)
        assert totals == want[1].tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--members", type=int, default=100)
    ap.add_argument("--large", type=int, default=1000)
    ap.add_argument("--dry", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"plane": [a.size, a.size], "dry": a.dry, "scipy": linear_sum_assignment is not None}
    for S in (a.members, a.large):
        e = edges_of(S, a.days, a.size, a.dry, S)
        costs, n_valid = sq.seam_costs(e)
        del e
        torch.cuda.empty_cache()
        if S == a.large:
            res[f"S{S}_B1"] = case(costs[:1], n_valid[:1], a.reps, a.warmup)
        res[f"S{S}_B{a.days - 1}"] = case(costs, n_valid, a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
