"""Device time of chaining scenarios across midnight (sequence.py): the seam costs of one boundary at S = 100 and S = 1000 members of a
256 x 256 plane (P = 65 536) against the vector-issue bound of one packed sum of absolute differences per two pixels of a pair and
against torch.cdist(p=1) on the same features; the min-plus recurrence over 29 boundaries at S = 1000 against (acc[:, None] + C).min(0);
the greedy matching at S = 1000 (rounds and time); and chain() for 100 members x 30 days of a 256 x 256 plane.  Prints one JSON line.

    python scripts/bench_sequence.py [--size 256] [--days 30] [--members 100] [--large 1000]

Synthetic seeded fields made on the device, `--dry` of the pixel-hours dry.  Times are HIP events around the whole call, median of 10
after 3 warm-up calls (--reps / --warmup), one process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import sequence as sq

# one v_sad_u16 (two pixels of a pair) per lane and issue slot: 256 compute units x 4 SIMDs x 32 lanes a clock at 2.4 GHz
SAD_LANES_PER_S = 256 * 4 * 32 * 2.4e9


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


def rain_into(buf, dry, g):
    buf.copy_(-2.0 * torch.log1p(-torch.rand(buf.shape, generator=g, device="cuda")) * (torch.rand(buf.shape, generator=g, device="cuda") >= dry))


def edges_of(S, D, size, dry, seed, step=25):
    """a SeamEdges of S members of D days, the hourly arrays made and dropped `step` members at a time"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    e = sq.SeamEdges()
    buf = torch.empty((min(step, S), D, 24, size, size), device="cuda")
    for s0 in range(0, S, step):
        n = min(step, S - s0)
        rain_into(buf[:n], dry, g)
        e.add(buf[:n])
    return e


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
    P = a.size * a.size
    res = {"sad_lanes_per_s": SAD_LANES_PER_S, "plane": [a.size, a.size], "dry": a.dry}
    big_costs = None
    for S in (a.members, a.large):
        e = edges_of(S, 2, a.size, a.dry, S)
        ms, (costs, n_valid) = timed(lambda: sq.seam_costs(e), a.reps, a.warmup)
        bound_ms = S * S * P / 2 / SAD_LANES_PER_S * 1e3
        f = e.features.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).float()        # (S, 2, 2, P): exact in fp32
        rows, cols = f[:, 0, 1].contiguous(), f[:, 1, 0].contiguous()
        ms_t, ref = timed(lambda: torch.cdist(rows, cols, p=1), a.reps, a.warmup)
        # cdist sums 65 536 fp32 terms: it is the route to beat, not the yardstick of the values (the tests have the exact one)
        rel = float(((ref.double() - costs[0].double()).abs() / costs[0].double().clamp(min=1)).max())
        res[f"costs_S{S}"] = {"members": S, "pixels": P, "pair_pixels": S * S * P, "hip_ms": ms, "bound_ms": bound_ms, "hip_fraction_of_bound": bound_ms / ms,
                             "pair_pixels_per_s": S * S * P / (ms * 1e-3), "torch_cdist_ms": ms_t, "cdist_max_rel_diff": rel,
                             "n_valid": int(n_valid[0])}
        if S == a.large:
            big_costs = costs
        del e, f, rows, cols, ref
        torch.cuda.empty_cache()

    S = a.large
    ms, (perm, rounds) = timed(lambda: sq.greedy_matching(big_costs, return_rounds=True), a.reps, a.warmup)
    res[f"matching_S{S}"] = {"members": S, "hip_ms": ms, "rounds_launched": rounds, "matched_total": int(torch.gather(big_costs[0], 1, perm[0].long()[:, None]).sum()),
                            "diagonal_total": int(big_costs[0].diagonal().sum())}

    B = a.days - 1
    g = torch.Generator(device="cuda").manual_seed(3)
    C = torch.randint(0, 1 << 30, (B, S, S), generator=g, device="cuda", dtype=torch.int64)
    ms, (acc, back) = timed(lambda: sq.min_plus(C), a.reps, a.warmup)

    def by_torch():
        cur, backs = torch.zeros(S, dtype=torch.int64, device="cuda"), []
        for b in range(B):
            cur, i = (cur[:, None] + C[b]).min(0)
            backs.append(i)
        return cur, torch.stack(backs)

    ms_t, (cur, _) = timed(by_torch, a.reps, a.warmup)
    assert torch.equal(cur, acc[-1])
    res[f"minplus_S{S}"] = {"members": S, "boundaries": B, "read_bytes": B * S * S * 8, "hip_ms": ms, "torch_ms": ms_t}
    del C, acc, back, big_costs
    torch.cuda.empty_cache()

    S, D = a.members, a.days
    g = torch.Generator(device="cuda").manual_seed(4)
    hourly = torch.empty((S, D, 24, a.size, a.size), device="cuda")
    for s in range(S):
        rain_into(hourly[s], a.dry, g)
    ms, r = timed(lambda: sq.chain(hourly), a.reps, a.warmup)
    e = sq.SeamEdges().add(hourly)
    parts = {"edges_ms": timed(lambda: sq.SeamEdges().add(hourly), a.reps, a.warmup)[0], "costs_ms": timed(lambda: sq.seam_costs(e), a.reps, a.warmup)[0]}
    costs = sq.seam_costs(e)[0]
    parts["matching_ms"], (_, rounds) = timed(lambda: sq.greedy_matching(costs, return_rounds=True), a.reps, a.warmup)
    parts["best_path_ms"] = timed(lambda: sq.best_path(costs), a.reps, a.warmup)[0]
    res["chain"] = {"members": S, "days": D, "hourly_bytes": hourly.numel() * 4, "edge_bytes_read": S * D * 2 * P * 4, "hip_ms": ms,
                    "costs_bound_ms": (D - 1) * S * S * P / 2 / SAD_LANES_PER_S * 1e3, "rounds_launched": rounds, **parts,
                    "mm_per_h_random": float(np.nanmean(r.random)), "mm_per_h_diagonal": float(np.nanmean(r.diagonal)),
                    "mm_per_h_matched": float(np.nanmean(r.matched)), "mm_per_h_path": float(np.nanmean(r.path_cost))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
