"""Device time of scenario reduction (reduction.py): S = 100 and S = 1000 scenarios of one 256 x 256 day at pool 1 and pool 4, k = 20.
Features, distances and selection are timed separately: the features against the bytes they read, the distances against the
vector-issue bound of one packed sum of absolute differences per two positions of a pair (only the tiles on and above the diagonal
are computed, so the bound counts S (S + 1) / 2 pairs rounded up to whole 64 x 64 tiles) and against torch.cdist(p=1) on the same
features, the selection against a torch.minimum(...).sum(1).argmin() loop on the same matrix.  Prints one JSON line.

    python scripts/bench_reduction.py [--size 256] [--members 100] [--large 1000] [--k 20]

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

from pr_disagg_radar_gan_amd import reduction as rd

# one v_sad_u16 (two positions of a pair) per lane and issue slot: 256 compute units x 4 SIMDs x 32 lanes a clock at 2.4 GHz
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


def torch_select(dist, k):
    """the selection restated in torch on the device: one minimum, row sum and argmin a step, the selected rows pushed out of reach"""
    S = dist.shape[0]
    m = torch.full((S,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dist.device)
    out = torch.zeros(S, dtype=torch.bool, device=dist.device)
    chosen = []
    for _ in range(k):
        z = torch.minimum(dist, m[None, :]).sum(1)
        u = torch.where(out, torch.iinfo(torch.int64).max, z).argmin()
        m = torch.minimum(m, dist[u])
        out[u] = True
        chosen.append(u)
    return torch.stack(chosen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--members", type=int, default=100)
    ap.add_argument("--large", type=int, default=1000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--dry", type=float, default=0.7)
    ap.add_argument("--step", type=int, default=25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"sad_lanes_per_s": SAD_LANES_PER_S, "day": [24, a.size, a.size], "dry": a.dry, "k": a.k}
    buf = torch.empty((a.step, 24, a.size, a.size), device="cuda")
    for S in (a.members, a.large):
        for pool in (1, 4):
            g = torch.Generator(device="cuda").manual_seed(S)
            feats = rd.ScenarioFeatures(pool)
            for s0 in range(0, S, a.step):
                n = min(a.step, S - s0)
                rain_into(buf[:n], a.dry, g)
                feats.add(buf[:n])
            # the features of one buffer of members (the last made), a state of their own each call
            n = min(a.step, S)
            ms_f, _ = timed(lambda: rd.ScenarioFeatures(pool).add(buf[:n]), a.reps, a.warmup)
            pf = feats.n_positions
            ms_d, (dist, n_valid) = timed(lambda: rd.member_distances(feats), a.reps, a.warmup)
            tiles = -(-S // 64)
            bound_ms = tiles * (tiles + 1) / 2 * 64 * 64 * pf / 2 / SAD_LANES_PER_S * 1e3
            f = feats.features.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).float()[:, :pf]    # exact in fp32
            cdist_reps = a.reps if S * S * pf < 1 << 36 else min(a.reps, 3)               # (seconds a call at S = 1000: fewer of them)
            ms_c, ref = timed(lambda: torch.cdist(f, f, p=1), cdist_reps, 1)
            # cdist sums fp32 terms: it is the route to beat, not the yardstick of the values (the tests have the exact one)
            rel = float(((ref.double() - dist.double()).abs() / dist.double().clamp(min=1)).max())
            del f, ref
            k = min(a.k, S)
            ms_s, r = timed(lambda: rd.select(dist, k, n_valid), a.reps, a.warmup)
            ms_t, chosen_t = timed(lambda: torch_select(dist, k).cpu(), a.reps, a.warmup)
            assert chosen_t.tolist() == r.chosen.tolist()
            res[f"S{S}_pool{pool}"] = {
                "members": S, "pool": pool, "positions": pf, "n_valid": int(n_valid),
                "features_members": n, "features_ms": ms_f, "features_read_gb_per_s": n * 24 * a.size * a.size * 4 / (ms_f * 1e-3) / 1e9,
                "distances_ms": ms_d, "distances_bound_ms": bound_ms, "distances_fraction_of_bound": bound_ms / ms_d,
                "pair_positions_per_s": S * S * pf / (ms_d * 1e-3), "torch_cdist_ms": ms_c, "torch_cdist_reps": cdist_reps, "cdist_max_rel_diff": rel,
                "select_ms": ms_s, "torch_select_ms": ms_t, "chosen": r.chosen.tolist(), "counts": r.counts.tolist(),
                "mean_distance_mm_first_last": [float(r.mean_distance_mm[0]), float(r.mean_distance_mm[-1])]}
            del feats, dist
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
