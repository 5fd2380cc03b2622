"""Device time of the joint-field scores (multivariate.py): (a) the energy score of one day, m members at nd x nd, against
torch.cdist in fp64 on the same device and against the fp64 vector-FMA issue bound (two instructions per pair-component); (b) the
variogram score of the same day (radius 2, lag 1, p = 0.5) against a torch restatement of ONE displacement by shifted slices; (c) the
shared-ensemble forms for many days against one climatological ensemble.  Prints one JSON line.

    python scripts/bench_multivariate.py [--nd 16] [--members 1000] [--days 1000] [--clim 5000] [--skip-shared]

Synthetic seeded fields (gamma with dry pixels).  Times are HIP events around the whole call, median of 10 after 3 warm-up calls
(--reps / --warmup)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import multivariate as mv

FP64_FMA_PER_S = 256 * 4 * 16 * 2.4e9         # 256 CUs x 4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz: vector fp64 instructions (lanes) per second


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nd", type=int, default=16)
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--days", type=int, default=1000)
    ap.add_argument("--clim", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-shared", action="store_true")
    a = ap.parse_args()
    nd, m = a.nd, a.members
    rng = np.random.default_rng(nd)

    def fields(count):
        f = rng.gamma(0.5, 1.5, (count, 24, nd, nd)).astype(np.float32)
        f[rng.random(f.shape) < 0.6] = 0.0
        return torch.from_numpy(f).cuda()

    ens, obs = fields(m), fields(1)[0]
    d = 24 * nd * nd
    ms_es, (so, sp) = timed(lambda: mv.energy_terms(ens, obs), a.reps, a.warmup)

    def es_torch():
        x = torch.cat([ens.reshape(m, d), obs.reshape(1, d)]).double()
        dist = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist")
        return dist[m, :m].sum(), torch.triu(dist[:m, :m], 1).sum()

    ms_es_torch, (to, tp) = timed(es_torch, a.reps, a.warmup)
    pair_components = (m + 1) * m / 2 * d
    bound_ms = 2 * pair_components / FP64_FMA_PER_S * 1e3
    res = {"metric": "multivariate_scores", "nd": nd, "members": m, "reps": a.reps, "warmup": a.warmup,
           "energy_ms": round(ms_es, 3), "energy_torch_cdist_fp64_ms": round(ms_es_torch, 3), "energy_torch_over_kernel": round(ms_es_torch / ms_es, 2),
           "energy_fp64_issue_bound_ms": round(bound_ms, 3), "energy_bound_over_time": round(bound_ms / ms_es, 3),
           "energy_rel_diff_torch": [abs(so.item() - to.item()) / to.item(), abs(sp.item() - tp.item()) / tp.item()]}

    ms_vs, (vs, sq, cnt) = timed(lambda: mv.variogram_score(ens, obs, p=0.5, radius=2, max_lag=1, return_tables=True), a.reps, a.warmup)

    def vs_torch_one():                                                    # the displacement (1, 1, 2) alone
        va = (ens[:, :-1, :-1, :-2] - ens[:, 1:, 1:, 2:]).abs().sqrt().double().mean(0)
        o = (obs[:-1, :-1, :-2] - obs[1:, 1:, 2:]).abs().sqrt().double()
        return ((o - va) ** 2).sum()

    ms_vs_torch, one = timed(vs_torch_one, a.reps, a.warmup)
    n_disp = len(mv.displacements(2, 1))
    res.update({"variogram_ms": round(ms_vs, 3), "variogram_displacements": n_disp, "variogram_torch_one_displacement_ms": round(ms_vs_torch, 3),
                "variogram_torch_all_over_kernel": round(ms_vs_torch * n_disp / ms_vs, 2),
                "variogram_rel_diff_torch": abs(sq[0, 1, 3, 4].item() - one.item()) / one.item(),
                "variogram_gsqrt_per_s": round(m * cnt.sum().item() / ms_vs / 1e6, 1)})
    if not a.skip_shared:
        del ens
        clim, days = fields(a.clim), fields(a.days)
        ms_se, _ = timed(lambda: mv.energy_terms(clim, days), max(a.reps // 3, 1), 1)
        ms_sv, _ = timed(lambda: mv.variogram_score(clim, days, p=0.5, radius=2, max_lag=1), max(a.reps // 3, 1), 1)
        pc = (a.clim * (a.clim - 1) / 2 + a.clim * a.days) * d
        res["shared"] = {"members": a.clim, "days": a.days, "energy_ms": round(ms_se, 3), "energy_fp64_issue_bound_ms": round(2 * pc / FP64_FMA_PER_S * 1e3, 3),
                         "variogram_ms": round(ms_sv, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
