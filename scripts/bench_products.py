"""Device time of the ensemble products (field_products.py).  Two cases:

  field    256 x 256, ndomain 16, overlap 4, S = 100 scenarios of one day, every tile wet, windows (1, 3, 6, 12, 24):
           (a) the fused blend (field_products.blend_peaks_device) against field.blend_device on the same buffers -- the same reads,
               K + 1/4 planes of writes instead of 24;
           (b) field_products.ensemble_products against field.disaggregate followed by a plain-torch rolling sum (a cumulative sum
               over the hours, differences, amax) and torch.quantile over the scenarios;
  members  S = 1000 members at P = 65 536 positions, gamma values with 60 % zeros, probs (0.1, 0.5, 0.9, 0.99), thresholds (1, 10):
           (c) field_products.member_stats_device against rdgan_box_stats on the same data seen as [1][S][P] (one column per
               workgroup, 4-byte reads a whole row apart; it yields quartiles where member_stats yields the asked quantiles);
           (d) against torch.quantile (which refuses more than 16 M elements, so it runs over slices of positions) plus mean and
               exceedance in torch.

    python scripts/bench_products.py [--field 256] [--scenarios 100] [--members 1000] [--positions 65536] [--reps 10] [--warmup 3]

Synthetic seeded data, a seeded init_generator.  Times are HIP events around the whole call (host work of the call included):
median, min and max of --reps calls after --warmup, one process; prints one JSON line.  Recorded, not asserted."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import _lib, models
from pr_disagg_radar_gan_amd import field as F
from pr_disagg_radar_gan_amd import field_products as FP
from pr_disagg_radar_gan_amd import weights as W

TORCH_QUANTILE_MAX = 16_000_000          # torch.quantile's limit on the number of input elements


def timed(fn, reps, warmup):
    """-> ({median, min, max} in ms, the last result)"""
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
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}, out


def torch_peaks(hourly, windows):
    """(S, 24, ny, nx) -> (S, K, ny, nx): rolling sums as differences of the cumulative sum over the hours, then the maximum"""
    c = torch.cat([torch.zeros_like(hourly[:, :1]), hourly.cumsum(1)], 1)
    return torch.stack([(c[:, w:] - c[:, :-w]).amax(1) for w in windows], 1)


def torch_quantile(x, probs):
    """torch.quantile over axis 0 of (S, P), in slices of positions that stay below its element limit"""
    S, P_ = x.shape
    step = max(1, TORCH_QUANTILE_MAX // S)
    return torch.cat([torch.quantile(x[:, i:i + step], probs, dim=0) for i in range(0, P_, step)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--positions", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    nd, n, S = 16, a.field, a.scenarios
    windows, probs = (1, 3, 6, 12, 24), (0.1, 0.5, 0.9, 0.99)
    K = len(windows)
    rng = np.random.default_rng(0)
    gen = models.Generator(W.init_generator(rng, nd), nd)
    daily = (rng.gamma(0.6, 8.0, (1, n, n)).astype(np.float32) + np.float32(0.01))
    dd = torch.from_numpy(daily).cuda()
    plan = F.tile_plan(n, n, nd, a.overlap)
    T = plan.n_tiles
    m = S * T
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    res = {"field": [n, n], "ndomain": nd, "overlap": a.overlap, "scenarios": S, "windows": list(windows), "tiles": T,
           "reps": a.reps, "warmup": a.warmup}

    # (a) the fused blend against the blend
    frac = torch.rand((m, W.NHOURS, nd, nd), generator=g, device="cuda")
    slots = np.arange(m, dtype=np.int32).reshape(S, T)
    out = torch.empty((S, W.NHOURS, n, n), dtype=torch.float32, device="cuda")
    pk = (torch.empty((S, K, n, n), dtype=torch.float32, device="cuda"), torch.empty((S, n, n), dtype=torch.uint8, device="cuda"))
    t_blend, o_blend = timed(lambda: F.blend_device(frac, slots, plan, dd, out=out), a.reps, a.warmup)
    t_fused, o_fused = timed(lambda: FP.blend_peaks_device(frac, slots, plan, dd, windows, out=pk), a.reps, a.warmup)
    t_peaks, o_two = timed(lambda: FP.peaks_device(out, windows), a.reps, a.warmup)
    res["blend"] = dict(t_blend, bytes=frac.numel() * 4 + out.numel() * 4)
    res["blend_peaks"] = dict(t_fused, bytes=frac.numel() * 4 + pk[0].numel() * 4 + pk[1].numel())
    res["hourly_peaks"] = dict(t_peaks, bytes=out.numel() * 4 + pk[0].numel() * 4 + pk[1].numel())
    for row in ("blend", "blend_peaks", "hourly_peaks"):
        res[row]["gbs"] = res[row]["bytes"] / res[row]["median_ms"] / 1e6
    res["blend_over_blend_peaks"] = t_blend["median_ms"] / t_fused["median_ms"]
    res["fused_equals_two_kernels"] = bool(torch.equal(o_fused[0].view(torch.int32), o_two[0].view(torch.int32))
                                           and torch.equal(o_fused[1], o_two[1]))
    del frac, out, pk, o_blend, o_fused, o_two
    torch.cuda.empty_cache()

    # (b) the whole path
    z = rng.normal(size=(S, 1, W.LATENT_DIM)).astype(np.float32)
    pt = torch.tensor(probs, dtype=torch.float32, device="cuda")

    def baseline():
        hourly, _ = F.disaggregate(gen, dd, S, overlap=a.overlap, latent=z)
        peaks = torch_peaks(hourly[:, 0], windows)
        return torch.stack([torch_quantile(peaks[:, k].reshape(S, n * n), pt) for k in range(K)]).view(K, len(probs), n, n), peaks.mean(0)

    t_prod, prod = timed(lambda: FP.ensemble_products(gen, dd, S, windows, probs, overlap=a.overlap, latent=z), a.reps, a.warmup)
    t_base, base = timed(baseline, a.reps, a.warmup)
    res["ensemble_products"] = t_prod
    res["disaggregate_torch_products"] = t_base
    res["torch_over_ensemble_products"] = t_base["median_ms"] / t_prod["median_ms"]
    res["ensemble_quantiles_max_rel_diff"] = float(((prod.quantiles[0] - base[0]).abs() / base[0].abs().clamp_min(1e-30)).max())
    del prod, base
    torch.cuda.empty_cache()

    # (c), (d) member statistics
    Sm, Pm = a.members, a.positions
    thr = (1.0, 10.0)
    x = torch.from_numpy((rng.gamma(0.5, 6.0, (Sm, Pm)) * (rng.random((Sm, Pm)) > 0.6)).astype(np.float32)).cuda()
    res["members"] = {"S": Sm, "P": Pm, "probs": list(probs), "thresholds": list(thr), "bytes": x.numel() * 4}
    t_ms, st = timed(lambda: FP.member_stats_device(x, probs, thr), a.reps, a.warmup)
    lib = _lib.load()
    stats = torch.empty((Pm, 12), dtype=torch.float64, device="cuda")

    def box():
        rc = lib.rdgan_box_stats(ctypes.c_void_p(x.data_ptr()), Sm, Pm, 1, ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(0),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, None, "rdgan_box_stats")
        return stats
    t_box, bs = timed(box, a.reps, a.warmup)
    pm = torch.tensor(probs, dtype=torch.float32, device="cuda")

    def torch_stats():
        return torch_quantile(x, pm), x.mean(0), torch.stack([(x > t).float().mean(0) for t in thr])
    t_tq, tq = timed(torch_stats, a.reps, a.warmup)
    res["member_stats"] = dict(t_ms, gbs=x.numel() * 4 / t_ms["median_ms"] / 1e6)
    res["box_stats_same_data"] = dict(t_box, gbs=x.numel() * 4 / t_box["median_ms"] / 1e6)
    res["torch_quantile_mean_exceed"] = t_tq
    res["box_stats_over_member_stats"] = t_box["median_ms"] / t_ms["median_ms"]
    res["torch_over_member_stats"] = t_tq["median_ms"] / t_ms["median_ms"]
    res["median_max_abs_diff_vs_box_stats"] = float((st.quantiles[1].double() - bs[:, 3]).abs().max())
    res["quantiles_max_rel_diff_vs_torch"] = float(((st.quantiles - tq[0]).abs() / tq[0].abs().clamp_min(1e-30)).max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
