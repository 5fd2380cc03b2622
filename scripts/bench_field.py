"""Device time of whole-field disaggregation (field.py) on a 256 x 256 field, ndomain 16, overlap 4, S = 100 scenarios
of D = 1 day, every tile wet: (a) the blend alone (field.blend_device, one call for the 100 units) as GB/s over the bytes it must
move -- the fraction buffer read once plus the output written once -- against a plain torch restatement of the same blend on the
same buffers (one weighted index_add_ over the tiles' pixels, then the multiplication by the daily plane); (b) the whole
field.disaggregate call, and the generator forwards of the same batches alone, which gives the split.  Prints one JSON line.
Recorded, not asserted.

    python scripts/bench_field.py [--field 256] [--scenarios 100] [--overlap 4] [--reps 10] [--warmup 3]

Synthetic seeded data, a seeded init_generator.  Times are HIP events around the whole call (host work of the call included), median
of --reps after --warmup calls, one process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import field as F
from pr_disagg_radar_gan_amd import models
from pr_disagg_radar_gan_amd import weights as W

HBM_ACHIEVABLE_GBS = 6290.0            # float4 copy on an MI355X (8 000 spec)


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


def torch_blend_tables(plan, device):
    """per (tile, i, j): the flat pixel it lands on and its weight wy * wx (fp32, as the kernel forms it)"""
    nd = plan.ndomain
    wy = np.zeros((plan.n_ty, nd), np.float32)
    wx = np.zeros((plan.n_tx, nd), np.float32)
    for tab_i, tab_w, origins, w in ((plan.ytab_idx, plan.ytab_w, plan.y_origins, wy), (plan.xtab_idx, plan.xtab_w, plan.x_origins, wx)):
        for c in range(tab_i.shape[0]):
            for k in range(tab_i.shape[1]):
                if tab_i[c, k] >= 0:
                    w[tab_i[c, k], c - origins[tab_i[c, k]]] = tab_w[c, k]
    ys = plan.y_origins[:, None] + np.arange(nd)[None]               # (n_ty, nd)
    xs = plan.x_origins[:, None] + np.arange(nd)[None]
    pix = ys[:, None, :, None] * plan.nx + xs[None, :, None, :]     # (n_ty, n_tx, nd, nd)
    wgt = wy[:, None, :, None] * wx[None, :, None, :]
    return torch.from_numpy(pix.reshape(-1).astype(np.int64)).to(device), torch.from_numpy(wgt.reshape(plan.n_tiles, 1, nd, nd)).to(device)


def torch_blend(frac, slots_dev, plan, daily, pix, wgt):
    """the blend in plain torch: gather the units' tiles, weight them, index_add_ them onto the field, multiply by the daily plane"""
    units, T, nd = slots_dev.shape[0], plan.n_tiles, plan.ndomain
    src = frac[slots_dev.reshape(-1)].view(units, T, W.NHOURS, nd, nd) * wgt[None]
    src = src.permute(0, 2, 1, 3, 4).reshape(units, W.NHOURS, T * nd * nd)
    out = torch.zeros((units, W.NHOURS, plan.ny * plan.nx), dtype=torch.float32, device=frac.device)
    out.index_add_(2, pix, src)
    return out.view(units, W.NHOURS, plan.ny, plan.nx) * daily[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    nd, n, S = 16, a.field, a.scenarios
    rng = np.random.default_rng(0)
    gen = models.Generator(W.init_generator(rng, nd), nd)
    daily = (rng.gamma(0.6, 8.0, (1, n, n)).astype(np.float32) + np.float32(0.01))
    dd = torch.from_numpy(daily).cuda()
    plan = F.tile_plan(n, n, nd, a.overlap)
    T = plan.n_tiles
    m = S * T
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    frac = torch.rand((m, W.NHOURS, nd, nd), generator=g, device="cuda")
    slots = np.arange(m, dtype=np.int32).reshape(S, T)
    out = torch.empty((S, W.NHOURS, n, n), dtype=torch.float32, device="cuda")
    res = {"field": [n, n], "ndomain": nd, "overlap": a.overlap, "scenarios": S, "days": 1, "tiles": T, "generator_rows": m}

    t_blend, o_hip = timed(lambda: F.blend_device(frac, slots, plan, dd, out=out), a.reps, a.warmup)
    nbytes = frac.numel() * 4 + out.numel() * 4
    res["blend_ms"] = t_blend
    res["blend_bytes"] = nbytes
    res["blend_gbs"] = nbytes / t_blend / 1e6
    res["blend_fraction_of_copy_rate"] = res["blend_gbs"] / HBM_ACHIEVABLE_GBS
    pix, wgt = torch_blend_tables(plan, dd.device)
    slots_dev = torch.from_numpy(slots.astype(np.int64)).cuda()
    t_torch, o_torch = timed(lambda: torch_blend(frac, slots_dev, plan, dd, pix, wgt), a.reps, a.warmup)
    res["torch_blend_ms"] = t_torch
    res["torch_over_hip"] = t_torch / t_blend
    res["torch_blend_max_rel_diff"] = float(((o_torch - o_hip).abs() / o_hip.abs().clamp_min(1e-30)).max())
    del o_torch, pix, wgt, slots_dev, frac
    torch.cuda.empty_cache()

    z = rng.normal(size=(S, 1, W.LATENT_DIM)).astype(np.float32)
    out5 = out.view(S, 1, W.NHOURS, n, n)
    t_all, (o, info) = timed(lambda: F.disaggregate(gen, dd, S, overlap=a.overlap, latent=z, out=out5), max(3, a.reps // 3), 1)
    res["disaggregate_ms"] = t_all
    res["n_active"] = info.n_active
    total = o[:, 0].sum(1)
    res["mass_max_rel_err"] = float(((total - dd) .abs() / dd).max())

    # the generator forwards of the same batches alone: groups of whole units of at most 1024 rows
    groups = F._group_units([T] * S, 1024)
    rows = max((u1 - u0) * T for u0, u1 in groups)
    eng = models.get_engine(nd, min(1024, rows))
    slab = gen.device_slab(eng)
    zz = torch.randn((rows, W.LATENT_DIM), generator=g, device="cuda")
    cc = torch.rand((rows, nd, nd, 1), generator=g, device="cuda")
    ff = torch.empty((rows, W.NHOURS, nd, nd, 1), dtype=torch.float32, device="cuda")

    def forwards():
        for u0, u1 in groups:
            k = (u1 - u0) * T
            for i in range(0, k, eng.max_batch):
                j = min(eng.max_batch, k - i)
                eng.gen_forward(slab, zz[i:i + j], cc[i:i + j], out=ff[i:i + j], gen_version=gen._version)
                eng.check_numerics()
    t_fwd, _ = timed(forwards, max(3, a.reps // 3), 1)
    res["forwards_alone_ms"] = t_fwd
    res["groups"] = len(groups)
    res["forward_share"] = t_fwd / t_all
    print(json.dumps(res))


if __name__ == "__main__":
    main()
