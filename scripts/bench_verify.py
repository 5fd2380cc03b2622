"""Device time of the verification of field ensembles (verification.py) at the project's field workload: S scenarios
of one 256 x 256 day (ndomain 16, overlap 4, a seeded init_generator), T = 4 thresholds, scales (1, 3, 5, 9, 17, 33, 65).

  (a) rdgan_verify_accumulate on the held ensemble -- at once and in groups of 16 members, as verify_field feeds it -- with the
      bytes it has to move (members and observation read, T + 2 counters read and written) over its time, beside a plain torch
      formulation of the same counts on the same tensors (comparisons summed over the member axis);
  (b) rdgan_verify_reduce;
  (c) rdgan_verify_fss for the scale 3 alone, 65 alone and all seven, beside torch box sums (avg_pool2d with divisor 1 on the same
      C and E planes, exact in fp32 at these counts; its fp64 totals differ in the last bits once they pass 2^53) for 3 and 65;
  (d) the same at --members-large members, accumulated in chunks of --scenarios;
  (e) verify_field against field.disaggregate run over the same scenario chunks into the same buffer (what verification adds to
      it) and against one disaggregate call for all scenarios (what a user would otherwise run; the chunks cost a tile scan, a
      latent upload and the engine set-up each).

    python scripts/bench_verify.py [--field 256] [--scenarios 100] [--members-large 1000] [--reps 10] [--warmup 3] [--out FILE]

Times are HIP events around the whole call (host work of the call included): median, min and max of --reps calls after --warmup, one
process.  Appends one JSON line to --out and prints it.  Recorded, not asserted; the equalities it reports are asserted by the tests."""
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
from pr_disagg_radar_gan_amd import verification as V
from pr_disagg_radar_gan_amd import weights as W


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


def torch_state(x, o, thr):
    exceed = torch.stack([(x > t).sum(0, dtype=torch.int32) for t in thr])
    return exceed, (x < o).sum(0, dtype=torch.int32), (x == o).sum(0, dtype=torch.int32), (torch.isnan(x).any(0) | torch.isnan(o)).to(torch.uint8)


def torch_fss(o, exceed, bad, S, thr, w):
    """(T, 24, 2) float64 sums of one width by zero-padded box sums of the planes"""
    ok = bad == 0
    out = []
    for t, th in enumerate(thr):
        C = torch.where(ok, exceed[t], 0).to(torch.float32)[:, None]
        E = (ok & (o > th)).to(torch.float32)[:, None]
        bc = torch.nn.functional.avg_pool2d(C, w, stride=1, padding=w // 2, divisor_override=1).double()
        be = torch.nn.functional.avg_pool2d(E, w, stride=1, padding=w // 2, divisor_override=1).double() * S
        out.append(torch.stack([((bc - be) ** 2).sum(dim=(1, 2, 3)), (bc ** 2 + be ** 2).sum(dim=(1, 2, 3))], 1))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=100)
    ap.add_argument("--members-large", type=int, default=1000)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_bench_verify.jsonl"))
    a = ap.parse_args()
    nd, n, S = 16, a.field, a.scenarios
    thr, scales = (0.1, 1.0, 5.0, 10.0), (1, 3, 5, 9, 17, 33, 65)
    T = len(thr)
    rng = np.random.default_rng(0)
    gen = models.Generator(W.init_generator(rng, nd), nd)
    obs = (rng.gamma(0.5, 2.0, (W.NHOURS, n, n)) * (rng.random((W.NHOURS, n, n)) < 0.5)).astype(np.float32)
    od = torch.from_numpy(obs).cuda()
    daily = od.sum(0)
    z = rng.normal(size=(S, 1, W.LATENT_DIM)).astype(np.float32)
    ens, _ = F.disaggregate(gen, daily, S, overlap=a.overlap, latent=z)
    P_ = od.numel()
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    thr64 = V.check_event_thresholds(thr)
    hthr = thr64.ctypes.data_as(ctypes.c_void_p)
    res = {"field": [n, n], "ndomain": nd, "overlap": a.overlap, "scenarios": S, "thresholds": list(thr), "scales": list(scales),
           "positions": P_, "reps": a.reps, "warmup": a.warmup}

    # (a) accumulate
    ver = V.EnsembleVerifier(od, thr)
    exceed, below, equal, bad = ver.state()

    def accumulate(x):
        rc = lib.rdgan_verify_accumulate(p(x), x.shape[0], x.stride(0), P_, p(od), hthr, T, p(exceed), p(below), p(equal), p(bad), st())
        _lib.check(rc, None, "rdgan_verify_accumulate")

    def in_groups(step):
        for s0 in range(0, S, step):
            accumulate(ens[s0:s0 + step])

    groups = (S + 15) // 16
    state_bytes = (T + 2) * P_ * 4 * 2
    t_once, _ = timed(lambda: accumulate(ens), a.reps, a.warmup)
    t_grp, _ = timed(lambda: in_groups(16), a.reps, a.warmup)
    t_torch, ts = timed(lambda: torch_state(ens, od, thr), a.reps, a.warmup)
    res["accumulate"] = dict(t_once, bytes=ens.numel() * 4 + P_ * 4 + state_bytes)
    res["accumulate_groups_of_16"] = dict(t_grp, bytes=ens.numel() * 4 + groups * (P_ * 4 + state_bytes))
    for row in ("accumulate", "accumulate_groups_of_16"):
        res[row]["gbs"] = res[row]["bytes"] / res[row]["median_ms"] / 1e6
    res["torch_counts_same_tensors"] = t_torch
    res["torch_over_accumulate"] = t_torch["median_ms"] / t_once["median_ms"]
    for t in ver.state():
        t.zero_()
    accumulate(ens)
    res["accumulate_equals_torch"] = bool(all(torch.equal(g, w) for g, w in zip(ver.state(), ts)))
    ver.n_members = S
    del ts

    # (b), (c) reduce and FSS on that state
    def reduce_and_fss(S_all, widths, n_bins=11):
        wd = V.check_scales(widths, S_all)
        rank = torch.empty((W.NHOURS, S_all + 1), dtype=torch.int64, device="cuda")
        rel = torch.empty((T, W.NHOURS, n_bins, 3), dtype=torch.int64, device="cuda")
        brier = torch.empty((T, W.NHOURS, 4), dtype=torch.int64, device="cuda")
        fss = torch.empty((T, len(wd), W.NHOURS, 2), dtype=torch.float64, device="cuda")
        nbytes = lib.rdgan_verify_fss_workspace_bytes(n, n, T, len(wd))
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")

        def red():
            rc = lib.rdgan_verify_reduce(p(od), p(exceed), p(below), p(equal), p(bad), P_, n * n, S_all, hthr, T, n_bins, 0, p(rank), p(rel),
                                         p(brier), st())
            _lib.check(rc, None, "rdgan_verify_reduce")

        def fs():
            rc = lib.rdgan_verify_fss(p(od), p(exceed), p(bad), 1, n, n, S_all, hthr, T, wd.ctypes.data_as(ctypes.c_void_p), len(wd), p(fss),
                                      p(ws), nbytes, st())
            _lib.check(rc, None, "rdgan_verify_fss")
            return fss
        return red, fs

    red, fs_all = reduce_and_fss(S, scales)
    res["reduce"] = timed(red, a.reps, a.warmup)[0]
    res["fss_all_scales"], f_all = timed(fs_all, a.reps, a.warmup)
    f_all = f_all.clone()
    for i, w in ((1, 3), (6, 65)):
        t_w, f_w = timed(reduce_and_fss(S, (w,))[1], a.reps, a.warmup)
        t_tw, f_t = timed(lambda: torch_fss(od, exceed, bad, S, thr, w), a.reps, a.warmup)
        res[f"fss_w{w}"] = t_w
        res[f"torch_avg_pool2d_w{w}"] = t_tw
        res[f"fss_w{w}_equals_all_scales"] = bool(torch.equal(f_w[:, 0], f_all[:, i]))
        res[f"fss_w{w}_max_rel_diff_vs_torch"] = float(((f_w[:, 0] - f_t).abs() / f_t.abs().clamp_min(1.0)).max())
        res[f"fss_w{w}_largest_sum_over_2_53"] = float(f_w.max()) / 2.0 ** 53
    res["fss_w65_over_w3"] = res["fss_w65"]["median_ms"] / res["fss_w3"]["median_ms"]
    res["torch_w65_over_w3"] = res["torch_avg_pool2d_w65"]["median_ms"] / res["torch_avg_pool2d_w3"]["median_ms"]

    # (d) the large ensemble, accumulated in chunks of S (the same buffer each time: the kernel's work does not depend on the values)
    SL = a.members_large
    chunks = SL // S
    red_l, fs_l = reduce_and_fss(chunks * S, scales)
    res["large"] = {"members": chunks * S, "chunk": S}
    t_l, _ = timed(lambda: [accumulate(ens) for _ in range(chunks)], max(2, a.reps // 3), 1)
    res["large"]["accumulate"] = dict(t_l, gbs=chunks * res["accumulate"]["bytes"] / t_l["median_ms"] / 1e6)
    for t in ver.state():
        t.zero_()
    for _ in range(chunks):
        accumulate(ens)
    res["large"]["reduce"] = timed(red_l, a.reps, a.warmup)[0]
    res["large"]["fss_all_scales"] = timed(fs_l, a.reps, a.warmup)[0]
    del ens
    torch.cuda.empty_cache()

    # (e) the whole path: what verification adds to the disaggregation it rides on
    step = 16
    buf = torch.empty((step, W.NHOURS, n, n), dtype=torch.float32, device="cuda")

    def disaggregate_chunks():
        for s0 in range(0, S, step):
            k = min(step, S - s0)
            F.disaggregate(gen, daily, k, overlap=a.overlap, latent=z[s0:s0 + k], out=buf[:k])

    t_dis, _ = timed(disaggregate_chunks, a.reps, a.warmup)
    t_one, _ = timed(lambda: F.disaggregate(gen, daily, S, overlap=a.overlap, latent=z), a.reps, a.warmup)      # holds the 0.63 GB
    t_vf, v = timed(lambda: V.verify_field(gen, od, S, thr, scales=scales, latent=z, scenario_chunk=step, overlap=a.overlap), a.reps, a.warmup)
    res["disaggregate_same_chunks"] = t_dis
    res["verify_field"] = t_vf
    res["disaggregate_one_call"] = t_one
    res["verify_field_over_disaggregate_same_chunks"] = t_vf["median_ms"] / t_dis["median_ms"]
    res["verify_field_over_disaggregate_one_call"] = t_vf["median_ms"] / t_one["median_ms"]
    res["fss"] = [[None if np.isnan(f) else round(float(f), 4) for f in row] for row in v.fss()]
    res["brier"] = [round(float(b), 5) for b in v.brier()[0]]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
