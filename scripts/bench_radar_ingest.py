"""Device time of the radar ingest (data_pipeline.hourly_from_radar_codes, csrc/rdgan_radar.hip.h):
 (1) k_radar_hourly alone on device-resident codes, each of its three paths (16 / 4 / 1 codes per lane, forced by the alignment of the
     view handed in), as GB/s of the algorithmic bytes n_days * ny * nx * (288 + 96 + 4), alternating with a torch device-to-device
     copy that moves the same number of bytes; on "radar" codes (mostly dry, rain cells, a missing border) and on uniformly random
     codes (the worst case for the data-dependent LDS lookup);
 (2) end to end from a host array, chunked, against the host-to-device copies alone (pinned, same bytes, same chunks) and the host
     staging copies alone;
 (3) the numpy restatement (tests/radar_np.py) of one day on the host, scaled to the run's days;
 (4) the valid-tile scan at (ndomain, stride) = (16, 16) and (16, 1): k_valid_tiles_daily against k_valid_tiles on the same array.
Prints one JSON line.  Recorded, not asserted.

    python scripts/bench_radar_ingest.py [--days 365] [--ny 880] [--nx 480] [--host-days 24] [--reps 5] [--warmup 2]

Times are HIP events around the call, median of --reps after --warmup calls."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pr_disagg_radar_gan_amd import data_pipeline as dp
from pr_disagg_radar_gan_amd._dev import ptr

HBM_ACHIEVABLE_GBS = 6290.0            # float4 copy on an MI355X (8 000 spec)
FPH = 12


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(fns, reps, warmup):
    """median ms of each of fns, calls interleaved a, b, a, b, ..."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            ts[k].append(event_ms(f)[0])
    return [float(np.median(t)) for t in ts]


def fill_codes(view, pattern, seed=0):
    """view: uint8 device tensor (n_days, 288, ny, nx), filled a few days at a time"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_days, fpd, ny, nx = view.shape
    step = max(1, (1 << 30) // (fpd * ny * nx))
    for d0 in range(0, n_days, step):
        part = view[d0:d0 + step]
        if pattern == "uniform":
            part.copy_(torch.randint(0, 256, part.shape, generator=g, device="cuda", dtype=torch.uint8))
            continue
        r = torch.randint(0, 256, part.shape, generator=g, device="cuda", dtype=torch.uint8)
        part.copy_(torch.where(r < 13, r * 6 + 1, torch.zeros_like(r)))            # 5 % drizzle codes 1..73
        del r
        for d in range(part.shape[0]):                                              # a rain cell of six hours per day, but every 7th
            if (d0 + d) % 7 == 3:
                continue
            y0, x0, h0 = (37 * (d0 + d)) % (ny - ny // 4), (53 * (d0 + d)) % (nx - nx // 4), ((d0 + d) % 18) * FPH
            shape = (6 * FPH, ny // 4, nx // 4)
            cell = torch.empty(shape, device="cuda").normal_(150, 12, generator=g).clamp_(0, 254)
            part[d, h0:h0 + 6 * FPH, y0:y0 + ny // 4, x0:x0 + nx // 4] = cell.to(torch.uint8)
        part[:, :, :, :nx // 16] = 255                                              # outside the composite's coverage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--days", type=int, default=365)
    ap.add_argument("--ny", type=int, default=880)
    ap.add_argument("--nx", type=int, default=480)
    ap.add_argument("--host-days", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-scan", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radar_ingest.py needs the GPU: nothing is measured without one")
    n_days, ny, nx = a.days, a.ny, a.nx
    plane = ny * nx
    assert plane % 16 == 0, "the three paths are forced by alignment alone: the plane must allow 16 codes per lane"
    fpd = 24 * FPH
    n_codes = n_days * fpd * plane
    algo_bytes = n_days * plane * (fpd + 96 + 4)
    res = dict(days=n_days, ny=ny, nx=nx, frames_per_hour=FPH, codes_gb=n_codes / 1e9, algorithmic_gb=algo_bytes / 1e9,
               hbm_copy_reference_gbs=HBM_ACHIEVABLE_GBS, device=torch.cuda.get_device_name(0))
    lib = dp._lib.load()
    buf = torch.empty(n_codes + 16, dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(dp.radar_lut()).cuda()
    hourly = torch.empty((n_days, 24, ny, nx), dtype=torch.float32, device="cuda")
    daily = torch.empty((n_days, ny, nx), dtype=torch.float32, device="cuda")
    missing = torch.zeros(1, dtype=torch.int64, device="cuda")
    half = algo_bytes // 2 // 16 * 16                                   # a copy reads and writes: half the bytes each way
    src = torch.empty(half // 4, dtype=torch.float32, device="cuda").zero_()
    dst = torch.empty_like(src)
    st = dp.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel(shift):
        view = buf[shift:shift + n_codes]
        return lambda: dp._lib.check(lib.rdgan_data_radar_hourly(ptr(view), ptr(lut), n_days, FPH, ny, nx, ptr(hourly), ptr(daily),
                                                                 ptr(missing), st), None, "rdgan_data_radar_hourly")

    copy = lambda: dst.copy_(src)
    res["kernel"] = {}
    for pattern in ("radar", "uniform"):
        fill_codes(buf[:n_codes].view(n_days, fpd, ny, nx), pattern)
        torch.cuda.synchronize()
        for name, shift in (("16_per_lane", 0), ("4_per_lane", 4), ("1_per_lane", 1)):
            reps = a.reps if shift != 1 else max(2, a.reps // 2)
            ms, ms_copy = alternate([kernel(shift), copy], reps, a.warmup if shift != 1 else 1)
            res["kernel"][f"{pattern}_{name}"] = dict(ms=ms, gbs=algo_bytes / ms / 1e6, copy_ms=ms_copy, copy_gbs=2 * half / ms_copy / 1e6,
                                                      of_copy=ms_copy / ms)
            print(pattern, name, res["kernel"][f"{pattern}_{name}"], flush=True)
    del src, dst

    # (4) the scan, on the hourly / daily arrays of the "radar" codes
    fill_codes(buf[:n_codes].view(n_days, fpd, ny, nx), "radar")
    missing.zero_()
    kernel(0)()
    torch.cuda.synchronize()
    res["missing_pixel_hours"] = int(missing.item())
    if not a.skip_scan:
        res["scan"] = {}
        for nd, stride in ((16, 16), (16, 1)):
            nbi, nbj = len(range(0, ny - nd, stride)), len(range(0, nx - nd, stride))
            v_new = torch.empty((n_days, nbi, nbj), dtype=torch.int32, device="cuda")
            v_old = torch.empty_like(v_new)
            new = lambda: lib.rdgan_data_valid_tiles_daily(ptr(daily), n_days, ny, nx, nd, stride, 5.0, 20, ptr(v_new), st)
            days_old = min(n_days, 0xFFFFFF // (nbi * nbj))            # k_valid_tiles: one workgroup per box, < 2^24 boxes per call
            old = lambda: dp._lib.check(lib.rdgan_data_valid_tiles(ptr(hourly), days_old, ny, nx, nd, stride, 5.0, 20, ptr(v_old), st))
            ms_new, ms_old = alternate([new, old], max(2, a.reps // 2), 1)
            res["scan"][f"nd{nd}_stride{stride}"] = dict(
                boxes=n_days * nbi * nbj, valid=int(v_new.sum().item()), daily_ms=ms_new, daily_ns_per_box=ms_new * 1e6 / (n_days * nbi * nbj),
                hourly_days=days_old, hourly_ms=ms_old, hourly_ns_per_box=ms_old * 1e6 / (days_old * nbi * nbj),
                identical=bool(torch.equal(v_new[:days_old], v_old[:days_old])))
            print("scan", nd, stride, res["scan"][f"nd{nd}_stride{stride}"], flush=True)
            del v_new, v_old

    # (2) end to end from a host array
    hd = min(a.host_days, n_days)
    host = buf[:hd * fpd * plane].view(hd, fpd, ny, nx).cpu().numpy()
    del buf, hourly, daily
    torch.cuda.empty_cache()
    cd = max(1, dp.CHUNK_BYTES // (fpd * plane))
    e2e = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dp.hourly_from_radar_codes(host)                          # (ends in the read of the missing counter: synchronised)
        e2e.append((time.perf_counter() - t0) * 1e3)
        del out
    pinned = torch.empty(cd * fpd * plane, dtype=torch.uint8, pin_memory=True)
    staged = torch.empty(cd * fpd * plane, dtype=torch.uint8, device="cuda")
    flat = host.reshape(-1)

    def uploads():
        for d0 in range(0, hd, cd):
            n = min(cd, hd - d0) * fpd * plane
            staged[:n].copy_(pinned[:n], non_blocking=True)

    h2d_ms = float(np.median([event_ms(uploads)[0] for _ in range(3)]))
    t0 = time.perf_counter()
    for d0 in range(0, hd, cd):
        n = min(cd, hd - d0) * fpd * plane
        np.copyto(pinned.numpy()[:n], flat[d0 * fpd * plane:d0 * fpd * plane + n])
    stage_ms = (time.perf_counter() - t0) * 1e3
    hb = hd * fpd * plane
    res["end_to_end"] = dict(host_days=hd, chunk_days=cd, host_gb=hb / 1e9, ms=float(np.median(e2e)), first_ms=e2e[0],
                             codes_gbs=hb / np.median(e2e) / 1e6, h2d_only_ms=h2d_ms, h2d_gbs=hb / h2d_ms / 1e6,
                             host_staging_copy_only_ms=stage_ms)
    print("end_to_end", res["end_to_end"], flush=True)

    # (3) the numpy restatement of one day on the host
    from tests import radar_np as rn
    lut_h = dp.radar_lut()
    t0 = time.perf_counter()
    h = rn.hourly(host[:1], lut_h, FPH)
    rn.daily(h)
    one = time.perf_counter() - t0
    res["numpy_restatement"] = dict(one_day_s=one, scaled_to_days_s=one * n_days, processes=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
