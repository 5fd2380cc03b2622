"""Ensemble products of whole fields (csrc/rdgan_products.hip.h): per-pixel k-hour peaks of hourly maps, the
peaks of field.disaggregate's scenarios formed inside the blend (the hourly ensemble is never written), and statistics across the
members of an ensemble -- quantiles, mean, exceedance frequencies.

    peaks[u, i, y, x] = max over h0 = 0 .. 24 - windows[i] of v[h0] + .. + v[h0 + windows[i] - 1]      (fp32, left to right)
    peak_hour[u, y, x] = the first h0 reaching the maximum of windows[0]; 255 where the pixel holds a NaN

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream
from ._hourly import MAX_MEMBERS, member_layout
from .engine import require_gpu

MAX_WINDOWS, MAX_PROBS, MAX_THRESHOLDS = 8, 16, 16                       # RD_PEAKS_MAXK, RD_MS_MAXQ, RD_MS_MAXT (MAX_MEMBERS: RD_MS_MAXS)
DEFAULT_WINDOWS = (1, 3, 6, 12, 24)
DEFAULT_PROBS = (0.1, 0.5, 0.9, 0.99)

MemberStats = namedtuple("MemberStats", "quantiles mean exceedance n_nan_positions")
FieldProducts = namedtuple("FieldProducts", "windows probs quantiles mean exceedance peak_hour info")


def check_windows(windows):
    """-> the window list as a contiguous int32 array: 1 .. 8 entries, each in 1 .. 24, strictly increasing"""
    w = np.asarray(windows)
    if w.ndim != 1 or not 1 <= w.shape[0] <= MAX_WINDOWS:
        raise ValueError(f"windows must be a list of 1 .. {MAX_WINDOWS} window lengths, got {windows!r}")
    if not np.issubdtype(w.dtype, np.integer):
        if not (np.issubdtype(w.dtype, np.floating) and np.all(w == np.round(w))):
            raise ValueError(f"windows must be whole hours, got {windows!r}")
    w = w.astype(np.int64)
    if w.min() < 1 or w.max() > W.NHOURS:
        raise ValueError(f"every window must lie in 1 .. {W.NHOURS}, got {windows!r}")
    if np.any(np.diff(w) <= 0):
        raise ValueError(f"windows must be strictly increasing, got {windows!r}")
    return np.ascontiguousarray(w, dtype=np.int32)


def check_probs(probs):
    p = np.asarray(probs, dtype=np.float64)
    if p.ndim != 1 or not 1 <= p.shape[0] <= MAX_PROBS:
        raise ValueError(f"probs must be a list of 1 .. {MAX_PROBS} probabilities")
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError(f"every probability must lie in [0, 1], got {probs!r}")
    return np.ascontiguousarray(p)


def check_thresholds(thresholds):
    t = np.asarray(() if thresholds is None else thresholds, dtype=np.float64)
    if t.ndim != 1 or t.shape[0] > MAX_THRESHOLDS:
        raise ValueError(f"thresholds must be a list of at most {MAX_THRESHOLDS} values")
    if not np.all(np.isfinite(t)):
        raise ValueError(f"every threshold must be finite, got {thresholds!r}")
    return np.ascontiguousarray(t)


def peaks_device(hourly, windows=DEFAULT_WINDOWS):
    """hourly (..., 24, ny, nx) float32 CUDA, any leading axes (none: one unit) -> (peaks (units, K, ny, nx) float32, peak_hour
    (units, ny, nx) uint8), units = the product of the leading axes."""
    win = check_windows(windows)
    if not isinstance(hourly, torch.Tensor) or hourly.dim() < 3 or hourly.shape[-3] != W.NHOURS:
        raise ValueError("hourly: expected a tensor of shape (..., 24, ny, nx)")
    ny, nx = int(hourly.shape[-2]), int(hourly.shape[-1])
    units = int(np.prod(hourly.shape[:-3], dtype=np.int64))
    if units < 1 or ny < 1 or nx < 1:
        raise ValueError(f"hourly holds no value: shape {tuple(hourly.shape)}")
    require_gpu()
    lib = _lib.load()
    F._check_f32_cuda(hourly, hourly.shape, "hourly")
    peaks = torch.empty((units, len(win), ny, nx), dtype=torch.float32, device=hourly.device)
    hour = torch.empty((units, ny, nx), dtype=torch.uint8, device=hourly.device)
    rc = lib.rdgan_hourly_peaks(_p(hourly), units, ny, nx, _hp(win), len(win), _p(peaks), _p(hour), _stream(hourly))
    _lib.check(rc, None, "rdgan_hourly_peaks")
    return peaks, hour


def blend_peaks_device(frac, slots, plan, daily, windows=DEFAULT_WINDOWS, first_unit=0, out=None):
    """The fused kernel alone: field.blend_device's arguments and the window list; -> (peaks (units, K, ny, nx) float32, peak_hour
    (units, ny, nx) uint8), equal to peaks_device(field.blend_device(...)) bit for bit.  out: the pair of tensors to write."""
    win = check_windows(windows)
    nd = plan.ndomain
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    if slots.ndim != 2 or slots.shape[0] < 1 or slots.shape[1] != plan.n_tiles:
        raise ValueError(f"slots must have shape (units, {plan.n_tiles}), got {slots.shape}")
    if isinstance(frac, torch.Tensor) and frac.dim() == 5 and frac.shape[-1] == 1:
        frac = frac.view(frac.shape[:-1])
    m = int(frac.shape[0]) if hasattr(frac, "shape") and len(frac.shape) else 0
    if slots.min() < -1 or slots.max() >= m:
        raise ValueError(f"slots must lie in -1 .. {m - 1}")
    require_gpu()
    lib = _lib.load()
    F._check_f32_cuda(frac, (m, W.NHOURS, nd, nd), "frac")
    if not (isinstance(daily, torch.Tensor) and daily.dim() == 3):
        raise ValueError("daily: expected a (n_days, ny, nx) CUDA tensor")
    F._check_f32_cuda(daily, (daily.shape[0], plan.ny, plan.nx), "daily")
    units = slots.shape[0]
    if out is None:
        out = (torch.empty((units, len(win), plan.ny, plan.nx), dtype=torch.float32, device=frac.device),
               torch.empty((units, plan.ny, plan.nx), dtype=torch.uint8, device=frac.device))
    peaks, hour = out
    F._check_f32_cuda(peaks, (units, len(win), plan.ny, plan.nx), "peaks out")
    if not (isinstance(hour, torch.Tensor) and hour.is_cuda and hour.dtype == torch.uint8 and hour.is_contiguous()
            and tuple(hour.shape) == (units, plan.ny, plan.nx)):
        raise ValueError(f"peak_hour out: expected a contiguous uint8 CUDA tensor of shape {(units, plan.ny, plan.nx)}")
    yi, yw, xi, xw = plan.device_tables(frac.device)
    rc = lib.rdgan_field_blend_peaks(_p(frac), m, _hp(slots), units, int(first_unit), _p(yi), _p(yw), _p(xi), _p(xw),
                                     _p(daily), int(daily.shape[0]), plan.ny, plan.nx, nd, plan.overlap, _hp(win), len(win),
                                     _p(peaks), _p(hour), _stream(frac))
    _lib.check(rc, None, "rdgan_field_blend_peaks")
    return peaks, hour


def member_stats_device(x, probs, thresholds=()):
    """Statistics across the members of an ensemble.  x (S, *shape) float32 CUDA, 1 <= S <= 4096; a view whose member axis has a
    stride above prod(shape) is accepted as it stands.  -> MemberStats(quantiles (Q, *shape), mean (*shape), exceedance (T, *shape),
    n_nan_positions): np.quantile(x, probs, axis=0) (method "linear", fp64, rounded once to fp32), the mean (fp64 sum), the share
    of members above each threshold; NaN at every position where a member is NaN, n_nan_positions (an int) counting those."""
    p, t = check_probs(probs), check_thresholds(thresholds)
    S, P, stride, shape = member_layout(x)
    require_gpu()
    lib = _lib.load()
    if not (x.is_cuda and x.dtype == torch.float32):
        raise ValueError("x: expected a float32 CUDA tensor")
    dev = x.device
    quant = torch.empty((len(p),) + shape, dtype=torch.float32, device=dev)
    mean = torch.empty(shape, dtype=torch.float32, device=dev)
    exceed = torch.empty((len(t),) + shape, dtype=torch.float32, device=dev)
    n_nan = torch.empty(1, dtype=torch.int64, device=dev)
    rc = lib.rdgan_member_stats(_p(x), S, stride, P, _hp(p), len(p), _hp(t) if len(t) else _p(None), len(t), _p(quant),
                                _p(mean), _p(exceed if len(t) else None), _p(n_nan), _stream(x))
    _lib.check(rc, None, "rdgan_member_stats")
    return MemberStats(quant, mean, exceed, int(n_nan.item()))


def disaggregate_peaks(gen, daily, n_scenarios, windows=DEFAULT_WINDOWS, overlap=4, latent_mode="shared", seed=None, latent=None,
                       chunk=1024, norm_scale=W.NORM_SCALE):
    """field.disaggregate with the k-hour peaks in place of the hourly maps: the same tile plan, scan, dry-tile skipping, latent
    handling and grouping (field._run_groups), each group blended by the fused kernel, so the S * D * 24 * ny * nx hourly values are
    never allocated.  -> (peaks (S, [D,] K, ny, nx) float32 CUDA, peak_hour (S, [D,] ny, nx) uint8 CUDA, FieldInfo); with the same
    `latent` equal to peaks_device(field.disaggregate(...)[0]) bit for bit."""
    win = check_windows(windows)
    S, K = int(n_scenarios), len(win)
    daily, squeeze_day, D, ny, nx, plan, z_shape = F._check_request(gen, daily, S, overlap, latent_mode, latent, chunk, norm_scale)
    dd, info, active_tiles = F._scan_request(daily, D, ny, nx, plan)
    peaks = torch.empty((S * D, K, ny, nx), dtype=torch.float32, device=dd.device)
    hour = torch.empty((S * D, ny, nx), dtype=torch.uint8, device=dd.device)

    def dry(u0, u1):                                 # zeros and NaNs straight from the plane; hour 0, or 255 at a NaN pixel
        for u in range(u0, u1):
            peaks[u].copy_((dd[u % D] * 0.0)[None].expand(K, -1, -1))
            hour[u].copy_(torch.isnan(dd[u % D]).to(torch.uint8) * 255)

    def blend(frac, slots, u0, u1):
        blend_peaks_device(frac, slots, plan, dd, win, first_unit=u0, out=(peaks[u0:u1], hour[u0:u1]))

    if info.n_active == 0:
        with torch.cuda.device(dd.device):
            dry(0, S * D)
    else:
        F._run_groups(gen, dd, plan, S, active_tiles, latent_mode, seed, latent, z_shape, int(chunk), norm_scale, blend, dry)
    if squeeze_day:
        return peaks.view(S, K, ny, nx), hour.view(S, ny, nx), info
    return peaks.view(S, D, K, ny, nx), hour.view(S, D, ny, nx), info


def _threshold_table(thresholds, K):
    """None, a sequence (the same for every window) or a (K, T) array -> None or a (K, T) float64 array, every row checked"""
    if thresholds is None:
        return None
    t = np.asarray(thresholds, dtype=np.float64)
    if t.ndim == 1:
        t = np.broadcast_to(t, (K, t.shape[0]))
    if t.ndim != 2 or t.shape[0] != K or t.shape[1] < 1:
        raise ValueError(f"thresholds must be None, a non-empty sequence or an array of shape ({K}, T), got shape {t.shape}")
    return np.stack([check_thresholds(row) for row in t])


def ensemble_products(gen, daily, n_scenarios, windows=DEFAULT_WINDOWS, probs=DEFAULT_PROBS, thresholds=None, overlap=4,
                      latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Per-pixel statistics of the k-hour peaks across n_scenarios (<= 4096) scenarios of whole daily fields: disaggregate_peaks,
    then one member_stats launch per (day, window).  thresholds: None, a sequence in mm (the same for every window) or a (K, T)
    array (per window).  -> FieldProducts(windows, probs, quantiles ([D,] K, Q, ny, nx), mean ([D,] K, ny, nx), exceedance
    ([D,] K, T, ny, nx) or None, peak_hour (S, [D,] ny, nx), info), all float32 CUDA but peak_hour (uint8)."""
    win, p = check_windows(windows), check_probs(probs)
    K, Q, S = len(win), len(p), int(n_scenarios)
    thr = _threshold_table(thresholds, K)
    if S > MAX_MEMBERS:
        raise ValueError(f"the number of scenarios must lie in 1 .. {MAX_MEMBERS}, got {S}")
    peaks, hour, info = disaggregate_peaks(gen, daily, S, win, overlap, latent_mode, seed, latent, chunk, norm_scale)
    squeeze_day = peaks.dim() == 4
    ny, nx = int(peaks.shape[-2]), int(peaks.shape[-1])
    pk = peaks.view(S, -1, K, ny, nx)
    D, dev = int(pk.shape[1]), peaks.device
    quant = torch.empty((D, K, Q, ny, nx), dtype=torch.float32, device=dev)
    mean = torch.empty((D, K, ny, nx), dtype=torch.float32, device=dev)
    exceed = None if thr is None else torch.empty((D, K, thr.shape[1], ny, nx), dtype=torch.float32, device=dev)
    for d in range(D):
        for k in range(K):
            st = member_stats_device(pk[:, d, k], p, () if thr is None else thr[k])          # a view: member stride D * K * ny * nx
            quant[d, k], mean[d, k] = st.quantiles, st.mean
            if exceed is not None:
                exceed[d, k] = st.exceedance
    if squeeze_day:
        quant, mean, exceed = quant[0], mean[0], None if exceed is None else exceed[0]
    return FieldProducts(tuple(int(w) for w in win), tuple(float(q) for q in p), quant, mean, exceed, hour, info)
