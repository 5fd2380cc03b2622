"""numpy restatement of the ensemble products (pr_disagg_radar_gan_amd/field_products.py, csrc/rdgan_products.hip.h), written from the
definitions and not from the product code: k-hour peaks with fp32 window sums taken left to right, the first hour reaching the
maximum, the NaN rules, and quantile / mean / exceedance across members in fp64 rounded once to fp32."""
import numpy as np

NHOURS = 24


def check_windows(windows):
    w = [int(v) for v in windows]
    if not 1 <= len(w) <= 8 or any(not 1 <= v <= NHOURS for v in w) or any(b <= a for a, b in zip(w, w[1:])):
        raise ValueError(windows)
    return w


def window_sums(x, w):
    """x (..., 24, ny, nx) float32 -> (..., 25 - w, ny, nx) float32: s[h0] = ((x[h0] + x[h0 + 1]) + ..) + x[h0 + w - 1], each add
    rounded to fp32"""
    x = np.asarray(x, dtype=np.float32)
    n = NHOURS - w + 1
    s = x[..., 0:n, :, :].copy()
    for j in range(1, w):
        s = (s + x[..., j:j + n, :, :]).astype(np.float32)
    return s


def first_max(s):
    """(best, hour) along axis -3: the running maximum taken with `>` from h0 = 0 on, so the FIRST h0 reaching it wins and a NaN
    sum never replaces what came before"""
    best = s[..., 0, :, :].copy()
    hour = np.zeros(best.shape, dtype=np.uint8)
    for h0 in range(1, s.shape[-3]):
        with np.errstate(invalid="ignore"):
            take = s[..., h0, :, :] > best
        best = np.where(take, s[..., h0, :, :], best)
        hour = np.where(take, np.uint8(h0), hour)
    return best.astype(np.float32), hour.astype(np.uint8)


def hourly_peaks(x, windows):
    """x (units, 24, ny, nx) float32 -> (peaks (units, K, ny, nx) float32, peak_hour (units, ny, nx) uint8).  A pixel with a NaN
    among its 24 hours: NaN in every window, hour 255."""
    w = check_windows(windows)
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 4 and x.shape[1] == NHOURS
    nan = np.isnan(x).any(axis=1)
    peaks = np.empty((x.shape[0], len(w)) + x.shape[2:], dtype=np.float32)
    hour = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i, wi in enumerate(w):
            best, h = first_max(window_sums(x, wi))
            peaks[:, i] = np.where(nan, np.float32(np.nan), best)
            if i == 0:
                hour = np.where(nan, np.uint8(255), h).astype(np.uint8)
    return peaks, hour


def hourly_peaks_f64(x, windows):
    """the same in fp64 with plain loops: the brute force the fp32 restatement is checked against, and the unrounded reference of
    the blend comparison.  -> (peaks, peak_hour, margin): margin (units, ny, nx) = how far the best window sum of windows[0] lies
    above the runner-up at any other hour (inf when there is a single position)"""
    w = check_windows(windows)
    x = np.asarray(x, dtype=np.float64)
    U, _, ny, nx = x.shape
    peaks = np.empty((U, len(w), ny, nx))
    hour = np.zeros((U, ny, nx), dtype=np.uint8)
    margin = np.full((U, ny, nx), np.inf)
    for u in range(U):
        for y in range(ny):
            for c in range(nx):
                v = x[u, :, y, c]
                if np.isnan(v).any():
                    peaks[u, :, y, c] = np.nan
                    hour[u, y, c] = 255
                    margin[u, y, c] = np.nan
                    continue
                for i, wi in enumerate(w):
                    sums = [float(np.sum(v[h0:h0 + wi])) for h0 in range(NHOURS - wi + 1)]
                    best = 0
                    for h0 in range(1, len(sums)):
                        if sums[h0] > sums[best]:
                            best = h0
                    peaks[u, i, y, c] = sums[best]
                    if i == 0:
                        hour[u, y, c] = best
                        rest = [s for h0, s in enumerate(sums) if h0 != best]
                        if rest:
                            margin[u, y, c] = sums[best] - max(rest)
    return peaks, hour, margin


def member_stats(x, probs, thresholds=()):
    """x (S, *shape) float32 -> (quantiles (Q, *shape), mean (*shape), exceedance (T, *shape), n_nan_positions), float32: numpy's
    "linear" quantile, the mean and #{x > thr} / S in fp64, rounded once; NaN everywhere at a position where a member is NaN"""
    x = np.asarray(x, dtype=np.float32)
    S = x.shape[0]
    if not 1 <= S <= 4096:
        raise ValueError(S)
    probs = np.asarray(probs, dtype=np.float64)
    thresholds = np.asarray(thresholds, dtype=np.float64)
    if probs.ndim != 1 or not 1 <= len(probs) <= 16 or not np.all((probs >= 0) & (probs <= 1)):
        raise ValueError(probs)
    if thresholds.ndim != 1 or len(thresholds) > 16 or not np.all(np.isfinite(thresholds)):
        raise ValueError(thresholds)
    x64 = x.astype(np.float64)
    nan = np.isnan(x64).any(axis=0)
    filled = np.where(nan[None], 0.0, x64)
    quant = np.quantile(filled, probs, axis=0, method="linear").astype(np.float32)
    mean = (filled.sum(axis=0) / S).astype(np.float32)
    exceed = np.stack([(filled > t).sum(axis=0).astype(np.float64) / S for t in thresholds]).astype(np.float32) \
        if len(thresholds) else np.empty((0,) + x.shape[1:], dtype=np.float32)
    quant[:, nan] = np.nan
    mean[nan] = np.nan
    exceed[:, nan] = np.nan
    return quant, mean, exceed, int(nan.sum())
