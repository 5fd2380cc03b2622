"""The numpy restatement of pr_disagg_radar_gan_amd/extremes.py, written from the definitions of DESIGN.md section 26: block maxima
in integers, the sums over the order statistics, and the fp64 formulas from sums to return levels.  Checked on the CPU by
tests/test_extremes_host.py; the yardstick of tests/test_hip_extremes.py."""
import math

import numpy as np

UNIT = 1024
MAX_DEPTH = 2048.0
LN2, LN3 = math.log(2.0), math.log(3.0)
EULER_GAMMA = 0.5772156649015329
GEV_SWITCH = 1e-6

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def quantise(x):
    """x float -> (q int64, bad bool): q = rint(x * 1024) in fp32, ties to even; bad: NaN, +-inf, negative or >= 2048"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        bad = ~((x >= 0) & (x < np.float32(MAX_DEPTH)))
        q = np.rint(np.where(bad, np.float32(0), x) * np.float32(UNIT)).astype(np.int64)
    return q, bad


def block_maxima_np(hourly, block, n_blocks, windows):
    """hourly (..., 24, ny, nx), block one id per day -> bmax (NB, K, ny, nx) int64 (-1: no good day), ndays, nvoid (NB, ny, nx) int32.
    Windows lie within the day."""
    x = np.asarray(hourly)
    ny, nx = x.shape[-2:]
    x = x.reshape(-1, 24, ny, nx)
    block = np.asarray(block).ravel()
    assert len(block) == len(x)
    bmax = np.full((n_blocks, len(windows), ny, nx), -1, np.int64)
    ndays = np.zeros((n_blocks, ny, nx), np.int32)
    nvoid = np.zeros((n_blocks, ny, nx), np.int32)
    for d, b in enumerate(block):
        q, bad = quantise(x[d])
        void = bad.any(axis=0)
        ndays[b] += ~void
        nvoid[b] += void
        c = np.concatenate([np.zeros((1, ny, nx), np.int64), np.cumsum(q, axis=0)])
        for k, w in enumerate(windows):
            depth = (c[w:] - c[:24 - w + 1]).max(axis=0)
            bmax[b, k] = np.where(void, bmax[b, k], np.maximum(bmax[b, k], depth))
    return bmax, ndays, nvoid


def lmoment_sums_np(table, ndays=None, min_days=1):
    """table (S, B, M) -> n (S, M) int32, A (S, M, 3) int64, sorted (S, B, M) int64 (ascending, then -1).  Python integers inside: no
    overflow can hide."""
    table = np.asarray(table, dtype=np.int64)
    S, B, M = table.shape
    n = np.zeros((S, M), np.int32)
    A = np.zeros((S, M, 3), np.int64)
    srt = np.full((S, B, M), -1, np.int64)
    for s in range(S):
        for m in range(M):
            col = table[s, :, m]
            keep = col >= 0
            if ndays is not None:
                keep &= np.asarray(ndays)[s, :, m] >= min_days
            xs = sorted(int(v) for v in col[keep])
            n[s, m] = len(xs)
            srt[s, :len(xs), m] = xs
            a = [sum(xs), sum(j * v for j, v in enumerate(xs)), sum(j * (j - 1) * v for j, v in enumerate(xs))]
            assert all(v < 2 ** 63 for v in a)
            A[s, m] = a
    return n, A, srt


def lmoments_np(n, A, unit=float(UNIT)):
    """-> l1, l2 (mm), t3; NaN where n is too small, and t3 where l2 = 0.  l2 from the exact integer 2 A1 - (n - 1) A0."""
    n = np.asarray(n)
    nf = n.astype(np.float64)
    A = np.asarray(A, dtype=np.int64)
    A0, A1, A2 = A[..., 0], A[..., 1], A[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        b0 = A0.astype(np.float64) / nf
        b1 = A1.astype(np.float64) / (nf * (nf - 1.0))
        b2 = A2.astype(np.float64) / (nf * (nf - 1.0) * (nf - 2.0))
        l1 = np.where(n >= 1, b0, np.nan)
        l2 = np.where(n >= 2, (2 * A1 - (n.astype(np.int64) - 1) * A0).astype(np.float64) / (nf * (nf - 1.0)), np.nan)
        l3 = 6.0 * b2 - 6.0 * b1 + b0
        t3 = np.where((n >= 3) & (l2 != 0), l3 / l2, np.nan)
    return l1 / unit, l2 / unit, t3


def gumbel_np(l1, l2):
    l2 = np.where(np.asarray(l2) != 0, l2, np.nan)
    scale = l2 / LN2
    return l1 - EULER_GAMMA * scale, scale


def gev_np(l1, l2, t3):
    """Hosking (1985), his sign of k; the Gumbel limit (shape 0) where |k| < GEV_SWITCH"""
    l1, l2, t3 = (np.asarray(a, dtype=np.float64) for a in (l1, l2, t3))
    with np.errstate(invalid="ignore", divide="ignore"):
        c = 2.0 / (3.0 + t3) - LN2 / LN3
        k = 7.8590 * c + 2.9554 * c * c
        small = np.abs(k) < GEV_SWITCH
        ks = np.where(small | np.isnan(k), 1.0, k)
        lg = _lgamma(1.0 + ks)
        scale = l2 * ks / (-np.expm1(-ks * LN2) * np.exp(lg))
        loc = l1 - scale * (-np.expm1(lg)) / ks
        gl, gs = l1 - EULER_GAMMA * l2 / LN2, l2 / LN2
    nan = np.isnan(k)
    pick = lambda a, b: np.where(nan, np.nan, np.where(small, b, a))
    return pick(loc, gl), pick(scale, gs), pick(k, 0.0)


def quantile_np(loc, scale, shape, T):
    ly = math.log(-math.log1p(-1.0 / float(T)))
    shape = np.asarray(shape, dtype=np.float64)
    zero = shape == 0
    ks = np.where(zero, 1.0, shape)
    with np.errstate(invalid="ignore"):
        return np.where(zero, loc - scale * ly, loc + scale * (-np.expm1(ks * ly)) / ks)


def empirical_np(n, srt, T, unit=float(UNIT)):
    """srt (S, B, *shape), n (S, *shape): linear interpolation of the sorted maxima at the Weibull positions j / (n + 1)"""
    n = np.asarray(n)
    srt = np.asarray(srt)
    out = np.full((len(T),) + n.shape, np.nan)
    for i, t in enumerate(T):
        F = 1.0 - 1.0 / float(t)
        for idx in np.ndindex(n.shape):
            m = int(n[idx])
            at = F * (m + 1.0)
            if m < 1 or at < 1.0 or at > m:
                continue
            col = srt[(idx[0], slice(None)) + idx[1:]][:m].astype(np.float64) / (unit if np.isscalar(unit) else unit[idx])
            j = int(math.floor(at))
            hi = col[min(j, m - 1)]
            out[(i,) + idx] = col[j - 1] + (at - j) * (hi - col[j - 1])
    return out


def return_levels_np(n, A, T, dist, srt=None, unit=float(UNIT)):
    l1, l2, t3 = lmoments_np(n, A, unit)
    if dist == "empirical":
        return empirical_np(n, srt, T, unit)
    if dist == "gumbel":
        loc, scale = gumbel_np(l1, l2)
        shape = np.zeros_like(loc)
    else:
        loc, scale, shape = gev_np(l1, l2, t3)
    return np.stack([quantile_np(loc, scale, shape, t) for t in T])


def wet_spells(rng, days, ny, nx, wet=0.35):
    """(days, 24, ny, nx) float32 from a seeded generator: spells of a few hours of gamma rain that drift over the plane, dry
    otherwise, with some values on quantisation ties"""
    x = np.zeros((days, 24, ny, nx), np.float32)
    yy, xx = np.mgrid[:ny, :nx]
    for d in range(days):
        for _ in range(rng.integers(0, 4)):
            h0, length = rng.integers(0, 24), rng.integers(1, 9)
            cy, cx, r = rng.random() * ny, rng.random() * nx, 1.0 + rng.random() * max(ny, nx) * wet
            for h in range(h0, min(24, h0 + length)):
                mask = (yy - cy) ** 2 + (xx - cx - 0.5 * (h - h0)) ** 2 <= r * r
                x[d, h] += (rng.gamma(0.8, 3.0, (ny, nx)) * mask).astype(np.float32)
    ties = rng.random(x.shape) < 0.03
    x[ties] = ((rng.integers(0, 8192, x.shape) + 0.5) / 1024).astype(np.float32)[ties]
    return x
