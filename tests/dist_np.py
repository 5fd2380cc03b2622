"""fp64 numpy mirrors of csrc/rdgan_dist.hip.h, written from the definitions: the two-sample KS statistic by searchsorted(side='right')
on the pooled data, the box-plot statistics following matplotlib.cbook.boxplot_stats(whis=1.5) step by step, ECDF counts by
searchsorted on the sorted data.  Test-only."""
import numpy as np

STAT_FIELDS = ("n", "mean", "q1", "med", "q3", "iqr", "whislo", "whishi", "cilo", "cihi", "n_fliers_lo", "n_fliers_hi")


def ks_counts(a, b):
    """One column pair -> (i, j, D): both ECDFs evaluated with <= at every pooled data value; the FIRST value (ascending) where
    |i / n - j / m| is largest -- decided on the integer |i m - j n| -- gives (i, j); D = abs(i / n - j / m) in fp64.  NaN in either
    sample: (-1, -1, nan)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    n, m = len(a), len(b)
    if np.isnan(a).any() or np.isnan(b).any():
        return -1, -1, np.nan
    a, b = np.sort(a), np.sort(b)
    pooled = np.unique(np.concatenate([a, b]))                       # ascending
    i = np.searchsorted(a, pooled, side="right").astype(np.int64)
    j = np.searchsorted(b, pooled, side="right").astype(np.int64)
    k = int(np.argmax(np.abs(i * m - j * n)))                        # argmax returns the first maximum
    i, j = int(i[k]), int(j[k])
    return i, j, abs(i / n - j / m)


def ks_columns(a, b):
    """a (batch, n, ncol), b (batch, m, ncol) -> counts (batch, ncol, 2) int64, D (batch, ncol)"""
    B, _, C = a.shape
    counts, d = np.zeros((B, C, 2), np.int64), np.zeros((B, C))
    for bt in range(B):
        for c in range(C):
            counts[bt, c, 0], counts[bt, c, 1], d[bt, c] = ks_counts(a[bt, :, c], b[bt, :, c])
    return counts, d


def _percentile_linear(xs, q):
    """np.percentile's default method on the ascending xs, spelled out: virtual index (n - 1) q, numpy's lerp"""
    n = len(xs)
    vi = (n - 1) * q
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    g = vi - lo
    a, b = xs[lo], xs[hi]
    diff = b - a
    return b - diff * (1.0 - g) if g >= 0.5 else a + diff * g


def box_stats(x):
    """matplotlib.cbook.boxplot_stats(x, whis=1.5) of one column (cast to float64) -> dict of STAT_FIELDS plus 'sorted', and
    'margin': how far, relative to the fence, the closest datum lies from either whisker fence (inf if the iqr is 0 or n < 2)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    n = len(x)
    if np.isnan(x).any():
        out = {k: np.nan for k in STAT_FIELDS}
        out["n"] = float(n)
        return out
    xs = np.sort(x)
    q1, med, q3 = (_percentile_linear(xs, q) for q in (0.25, 0.5, 0.75))
    assert (q1, med, q3) == tuple(np.percentile(x, [25, 50, 75]))
    iqr = q3 - q1
    loval, hival = q1 - 1.5 * iqr, q3 + 1.5 * iqr
    wiskhi = x[x <= hival]
    whishi = q3 if len(wiskhi) == 0 or wiskhi.max() < q3 else wiskhi.max()
    wisklo = x[x >= loval]
    whislo = q1 if len(wisklo) == 0 or wisklo.min() > q1 else wisklo.min()
    notch = 1.57 * iqr / np.sqrt(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = min(np.abs(x - hival).min() / abs(hival), np.abs(x - loval).min() / abs(loval)) if iqr > 0 else np.inf
    return {"n": float(n), "mean": float(np.mean(xs)), "q1": q1, "med": med, "q3": q3, "iqr": iqr, "whislo": whislo, "whishi": whishi,
            "cilo": med - notch, "cihi": med + notch, "n_fliers_lo": float((x < whislo).sum()), "n_fliers_hi": float((x > whishi).sum()),
            "sorted": xs, "margin": float(margin)}


def ecdf_counts(x, grid):
    """counts[j] = #{x <= grid[j]} over the non-NaN values, the number above the last threshold, the number of NaNs"""
    x = np.asarray(x).ravel()
    nan = np.isnan(x)
    xs = np.sort(x[~nan])
    counts = np.searchsorted(xs, np.asarray(grid, dtype=x.dtype), side="right").astype(np.int64)
    return counts, int(len(xs) - counts[-1]), int(nan.sum())
