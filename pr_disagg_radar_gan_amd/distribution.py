"""The distribution checks of the reference's evaluation (generate_and_evaluate.py:431-604, G below) on the device
(csrc/rdgan_dist.hip.h): the ECDFs of G:431-465, the daily-cycle box plots of G:472-502 and the
condition-sensitivity check of G:548-604 (two ensembles from ONE latent block, scipy.stats.ks_2samp per hour, box plots).

The statistics come from the device: the two-sample Kolmogorov-Smirnov statistic as the pair of counts where the two ECDFs differ
most, the box-plot statistics as matplotlib.cbook.boxplot_stats defines them, ECDF counts on a grid of thresholds in one pass.  The
KS p-value is taken on the host in fp64 by the package's own code (no scipy): exact for equal sample sizes, asymptotic otherwise.
The figures themselves are not drawn here.  No CPU fallback: without a visible MI355X every device entry point raises RdganError;
argument errors are ValueErrors raised before any device call."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, ensemble
from . import weights as W
from ._dev import device_f32, ptr as _p, stream as _stream
from .engine import require_gpu

NHOURS = 24
MAX_N = 16384                   # RD_DIST_MAXN of csrc/rdgan_dist.hip.h: a column is sorted in LDS
MAX_GRID = 4096                 # RD_ECDF_MAXT
STAT_FIELDS = ("n", "mean", "q1", "med", "q3", "iqr", "whislo", "whishi", "cilo", "cihi", "n_fliers_lo", "n_fliers_hi")


def _columns_shape(x, name):
    """(batch, n, ncol) of a sample array: (n,), (n, ncol) or (batch, n, ncol)"""
    shape = tuple(x.shape)
    if len(shape) == 1:
        shape = (1, shape[0], 1)
    elif len(shape) == 2:
        shape = (1,) + shape
    elif len(shape) != 3:
        raise ValueError(f"{name} must have shape (n,), (n, ncol) or (batch, n, ncol), got {tuple(x.shape)}")
    if not 1 <= shape[1] <= MAX_N:
        raise ValueError(f"{name}: 1 .. {MAX_N} values per column, got {shape[1]}")
    if shape[0] < 1 or shape[2] < 1 or shape[0] * shape[2] >= 2 ** 31:
        raise ValueError(f"{name}: 1 .. 2^31 - 1 columns, got shape {tuple(x.shape)}")
    return shape


def _check_kind(a, name):
    if isinstance(a, torch.Tensor) and not a.is_cuda:
        raise ValueError(f"{name}: expected a CUDA tensor or a numpy array")


# ---------------------------------------------------------------------------------------------------------------------------------
# two-sample Kolmogorov-Smirnov
# ---------------------------------------------------------------------------------------------------------------------------------
def ks_pvalue_exact_equal_n(n, h):
    """P(D_{n,n} >= h / n), two-sided, for two samples of n values each whose ECDFs differ by at most h / n: the probability that a
    lattice path from (0, 0) to (n, n) leaves the band |x - y| < h, summed by the Horner-like recurrence scipy uses for these sizes
    (method='auto' of the reference's ks_2samp call, G:583), in its order of operations, fp64."""
    n, h = int(n), int(h)
    if n < 1 or not 0 <= h <= n:
        raise ValueError(f"need n >= 1 and 0 <= h <= n, got n = {n}, h = {h}")
    if h == 0:
        return 1.0
    P = 0.0
    k = n // h
    while k >= 0:
        p1 = 1.0
        for j in range(h):
            p1 = (n - k * h - j) * p1 / (n + k * h + j + 1)
        P = p1 * (1.0 - P)
        k -= 1
    return min(1.0, 2.0 * P)


def kolmogorov_sf(z):
    """The survival function of Kolmogorov's limiting distribution, 2 sum_{k >= 1} (-1)^(k - 1) exp(-2 k^2 z^2); for small z the
    series of the distribution function, 1 - sqrt(2 pi) / z sum_{k >= 1} exp(-(2k - 1)^2 pi^2 / (8 z^2)), which converges there."""
    z = float(z)
    if math.isnan(z):
        return z
    if z <= 0:
        return 1.0
    if z < 1.0:
        t = -math.pi * math.pi / (8.0 * z * z)
        s = 0.0
        for k in range(1, 12):
            s += math.exp((2 * k - 1) ** 2 * t)
        return 1.0 - math.sqrt(2.0 * math.pi) / z * s
    s = 0.0
    for k in range(1, 101):
        term = math.exp(-2.0 * k * k * z * z)
        s += term if k % 2 else -term
        if term < 1e-18 * abs(s):
            break
    return min(1.0, max(0.0, 2.0 * s))


def ks_pvalue_asymptotic(n, m, d):
    """The asymptotic two-sided p-value for unequal sample sizes: kolmogorov_sf(sqrt(en) d), en = n m / (n + m).  It is Smirnov's
    limit, not an exact probability: at the sizes used here it differs from the exact value, and from the finite-n correction
    current scipy applies in method='asymp', in the second digit."""
    n, m, d = float(n), float(m), float(d)
    if math.isnan(d):
        return d
    return kolmogorov_sf(math.sqrt(n * m / (n + m)) * d)


def ks_statistic_device(a, b):
    """The device half of ks_2samp: a (batch, n, ncol), b (batch, m, ncol) (or (n, ncol) / (n,)), float32, numpy or CUDA ->
    (counts, d): counts (batch, ncol, 2) int32 CUDA, the pair (#{a <= v}, #{b <= v}) at the first data value v where the ECDFs
    differ most, and d (batch, ncol) float64 CUDA = |i / n - j / m|.  A column holding a NaN gives (-1, -1) and NaN."""
    _check_kind(a, "a"), _check_kind(b, "b")
    sa, sb = _columns_shape(a, "a"), _columns_shape(b, "b")
    if sa[0] != sb[0] or sa[2] != sb[2]:
        raise ValueError(f"a and b differ in batch or columns: {tuple(a.shape)} and {tuple(b.shape)}")
    require_gpu()
    lib = _lib.load()
    a = device_f32(a, "a")
    b = device_f32(b, "b", a.device).to(a.device)
    counts = torch.empty((sa[0], sa[2], 2), dtype=torch.int32, device=a.device)
    d = torch.empty((sa[0], sa[2]), dtype=torch.float64, device=a.device)
    _lib.check(lib.rdgan_ks_2samp(_p(a), _p(b), sa[1], sb[1], sa[2], sa[0], _p(counts), _p(d), _stream(a)), None, "rdgan_ks_2samp")
    return counts, d


def ks_2samp(a, b):
    """scipy.stats.ks_2samp(a, b) of G:583, two-sided, for every column: a (batch, n, ncol), b (batch, m, ncol) -> (statistic,
    pvalue), float64 numpy arrays (batch, ncol); (n, ncol) input gives (ncol,), 1-D input two floats.  The statistic comes from the
    device (ks_statistic_device); the p-value from the host: for n = m the exact probability (ks_pvalue_exact_equal_n with
    h = |i - j|), for n != m the ASYMPTOTIC Kolmogorov form (ks_pvalue_asymptotic; the exact p-value for unequal sizes is not
    implemented).  A column holding a NaN gives (NaN, NaN).  1 <= n, m <= 16384."""
    ndim = len(tuple(a.shape))
    counts, d = ks_statistic_device(a, b)
    n, m = _columns_shape(a, "a")[1], _columns_shape(b, "b")[1]
    counts, d = counts.cpu().numpy(), d.cpu().numpy()
    p = np.empty_like(d)
    cache = {}
    for idx in np.ndindex(d.shape):
        i, j = int(counts[idx][0]), int(counts[idx][1])
        if i < 0:
            p[idx] = np.nan
        elif n == m:
            h = abs(i - j)
            if h not in cache:
                cache[h] = ks_pvalue_exact_equal_n(n, h)
            p[idx] = cache[h]
        else:
            p[idx] = ks_pvalue_asymptotic(n, m, d[idx])
    if ndim == 1:
        return float(d[0, 0]), float(p[0, 0])
    if ndim == 2:
        return d[0], p[0]
    return d, p


# ---------------------------------------------------------------------------------------------------------------------------------
# box-plot statistics
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class BoxStats:
    """matplotlib.cbook.boxplot_stats(x, whis=1.5) per column, float64 numpy arrays (batch, ncol): n, mean, q1, med, q3, iqr,
    whislo, whishi, cilo, cihi, and the number of fliers below whislo / above whishi.  sorted (batch, n, ncol) float32 CUDA, the
    ascending columns (None unless asked for)."""
    n: np.ndarray
    mean: np.ndarray
    q1: np.ndarray
    med: np.ndarray
    q3: np.ndarray
    iqr: np.ndarray
    whislo: np.ndarray
    whishi: np.ndarray
    cilo: np.ndarray
    cihi: np.ndarray
    n_fliers_lo: np.ndarray
    n_fliers_hi: np.ndarray
    sorted: Optional[torch.Tensor] = None

    def fliers(self, b, c):
        """The fliers of column (b, c) as boxplot_stats orders them (the low ones, then the high ones, each ascending), numpy."""
        if self.sorted is None:
            raise ValueError("boxplot_stats(x, keep_sorted=True) keeps the sorted columns the fliers are read from")
        if np.isnan(self.n_fliers_lo[b, c]):
            return np.full(0, np.nan, np.float32)
        lo, hi = int(self.n_fliers_lo[b, c]), int(self.n_fliers_hi[b, c])
        col = self.sorted[b, :, c]
        return torch.cat([col[:lo], col[col.shape[0] - hi:]]).cpu().numpy()

    def column(self, b, c):
        """One column as the dict boxplot_stats returns (without the fliers unless the sorted columns were kept)."""
        out = {k: float(getattr(self, k)[b, c]) for k in STAT_FIELDS[1:10]}
        if self.sorted is not None:
            out["fliers"] = self.fliers(b, c)
        return out


def boxplot_stats(x, keep_sorted=True):
    """matplotlib.cbook.boxplot_stats(column, whis=1.5) -- what sns.boxplot draws at G:495, 499, 600 -- for every column of
    x (batch, n, ncol) (or (n, ncol) / (n,), batch and ncol then 1), float32, numpy or CUDA, 1 <= n <= 16384 -> BoxStats.  One
    launch for all columns.  A column holding a NaN gives NaN in every field but n."""
    _check_kind(x, "x")
    shape = _columns_shape(x, "x")
    require_gpu()
    lib = _lib.load()
    x = device_f32(x, "x")
    stats = torch.empty((shape[0], shape[2], len(STAT_FIELDS)), dtype=torch.float64, device=x.device)
    srt = torch.empty(shape, dtype=torch.float32, device=x.device) if keep_sorted else None
    _lib.check(lib.rdgan_box_stats(_p(x), shape[1], shape[2], shape[0], _p(stats), _p(srt), _stream(x)), None, "rdgan_box_stats")
    s = stats.cpu().numpy()
    return BoxStats(*[np.ascontiguousarray(s[..., k]) for k in range(len(STAT_FIELDS))], sorted=srt)


# ---------------------------------------------------------------------------------------------------------------------------------
# ECDF
# ---------------------------------------------------------------------------------------------------------------------------------
def ecdf(data):
    """G:431-435: (x, y) = (np.sort(data), np.arange(1, n + 1) / n), exact, on the device: data of any shape is flattened; x in
    the dtype of a CUDA input (float32 for numpy input), y float64, both CUDA tensors."""
    _check_kind(data, "data")
    require_gpu()
    t = data.detach() if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).cuda()
    if t.numel() < 1:
        raise ValueError("data is empty")
    x = torch.sort(t.reshape(-1)).values
    n = x.numel()
    # (a tensor divisor: dividing by a Python scalar multiplies by its reciprocal on the device, one ulp off numpy's quotient)
    y = torch.arange(1, n + 1, dtype=torch.float64, device=x.device) / torch.full((), n, dtype=torch.float64, device=x.device)
    return x, y


def log_grid(lo, hi, T=512):
    """T thresholds from lo to hi, equally spaced in log10 (the semilogx axes of G:448, 457), ascending float32 numpy; the last is
    raised to at least hi, so that a grid up to the data's maximum ends at y = 1."""
    lo, hi, T = float(lo), float(hi), int(T)
    if not (0 < lo < hi) or math.isinf(hi) or not 2 <= T <= MAX_GRID:
        raise ValueError(f"need 0 < lo < hi and 2 <= T <= {MAX_GRID}, got lo = {lo}, hi = {hi}, T = {T}")
    g = np.logspace(math.log10(lo), math.log10(hi), T).astype(np.float32)
    top = np.float32(hi)
    if top < hi:
        top = np.nextafter(top, np.float32(np.inf))
    g[-1] = max(g[-1], top)
    if not np.all(np.diff(g) > 0):
        raise ValueError(f"{T} thresholds between {lo} and {hi} are not distinct in float32")
    return g


def ecdf_on_grid(data, grid):
    """The ECDF of G:451-452 evaluated at the thresholds `grid` in one pass over the data, which is never sorted or copied:
    data of any shape and size up to 2^40 values, float32, numpy or CUDA; grid ascending, 1 <= T <= 4096 -> (counts, y): counts
    (T,) int64 numpy, counts[j] = #{x <= grid[j]} exactly; y = counts / (N - n_nan) float64.  NaNs belong to no threshold."""
    counts, _, n_nan, n = ecdf_counts_device(data, grid)
    counts = counts.cpu().numpy()
    denom = n - n_nan
    y = counts / denom if denom > 0 else np.full(counts.shape, np.nan)
    return counts, y


def ecdf_counts_device(data, grid):
    """ecdf_on_grid without the division: (counts (T,) int64 CUDA, n_above, n_nan, N)."""
    _check_kind(data, "data")
    g = np.ascontiguousarray(grid.detach().cpu().numpy() if isinstance(grid, torch.Tensor) else grid, dtype=np.float32)
    if g.ndim != 1 or not 1 <= g.shape[0] <= MAX_GRID:
        raise ValueError(f"grid must be 1-D with 1 .. {MAX_GRID} thresholds, got shape {g.shape}")
    if np.isnan(g).any() or np.any(np.diff(g) < 0):
        raise ValueError("grid must be ascending and free of NaN")
    n = int(np.prod(tuple(data.shape)))
    if not 1 <= n <= 2 ** 40:
        raise ValueError(f"1 .. 2^40 values, got {n}")
    require_gpu()
    lib = _lib.load()
    x = device_f32(data, "data").reshape(-1)
    gd = torch.from_numpy(g).to(x.device)
    T = g.shape[0]
    nbytes = lib.rdgan_ecdf_workspace_bytes(T)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=x.device)
    out = torch.empty(T + 2, dtype=torch.int64, device=x.device)
    _lib.check(lib.rdgan_ecdf_grid(_p(x), n, _p(gd), T, _p(out), _p(ws), nbytes, _stream(x)), None, "rdgan_ecdf_grid")
    tail = out[T:].cpu().tolist()
    return out[:T], int(tail[0]), int(tail[1]), n


# ---------------------------------------------------------------------------------------------------------------------------------
# the daily cycle, G:472-502
# ---------------------------------------------------------------------------------------------------------------------------------
AMEAN_KEYS = ("gen", "real", "fraction_gen", "fraction_real")


def _check_ameans(ameans):
    try:
        arrs = [ameans[k] for k in AMEAN_KEYS]
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"ameans must hold the keys {AMEAN_KEYS} (ensemble.generate_one_per_condition)") from None
    shape = tuple(arrs[0].shape)
    if len(shape) != 2 or shape[0] < 1 or any(tuple(a.shape) != shape for a in arrs):
        raise ValueError(f"the four area-mean arrays must share one shape (n, hours), got {[tuple(a.shape) for a in arrs]}")
    if shape[0] > MAX_N:
        raise ValueError(f"at most {MAX_N} days per call, got {shape[0]}")
    return arrs, shape


def daily_cycle(ameans):
    """The numbers behind the daily-cycle box plots of G:490-502: ameans, the dict ensemble.generate_one_per_condition returns
    (gen, real, fraction_gen, fraction_real, each (n, 24)) -> {key: BoxStats with fields (1, 24)}, the 4 x 24 columns in one
    launch."""
    arrs, shape = _check_ameans(ameans)
    require_gpu()
    dev = [device_f32(a, k) for a, k in zip(arrs, AMEAN_KEYS)]
    stats = boxplot_stats(torch.stack([d.to(dev[0].device) for d in dev]))
    out = {}
    for b, key in enumerate(AMEAN_KEYS):
        out[key] = BoxStats(*[getattr(stats, f)[b:b + 1] for f in STAT_FIELDS], sorted=stats.sorted[b:b + 1])
    return out


def _fmt(v):
    """a float as pandas' to_csv writes it: the shortest text that reads back to the same float32 / float64"""
    return str(v) if isinstance(v, np.float32) else repr(float(v))


def write_ameans_csv(path, ameans):
    """G:473-488: gen_and_real_ameans_*.csv, columns ',fraction,precip,typ,hour': per hour 1 .. 24 the n generated rows, then the n
    real ones, the index restarting at 0 in every block."""
    arrs, shape = _check_ameans(ameans)
    gen, real, fgen, freal = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in arrs]
    with open(path, "w") as f:
        f.write(",fraction,precip,typ,hour\n")
        for i in range(shape[1]):
            for frac, precip, typ in ((fgen, gen, "generated"), (freal, real, "real")):
                f.writelines(f"{r},{_fmt(frac[r, i])},{_fmt(precip[r, i])},{typ},{i + 1}\n" for r in range(shape[0]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the condition-sensitivity check, G:548-604
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class ConditionalCheck:
    """One pair of conditions (statistic / pvalue (24,), fractions (n, 24)) or P pairs (statistic / pvalue (P, 24), fractions
    (P, n, 24)): the area-mean fractions of the two ensembles (amean_fraction_gen1 / 2, G:563, 565; float32 numpy), the KS statistic
    and p-value per hour (G:581-584) and the box statistics per (condition, hour) (G:600): box1 / box2, BoxStats with fields (P, 24)
    and sorted columns (P, n, 24) -- P = 1 for one pair, as daily_cycle's, so box1.fliers(0, hour) / box1.column(0, hour) address a
    column in both cases; latent, the shared block (n, 100)."""
    fractions1: np.ndarray
    fractions2: np.ndarray
    statistic: np.ndarray
    pvalue: np.ndarray
    box1: BoxStats
    box2: BoxStats
    latent: Optional[np.ndarray] = None

    def write_csv(self, path, pair=None):
        """G:567-579: check_conditional_dist_samenoise_*.csv, columns ',fraction,cond,hour'."""
        f1, f2 = self._pair(pair)
        with open(path, "w") as f:
            f.write(",fraction,cond,hour\n")
            for i in range(f1.shape[1]):
                for frac, cond in ((f1, 1), (f2, 2)):
                    f.writelines(f"{r},{_fmt(frac[r, i])},{cond},{i + 1}\n" for r in range(f1.shape[0]))

    def write_pvalues(self, path, pair=None):
        """G:585: np.savetxt of the 24 p-values ('%.18e', one per line)."""
        p = self.pvalue if self.pvalue.ndim == 1 else self.pvalue[self._index(pair)]
        np.savetxt(path, p)

    def _index(self, pair):
        if self.fractions1.ndim == 2:
            return None
        if pair is None:
            raise ValueError("a batched result needs the number of the pair to write")
        return int(pair)

    def _pair(self, pair):
        k = self._index(pair)
        return (self.fractions1, self.fractions2) if k is None else (self.fractions1[k], self.fractions2[k])


def _check_from_fractions(f1, f2):
    """f1, f2 (P, n, 24) float32 CUDA -> statistic, pvalue (P, 24), box statistics of the 2 P x 24 columns in one launch each"""
    d, p = ks_2samp(f1, f2)
    box = boxplot_stats(torch.cat([f1, f2]))
    P = f1.shape[0]
    halves = [BoxStats(*[getattr(box, f)[s] for f in STAT_FIELDS], sorted=box.sorted[s]) for s in (slice(0, P), slice(P, 2 * P))]
    return d, p, halves


def conditional_distribution_check(gen, cond1_norm, cond2_norm, n_members=1000, latent=None):
    """The loop body of G:553-585 for one pair of normalised conditions (nd, nd, 1): two ensembles of n_members days from ONE latent
    block (ensemble.generate_same_noise_pair; `latent` (n_members, 100), or drawn from the global numpy RNG as G:552), their hourly
    area-mean fractions, ks_2samp per hour and the box statistics per (condition, hour) -> ConditionalCheck with statistic / pvalue (24,) and
    box1 / box2 of fields (1, 24).
    The latent block used is returned on the result."""
    if not 1 <= int(n_members) <= MAX_N:
        raise ValueError(f"1 .. {MAX_N} members, got {n_members}")
    require_gpu()
    e1, e2, latent = ensemble.generate_same_noise_pair(gen, cond1_norm, cond2_norm, n_members=int(n_members), latent=latent)
    f1, f2 = e1.mean(dim=(2, 3)).unsqueeze(0), e2.mean(dim=(2, 3)).unsqueeze(0)          # G:563, 565
    d, p, (b1, b2) = _check_from_fractions(f1, f2)
    return ConditionalCheck(f1[0].cpu().numpy(), f2[0].cpu().numpy(), d[0], p[0], b1, b2, latent)


def conditional_distribution_checks(gen, cond_pairs, n_members=1000, latent=None):
    """G:551-585 for P pairs of conditions, [(cond1_norm, cond2_norm), ...]: as the reference, ONE latent block serves every pair
    and both members of it (G:552 draws it once, outside the loop); the ensembles are generated pair by pair, then the KS of all
    P x 24 columns runs in one launch and the box statistics of all 2 P x 24 in another -> ConditionalCheck with statistic / pvalue / box fields (P, 24)."""
    pairs = list(cond_pairs)
    if not pairs or any(len(pr) != 2 for pr in pairs):
        raise ValueError("cond_pairs must be a non-empty list of (cond1_norm, cond2_norm)")
    if not 1 <= int(n_members) <= MAX_N:
        raise ValueError(f"1 .. {MAX_N} members, got {n_members}")
    require_gpu()
    if latent is None:
        latent = np.random.normal(size=(int(n_members), W.LATENT_DIM)).astype(np.float32)
    f1, f2 = [], []
    for c1, c2 in pairs:
        e1, e2, _ = ensemble.generate_same_noise_pair(gen, c1, c2, n_members=int(n_members), latent=latent)
        f1.append(e1.mean(dim=(2, 3)))
        f2.append(e2.mean(dim=(2, 3)))
    f1, f2 = torch.stack(f1), torch.stack(f2)
    d, p, (b1, b2) = _check_from_fractions(f1, f2)
    return ConditionalCheck(f1.cpu().numpy(), f2.cpu().numpy(), d, p, b1, b2, latent)
