"""Extremes of hourly fields (csrc/rdgan_extremes.hip.h): the intensity-duration-frequency analysis a
disaggregator is judged by.  Three steps, each usable on its own:

 1. BlockMaxima: for every pixel and every block of days (a year or a season, or member * B + year for an ensemble) the largest
    accumulation over any k consecutive hours.  Integers throughout, with the conventions of areal.py and catchments.py:
    q = rint(x * 1024) in units of 2^-10 mm; a pixel-hour is bad when x is NaN, +-inf, negative or >= 2048; a pixel-day that holds a
    bad hour is void -- it contributes nothing and is counted.  A window is w consecutive hours WITHIN the day: windows do not cross
    midnight, because days are independent units everywhere in this project (a 24-hour window is the day's sum, and the largest
    6-hour depth of a storm that straddles midnight is not seen whole).  The state does not depend on how the days are grouped into
    calls, on their order or on days_per_run.
 2. lmoment_sums: for S series of B block maxima at M positions the exact integer sums over the ascending order statistics
    A0 = sum x_(j), A1 = sum (j - 1) x_(j), A2 = sum (j - 1)(j - 2) x_(j), invariant under the order of tied values.  A table comes
    from BlockMaxima (pixels), or from the per-day depths of areal.areal_extremes / catchments.catchment_rainfall through
    block_maxima_of_depths.
 3. ExtremeStats: L-moments, Gumbel and GEV parameters (Hosking 1985), return levels, the band an ensemble spans and whether an
    observation lies inside it -- torch float64 on the device the sums lie on.

extremes() and extremes_field() are the one-call forms for an array that is held and for a generator whose scenarios are not.

Out of scope: windows across midnight and multi-day durations, maximum-likelihood fits, bootstrap confidence intervals, regional
pooling of L-moments, peaks over threshold, plots.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
import math
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import field as F, weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream, whole_number
from ._hourly import MAX_MEMBERS, MAX_PLANE, UNIT, admit, to_state_device
from .engine import require_gpu
from .field_products import check_probs, check_windows, member_stats_device

MAX_SERIES_BLOCKS = 128                                                      # RD_EX_MAXB: blocks of one series
MAX_VALUE = 1 << 40                                                          # RD_EX_MAXVALUE: a maximum is below this
MAX_STATE = 1 << 31                                                          # RD_EX_MAXSTATE: NB K ny nx
MAX_BLOCKS = 1 << 31                                                         # RD_EX_MAXBLOCKS
MAX_RUN = 4096                                                               # RD_EX_MAXRUN
MAX_TABLE = 1 << 40                                                          # S B M
EULER_GAMMA = 0.5772156649015329
GEV_SWITCH = 1e-6                                                            # |k| below which gev() takes the Gumbel limit
DISTS = ("gumbel", "gev", "empirical")

BlockMaximaResult = namedtuple("BlockMaximaResult", "bmax ndays nvoid")


def window_mask(windows):
    """the window list as the bit mask the kernels take: bit w - 1 for a window of w hours"""
    return int(sum(1 << (int(w) - 1) for w in windows))


def check_block(block, n, n_blocks):
    """-> the block of every day as a contiguous int32 array (n,): a 1-D array or tensor of whole numbers in 0 .. n_blocks - 1"""
    if isinstance(block, torch.Tensor):
        block = block.detach().cpu().numpy()
    b = np.asarray(block)
    if b.ndim != 1 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"block: expected a 1-D array of whole numbers, got {b.dtype} {b.shape}")
    if b.shape[0] != n:
        raise ValueError(f"block: {b.shape[0]} entries for {n} days")
    if b.size and (b.min() < 0 or b.max() >= n_blocks):
        raise ValueError(f"block: every entry must lie in 0 .. {n_blocks - 1}, got {int(b.min())} .. {int(b.max())}")
    return np.ascontiguousarray(b, dtype=np.int32)


class BlockMaxima:
    """The block maxima of the k-hour depths of every pixel, on the device.  windows: the durations in hours
    (field_products.check_windows); n_blocks: NB, fixed here; device: where a numpy input goes (None: "cuda"; a tensor input fixes
    it); days_per_run: the days a workgroup walks before it hands its maxima over, 1 .. 4096 -- None: the library's choice.  The
    result does not depend on it.  Windows lie within the day (the module's docstring)."""

    def __init__(self, windows, n_blocks, device=None, days_per_run=None):
        self.windows = check_windows(windows)
        self.n_blocks = whole_number(n_blocks, 1, MAX_BLOCKS, "n_blocks")
        self.days_per_run = None if days_per_run is None else whole_number(days_per_run, 1, MAX_RUN, "days_per_run")
        self.device = device
        self.reset()

    def reset(self):
        """forget the days added so far (and the plane shape); returns self"""
        self.plane_shape = None
        self.lib = None
        self.bmax = self.ndays = self.nvoid = None
        return self

    def add(self, hourly, block):
        """hourly (..., 24, ny, nx) float32 in mm/h: a CUDA tensor, whose leading axis may have any stride >= the size of one of
        its entries, or a numpy array, admitted as _hourly.admit admits it; the plane shape is fixed by the first call.  block: a
        1-D int array or tensor, the block of every day of hourly in the order of its flattened leading axes, each in
        0 .. n_blocks - 1, in any order -- a value outside is a ValueError before any launch.  Returns self."""
        hourly, from_host, shape, n, stride = admit(hourly, self.plane_shape)
        ny, nx = shape[-2:]
        K, NB = len(self.windows), self.n_blocks
        if ny * nx > MAX_PLANE:
            raise ValueError(f"hourly: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
        if NB * K * ny * nx > MAX_STATE:
            raise ValueError(f"{NB} blocks of {K} windows of {ny * nx} pixels are {NB * K * ny * nx} maxima, the limit is {MAX_STATE}")
        block = check_block(block, n, NB)
        if self.bmax is None:
            require_gpu()
            self.lib = _lib.load()
            device = (self.device or "cuda") if from_host else hourly.device
            self.bmax = torch.full((NB, K, ny * nx), -1, dtype=torch.int64, device=device)
            self.ndays = torch.zeros((NB, ny * nx), dtype=torch.int32, device=device)
            self.nvoid = torch.zeros((NB, ny * nx), dtype=torch.int32, device=device)
        device = self.bmax.device
        hourly = to_state_device(hourly, from_host, device)
        self.plane_shape = shape[-2:]
        with torch.cuda.device(device):
            rc = self.lib.rdgan_block_maxima_accumulate(_p(hourly), n, stride, ny, nx, _hp(block), NB, window_mask(self.windows),
                                                        self.days_per_run or 0, _p(self.bmax), _p(self.ndays), _p(self.nvoid),
                                                        _stream(self.bmax))
        _lib.check(rc, None, "rdgan_block_maxima_accumulate")
        return self

    def state(self):
        """(bmax (NB, K, ny nx) int64, ndays (NB, ny nx) int32, nvoid (NB, ny nx) int32): the state tensors themselves, on the
        device, in the flat order of include/rdgan.h"""
        if self.bmax is None:
            raise ValueError("nothing has been added")
        return self.bmax, self.ndays, self.nvoid

    def result(self):
        """-> BlockMaximaResult on the device: bmax (NB, K, ny, nx) int64 in 1/1024 mm, -1 where the block has no good day at the
        pixel; ndays, nvoid (NB, ny, nx) int32, the good and the void pixel-days"""
        bmax, ndays, nvoid = self.state()
        ny, nx = self.plane_shape
        NB, K = self.n_blocks, len(self.windows)
        return BlockMaximaResult(bmax.view(NB, K, ny, nx), ndays.view(NB, ny, nx), nvoid.view(NB, ny, nx))


def block_maxima_of_depths(depths, block, n_blocks):
    """The per-day depths of areal.areal_extremes(..., return_depths=True) or catchments.catchment_rainfall(..., return_depths=True),
    (n, ...) int64 with -1 for a void day, -> their maxima per block, (n_blocks, ...) int64 on the same device: -1 where a block has
    no day or only void ones.  Plain torch.  lmoment_sums takes the table after a reshape to (S, B, M)."""
    if not (isinstance(depths, torch.Tensor) and depths.dtype == torch.int64 and depths.dim() >= 1 and depths.shape[0] >= 1):
        raise ValueError("depths: expected an int64 tensor (n, ...)")
    n_blocks = whole_number(n_blocks, 1, MAX_BLOCKS, "n_blocks")
    b = torch.from_numpy(check_block(block, int(depths.shape[0]), n_blocks).astype(np.int64)).to(depths.device)
    index = b.view((-1,) + (1,) * (depths.dim() - 1)).expand_as(depths)
    out = torch.full((n_blocks,) + tuple(depths.shape[1:]), -1, dtype=torch.int64, device=depths.device)
    return out.scatter_reduce_(0, index, depths, "amax", include_self=True)


def _check_table(a, what, shape=None):
    """an (S, B, M) table of whole numbers: an integer CUDA tensor or an integer numpy array -> (a, from_host, (S, B, M))"""
    from_host = not isinstance(a, torch.Tensor)
    if from_host:
        a = np.asarray(a)
        integer = np.issubdtype(a.dtype, np.integer)
    else:
        if not a.is_cuda:
            raise ValueError(f"{what}: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
        integer = a.dtype in (torch.int32, torch.int64)
    if not integer:
        raise ValueError(f"{what}: expected whole numbers, got {a.dtype}")
    s = tuple(int(v) for v in a.shape)
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"{what}: expected shape (S, B, M) with no empty axis, got {s}")
    if shape is not None and s != shape:
        raise ValueError(f"{what}: expected shape {shape}, got {s}")
    return a, from_host, s


def lmoment_sums(table, ndays=None, min_days=1, return_sorted=False):
    """table (S, B, M) int64: S series of B block maxima at M positions, a CUDA tensor or a numpy array of whole numbers;
    1 <= B <= 128, every value below 2^40 (so that the sums stay below 2^63: 2^40 128^2 128 = 2^61).  A value below 0 means "no
    maximum" and is left out; with ndays (same shape, whole numbers) so is a block with fewer than min_days good days.
    -> (n (S, M) int32, A (S, M, 3) int64) on the device: the number of maxima used and, over their ascending order statistics
    x_(1) <= .. <= x_(n), A[..., 0] = sum x_(j), A[..., 1] = sum (j - 1) x_(j), A[..., 2] = sum (j - 1)(j - 2) x_(j); with
    return_sorted followed by sorted (S, B, M) int64: x_(1) .. x_(n), then -1 for every entry left out."""
    table, t_host, (S, B, M) = _check_table(table, "table")
    if B > MAX_SERIES_BLOCKS:
        raise ValueError(f"table: {B} blocks in a series, the limit is {MAX_SERIES_BLOCKS}")
    if S * B * M > MAX_TABLE:
        raise ValueError(f"table: {S * B * M} entries, the limit is {MAX_TABLE}")
    min_days = whole_number(min_days, 0, 2 ** 31 - 1, "min_days")
    if ndays is not None:
        ndays, n_host, _ = _check_table(ndays, "ndays", (S, B, M))
    if t_host and int(table.max()) >= MAX_VALUE:
        raise ValueError(f"table: every value must be below 2^40, got {int(table.max())}")
    require_gpu()
    lib = _lib.load()
    if t_host:
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).cuda()
    else:
        table = table.to(torch.int64).contiguous()
        if int(table.max()) >= MAX_VALUE:
            raise ValueError(f"table: every value must be below 2^40, got {int(table.max())}")
    dev = table.device
    if ndays is not None:
        ndays = (torch.from_numpy(np.ascontiguousarray(ndays)) if n_host else ndays).to(device=dev, dtype=torch.int32).contiguous()
    n = torch.empty((S, M), dtype=torch.int32, device=dev)
    A = torch.empty((S, M, 3), dtype=torch.int64, device=dev)
    srt = torch.empty((S, B, M), dtype=torch.int64, device=dev) if return_sorted else None
    with torch.cuda.device(dev):
        rc = lib.rdgan_lmoment_sums(_p(table), _p(ndays), min_days, S, B, M, _p(A), _p(n), _p(srt), _stream(table))
    _lib.check(rc, None, "rdgan_lmoment_sums")
    return (n, A, srt) if return_sorted else (n, A)


# ---------------------------------------------------------------------------------------------------------------------------------
# from sums to return levels: torch float64 wherever the sums lie
def check_periods(T):
    """-> the return periods, in blocks, as a float64 array: 1 .. 64 of them, each finite and above 1"""
    t = np.atleast_1d(np.asarray(T, dtype=np.float64))
    if t.ndim != 1 or not 1 <= t.shape[0] <= 64 or not np.all(np.isfinite(t) & (t > 1.0)):
        raise ValueError(f"T: expected 1 .. 64 finite return periods above 1, got {T!r}")
    return t


def gumbel_params(l1, l2):
    """(loc, scale) of the Gumbel distribution with these L-moments: scale = l2 / ln 2, loc = l1 - gamma scale"""
    scale = l2 / math.log(2.0)
    return l1 - EULER_GAMMA * scale, scale


def gev_params(l1, l2, t3):
    """(loc, scale, shape) of the GEV with these L-moments by Hosking's (1985) approximation, in his sign of the shape k (k > 0:
    bounded above): c = 2 / (3 + t3) - ln 2 / ln 3, k = 7.8590 c + 2.9554 c^2, scale = l2 k / ((1 - 2^-k) Gamma(1 + k)),
    loc = l1 - scale (1 - Gamma(1 + k)) / k.  Where |k| < GEV_SWITCH = 1e-6 the Gumbel limit is taken: the Gumbel parameters and
    shape 0 (the two differ there by about |k| in relative terms).  1 - 2^-k and 1 - Gamma(1 + k) are formed through expm1, so
    the subtractions cancel nothing; what remains is lgamma(1 + k) itself, good to about 2^-53 in absolute terms, which leaves
    (1 - Gamma(1 + k)) / k with a relative error of about 1e-16 / |k|: 1e-10 at the switch, 1e-15 at |k| = 0.1."""
    c = 2.0 / (3.0 + t3) - math.log(2.0) / math.log(3.0)
    k = 7.8590 * c + 2.9554 * c * c
    small = k.abs() < GEV_SWITCH
    ks = torch.where(small, torch.ones_like(k), k)                           # (a stand-in that divides)
    lg = torch.lgamma(1.0 + ks)
    scale = l2 * ks / (-torch.expm1(-ks * math.log(2.0)) * torch.exp(lg))
    loc = l1 - scale * (-torch.expm1(lg)) / ks
    gl, gs = gumbel_params(l1, l2)
    nan = torch.isnan(k)
    keep = lambda a, b: torch.where(small & ~nan, b, a)
    return keep(loc, gl), keep(scale, gs), keep(k, torch.zeros_like(k))


def quantile_level(loc, scale, shape, T):
    """the level exceeded once in T blocks on average, F = 1 - 1 / T: loc - scale ln(-ln F) where shape is 0, else
    loc + scale (1 - (-ln F)^shape) / shape"""
    ly = math.log(-math.log1p(-1.0 / float(T)))                              # ln(-ln F)
    zero = shape == 0
    ks = torch.where(zero, torch.ones_like(shape), shape)
    return torch.where(zero, loc - scale * ly, loc + scale * (-torch.expm1(ks * ly)) / ks)


@dataclass
class ExtremeStats:
    """The L-moment sums of S series of block maxima at the positions `shape`, on whatever device n and A lie on.
      windows   the durations in hours, or None where the positions have no window axis
      n         (S, *shape) int32: the maxima used
      A         (S, *shape, 3) int64: the sums of lmoment_sums
      unit      what one mm is in the table's values: 1024 for pixels, 1024 npix for sums over a catchment -- a number, or a tensor
                that broadcasts against (S, *shape)
      sorted    None, or (S, B, *shape) int64: the sorted maxima (return_sorted), which "empirical" needs
      window_axis  the axis of `shape` that runs over the windows (compare pools per window), or None"""
    windows: tuple
    n: torch.Tensor
    A: torch.Tensor
    unit: object = float(UNIT)
    sorted: torch.Tensor = None
    window_axis: int = 0

    @property
    def n_series(self):
        return int(self.n.shape[0])

    @property
    def shape(self):
        return tuple(int(v) for v in self.n.shape[1:])

    def _mm(self, a):
        return a / self.unit

    def lmoments(self):
        """-> (l1, l2, t3), float64 (S, *shape), l1 and l2 in mm: with b0 = A0 / n, b1 = A1 / (n (n - 1)),
        b2 = A2 / (n (n - 1)(n - 2)): l1 = b0, l2 = 2 b1 - b0, l3 = 6 b2 - 6 b1 + b0, t3 = l3 / l2.  l2 is formed as
        (2 A1 - (n - 1) A0) / (n (n - 1)), whose numerator is an exact integer, so a series of equal values gives exactly 0.
        NaN where n is too small (l1: n < 1, l2: n < 2, t3: n < 3) and t3 also where l2 = 0."""
        n = self.n.to(torch.float64)
        A0, A1, A2 = (self.A[..., i] for i in range(3))
        nan = torch.full_like(n, float("nan"))
        b0 = A0.to(torch.float64) / n
        b1 = A1.to(torch.float64) / (n * (n - 1.0))
        b2 = A2.to(torch.float64) / (n * (n - 1.0) * (n - 2.0))
        l1 = torch.where(self.n >= 1, b0, nan)
        l2 = torch.where(self.n >= 2, (2 * A1 - (self.n.to(torch.int64) - 1) * A0).to(torch.float64) / (n * (n - 1.0)), nan)
        l3 = 6.0 * b2 - 6.0 * b1 + b0
        t3 = torch.where((self.n >= 3) & (l2 != 0), l3 / l2, nan)
        return self._mm(l1), self._mm(l2), t3

    def gumbel(self):
        """-> (loc, scale) in mm by L-moments: scale = l2 / ln 2, loc = l1 - gamma scale; NaN where n < 2 or l2 = 0"""
        l1, l2, _ = self.lmoments()
        l2 = torch.where(l2 != 0, l2, torch.full_like(l2, float("nan")))
        return gumbel_params(l1, l2)

    def gev(self):
        """-> (loc, scale, shape), loc and scale in mm: gev_params of the L-moments; NaN where n < 3 or l2 = 0"""
        l1, l2, t3 = self.lmoments()
        return gev_params(l1, l2, t3)

    def _empirical(self, T):
        if self.sorted is None:
            raise ValueError('dist "empirical" needs the sorted maxima: return_sorted=True')
        B = int(self.sorted.shape[1])
        n = self.n.to(torch.float64)
        x = self._mm(self.sorted.to(torch.float64))
        out = []
        for t in T:
            at = (1.0 - 1.0 / float(t)) * (n + 1.0)                          # the plotting position j / (n + 1) = F at j = at
            ok = (at >= 1.0) & (at <= n)
            j = torch.clamp(torch.floor(at), 1.0, float(B))
            frac = at - j
            lo = (j.to(torch.int64) - 1).unsqueeze(1)
            hi = torch.minimum(lo + 1, torch.clamp(self.n.to(torch.int64) - 1, min=0).unsqueeze(1))
            xl, xh = torch.gather(x, 1, lo).squeeze(1), torch.gather(x, 1, hi).squeeze(1)
            out.append(torch.where(ok, xl + frac * (xh - xl), torch.full_like(n, float("nan"))))
        return torch.stack(out)

    def return_levels(self, T, dist="gumbel"):
        """The levels in mm exceeded once in T blocks on average, T > 1 in blocks (years, for annual maxima) -> float64
        (len(T), S, *shape).  dist "gumbel" and "gev": the fitted distributions' quantiles at F = 1 - 1 / T; "empirical": the
        sorted maxima interpolated linearly at the Weibull plotting positions j / (n + 1), NaN for an F outside
        [1 / (n + 1), n / (n + 1)] (needs return_sorted)."""
        T = check_periods(T)
        if dist not in DISTS:
            raise ValueError(f"dist must be one of {DISTS}, got {dist!r}")
        if dist == "empirical":
            return self._empirical(T)
        if dist == "gumbel":
            loc, scale = self.gumbel()
            shape = torch.zeros_like(loc)
        else:
            loc, scale, shape = self.gev()
        return torch.stack([quantile_level(loc, scale, shape, t) for t in T])

    def band(self, T, probs, dist="gumbel"):
        """Quantiles across the S series (the members of an ensemble) of the return levels: field_products.member_stats_device on
        the levels rounded to float32 -> float32 (len(probs), len(T), *shape); NaN where a member's level is NaN.  S <= 4096."""
        probs = check_probs(probs)
        if self.n_series > MAX_MEMBERS:
            raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {self.n_series}")
        levels = self.return_levels(T, dist)
        return member_stats_device(levels.transpose(0, 1).to(torch.float32).contiguous(), probs).quantiles


def compare(obs, gen, T, probs=(0.05, 0.5, 0.95), dist="gumbel"):
    """Does the observed curve lie inside the band the ensemble spans?  obs: the ExtremeStats of the observations (S = 1), gen: of the
    ensemble, at the same positions and windows.  -> dict: T; probs; obs (len(T), *shape) float32, the observed return levels;
    band (len(probs), len(T), *shape) float32, gen.band; inside (len(T), *shape) bool: band[0] <= obs <= band[-1], compared in
    float32, False where either side is NaN; share_inside: the share of the positions with both sides finite that lie inside, per
    T and window (len(T), K) -- or per T alone, (len(T),), where the positions have no window axis."""
    if not (isinstance(obs, ExtremeStats) and isinstance(gen, ExtremeStats)):
        raise ValueError("compare takes two ExtremeStats")
    if obs.n_series != 1:
        raise ValueError(f"obs: expected one series, got {obs.n_series}")
    if obs.shape != gen.shape or obs.window_axis != gen.window_axis:
        raise ValueError(f"the two statistics have different positions: {obs.shape} and {gen.shape}")
    if (obs.windows is None) != (gen.windows is None) or (obs.windows is not None and tuple(obs.windows) != tuple(gen.windows)):
        raise ValueError(f"the two statistics have different windows: {obs.windows} and {gen.windows}")
    probs = check_probs(probs)
    if len(probs) < 2 or np.any(np.diff(probs) <= 0):
        raise ValueError(f"probs: expected at least two increasing probabilities, got {probs!r}")
    band = gen.band(T, probs, dist)
    level = obs.return_levels(T, dist)[:, 0].to(torch.float32)
    valid = ~torch.isnan(level) & ~torch.isnan(band[0]) & ~torch.isnan(band[-1])
    inside = valid & (level >= band[0]) & (level <= band[-1])
    pooled = [a for a in range(1, level.dim()) if obs.window_axis is None or a != obs.window_axis + 1]
    count = lambda m: m.to(torch.float64).sum(dim=pooled) if pooled else m.to(torch.float64)
    return dict(T=tuple(float(t) for t in check_periods(T)), probs=tuple(float(p) for p in probs), obs=level, band=band, inside=inside,
                share_inside=count(inside) / count(valid))


# ---------------------------------------------------------------------------------------------------------------------------------
def _series_blocks(series, n_blocks):
    series = whole_number(series, 1, MAX_BLOCKS, "series")
    n_blocks = whole_number(n_blocks, 1, MAX_BLOCKS, "n_blocks")
    if n_blocks % series or n_blocks // series > MAX_SERIES_BLOCKS:
        raise ValueError(f"n_blocks = series * B with 1 <= B <= {MAX_SERIES_BLOCKS}, got n_blocks {n_blocks} for {series} series")
    return series, n_blocks // series


def _stats_of(bm, S, B, min_days, return_sorted):
    """the ExtremeStats of a BlockMaxima whose NB = S * B blocks are member * B + block"""
    bmax, ndays, _ = bm.state()
    ny, nx = bm.plane_shape
    K = len(bm.windows)
    table = bmax.view(S, B, K * ny * nx)
    # (a block has a maximum exactly where it has a good day, so min_days <= 1 needs no second table)
    nd = ndays.view(S, B, 1, ny * nx).expand(S, B, K, ny * nx).reshape(S, B, K * ny * nx) if min_days > 1 else None
    out = lmoment_sums(table, nd, min_days, return_sorted)
    srt = out[2].view(S, B, K, ny, nx) if return_sorted else None
    return ExtremeStats(tuple(int(w) for w in bm.windows), out[0].view(S, K, ny, nx), out[1].view(S, K, ny, nx, 3), float(UNIT), srt, 0)


def extremes(hourly, block, n_blocks, windows, series=1, min_days=1, return_sorted=False):
    """One call for an array that is held: hourly (..., 24, ny, nx) and the block of every day, as BlockMaxima.add takes them;
    n_blocks = series * B, block member * B + b being block b of series `member` (series = 1: block b itself).  min_days: a block
    with fewer good days at a pixel is left out there.  -> ExtremeStats over (S, K, ny, nx), unit 1024, windows within the day."""
    S, B = _series_blocks(series, n_blocks)
    min_days = whole_number(min_days, 0, 2 ** 31 - 1, "min_days")
    return _stats_of(BlockMaxima(windows, n_blocks).add(hourly, block), S, B, min_days, bool(return_sorted))


def extremes_field(gen, daily, n_scenarios, block, n_blocks_per_member, windows, min_days=1, return_sorted=False, scenario_chunk=16,
                   overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate the daily maps (D, ny, nx) (or one, (ny, nx)) into n_scenarios scenarios and take the extremes of every
    scenario without holding the hourly ensemble: block (D,) is the block of every day, 0 .. n_blocks_per_member - 1 = B - 1
    (B <= 128), and day d of scenario `member` enters block member * B + block[d] of a BlockMaxima.  -> ExtremeStats with
    S = n_scenarios.
    The scenarios are those of field._stream_scenarios: the latent array is drawn once for all scenarios, exactly as
    field.disaggregate draws it for the same seed, latent and numpy RNG state; disaggregate then runs for scenario_chunk scenarios at
    a time into one reused buffer and each result is added.  The result is the evaluation of the hourly values those disaggregate
    calls produce.  The generator's fp32 output depends in its last bits on the batch of tiles it runs in, so against
    extremes(disaggregate(...all scenarios...)[0], ...) the integer sums are equal when the batches are the same (`chunk` at most
    one unit's wet tiles, or one scenario chunk); otherwise the two differ as disaggregate's own outputs differ between values of
    `chunk`."""
    S, step = F._check_scenarios(n_scenarios, scenario_chunk)
    B = whole_number(n_blocks_per_member, 1, MAX_SERIES_BLOCKS, "n_blocks_per_member")
    min_days = whole_number(min_days, 0, 2 ** 31 - 1, "min_days")
    bm = BlockMaxima(windows, S * B)
    req = F._check_request(gen, daily, S, overlap, latent_mode, latent, chunk, norm_scale)
    D, ny, nx = req[2], req[3], req[4]
    if S * B * len(bm.windows) * ny * nx > MAX_STATE:
        raise ValueError(f"{S * B} blocks of {len(bm.windows)} windows of {ny * nx} pixels, the limit is {MAX_STATE} maxima")
    block = check_block(block, D, B).astype(np.int64)
    done = 0

    def sink(buf):
        nonlocal done
        n = int(buf.shape[0])
        bm.add(buf, ((np.arange(done, done + n, dtype=np.int64) * B)[:, None] + block[None, :]).ravel())
        done += n

    F._stream_scenarios(gen, req, req[0], S, step, sink, overlap, latent_mode, seed, latent, chunk, norm_scale)
    return _stats_of(bm, S, B, min_days, bool(return_sorted))
