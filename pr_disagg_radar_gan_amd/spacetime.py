"""Space-time structure of hourly fields (csrc/rdgan_spacetime.hip.h): does the rain move?  The wet/dry
agreement between hour h at pixel p and hour h + k at pixel p + d for every small displacement d, and for every pair of hours the
displacement that best maps one wet mask onto the other -- the diagnostic that sees rain areas which jump at random from one hour
to the next instead of travelling, where every single hour and every single pixel's day look right.

A plane is one (day, hour) map; a pixel is wet at threshold t when x > thr[t] in fp32, bad when it is NaN or +-inf (never wet).  A
displacement d = (dy, dx), |dy|, |dx| <= radius, dy in rows and dx in columns, points from the earlier hour to the later one: a
positive dx means the rain moved towards larger x.  Hours pair inside a day only.  A SpaceTimeStructure accumulates, over any
number of add() calls, the integer state include/rdgan.h lists for rdgan_spacetime_accumulate; the array is read on the device and
never copied to the host, and the state does not depend on how the days were split into calls or on planes_per_pass.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, whole_number
from ._hourly import MAX_PLANE, NHOURS, HourlyAccumulator, div as _div, evaluate_field, tv as _tv
from .verification import check_event_thresholds

MAX_RADIUS = 8                                                               # RD_ST_MAXR
MAX_LAG = 6                                                                  # RD_ST_MAXK
MAX_PASS = 65520                                                             # RD_ST_MAXPASS: planes of a pass, 2730 days
MAX_TILE_WORDS = 8                                                           # RD_ST_MAXCW
LDS_WORDS = 4096                                                             # RD_ST_LDS_WORDS
_DEFAULT_PASS_PIXELS = 1 << 28                                               # 9 bits per pixel at 8 thresholds: 288 MB at most by default


def check_radius(radius):
    return whole_number(radius, 1, MAX_RADIUS, "radius")


def check_max_lag(max_lag):
    return whole_number(max_lag, 1, MAX_LAG, "max_lag")


def check_planes_per_pass(planes_per_pass):
    """None, or a whole number of planes that holds at least one day"""
    return None if planes_per_pass is None else whole_number(planes_per_pass, NHOURS, MAX_PASS, "planes_per_pass, unless None,")


def check_plane(ny, nx, radius, what="hourly"):
    if min(ny, nx) < 2 * radius + 1:
        raise ValueError(f"{what}: a plane of {ny} x {nx} is smaller than 2 radius + 1 = {2 * radius + 1}")
    if ny * nx > MAX_PLANE:
        raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")


def n_displacements(radius):
    return (2 * radius + 1) ** 2


def per_threshold(radius, max_lag):
    """words of a threshold's block of the state"""
    return (3 * (max_lag + 1) + max_lag) * n_displacements(radius) + 3 * max_lag


def state_count(n_thresholds, radius, max_lag):
    """rdgan_spacetime_state_count, on the host"""
    return (max_lag + 1) * n_displacements(radius) + n_thresholds * per_threshold(radius, max_lag) + 2


def tile_shape(ny, nx, radius):
    """(rows, words) of the tile the correlate kernel walks a plane in (rd_st_tile of the kernel header): a plane with more rows
    than that is taken in row bands, one with more words in column bands"""
    words = min((nx + 63) // 64, MAX_TILE_WORDS)
    most = (LDS_WORDS - 4 * radius * (words + 2)) // (4 * words + 4)
    bands = -(-ny // most)
    return -(-ny // bands), words


def split_state(counts, n_thresholds, radius, max_lag):
    """the flat state of rdgan_spacetime_accumulate (numpy) -> dict of named int64 arrays; a displacement map is (2R + 1, 2R + 1)
    = [dy + R][dx + R]"""
    T, K, side = n_thresholds, max_lag, 2 * radius + 1
    D, PT = side * side, per_threshold(radius, max_lag)
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (state_count(T, radius, K),):
        raise ValueError(f"expected {state_count(T, radius, K)} counts, got {c.shape}")
    per = c[(K + 1) * D:(K + 1) * D + T * PT].reshape(T, PT)
    pooled = lambda j: per[:, j * (K + 1) * D:(j + 1) * (K + 1) * D].reshape(T, K + 1, side, side).copy()
    tail = 3 * (K + 1) * D + K * D
    return dict(pairs=c[:(K + 1) * D].reshape(K + 1, side, side).copy(), wet_first=pooled(0), wet_second=pooled(1), joint=pooled(2),
                shift_hist=per[:, 3 * (K + 1) * D:tail].reshape(T, K, side, side).copy(), no_shift=per[:, tail:tail + K].copy(),
                dist_best=per[:, tail + K:tail + 2 * K].copy(), dist_zero=per[:, tail + 2 * K:].copy(),
                n_days=int(c[-2]), n_bad_pixels=int(c[-1]))


@dataclass
class SpaceTimeStats:
    """What SpaceTimeStructure.result returns, numpy on the host, int64; T thresholds, lags k = 0 .. K for the pooled counts and
    1 .. K (index k - 1) for the shifts, a displacement map [dy + R][dx + R].  pairs (K + 1, 2R + 1, 2R + 1); wet_first,
    wet_second, joint (T, K + 1, 2R + 1, 2R + 1); shift_hist (T, K, 2R + 1, 2R + 1); no_shift, dist_best, dist_zero (T, K)."""
    thresholds: tuple
    radius: int
    max_lag: int
    n_days: int
    n_bad_pixels: int
    pairs: np.ndarray
    wet_first: np.ndarray
    wet_second: np.ndarray
    joint: np.ndarray
    shift_hist: np.ndarray
    no_shift: np.ndarray
    dist_best: np.ndarray
    dist_zero: np.ndarray

    def displacements(self):
        """(dy, dx), each (2R + 1, 2R + 1): the displacement of every cell of a map"""
        r = np.arange(-self.radius, self.radius + 1)
        return np.meshgrid(r, r, indexing="ij")

    def indicator_correlation(self):
        """(T, K + 1, 2R + 1, 2R + 1): the phi coefficient of "wet at h in p" and "wet at h + k in p + d" over the pairs;
        NaN where one of the two never or always happens"""
        n, a, b, j = (np.asarray(v, dtype=np.float64) for v in (self.pairs[None], self.wet_first, self.wet_second, self.joint))
        return _div(n * j - a * b, np.sqrt(a * (n - a) * b * (n - b)))

    def n_informative(self):
        """(T, K): pairs of hours with a shift"""
        return self.shift_hist.sum(axis=(2, 3))

    def shift_distribution(self):
        """(T, K, 2R + 1, 2R + 1): the share of the informative pairs with shift d"""
        return _div(self.shift_hist, self.n_informative()[:, :, None, None])

    def mean_shift(self):
        """(T, K, 2): the mean (dy, dx) of the informative pairs"""
        dy, dx = self.displacements()
        return np.stack([_div((self.shift_hist * dy).sum(axis=(2, 3)), self.n_informative()),
                         _div((self.shift_hist * dx).sum(axis=(2, 3)), self.n_informative())], axis=-1)

    def mean_speed(self):
        """(T, K): the mean of sqrt(dy^2 + dx^2), pixels per k hours"""
        dy, dx = self.displacements()
        return _div((self.shift_hist * np.sqrt(dy * dy + dx * dx)).sum(axis=(2, 3)), self.n_informative())

    def stationary_fraction(self):
        """(T, K): the share of the informative pairs that did not move"""
        return _div(self.shift_hist[:, :, self.radius, self.radius], self.n_informative())

    def informative_fraction(self):
        """(T, K): the share of the pairs of hours that are informative"""
        return _div(self.n_informative(), self.n_informative() + self.no_shift)

    def shift_gain(self):
        """(T, K): 1 - dist_best / dist_zero, how much of the hour-to-hour disagreement the best shift removes"""
        return 1.0 - _div(self.dist_best, self.dist_zero)


def compare(a, b):
    """Two SpaceTimeStats with the same thresholds, radius and max_lag (real days against generated days) -> dict: tv_shift
    (T, K), the total-variation distance of the shift distributions; the differences a - b of mean_speed, stationary_fraction and
    shift_gain (T, K); max_abs_correlation (T, K + 1), the largest absolute difference of the correlation maps"""
    if not (isinstance(a, SpaceTimeStats) and isinstance(b, SpaceTimeStats)):
        raise ValueError("compare takes two SpaceTimeStats")
    if tuple(a.thresholds) != tuple(b.thresholds):
        raise ValueError(f"the two statistics have different thresholds: {a.thresholds} and {b.thresholds}")
    if a.radius != b.radius or a.max_lag != b.max_lag:
        raise ValueError(f"the two statistics have different radius or max_lag: {a.radius}, {a.max_lag} and {b.radius}, {b.max_lag}")
    T, K = a.shift_hist.shape[:2]
    with np.errstate(invalid="ignore"):
        corr = np.abs(a.indicator_correlation() - b.indicator_correlation()).reshape(T, K + 1, -1)
    # (over the displacements at which both maps are defined; NaN where there is none)
    gap = np.where(np.isnan(corr).all(axis=-1), np.nan, np.where(np.isnan(corr), -np.inf, corr).max(axis=-1))
    return dict(thresholds=tuple(a.thresholds),
                tv_shift=_tv(a.shift_distribution().reshape(T, K, -1), b.shift_distribution().reshape(T, K, -1)),
                mean_speed=a.mean_speed() - b.mean_speed(), stationary_fraction=a.stationary_fraction() - b.stationary_fraction(),
                shift_gain=a.shift_gain() - b.shift_gain(), max_abs_correlation=gap)


def stats_from_state(counts, thresholds, radius, max_lag):
    """the flat state (numpy) -> SpaceTimeStats"""
    thr = check_event_thresholds(thresholds)
    radius, max_lag = check_radius(radius), check_max_lag(max_lag)
    return SpaceTimeStats(thresholds=tuple(float(t) for t in thr), radius=radius, max_lag=max_lag,
                          **split_state(counts, len(thr), radius, max_lag))


class SpaceTimeStructure(HourlyAccumulator):
    """The state of a space-time evaluation on the device.  thresholds: the wet-pixel events in the unit of the data; radius: the
    largest displacement, in pixels, along either axis (1 .. 8); max_lag: the largest lag in hours (1 .. 6); planes_per_pass: how
    many (day, hour) planes the workspace holds at a time, at least 24 and taken in whole days, (T + 1) bits per pixel -- None: up
    to 2^28 pixels.  The result does not depend on it.  add(hourly) is HourlyAccumulator's; state(): counts
    (state_count(T, radius, max_lag),) int64."""
    entry, workspace_entry = "rdgan_spacetime_accumulate", "rdgan_spacetime_workspace_bytes"

    def __init__(self, thresholds, radius=4, max_lag=1, planes_per_pass=None):
        self.thr = check_event_thresholds(thresholds)
        self.radius = check_radius(radius)
        self.max_lag = check_max_lag(max_lag)
        self.planes_per_pass = check_planes_per_pass(planes_per_pass)
        self.reset()

    def _state_tensors(self, device):
        self.counts = torch.zeros(state_count(len(self.thr), self.radius, self.max_lag), dtype=torch.int64, device=device)

    def _check_plane(self, ny, nx, what):
        check_plane(ny, nx, self.radius, what)

    def _pass_units(self, n, ny, nx):
        per_pass = self.planes_per_pass or max(NHOURS, _DEFAULT_PASS_PIXELS // (ny * nx))
        return max(NHOURS, min(per_pass, n * NHOURS, MAX_PASS) // NHOURS * NHOURS)

    def _workspace_args(self, n, ny, nx):
        return ny, nx, len(self.thr), self._pass_units(n, ny, nx)

    def _entry_args(self, ny, nx, out):
        return ny, nx, _hp(self.thr), len(self.thr), self.radius, self.max_lag, _p(self.counts)

    def result(self):
        """-> SpaceTimeStats"""
        return stats_from_state(self.state().cpu().numpy(), self.thr, self.radius, self.max_lag)


def spacetime_structure(hourly, thresholds, radius=4, max_lag=1, planes_per_pass=None):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> SpaceTimeStats"""
    return SpaceTimeStructure(thresholds, radius, max_lag, planes_per_pass).add(hourly).result()


def spacetime_structure_field(gen, daily, n_scenarios, thresholds, radius=4, max_lag=1, planes_per_pass=None, scenario_chunk=16,
                              overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their space-time structure without holding them:
    _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on a SpaceTimeStructure.
    -> SpaceTimeStats"""
    return evaluate_field(SpaceTimeStructure(thresholds, radius, max_lag, planes_per_pass), gen, daily, n_scenarios, scenario_chunk,
                          overlap, latent_mode, seed, latent, chunk, norm_scale)
