"""Scaling of hourly fields (csrc/rdgan_scaling.hip.h): how the variability of rain changes with the scale it
is looked at.  For every day of an hourly array the field is summed over dyadic boxes of 2^a x 2^a pixels (a = 0 .. A, anchored at
pixel (0, 0), wholly inside the plane) and over the aligned windows of 1, 2, 4, 8 and 24 hours of the day; of the box sums R at every
pair of levels the state keeps the count, the wet count, the first two moments exactly, the maximum and a histogram of eight bins
per octave.  From it: the wet fraction against scale (box counting), the moments of the box-mean intensity and their scaling
exponents over space and over time -- the moment-scaling function a multiplicative cascade is defined by -- and the quantiles of the
areal-temporal means.  A generator that is too intermittent at one hour or too smooth at 8 x 8 pixels shows here although every pixel
distribution and every spectrum slope is right.

Everything is defined in integers: q = rint(x * 1024) in units of 2^-10 mm; a pixel-hour is bad when x is NaN, +-inf, negative or
>= 2048, and a box-window that holds a bad pixel-hour is void.  A ScalingStructure accumulates, over any number of add() calls, the
integer state include/rdgan.h lists for rdgan_scaling_accumulate; the array is read on the device and never copied to the host, and
the state does not depend on how the days were split into calls.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import weights as W
from ._dev import ptr as _p, whole_number
from ._hourly import MAX_PLANE, NHOURS, UNIT, HourlyAccumulator, div as _div, evaluate_field, tv as _tv

MAX_SPACE_LEVELS = 6                                                         # RD_SC_MAXA
DURATIONS = (1, 2, 4, 8, 24)                                                 # hours of the time levels b = 0 .. 4
N_TIME = len(DURATIONS)                                                      # RD_SC_NT
N_BINS = 288                                                                 # RD_SC_BINS
N_FIXED = 8                                                                  # RD_SC_HIST: words of a record in front of the histogram
RECORD = N_FIXED + N_BINS                                                    # RD_SC_REC
SPLIT = 19                                                                   # RD_SC_SPLIT: R = h 2^19 + l in the second moment
WORKSPACE = 8                                                                # RD_SC_WORKSPACE
# the words of the record of one (a, b) (RD_SC_NBOXES ..)
_NBOXES, _NVOID, _NWET, _SUM1, _SUM2_HH, _SUM2_HL, _SUM2_LL, _MAX_R = range(N_FIXED)
WORDS = ("n_boxes", "n_void", "n_wet", "sum1", "sum2_hh", "sum2_hl", "sum2_ll", "max_R")
DEFAULT_ORDERS = (1.0, 2.0, 3.0)                                             # the moment orders compare() looks at


def check_space_levels(space_levels):
    return None if space_levels is None else whole_number(space_levels, 0, MAX_SPACE_LEVELS, "space_levels, unless None,")


def largest_space_levels(ny, nx):
    """the largest A <= 6 with 2^A <= min(ny, nx)"""
    return min(MAX_SPACE_LEVELS, int(min(ny, nx)).bit_length() - 1)


def state_count(space_levels):
    return (space_levels + 1) * N_TIME * RECORD + 2


def split_state(counts, space_levels):
    """the flat state of rdgan_scaling_accumulate (numpy) -> dict of named int64 arrays, (A + 1, 5) each, hist (A + 1, 5, 288)"""
    A = space_levels
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (state_count(A),):
        raise ValueError(f"expected {state_count(A)} counts, got {c.shape}")
    per = c[:-2].reshape(A + 1, N_TIME, RECORD)
    out = {name: per[:, :, i].copy() for i, name in enumerate(WORDS)}
    out.update(hist=per[:, :, N_FIXED:].copy(), n_days_total=int(c[-2]), n_bad=int(c[-1]))
    return out


def bin_edges():
    """(289,) int64: bin i holds the R with edges[i] <= R < edges[i + 1]; 0, 1 .. 7, then eight bins per octave up to 2^38"""
    fine = [(8 + m) << (e - 3) for e in range(3, 38) for m in range(8)]
    return np.array(list(range(8)) + fine + [1 << 38], dtype=np.int64)


def bin_of(R):
    """the bin of a box sum R >= 0 (numpy, any shape), the kernel's rule: 0 for R = 0, R itself up to 7, then, with e =
    floor(log2 R), 8 + 8 (e - 3) + the three bits below the leading one"""
    R = np.asarray(R, dtype=np.int64)
    if np.any(R < 0) or np.any(R >= 1 << 38):
        raise ValueError("bin_of: R must lie in 0 .. 2^38 - 1")
    return np.searchsorted(bin_edges(), R, side="right") - 1


def bin_values():
    """(288,) float64: the value a bin stands for -- R itself in the bins of one value, the geometric midpoint of the edges above"""
    e = bin_edges().astype(np.float64)
    mid = np.sqrt(e[:-1] * e[1:])
    mid[:8] = np.arange(8)
    return mid


@dataclass
class ScalingFit:
    """What ScalingStats.exponents returns.  slopes, intercepts, residuals (Q, M): the least-squares line of log M_q against log
    scale for every order of qs and every level of the other axis (M = 5 time levels for axis "space", A + 1 space levels for
    "time"); residuals is the root mean square of the log-residuals, NaN for a fit through two points' worth of freedom or less --
    it is what says whether there is a scaling law at all.  scales: the pixels or hours of the levels used."""
    axis: str
    qs: tuple
    levels: tuple
    scales: tuple
    slopes: np.ndarray
    intercepts: np.ndarray
    residuals: np.ndarray


@dataclass
class ScalingStats:
    """What ScalingStructure.result returns, numpy on the host, int64; A = space_levels.  n_boxes, n_void, n_wet, sum1, sum2_hh,
    sum2_hl, sum2_ll, max_R (A + 1, 5) by space level a (boxes of 2^a pixels a side) and time level b (1, 2, 4, 8, 24 hours), box
    sums in 1/1024 mm; hist (A + 1, 5, 288) by bin_of(R).  n_days_total and n_bad (bad pixel-hours) once."""
    space_levels: int
    n_days_total: int
    n_bad: int
    n_boxes: np.ndarray
    n_void: np.ndarray
    n_wet: np.ndarray
    sum1: np.ndarray
    sum2_hh: np.ndarray
    sum2_hl: np.ndarray
    sum2_ll: np.ndarray
    max_R: np.ndarray
    hist: np.ndarray

    def widths(self):
        return tuple(1 << a for a in range(self.space_levels + 1))

    def _cells(self):
        """(A + 1, 5) float64: the pixel-hours of a box-window times 1024 -- R over it is the box-mean intensity in mm/h"""
        return np.outer(np.square(np.array(self.widths(), dtype=np.float64)), np.array(DURATIONS, dtype=np.float64)) * UNIT

    def sum2(self):
        """(A + 1, 5) Python ints: the exact sum of R^2 over the valid box-windows"""
        out = np.empty(self.n_boxes.shape, dtype=object)
        for i in np.ndindex(out.shape):
            out[i] = (int(self.sum2_hh[i]) << (2 * SPLIT)) + (int(self.sum2_hl[i]) << (SPLIT + 1)) + int(self.sum2_ll[i])
        return out

    def wet_fraction(self):
        """(A + 1, 5): the share of the valid box-windows with rain; NaN without a valid one"""
        return _div(self.n_wet, self.n_boxes)

    def mean_intensity(self):
        """(A + 1, 5): the mean of the box-mean intensity, mm/h; NaN without a valid box-window"""
        return _div(self.sum1, self.n_boxes * self._cells())

    def max_intensity(self):
        """(A + 1, 5): the largest box-mean intensity, mm/h; NaN without a valid box-window"""
        return np.where(self.n_boxes > 0, self.max_R / self._cells(), np.nan)

    def moment(self, q):
        """(A + 1, 5): the mean over the valid box-windows of I^q, I the box-mean intensity in mm/h, for q >= 0.  Exact from the
        state for q = 0 (0^0 counts as 0: the share of wet boxes, the box-counting convention), 1 and 2; for any other q from the
        histogram with a bin's value (bin_values) for every R in it, within the factor (9/8)^(q/2) of the exact moment.  NaN without
        a valid box-window."""
        q = float(q)
        if not q >= 0.0 or q == np.inf:
            raise ValueError(f"moment: q must be a finite number >= 0, got {q!r}")
        if q == 0.0:
            return self.wet_fraction()
        if q == 1.0:
            return self.mean_intensity()
        cells = self._cells()
        if q == 2.0:
            s2 = self.sum2()
            exact = np.array([[float(s2[i, j]) for j in range(N_TIME)] for i in range(s2.shape[0])])
            return _div(exact, self.n_boxes * cells * cells)
        values = bin_values()[None, None, :] / cells[:, :, None]                         # mm/h
        with np.errstate(over="ignore"):
            total = (self.hist[:, :, 1:] * values[:, :, 1:] ** q).sum(axis=2)
        return _div(total, self.n_boxes)

    def exponents(self, qs, axis="space", levels=None):
        """Least-squares slopes of log M_q against log scale -> ScalingFit.  axis "space": over the space levels (scale 2^a pixels),
        one fit per time level; "time": over the time levels (scale T hours), one per space level.  levels: the indices along the
        axis that enter the fit (None: all), at least two.  A fit with a level whose moment is NaN or 0 is NaN."""
        qs = _check_orders(qs)
        if axis not in ("space", "time"):
            raise ValueError(f"axis must be 'space' or 'time', got {axis!r}")
        n_axis = self.space_levels + 1 if axis == "space" else N_TIME
        if levels is None:
            levels = tuple(range(n_axis))
        try:
            levels = tuple(whole_number(v, 0, n_axis - 1, "every value of levels") for v in levels)
        except TypeError:
            raise ValueError("levels: expected a list of whole numbers") from None
        if len(set(levels)) != len(levels):
            raise ValueError(f"levels must be distinct, got {levels}")
        scales = tuple((self.widths() if axis == "space" else DURATIONS)[v] for v in levels)
        n_other = N_TIME if axis == "space" else self.space_levels + 1
        slopes = np.full((len(qs), n_other), np.nan)
        intercepts, residuals = slopes.copy(), slopes.copy()
        if len(levels) >= 2:
            x = np.log(np.array(scales, dtype=np.float64))
            xc = x - x.mean()
            for k, q in enumerate(qs):
                m = self.moment(q)
                m = m[list(levels), :] if axis == "space" else m[:, list(levels)].T           # (levels, other)
                with np.errstate(divide="ignore", invalid="ignore"):
                    y = np.where(m > 0, np.log(m), np.nan)
                slope = (xc[:, None] * y).sum(axis=0) / (xc * xc).sum()
                icpt = y.mean(axis=0) - slope * x.mean()
                slopes[k], intercepts[k] = slope, icpt
                if len(levels) > 2:
                    residuals[k] = np.sqrt(np.mean(np.square(y - (icpt[None, :] + slope[None, :] * x[:, None])), axis=0))
        return ScalingFit(axis=axis, qs=qs, levels=levels, scales=scales, slopes=slopes, intercepts=intercepts, residuals=residuals)

    def box_dimension(self, axis="space", levels=None):
        """The box-counting dimension of the wet set: the wet boxes of side s number n_boxes M_0 ~ s^(slope - d), d = 2 over space and 1
        over time, so the dimension is d minus the slope of the q = 0 moment.  -> (dimension, residuals), (5,) for "space", (A + 1,)
        for "time"; a field that is wet everywhere has 2 and 1, NaN without a wet box at a level."""
        fit = self.exponents((0.0,), axis, levels)
        return (2.0 if axis == "space" else 1.0) - fit.slopes[0], fit.residuals[0]

    def quantiles(self, p):
        """(len(p), A + 1, 5): the p-quantiles of the box-mean intensity per scale, mm/h, from the histogram: the value (bin_values)
        of the first bin at which the cumulated count reaches p n_boxes.  NaN without a valid box-window."""
        try:
            p = np.array([float(v) for v in p], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("quantiles: expected a list of numbers") from None
        if not np.all((p >= 0) & (p <= 1)):
            raise ValueError(f"quantiles: every p must lie in 0 .. 1, got {tuple(p)}")
        cum = self.hist.cumsum(axis=2)
        need = np.maximum(np.ceil(p[:, None, None] * self.n_boxes[None]), 1)
        first = (cum[None] < need[..., None]).sum(axis=-1).clip(max=N_BINS - 1)
        values = bin_values()[first] / self._cells()[None]
        return np.where(self.n_boxes[None] > 0, values, np.nan)


def _check_orders(qs):
    try:
        qs = tuple(float(q) for q in qs)
    except (TypeError, ValueError):
        raise ValueError("qs: expected a list of numbers") from None
    if not qs or not all(0.0 <= q < np.inf for q in qs):
        raise ValueError(f"qs: expected finite moment orders >= 0, got {qs}")
    return qs


def compare(a, b, qs=DEFAULT_ORDERS):
    """Two ScalingStats with the same space levels (real days against generated days) -> dict: the differences a - b of
    wet_fraction (A + 1, 5), of log moment(q) (Q, A + 1, 5) and of the exponents over space (Q, 5) and over time (Q, A + 1) with both
    sides' residuals, and the total-variation distance of the histograms (A + 1, 5)"""
    if not (isinstance(a, ScalingStats) and isinstance(b, ScalingStats)):
        raise ValueError("compare takes two ScalingStats")
    if a.space_levels != b.space_levels:
        raise ValueError(f"the two statistics have different space levels: {a.space_levels} and {b.space_levels}")
    qs = _check_orders(qs)
    with np.errstate(divide="ignore", invalid="ignore"):
        logm = np.stack([np.log(a.moment(q)) - np.log(b.moment(q)) for q in qs])
    out = dict(space_levels=a.space_levels, qs=qs, wet_fraction=a.wet_fraction() - b.wet_fraction(), log_moment=logm,
               tv_hist=_tv(_div(a.hist, a.n_boxes[:, :, None]), _div(b.hist, b.n_boxes[:, :, None])))
    for axis in ("space", "time"):
        fa, fb = a.exponents(qs, axis), b.exponents(qs, axis)
        out["exponents_" + axis] = fa.slopes - fb.slopes
        out["residuals_" + axis] = (fa.residuals, fb.residuals)
    return out


def stats_from_state(counts, space_levels):
    """the flat state (numpy) -> ScalingStats"""
    A = whole_number(space_levels, 0, MAX_SPACE_LEVELS, "space_levels")
    return ScalingStats(space_levels=A, **split_state(counts, A))


class ScalingStructure(HourlyAccumulator):
    """The state of a scaling evaluation on the device.  space_levels: the largest space level A, boxes of up to 2^A pixels a side,
    0 .. 6 and 2^A at most the smaller side of the plane (None: the largest that fits the first plane); device: where a numpy
    input goes (None: "cuda"; a tensor input fixes it).  state(): counts ((A + 1) 5 296 + 2,) int64.  The levels of a smaller A are
    the first levels of a larger one."""
    entry, workspace_entry = "rdgan_scaling_accumulate", "rdgan_scaling_workspace_bytes"

    def __init__(self, space_levels=None, device=None):
        self._requested = check_space_levels(space_levels)
        self.device = device
        self.reset()

    def reset(self):
        super().reset()
        self.space_levels = self._requested
        return self

    def add(self, hourly):
        """hourly (..., 24, ny, nx) float32 in mm/h: a CUDA tensor or a numpy array, admitted as HourlyAccumulator.add admits it.
        The plane shape is fixed by the first call.  Returns self."""
        return super().add(hourly)

    def _levels_for(self, ny, nx):
        if self.counts is not None or self._requested is not None:
            return self.space_levels
        return largest_space_levels(ny, nx)

    def _check_plane(self, ny, nx, what):
        if ny * nx > MAX_PLANE:
            raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
        A = self._levels_for(ny, nx)
        if (1 << A) > min(ny, nx):
            raise ValueError(f"{what}: boxes of {1 << A} pixels a side (space_levels {A}) do not fit the plane {(ny, nx)}")

    def _check_args(self, shape, n, out):
        self.space_levels = self._levels_for(shape[-2], shape[-1])
        return ()

    def _state_tensors(self, device):
        self.counts = torch.zeros(state_count(self.space_levels), dtype=torch.int64, device=device)

    def _workspace_args(self, n, ny, nx):
        return ny, nx, self.space_levels

    def _entry_args(self, ny, nx, out):
        return ny, nx, self.space_levels, _p(self.counts)

    def result(self):
        """-> ScalingStats"""
        return stats_from_state(self.state().cpu().numpy(), self.space_levels)


def scaling_structure(hourly, space_levels=None):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> ScalingStats"""
    return ScalingStructure(space_levels).add(hourly).result()


def scaling_structure_field(gen, daily, n_scenarios, space_levels=None, scenario_chunk=16, overlap=4, latent_mode="shared", seed=None,
                            latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their scaling structure without holding them:
    _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on a ScalingStructure.
    -> ScalingStats"""
    return evaluate_field(ScalingStructure(space_levels), gen, daily, n_scenarios, scenario_chunk, overlap, latent_mode, seed, latent,
                          chunk, norm_scale)
