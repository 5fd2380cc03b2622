"""Areal extremes of hourly fields (csrc/rdgan_areal.hip.h): depth-area-duration.  How much water falls on
an AREA in k hours: for every day of an hourly array the largest accumulation over any k consecutive hours and any w x w box of
pixels, for every window k and width w, and statistics of those maxima over the days -- their mean and maximum, the share of days
at or above given levels, the hour the wettest window starts, and the storm-centred areal reduction factor, the ratio of the
areal maximum to the pixel maximum of the same duration.  A generator whose peaks are too speckled gets the areal maxima too low
although every pixel-wise distribution is right; one whose peaks are too smooth gets them too high.

Everything is defined in integers: q = rint(x * 1024) in units of 2^-10 mm; a pixel-hour is bad when x is NaN, +-inf, negative or
>= 2048, and a (window, box) that holds a bad pixel-hour is left out; boxes lie wholly inside the plane.  Amax[day][k][w] is the
largest box sum, h* the smallest start hour that attains it.  An ArealExtremes accumulates, over any number of add() calls, the
integer state include/rdgan.h lists for rdgan_areal_accumulate; the array is read on the device and never copied to the host, and
the state does not depend on how the days were split into calls or on workspace_days.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, whole_number
from ._hourly import MAX_DEPTH, MAX_PLANE, NHOURS, UNIT, HourlyAccumulator, admit, check_out_tensor, div as _div, evaluate_field, tv as _tv
from .engine import require_gpu

MAX_WINDOWS = 8                                                              # RD_AR_MAXK
MAX_WIDTHS = 8                                                               # RD_AR_MAXW
MAX_WIDTH = 64                                                               # RD_AR_MAXWIDTH
MAX_LEVELS = 16                                                              # RD_AR_MAXL
MAX_LEVEL = float(MAX_DEPTH * NHOURS)                                        # mm: what a window can hold
N_ARF = 21                                                                   # RD_AR_NARF: arf_hist[0 .. 20]
N_FIXED = 52                                                                 # RD_AR_FIXED: words of a record besides level_count
MAX_PASS = 65535                                                             # RD_AR_MAXPASS: days of a pass
# offsets behind level_count[L + 1] in the record of one (k, w) (RD_AR_START ..)
_START, _ARF, _SUM_A, _SUM_A1, _SUM_ALL, _MAX_A, _NDAYS, _NVOID, _NDRY = 0, 24, 45, 46, 47, 48, 49, 50, 51
_DEFAULT_PASS_PIXELS = 1 << 22                                               # 480 MB of workspace at most by default
DEFAULT_LEVELS = (1.0, 2.0, 5.0, 10.0, 20.0, 50.0, 100.0)                    # mm, of raindisagg_gan_pretrained.areal_extremes_field


def _increasing_ints(values, n_max, hi, what):
    try:
        values = tuple(values)
    except TypeError:
        raise ValueError(f"{what}: expected a list of whole numbers") from None
    if not 1 <= len(values) <= n_max:
        raise ValueError(f"{what}: expected 1 .. {n_max} values, got {len(values)}")
    values = tuple(whole_number(v, 1, hi, f"every value of {what}") for v in values)
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError(f"{what} must be strictly increasing, got {values}")
    return np.array(values, dtype=np.int32)


def check_windows(windows):
    """-> int32 array: 1 .. 8 durations in hours, strictly increasing in 1 .. 24"""
    return _increasing_ints(windows, MAX_WINDOWS, NHOURS, "windows")


def check_widths(widths):
    """-> int32 array: 1 .. 8 box widths in pixels, strictly increasing in 1 .. 64"""
    return _increasing_ints(widths, MAX_WIDTHS, MAX_WIDTH, "widths")


def check_levels(levels):
    """-> float64 array: 0 .. 16 depths in mm, finite, strictly increasing in [0, 2048 * 24]"""
    try:
        lv = np.array([float(v) for v in levels], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("levels: expected a list of numbers") from None
    if lv.size > MAX_LEVELS:
        raise ValueError(f"levels: at most {MAX_LEVELS} values, got {lv.size}")
    if not (np.all(np.isfinite(lv)) and np.all(lv >= 0) and np.all(lv <= MAX_LEVEL) and np.all(np.diff(lv) > 0)):
        raise ValueError(f"levels must be finite, strictly increasing and lie in 0 .. {MAX_LEVEL} mm, got {tuple(lv)}")
    return lv


def check_workspace_days(workspace_days):
    return None if workspace_days is None else whole_number(workspace_days, 1, MAX_PASS, "workspace_days, unless None,")


def state_count(n_windows, n_widths, n_levels):
    return n_windows * n_widths * (n_levels + 1 + N_FIXED) + 2


def split_state(counts, n_windows, n_widths, n_levels):
    """the flat state of rdgan_areal_accumulate (numpy) -> dict of named int64 arrays, (K, W, ...) each"""
    K, Wn, L = n_windows, n_widths, n_levels
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (state_count(K, Wn, L),):
        raise ValueError(f"expected {state_count(K, Wn, L)} counts, got {c.shape}")
    per = c[:-2].reshape(K, Wn, L + 1 + N_FIXED)
    fixed = per[:, :, L + 1:]
    word = lambda i: fixed[:, :, i].copy()
    return dict(level_count=per[:, :, :L + 1].copy(), start_hour=fixed[:, :, _START:_ARF].copy(), arf_hist=fixed[:, :, _ARF:_SUM_A].copy(),
                sum_A=word(_SUM_A), sum_A1=word(_SUM_A1), sum_A_all=word(_SUM_ALL), max_A=word(_MAX_A), n_days=word(_NDAYS),
                n_void=word(_NVOID), n_dry=word(_NDRY), n_days_total=int(c[-2]), n_bad=int(c[-1]))


@dataclass
class ArealStats:
    """What ArealExtremes.result returns, numpy on the host, int64; K windows, W widths, L levels.  level_count (K, W, L + 1): days
    by the number of levels the day's maximum reaches; start_hour (K, W, 24); arf_hist (K, W, 21): days by floor(20 ARF), the last
    bin ARF >= 1; sum_A, sum_A1, sum_A_all, max_A, n_days, n_void, n_dry (K, W), depths in 1/1024 mm.  n_days_total and n_bad
    (bad pixel-hours) once."""
    windows: tuple
    widths: tuple
    levels: tuple
    n_days_total: int
    n_bad: int
    level_count: np.ndarray
    start_hour: np.ndarray
    arf_hist: np.ndarray
    sum_A: np.ndarray
    sum_A1: np.ndarray
    sum_A_all: np.ndarray
    max_A: np.ndarray
    n_days: np.ndarray
    n_void: np.ndarray
    n_dry: np.ndarray

    def _area(self):
        return np.asarray(self.widths, dtype=np.int64)[None, :] ** 2

    def mean_depth(self):
        """(K, W): the mean over the counted days of the largest areal-mean accumulation, mm; NaN without a counted day"""
        return _div(self.sum_A_all, self.n_days * self._area() * UNIT)

    def max_depth(self):
        """(K, W): the largest areal-mean accumulation of any day, mm; NaN without a counted day"""
        return np.where(self.n_days > 0, self.max_A / (self._area() * float(UNIT)), np.nan)

    def exceedance(self):
        """(K, W, L): the share of counted days whose largest areal-mean accumulation is at or above each level"""
        above = self.level_count[:, :, ::-1].cumsum(axis=2)[:, :, ::-1][:, :, 1:]          # days that reach at least l + 1 levels
        return _div(above, self.n_days[:, :, None])

    def start_hour_distribution(self):
        """(K, W, 24): the share of counted days whose wettest window starts in hour h"""
        return _div(self.start_hour, self.start_hour.sum(axis=2, keepdims=True))

    def arf(self):
        """(K, W): the pooled storm-centred areal reduction factor, the areal maxima over the pixel maxima of the same duration,
        over the days with rain; NaN without one"""
        return _div(self.sum_A, self._area() * self.sum_A1)

    def arf_distribution(self):
        """(K, W, 21): the share of days with rain by floor(20 ARF) of the day, the last bin ARF >= 1"""
        return _div(self.arf_hist, self.arf_hist.sum(axis=2, keepdims=True))


def compare(a, b):
    """Two ArealStats with the same windows, widths and levels (real days against generated days) -> dict: the differences a - b
    of mean_depth and arf (K, W) and of exceedance (K, W, L), and the total-variation distances of the start-hour and ARF
    distributions (tv_start_hour, tv_arf, each (K, W))"""
    if not (isinstance(a, ArealStats) and isinstance(b, ArealStats)):
        raise ValueError("compare takes two ArealStats")
    for name in ("windows", "widths", "levels"):
        if tuple(getattr(a, name)) != tuple(getattr(b, name)):
            raise ValueError(f"the two statistics have different {name}: {getattr(a, name)} and {getattr(b, name)}")
    return dict(windows=tuple(a.windows), widths=tuple(a.widths), levels=tuple(a.levels),
                mean_depth=a.mean_depth() - b.mean_depth(), exceedance=a.exceedance() - b.exceedance(), arf=a.arf() - b.arf(),
                tv_start_hour=_tv(a.start_hour_distribution(), b.start_hour_distribution()),
                tv_arf=_tv(a.arf_distribution(), b.arf_distribution()))


def stats_from_state(counts, windows, widths, levels):
    """the flat state (numpy) -> ArealStats"""
    k, w, lv = check_windows(windows), check_widths(widths), check_levels(levels)
    return ArealStats(windows=tuple(int(v) for v in k), widths=tuple(int(v) for v in w), levels=tuple(float(v) for v in lv),
                      **split_state(counts, len(k), len(w), len(lv)))


class ArealExtremes(HourlyAccumulator):
    """The state of an areal-extremes evaluation on the device.  windows: the durations k in hours; widths: the box widths w in
    pixels, each at most the smaller side of the plane; levels: depths in mm of areal-mean accumulation whose exceedance is counted
    (may be empty); device: where a numpy input goes (None: "cuda"; a tensor input fixes it); workspace_days: how many days the
    workspace holds at a time, 120 bytes per pixel -- None: up to 2^22 pixels, 480 MB (one day if a day is larger).  The result does
    not depend on it.  state(): counts (K W (L + 53) + 2,) int64."""
    entry, workspace_entry, out_name = "rdgan_areal_accumulate", "rdgan_areal_workspace_bytes", "depths_out"

    def __init__(self, windows, widths, levels=(), device=None, workspace_days=None):
        self.windows, self.widths, self.levels = check_windows(windows), check_widths(widths), check_levels(levels)
        self.device = device
        self.workspace_days = check_workspace_days(workspace_days)
        self.reset()

    def add(self, hourly, depths_out=None):
        """hourly (..., 24, ny, nx) float32 in mm/h: a CUDA tensor or a numpy array, admitted as HourlyAccumulator.add admits
        it.  The plane shape is fixed by the first call.  depths_out: None, or a contiguous int64 CUDA tensor (n, K, W), n the
        days of hourly, that receives the day's maxima in 1/1024 mm, -1 for a day with no admissible box.  Returns self."""
        return super().add(hourly, depths_out)

    def _state_tensors(self, device):
        self.counts = torch.zeros(state_count(len(self.windows), len(self.widths), len(self.levels)), dtype=torch.int64, device=device)

    def _check_plane(self, ny, nx, what):
        if ny * nx > MAX_PLANE:
            raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
        if int(self.widths[-1]) > min(ny, nx):
            raise ValueError(f"{what}: the width {int(self.widths[-1])} is larger than the plane {(ny, nx)}; boxes are never clipped")

    def _check_args(self, shape, n, depths_out):
        check_out_tensor(depths_out, self.out_name, torch.int64, (n, len(self.windows), len(self.widths)))
        return ()

    def _pass_units(self, n, ny, nx):
        per_pass = self.workspace_days or max(1, _DEFAULT_PASS_PIXELS // (ny * nx))
        return min(per_pass, n, MAX_PASS)

    def _entry_args(self, ny, nx, depths_out):
        return (ny, nx, _hp(self.windows), len(self.windows), _hp(self.widths), len(self.widths), _hp(self.levels), len(self.levels),
                _p(self.counts), _p(depths_out))

    def result(self):
        """-> ArealStats"""
        return stats_from_state(self.state().cpu().numpy(), self.windows, self.widths, self.levels)


def areal_extremes(hourly, windows, widths, levels=(), return_depths=False, workspace_days=None):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> ArealStats, or (ArealStats, depths) with return_depths:
    depths an int64 CUDA tensor (n, K, W) of the days' maxima in 1/1024 mm (-1: no admissible box), for return levels across days
    or members"""
    ae = ArealExtremes(windows, widths, levels, workspace_days=workspace_days)
    if not return_depths:
        return ae.add(hourly).result()
    hourly, from_host, shape, n, _ = admit(hourly)
    ae._check_plane(shape[-2], shape[-1], "hourly")
    require_gpu()
    depths = torch.empty((n, len(ae.windows), len(ae.widths)), dtype=torch.int64, device="cuda" if from_host else hourly.device)
    return ae.add(hourly, depths_out=depths).result(), depths


def areal_extremes_field(gen, daily, n_scenarios, windows, widths, levels=(), workspace_days=None, scenario_chunk=16, overlap=4,
                         latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their areal extremes without holding them:
    _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on an ArealExtremes.  -> ArealStats"""
    return evaluate_field(ArealExtremes(windows, widths, levels, workspace_days=workspace_days), gen, daily, n_scenarios, scenario_chunk,
                          overlap, latent_mode, seed, latent, chunk, norm_scale)
