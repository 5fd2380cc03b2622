"""Storms of hourly fields (csrc/rdgan_storms.hip.h): follow a rain area through the day.  Threshold the
24 hours of a day, link the wet pixels of an hour as cells.py does and the wet pixels of consecutive hours that lie within `reach`
pixels of each other, and take the connected wet volumes ("storms"): how long a rain system lives, when it starts, and how much of
the day's water falls in long-lived systems and how much in one-hour flecks -- the diagnostic that sees cells that are born and
die every hour although every single hour and every single pixel looks right.

A voxel (h, y, x) of a day is wet at threshold t when x > thr[t] in fp32, bad when it is NaN or +-inf (never wet); its day-local
index is v = h ny nx + y nx + x.  A storm is a maximal set of wet voxels of one day connected by links; days never link.  Its
class is c = space_edge + 2 time_edge: space_edge when the rim of the plane or a bad pixel cuts it off (the edge flag of cells.py),
time_edge when it is wet in hour 0 or hour 23, so that the day censors its duration.  A StormStructure accumulates, over any number
of add() calls, the integer state include/rdgan.h lists for rdgan_storms_accumulate; the array is read on the device and never
copied to the host, and the state does not depend on how the days were split into calls or on days_per_pass.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, whole_number
from ._hourly import MAX_PLANE, NHOURS, admit, div as _div, evaluate_field, tv as _tv
from .cells import VOLUME_UNIT, LabelAccumulator, check_connectivity
from .engine import require_gpu
from .verification import check_event_thresholds

N_COUNTS = 622                                                               # RD_SM_NC: counters per threshold
N_CLASSES = 4                                                                # RD_SM_NCLASS: space_edge + 2 time_edge
N_BINS = 28                                                                  # RD_SM_NBINS: floor(log2(size)) = 0 .. 27
N_SPD = 65                                                                   # RD_SM_NSPD: storms_per_day[0 .. 64], the last bin open
N_LONGEST = 25                                                               # RD_SM_NLONG: longest_duration[0 .. 24]
MAX_DAY = 1 << 27                                                            # RD_SM_MAXDAY: voxels of a day
MAX_PASS = 2730                                                              # RD_SM_MAXPASS: days of a pass
MAX_REACH = 4                                                                # RD_SM_MAXREACH
# offsets of a threshold's counters (RD_SM_WET ..)
_WET, _STORMS, _DUR, _START, _HIST, _SSUM, _SSQ, _SBD, _VBD, _SPD, _LONGEST = 0, 24, 28, 124, 220, 332, 336, 340, 436, 532, 597
_DEFAULT_PASS_VOXELS = 1 << 24                                               # 384 MB of workspace at most by default


def check_reach(reach):
    return whole_number(reach, 0, MAX_REACH, "reach")


def check_days_per_pass(days_per_pass):
    return None if days_per_pass is None else whole_number(days_per_pass, 1, MAX_PASS, "days_per_pass, unless None,")


def split_state(counts, n_thresholds):
    """the flat state of rdgan_storms_accumulate (numpy) -> dict of named int64 arrays"""
    T = n_thresholds
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (T * N_COUNTS + 2,):
        raise ValueError(f"expected {T * N_COUNTS + 2} counts, got {c.shape}")
    per = c[:T * N_COUNTS].reshape(T, N_COUNTS)
    by_hour = lambda lo, hi: per[:, lo:hi].reshape(T, N_CLASSES, NHOURS).copy()
    return dict(wet_pixels=per[:, _WET:_STORMS].copy(), storms=per[:, _STORMS:_DUR].copy(), duration_hist=by_hour(_DUR, _START),
                start_hour=by_hour(_START, _HIST), size_hist=per[:, _HIST:_SSUM].reshape(T, N_CLASSES, N_BINS).copy(),
                size_sum=per[:, _SSUM:_SSQ].copy(), size_sq_sum=per[:, _SSQ:_SBD].copy(), size_by_duration=by_hour(_SBD, _VBD),
                volume_by_duration=by_hour(_VBD, _SPD), storms_per_day=per[:, _SPD:_LONGEST].copy(),
                longest_duration=per[:, _LONGEST:].copy(), n_days=int(c[-2]), n_bad_pixels=int(c[-1]))


@dataclass
class StormStats:
    """What StormStructure.result returns, numpy on the host, int64; T thresholds, class c = space_edge + 2 time_edge, durations
    d = 1 .. 24 at index d - 1, size bin b = floor(log2(size)).  wet_pixels (T, 24); storms, size_sum, size_sq_sum (T, 4);
    duration_hist, start_hour, size_by_duration, volume_by_duration (T, 4, 24); size_hist (T, 4, 28); storms_per_day (T, 65), the
    last bin open; longest_duration (T, 25), index 0 the days without a wet voxel.  n_pixels is the size of a plane."""
    thresholds: tuple
    connectivity: int
    reach: int
    n_pixels: int
    n_days: int
    n_bad_pixels: int
    wet_pixels: np.ndarray
    storms: np.ndarray
    duration_hist: np.ndarray
    start_hour: np.ndarray
    size_hist: np.ndarray
    size_sum: np.ndarray
    size_sq_sum: np.ndarray
    size_by_duration: np.ndarray
    volume_by_duration: np.ndarray
    storms_per_day: np.ndarray
    longest_duration: np.ndarray

    def _by_class(self, a, complete_only):
        return a[:, 0] if complete_only else a.sum(axis=1)

    def duration_distribution(self, complete_only=False):
        """(T, 24): the share of storms that last d hours; complete_only keeps class 0, the storms neither the rim, a bad pixel
        nor the day cuts off"""
        h = self._by_class(self.duration_hist, complete_only)
        return _div(h, h.sum(axis=1, keepdims=True))

    def mean_duration(self, complete_only=False):
        """(T,): hours per storm, NaN without a storm"""
        h = self._by_class(self.duration_hist, complete_only)
        return _div((h * np.arange(1, NHOURS + 1)).sum(axis=1), h.sum(axis=1))

    def start_hour_distribution(self, complete_only=False):
        """(T, 24): the share of storms that start in hour h (the storms wet in hour 0 may have started the day before)"""
        h = self._by_class(self.start_hour, complete_only)
        return _div(h, h.sum(axis=1, keepdims=True))

    def size_distribution(self, complete_only=False):
        """(T, 28): the share of storms with floor(log2(size)) = b, size in pixel-hours"""
        h = self._by_class(self.size_hist, complete_only)
        return _div(h, h.sum(axis=1, keepdims=True))

    def mean_size(self, complete_only=False):
        """(T,): pixel-hours per storm, NaN without a storm"""
        return _div(self._by_class(self.size_sum, complete_only), self._by_class(self.storms, complete_only))

    def size_weighted_mean_duration(self, complete_only=False):
        """(T,): the duration of the storm a wet voxel lies in, averaged over the wet voxels"""
        s = self._by_class(self.size_by_duration, complete_only)
        return _div((s * np.arange(1, NHOURS + 1)).sum(axis=1), s.sum(axis=1))

    def volume_share_by_duration(self):
        """(T, 24): the share of the water above the threshold that falls in storms of duration d; NaN without a wet voxel"""
        v = self.volume_by_duration.sum(axis=1)
        return _div(v, v.sum(axis=1, keepdims=True))

    def mean_intensity_by_duration(self, complete_only=False):
        """(T, 24): the mean amount per pixel-hour, in the unit of the data, of the storms of duration d: volume_by_duration over
        size_by_duration; NaN for a duration without a storm"""
        return _div(self._by_class(self.volume_by_duration, complete_only) * VOLUME_UNIT, self._by_class(self.size_by_duration, complete_only))

    def mean_storms_per_day(self):
        """(T,): NaN without a day"""
        return _div(self.storms.sum(axis=1), self.n_days)

    def storms_per_day_distribution(self):
        """(T, 65): the share of days with k storms, the last bin 64 or more"""
        return _div(self.storms_per_day, self.storms_per_day.sum(axis=1, keepdims=True))

    def longest_duration_distribution(self):
        """(T, 25): the share of days whose longest storm lasts k hours, k = 0 the days without a wet voxel"""
        return _div(self.longest_duration, self.longest_duration.sum(axis=1, keepdims=True))

    def one_hour_fraction(self):
        """(T,): the share of wet voxels that lie in storms of a single hour"""
        return _div(self.size_by_duration[:, :, 0].sum(axis=1), self.size_sum.sum(axis=1))


def compare(a, b):
    """Two StormStats with the same thresholds, connectivity and reach (real days against generated days) -> dict, per threshold:
    the total-variation distances of the duration, start-hour, size and longest-duration distributions (tv_duration,
    tv_duration_complete, tv_start_hour, tv_size, tv_longest_duration, each (T,)); and the differences a - b of mean duration, mean
    storms per day and one-hour fraction (T,), and of the volume share by duration (T, 24)"""
    if not (isinstance(a, StormStats) and isinstance(b, StormStats)):
        raise ValueError("compare takes two StormStats")
    if tuple(a.thresholds) != tuple(b.thresholds):
        raise ValueError(f"the two statistics have different thresholds: {a.thresholds} and {b.thresholds}")
    if (a.connectivity, a.reach) != (b.connectivity, b.reach):
        raise ValueError(f"the two statistics have different links: connectivity {a.connectivity} and {b.connectivity}, "
                         f"reach {a.reach} and {b.reach}")
    return dict(thresholds=tuple(a.thresholds),
                tv_duration=_tv(a.duration_distribution(), b.duration_distribution()),
                tv_duration_complete=_tv(a.duration_distribution(True), b.duration_distribution(True)),
                tv_start_hour=_tv(a.start_hour_distribution(), b.start_hour_distribution()),
                tv_size=_tv(a.size_distribution(), b.size_distribution()),
                tv_longest_duration=_tv(a.longest_duration_distribution(), b.longest_duration_distribution()),
                mean_duration=a.mean_duration() - b.mean_duration(),
                mean_storms_per_day=a.mean_storms_per_day() - b.mean_storms_per_day(),
                one_hour_fraction=a.one_hour_fraction() - b.one_hour_fraction(),
                volume_share_by_duration=a.volume_share_by_duration() - b.volume_share_by_duration())


def stats_from_state(counts, thresholds, connectivity, reach, n_pixels):
    """the flat state (numpy) -> StormStats"""
    thr = check_event_thresholds(thresholds)
    return StormStats(thresholds=tuple(float(t) for t in thr), connectivity=check_connectivity(connectivity), reach=check_reach(reach),
                      n_pixels=int(n_pixels), **split_state(counts, len(thr)))


class StormStructure(LabelAccumulator):
    """The state of a storm evaluation on the device.  thresholds: the wet-voxel events in the unit of the data; connectivity: 4
    (edges) or 8 (edges and corners) inside an hour; reach: how many pixels (Chebyshev) rain may move from one hour to the next
    and stay the same storm, 0 .. 4; days_per_pass: how many days the workspace holds at a time, 24 bytes per voxel -- None: up to
    2^24 voxels, 384 MB (one day if a day is larger).  The result does not depend on it.  add() writes the labels as day-local
    voxel indices, -1 where dry; state(): counts (T * 622 + 2,) int64."""
    entry, workspace_entry, n_counts = "rdgan_storms_accumulate", "rdgan_storms_workspace_bytes", N_COUNTS

    def __init__(self, thresholds, connectivity=8, reach=1, days_per_pass=None):
        self.thr = check_event_thresholds(thresholds)
        self.connectivity = check_connectivity(connectivity)
        self.reach = check_reach(reach)
        self.days_per_pass = check_days_per_pass(days_per_pass)
        self.reset()

    def _check_plane(self, ny, nx, what):
        if ny * nx > MAX_PLANE or NHOURS * ny * nx > MAX_DAY:
            raise ValueError(f"{what}: a day has {NHOURS * ny * nx} voxels, the limit is {MAX_DAY}")

    def _pass_units(self, n, ny, nx):
        per_pass = self.days_per_pass or max(1, _DEFAULT_PASS_VOXELS // (NHOURS * ny * nx))
        return min(per_pass, n, MAX_PASS)

    def _entry_args(self, ny, nx, labels_out, label_threshold):
        return ny, nx, _hp(self.thr), len(self.thr), self.connectivity, self.reach, _p(self.counts), _p(labels_out), label_threshold

    def result(self):
        """-> StormStats"""
        return stats_from_state(self.state().cpu().numpy(), self.thr, self.connectivity, self.reach,
                                self.plane_shape[0] * self.plane_shape[1])


def storm_structure(hourly, thresholds, connectivity=8, reach=1, days_per_pass=None):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> StormStats"""
    return StormStructure(thresholds, connectivity, reach, days_per_pass).add(hourly).result()


def label_storms(hourly, threshold, connectivity=8, reach=1):
    """The canonical labels of the storms of hourly (..., 24, ny, nx; a float32 CUDA tensor or numpy) at one threshold: an int32
    CUDA tensor of the same shape, every voxel of a storm holding the smallest day-local index h ny nx + y nx + x of the storm, -1
    elsewhere"""
    ss = StormStructure((threshold,), connectivity, reach)
    hourly, from_host, shape, _, _ = admit(hourly)
    ss._check_plane(shape[-2], shape[-1], "hourly")
    require_gpu()
    labels = torch.empty(shape, dtype=torch.int32, device="cuda" if from_host else hourly.device)
    ss.add(hourly, labels_out=labels)
    return labels


def storm_structure_field(gen, daily, n_scenarios, thresholds, connectivity=8, reach=1, days_per_pass=None, scenario_chunk=16,
                          overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their storms without holding them:
    _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on a StormStructure.  -> StormStats"""
    return evaluate_field(StormStructure(thresholds, connectivity, reach, days_per_pass), gen, daily, n_scenarios, scenario_chunk,
                          overlap, latent_mode, seed, latent, chunk, norm_scale)
