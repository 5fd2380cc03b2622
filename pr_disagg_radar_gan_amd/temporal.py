"""Temporal structure of hourly fields (csrc/rdgan_temporal.hip.h): how long the wet spells are, how often a
wet hour follows a dry one, how many hours of a day are wet, how persistent the intensities are from hour to hour -- the one thing
a temporal disaggregation adds, and the one thing no other evaluation here looks at.

A series is the 24 hours of one pixel of one day, cut at the day boundary; hour h is wet for threshold t when x[h] > thr[t] in
fp32.  A TemporalStructure accumulates, over any number of add() calls, the counts and fp64 sums include/rdgan.h lists for
rdgan_temporal_accumulate; the array is read once and never copied to the host.  The counts do not depend on how the series were
split into calls; the sums agree bit for bit between identical sequences of calls.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, whole_number
from ._hourly import NHOURS, HourlyAccumulator, div as _div, evaluate_field, tensor_layout, tv as _tv    # noqa: F401 (tensor_layout is public here)
from .verification import check_event_thresholds

MAX_LAG = 12                                                                 # RD_TS_MAXK
N_COUNTS = 286                                                               # RD_TS_NC: counters per threshold
THREADS, MAX_BLOCKS = 256, 1024                                              # RD_TS_THREADS, RD_TS_MAXBLOCKS
# offsets of a threshold's counters (RD_TS_WH ..)
_WH, _LW, _WS, _DS, _FW, _LAST, _TR = 0, 25, 50, 98, 146, 170, 194


def check_max_lag(max_lag):
    return whole_number(max_lag, 1, MAX_LAG, "max_lag")


def n_sums(n_thresholds, max_lag):
    return 2 * NHOURS + max_lag + NHOURS * n_thresholds


def split_state(counts, sums, n_thresholds, max_lag):
    """the flat state of rdgan_temporal_accumulate (numpy) -> dict of named arrays"""
    T, K = n_thresholds, max_lag
    c = np.asarray(counts, dtype=np.int64)
    s = np.asarray(sums, dtype=np.float64)
    if c.shape != (T * N_COUNTS + 2,) or s.shape != (n_sums(T, K),):
        raise ValueError(f"expected {T * N_COUNTS + 2} counts and {n_sums(T, K)} sums, got {c.shape} and {s.shape}")
    per = c[:T * N_COUNTS].reshape(T, N_COUNTS)
    return dict(wet_hours=per[:, _WH:_LW].copy(), longest_wet=per[:, _LW:_WS].copy(),
                wet_spell=per[:, _WS:_DS].reshape(T, 2, NHOURS).copy(), dry_spell=per[:, _DS:_FW].reshape(T, 2, NHOURS).copy(),
                first_wet=per[:, _FW:_LAST].copy(), last_wet=per[:, _LAST:_TR].copy(),
                trans=per[:, _TR:].reshape(T, NHOURS - 1, 2, 2).copy(), n_valid=int(c[-2]), n_bad=int(c[-1]),
                moments=s[:2 * NHOURS].reshape(NHOURS, 2).copy(), lag=s[2 * NHOURS:2 * NHOURS + K].copy(),
                wet_amount=s[2 * NHOURS + K:].reshape(T, NHOURS).copy())


@dataclass
class TemporalStats:
    """What TemporalStructure.result returns, numpy on the host; T thresholds, K lags.  wet_hours, longest_wet (T, 25); wet_spell,
    dry_spell (T, 2, 24) = [edge class][L - 1]; first_wet, last_wet (T, 24); trans (T, 23, 2, 2) = [h][wet(h)][wet(h + 1)], int64;
    moments (24, 2) = (sum x[h], sum x[h]^2), lag (K,), wet_amount (T, 24), float64; all over the n_valid good series."""
    thresholds: tuple
    max_lag: int
    n_valid: int
    n_bad: int
    wet_hours: np.ndarray
    longest_wet: np.ndarray
    wet_spell: np.ndarray
    dry_spell: np.ndarray
    first_wet: np.ndarray
    last_wet: np.ndarray
    trans: np.ndarray
    moments: np.ndarray
    lag: np.ndarray
    wet_amount: np.ndarray

    def _wet_by_hour(self):
        """(T, 24) series with hour h wet: from the transitions, hour 23 from the pairs that end there"""
        first = self.trans[:, :, 1, :].sum(axis=-1)                          # wet(h), h = 0 .. 22
        return np.concatenate([first, self.trans[:, -1:, :, 1].sum(axis=-1)], axis=1)

    def wet_fraction(self, by_hour=False):
        """the share of wet hours, (T,) -- or (T, 24) by hour of day; NaN without a valid series"""
        if by_hour:
            return _div(self._wet_by_hour(), self.n_valid)
        k = np.arange(NHOURS + 1)
        return _div((self.wet_hours * k).sum(axis=1), NHOURS * self.n_valid)

    def wet_hours_distribution(self):
        """(T, 25): the share of series with k wet hours"""
        return _div(self.wet_hours, self.wet_hours.sum(axis=1, keepdims=True))

    def _spells(self, kind, interior_only=False):
        if kind not in ("wet", "dry"):
            raise ValueError(f"kind must be 'wet' or 'dry', got {kind!r}")
        s = self.wet_spell if kind == "wet" else self.dry_spell
        return s[:, 0] if interior_only else s.sum(axis=1)

    def spell_lengths(self, kind="wet", interior_only=False):
        """(T, 24): the share of runs of length L = 1 .. 24; interior_only leaves out the runs the day boundary cuts off"""
        s = self._spells(kind, interior_only)
        return _div(s, s.sum(axis=1, keepdims=True))

    def mean_spell_length(self, kind="wet"):
        """(T,): the mean run length in hours, NaN without a run"""
        s = self._spells(kind)
        return _div((s * np.arange(1, NHOURS + 1)).sum(axis=1), s.sum(axis=1))

    def transition_probabilities(self):
        """(p01, p11), each (T, 23): P(wet(h + 1) | dry(h)) and P(wet(h + 1) | wet(h)), NaN where the denominator is 0"""
        t = self.trans
        return _div(t[:, :, 0, 1], t[:, :, 0].sum(axis=-1)), _div(t[:, :, 1, 1], t[:, :, 1].sum(axis=-1))

    def onset_distribution(self):
        """(T, 24): the share of wet days whose first wet hour is h"""
        return _div(self.first_wet, self.first_wet.sum(axis=1, keepdims=True))

    def autocorrelation(self):
        """(K,): the pooled lag-k Pearson correlation of x[h] with x[h + k] over all pairs inside a day"""
        s1, s2 = self.moments[:, 0], self.moments[:, 1]
        out = np.full(self.max_lag, np.nan)
        for k in range(1, self.max_lag + 1):
            n = float(self.n_valid) * (NHOURS - k)
            if n <= 0:
                continue
            ma, mb = s1[:NHOURS - k].sum() / n, s1[k:].sum() / n
            va, vb = s2[:NHOURS - k].sum() / n - ma * ma, s2[k:].sum() / n - mb * mb
            if va > 0 and vb > 0:
                out[k - 1] = (self.lag[k - 1] / n - ma * mb) / np.sqrt(va * vb)
        return out

    def wet_intensity_cycle(self):
        """(T, 24): the mean amount of a wet hour by hour of day, NaN where the hour is never wet"""
        return _div(self.wet_amount, self._wet_by_hour())


def compare(a, b):
    """Two TemporalStats with the same thresholds (real days against generated days) -> dict, per threshold: the total-variation
    distance of the wet-hours, wet-spell and dry-spell distributions (tv_wet_hours, tv_wet_spell, tv_dry_spell, each (T,)); the
    differences a - b of wet fraction (T,), p01 and p11 (T, 23); and of the autocorrelations (K,) with K the smaller max_lag"""
    if not (isinstance(a, TemporalStats) and isinstance(b, TemporalStats)):
        raise ValueError("compare takes two TemporalStats")
    if tuple(a.thresholds) != tuple(b.thresholds):
        raise ValueError(f"the two statistics have different thresholds: {a.thresholds} and {b.thresholds}")
    K = min(a.max_lag, b.max_lag)
    pa, pb = a.transition_probabilities(), b.transition_probabilities()
    return dict(thresholds=tuple(a.thresholds),
                tv_wet_hours=_tv(a.wet_hours_distribution(), b.wet_hours_distribution()),
                tv_wet_spell=_tv(a.spell_lengths("wet"), b.spell_lengths("wet")),
                tv_dry_spell=_tv(a.spell_lengths("dry"), b.spell_lengths("dry")),
                wet_fraction=a.wet_fraction() - b.wet_fraction(), p01=pa[0] - pb[0], p11=pa[1] - pb[1],
                autocorrelation=a.autocorrelation()[:K] - b.autocorrelation()[:K])


def stats_from_state(counts, sums, thresholds, max_lag):
    """the flat state (numpy) -> TemporalStats"""
    thr = check_event_thresholds(thresholds)
    d = split_state(counts, sums, len(thr), check_max_lag(max_lag))
    return TemporalStats(thresholds=tuple(float(t) for t in thr), max_lag=int(max_lag), **d)


class TemporalStructure(HourlyAccumulator):
    """The state of a temporal-structure evaluation on the device.  thresholds: the wet-hour events in the unit of the data;
    max_lag: the lags 1 .. max_lag of the lagged products.  add(hourly) is HourlyAccumulator's."""
    entry, workspace_entry = "rdgan_temporal_accumulate", "rdgan_temporal_workspace_bytes"

    def __init__(self, thresholds, max_lag=6):
        self.thr = check_event_thresholds(thresholds)
        self.max_lag = check_max_lag(max_lag)
        self.sums = None
        self.reset()

    def _state_tensors(self, device):
        T = len(self.thr)
        self.counts = torch.zeros(T * N_COUNTS + 2, dtype=torch.int64, device=device)
        self.sums = torch.zeros(n_sums(T, self.max_lag), dtype=torch.float64, device=self.counts.device)

    def _workspace_args(self, n, ny, nx):
        return n, ny * nx, len(self.thr), self.max_lag

    def _entry_args(self, ny, nx, out):
        return ny * nx, _hp(self.thr), len(self.thr), self.max_lag, _p(self.counts), _p(self.sums)

    def state(self):
        """(counts (T * 286 + 2,) int64, sums (48 + K + 24 T,) float64): the tensors themselves, on the device, in the flat order
        of include/rdgan.h"""
        return super().state(), self.sums

    def result(self):
        """-> TemporalStats"""
        counts, sums = self.state()
        return stats_from_state(counts.cpu().numpy(), sums.cpu().numpy(), self.thr, self.max_lag)


def temporal_structure(hourly, thresholds, max_lag=6):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> TemporalStats"""
    return TemporalStructure(thresholds, max_lag).add(hourly).result()


def temporal_structure_field(gen, daily, n_scenarios, thresholds, max_lag=6, scenario_chunk=16, overlap=4, latent_mode="shared",
                             seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their temporal structure without holding them:
    _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on a TemporalStructure.
    -> TemporalStats"""
    return evaluate_field(TemporalStructure(thresholds, max_lag), gen, daily, n_scenarios, scenario_chunk, overlap, latent_mode, seed,
                          latent, chunk, norm_scale)
