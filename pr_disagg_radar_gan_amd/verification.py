"""Verify field ensembles against the observed hours (csrc/rdgan_verify.hip.h): the rank histogram of the
observation among the members with ties broken at random, the Brier score with its reliability table and the skill against the
sample base rate, and the fractions skill score per threshold and neighbourhood width.

The ensemble is never held: an EnsembleVerifier accumulates, over any number of add() calls, per position p of ([D,] 24, ny, nx)

    exceed[t][p] = #{s : x_s[p] > thr[t]}    below[p] = #{s : x_s[p] < o[p]}    equal[p] = #{s : x_s[p] == o[p]}    (int32)
    bad[p] = 1 where o[p] or any member seen so far is NaN                                                           (uint8)

and result() reduces that state.  Every accumulated value is an integer, or an fp64 sum of integers, so the result does not depend
on how the members were split into calls.  It works on tiles as on fields: rainfarm.downscale_device and
ensemble.generate_ensemble_device members go straight into add().

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._hourly import MAX_MEMBERS, ObservedRequest, ObservedVerifier, admit_array, check_pair

MAX_THRESHOLDS, MAX_SCALES, MAX_BINS = 8, 8, 64                             # RD_VF_MAXT, RD_VF_MAXW, RD_VF_MAXBINS (MAX_MEMBERS: RD_VF_MAXS)
MAX_BOX_MEMBERS = 1 << 26                                                   # S * w_max^2 stays below this
DEFAULT_SCALES = (1, 3, 5, 9, 17)


def check_event_thresholds(thresholds):
    """-> the thresholds as a contiguous float64 array holding their fp32 roundings (what the kernels compare with): 1 .. 8
    values, finite, >= 0, strictly increasing after the rounding"""
    try:
        t = np.asarray(thresholds, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"thresholds must be a list of numbers, got {thresholds!r}") from None
    if t.ndim != 1 or not 1 <= t.shape[0] <= MAX_THRESHOLDS:
        raise ValueError(f"thresholds must be a list of 1 .. {MAX_THRESHOLDS} values, got {thresholds!r}")
    if not np.all(np.isfinite(t)) or np.any(np.abs(t) > np.finfo(np.float32).max):
        raise ValueError(f"every threshold must be finite in fp32, got {thresholds!r}")
    t = t.astype(np.float32).astype(np.float64)
    if np.any(t < 0):
        raise ValueError(f"every threshold must be >= 0, got {thresholds!r}")
    if np.any(np.diff(t) <= 0):
        raise ValueError(f"thresholds must be strictly increasing in fp32, got {thresholds!r}")
    return np.ascontiguousarray(t)


def check_scales(scales, n_members=1):
    """-> the neighbourhood widths as a contiguous int32 array: 1 .. 8 odd whole numbers >= 1, strictly increasing, with
    n_members * w_max^2 < 2^26 (box sums stay exact integers)"""
    w = np.asarray(scales)
    if w.ndim != 1 or not 1 <= w.shape[0] <= MAX_SCALES:
        raise ValueError(f"scales must be a list of 1 .. {MAX_SCALES} widths, got {scales!r}")
    if not np.issubdtype(w.dtype, np.integer):
        if not (np.issubdtype(w.dtype, np.floating) and np.all(np.isfinite(w)) and np.all(w == np.round(w))):
            raise ValueError(f"scales must be whole numbers of pixels, got {scales!r}")
    if np.any(np.abs(w) > 8192):
        raise ValueError(f"every scale must lie in 1 .. 8191, got {scales!r}")
    w = w.astype(np.int64)
    if w.min() < 1 or np.any(w % 2 == 0):
        raise ValueError(f"every scale must be odd and >= 1, got {scales!r}")
    if np.any(np.diff(w) <= 0):
        raise ValueError(f"scales must be strictly increasing, got {scales!r}")
    if int(n_members) * int(w.max()) ** 2 >= MAX_BOX_MEMBERS:
        raise ValueError(f"n_members * max(scales)^2 must stay below 2^26, got {int(n_members)} * {int(w.max())}^2")
    return np.ascontiguousarray(w, dtype=np.int32)


def _check_bins(n_bins, n_members):
    """(a whole-valued float such as 11.0 counts as its integer)"""
    return whole_number(n_bins, 2, min(int(n_members) + 1, MAX_BINS), f"n_bins (at most n_members + 1 and {MAX_BINS})", whole_floats=True)


def _check_seed(seed):
    return whole_number(seed, 0, (1 << 64) - 1, "the rank seed")


@dataclass
class Verification:
    """What EnsembleVerifier.result returns, numpy on the host.  rank_hist (24, S + 1) int64; reliability (T, 24, n_bins, 3) int64 =
    (count, sum e, sum c); brier_sums (T, 24, 4) int64 = (N, sum e, sum c e, sum c^2); fss_sums (T, W, 24, 2) float64 = (num, den);
    c = the number of members above the threshold, e = 1 where the observation is."""
    thresholds: tuple
    scales: tuple
    n_members: int
    n_valid: int
    rank_hist: np.ndarray
    reliability: np.ndarray
    brier_sums: np.ndarray
    fss_sums: np.ndarray

    def rank_histogram(self, by_hour=False):
        """counts of the observation's rank among the members, (S + 1,) -- or (24, S + 1) by hour; flat for a calibrated ensemble"""
        return self.rank_hist.copy() if by_hour else self.rank_hist.sum(axis=0)

    def brier(self, by_hour=False):
        """(BS, base_rate, BSS), each (T,) -- or (T, 24): BS = mean (c / S - e)^2, base rate = mean e, BSS = 1 - BS / (base (1 -
        base)); NaN without a valid position, BSS NaN where the event never or always happens"""
        b = self.brier_sums.astype(np.float64)
        if not by_hour:
            b = b.sum(axis=1)
        n, se, sce, sc2 = (b[..., k] for k in range(4))
        S = float(self.n_members)
        with np.errstate(divide="ignore", invalid="ignore"):
            bs = (sc2 - 2.0 * S * sce + S * S * se) / (S * S * n)
            base = se / n
            ref = base * (1.0 - base)
            bss = np.where(ref > 0, 1.0 - bs / ref, np.nan)
        return bs, base, bss

    def reliability_curve(self, t):
        """(forecast, observed, count), each (n_bins,), for threshold index t over all hours: the mean forecast probability
        sum c / (S count) and the observed frequency sum e / count of each probability bin, NaN for an empty bin"""
        if not -len(self.thresholds) <= int(t) < len(self.thresholds):
            raise ValueError(f"t must index one of the {len(self.thresholds)} thresholds, got {t!r}")
        r = self.reliability[int(t)].sum(axis=0).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return r[:, 2] / (self.n_members * r[:, 0]), r[:, 1] / r[:, 0], self.reliability[int(t)].sum(axis=0)[:, 0]

    def fss(self, by_hour=False):
        """the fractions skill score 1 - num / den, (T, W) -- or (T, W, 24); NaN where neither forecast nor observation has an event"""
        f = self.fss_sums if by_hour else self.fss_sums.sum(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(f[..., 1] > 0, 1.0 - f[..., 0] / f[..., 1], np.nan)


class EnsembleVerifier(ObservedVerifier):
    """The state of a verification on the device.  obs (..., 24, ny, nx): a numpy array or a float32 CUDA tensor (used where it
    lies); thresholds: the events, in the unit of obs."""

    def __init__(self, obs, thresholds):
        self.thr = check_event_thresholds(thresholds)
        self._admit_obs(obs)
        dev = self.obs.device
        self.n_members = 0
        self.exceed = torch.zeros((len(self.thr),) + self.shape, dtype=torch.int32, device=dev)
        self.below = torch.zeros(self.shape, dtype=torch.int32, device=dev)
        self.equal = torch.zeros(self.shape, dtype=torch.int32, device=dev)
        self.bad = torch.isnan(self.obs).to(torch.uint8)

    def _check_members(self, s):
        if self.n_members + s > MAX_MEMBERS:
            raise ValueError(f"a verification holds at most {MAX_MEMBERS} members: {self.n_members} held, {s} more offered")

    def add(self, members):
        """members (s, *obs.shape) float32: a CUDA tensor, whose member axis may have any stride >= prod(obs.shape) (a view of a
        wider buffer, as member_stats_device accepts it), or a numpy array.  Returns self."""
        members, s, stride = self._admit_members(members)
        with torch.cuda.device(self.obs.device):
            rc = self.lib.rdgan_verify_accumulate(_p(members), s, stride, self.P, _p(self.obs), _hp(self.thr), len(self.thr),
                                                  _p(self.exceed), _p(self.below), _p(self.equal), _p(self.bad),
                                                  _stream(self.obs))
        _lib.check(rc, None, "rdgan_verify_accumulate")
        self.n_members += s
        return self

    def state(self):
        """(exceed (T, *shape) int32, below, equal (*shape) int32, bad (*shape) uint8): the tensors themselves, on the device"""
        return self.exceed, self.below, self.equal, self.bad

    def result(self, scales=DEFAULT_SCALES, n_bins=11, seed=0):
        """Reduce the state.  scales: the FSS neighbourhood widths in pixels; n_bins: the probability bins of the reliability table,
        bin = (c n_bins) // (S + 1); seed: of the hash that breaks rank ties.  -> Verification"""
        S = self.n_members
        if S < 1:
            raise ValueError("no member has been added")
        wd, n_bins, seed = check_scales(scales, S), _check_bins(n_bins, S), _check_seed(seed)
        T, Wn, dev = len(self.thr), len(wd), self.obs.device
        with torch.cuda.device(dev):
            rank = torch.empty((W.NHOURS, S + 1), dtype=torch.int64, device=dev)
            rel = torch.empty((T, W.NHOURS, n_bins, 3), dtype=torch.int64, device=dev)
            brier = torch.empty((T, W.NHOURS, 4), dtype=torch.int64, device=dev)
            fss = torch.empty((T, Wn, W.NHOURS, 2), dtype=torch.float64, device=dev)
            st = _stream(self.obs)
            rc = self.lib.rdgan_verify_reduce(_p(self.obs), _p(self.exceed), _p(self.below), _p(self.equal), _p(self.bad),
                                              self.P, self.ny * self.nx, S, _hp(self.thr), T, n_bins, ctypes.c_uint64(seed),
                                              _p(rank), _p(rel), _p(brier), st)
            _lib.check(rc, None, "rdgan_verify_reduce")
            nbytes = workspace_bytes(self.lib, "rdgan_verify_fss_workspace_bytes", self.ny, self.nx, T, Wn)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            rc = self.lib.rdgan_verify_fss(_p(self.obs), _p(self.exceed), _p(self.bad), self.n_days, self.ny, self.nx, S,
                                           _hp(self.thr), T, _hp(wd), Wn, _p(fss), _p(ws), nbytes, st)
            _lib.check(rc, None, "rdgan_verify_fss")
            rank, rel, brier, fss = rank.cpu().numpy(), rel.cpu().numpy(), brier.cpu().numpy(), fss.cpu().numpy()
        return Verification(tuple(float(t) for t in self.thr), tuple(int(w) for w in wd), S, int(brier[0, :, 0].sum()), rank, rel,
                            brier, fss)


def verify_hourly(ens, obs, thresholds, **result_kw):
    """One call for an ensemble that is held: ens (S, *obs.shape), obs (..., 24, ny, nx); result_kw: scales, n_bins, seed of
    EnsembleVerifier.result.  -> Verification"""
    thr = check_event_thresholds(thresholds)
    obs, ens = admit_array(obs, "obs")[0], admit_array(ens, "ens")[0]
    check_pair(ens.shape, obs.shape)
    S = int(ens.shape[0])
    unknown = set(result_kw) - {"scales", "n_bins", "seed"}
    if unknown:
        raise ValueError(f"unknown arguments {sorted(unknown)}")
    check_scales(result_kw.get("scales", DEFAULT_SCALES), S)
    _check_bins(result_kw.get("n_bins", 11), S)
    _check_seed(result_kw.get("seed", 0))
    return EnsembleVerifier(obs, thr).add(ens).result(**result_kw)


def verify_field(gen, observed, n_scenarios, thresholds, scales=DEFAULT_SCALES, n_bins=11, rank_seed=0, daily=None, scenario_chunk=16,
                 overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a day and verify the scenarios against its observed hours without holding them.  observed ([D,] 24, ny, nx): a
    numpy array, a float32 CUDA tensor or a DeviceDataset (its hourly tensor and daily plane are used where they lie); daily: the
    condition, ([D,] ny, nx), by default the sum of the observed hours.  The latent array is drawn once for all n_scenarios (<= 4096)
    scenarios, exactly as field.disaggregate draws it for the same seed, latent and numpy RNG state; disaggregate then runs for
    scenario_chunk scenarios at a time into one reused buffer and each result is added to an EnsembleVerifier.  The result equals
    verify_hourly(disaggregate(...all scenarios...)[0], observed, ...) exactly, for any scenario_chunk and chunk.
    -> Verification"""
    thr = check_event_thresholds(thresholds)
    S, step = F._check_scenarios(n_scenarios, scenario_chunk, MAX_MEMBERS)
    wd, n_bins, rank_seed = check_scales(scales, S), _check_bins(n_bins, S), _check_seed(rank_seed)
    request = ObservedRequest(gen, observed, daily, lambda shape: None, S, overlap, latent_mode, latent, chunk, norm_scale)
    ver = EnsembleVerifier(request.obs, thr)
    request.stream(ver.obs, step, ver.add, seed)
    return ver.result(scales=wd, n_bins=n_bins, seed=rank_seed)
