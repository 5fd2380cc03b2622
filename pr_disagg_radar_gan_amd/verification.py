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
from .engine import require_gpu
from .field_products import _member_layout

MAX_THRESHOLDS, MAX_SCALES, MAX_MEMBERS, MAX_BINS = 8, 8, 4096, 64          # RD_VF_MAXT, RD_VF_MAXW, RD_VF_MAXS, RD_VF_MAXBINS
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
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 2 <= int(n_bins) <= min(int(n_members) + 1, MAX_BINS):
        raise ValueError(f"n_bins must lie in 2 .. min(n_members + 1, {MAX_BINS}) = {min(int(n_members) + 1, MAX_BINS)}, got {n_bins!r}")
    return int(n_bins)


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"the rank seed must be an integer in 0 .. 2^64 - 1, got {seed!r}")
    return int(seed)


def _check_obs_shape(shape, what="obs"):
    shape = tuple(int(n) for n in shape)
    if len(shape) < 3 or shape[-3] != W.NHOURS or min(shape) < 1:
        raise ValueError(f"{what}: expected shape (..., 24, ny, nx) with no empty axis, got {shape}")
    return shape


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


class EnsembleVerifier:
    """The state of a verification on the device.  obs (..., 24, ny, nx): a numpy array or a float32 CUDA tensor (used where it
    lies); thresholds: the events, in the unit of obs."""

    def __init__(self, obs, thresholds):
        self.thr = check_event_thresholds(thresholds)
        if isinstance(obs, torch.Tensor):
            if not (obs.is_cuda and obs.dtype == torch.float32):
                raise ValueError("obs: expected a numpy array or a float32 CUDA tensor")
            self.shape = _check_obs_shape(obs.shape)
        else:
            obs = np.asarray(obs)
            if not (np.issubdtype(obs.dtype, np.floating) or np.issubdtype(obs.dtype, np.integer)):
                raise ValueError("obs: expected an array of numbers")
            self.shape = _check_obs_shape(obs.shape)
        require_gpu()
        self.lib = _lib.load()
        if isinstance(obs, torch.Tensor):
            self.obs = obs.detach().contiguous()
        else:
            self.obs = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).cuda()
        dev = self.obs.device
        self.P = int(np.prod(self.shape, dtype=np.int64))
        self.ny, self.nx = self.shape[-2], self.shape[-1]
        self.n_members = 0
        self.exceed = torch.zeros((len(self.thr),) + self.shape, dtype=torch.int32, device=dev)
        self.below = torch.zeros(self.shape, dtype=torch.int32, device=dev)
        self.equal = torch.zeros(self.shape, dtype=torch.int32, device=dev)
        self.bad = torch.isnan(self.obs).to(torch.uint8)

    def add(self, members):
        """members (s, *obs.shape) float32: a CUDA tensor, whose member axis may have any stride >= prod(obs.shape) (a view of a
        wider buffer, as member_stats_device accepts it), or a numpy array.  Returns self."""
        if isinstance(members, torch.Tensor):
            if not members.is_cuda:                    # (a host view's strides would not survive the copy to the device)
                raise ValueError("members: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
            host = None
        else:
            host = members = torch.from_numpy(np.ascontiguousarray(members, dtype=np.float32))       # dense: member stride P
        s, P, stride, shape = _member_layout(members)
        if shape != self.shape:
            raise ValueError(f"members: expected shape (s,) + {self.shape}, got {tuple(members.shape)}")
        if self.n_members + s > MAX_MEMBERS:
            raise ValueError(f"a verification holds at most {MAX_MEMBERS} members: {self.n_members} held, {s} more offered")
        if members.dtype != torch.float32:
            raise ValueError("members: expected float32")
        if host is not None:
            members, stride = host.to(self.obs.device), P
        elif members.device != self.obs.device:
            raise ValueError(f"members lie on {members.device}, the observation on {self.obs.device}")
        with torch.cuda.device(self.obs.device):
            rc = self.lib.rdgan_verify_accumulate(F._p(members), s, stride, P, F._p(self.obs), F._hp(self.thr), len(self.thr),
                                                  F._p(self.exceed), F._p(self.below), F._p(self.equal), F._p(self.bad),
                                                  F._stream(self.obs))
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
        n_days = self.P // (W.NHOURS * self.ny * self.nx)
        with torch.cuda.device(dev):
            rank = torch.empty((W.NHOURS, S + 1), dtype=torch.int64, device=dev)
            rel = torch.empty((T, W.NHOURS, n_bins, 3), dtype=torch.int64, device=dev)
            brier = torch.empty((T, W.NHOURS, 4), dtype=torch.int64, device=dev)
            fss = torch.empty((T, Wn, W.NHOURS, 2), dtype=torch.float64, device=dev)
            st = F._stream(self.obs)
            rc = self.lib.rdgan_verify_reduce(F._p(self.obs), F._p(self.exceed), F._p(self.below), F._p(self.equal), F._p(self.bad),
                                              self.P, self.ny * self.nx, S, F._hp(self.thr), T, n_bins, ctypes.c_uint64(seed),
                                              F._p(rank), F._p(rel), F._p(brier), st)
            _lib.check(rc, None, "rdgan_verify_reduce")
            nbytes = self.lib.rdgan_verify_fss_workspace_bytes(self.ny, self.nx, T, Wn)
            if nbytes < 0:
                raise _lib.RdganError(f"rdgan_verify_fss_workspace_bytes failed with code {nbytes}")
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            rc = self.lib.rdgan_verify_fss(F._p(self.obs), F._p(self.exceed), F._p(self.bad), n_days, self.ny, self.nx, S,
                                           F._hp(self.thr), T, F._hp(wd), Wn, F._p(fss), F._p(ws), nbytes, st)
            _lib.check(rc, None, "rdgan_verify_fss")
            rank, rel, brier, fss = rank.cpu().numpy(), rel.cpu().numpy(), brier.cpu().numpy(), fss.cpu().numpy()
        return Verification(tuple(float(t) for t in self.thr), tuple(int(w) for w in wd), S, int(brier[0, :, 0].sum()), rank, rel,
                            brier, fss)


def verify_hourly(ens, obs, thresholds, **result_kw):
    """One call for an ensemble that is held: ens (S, *obs.shape), obs (..., 24, ny, nx); result_kw: scales, n_bins, seed of
    EnsembleVerifier.result.  -> Verification"""
    thr = check_event_thresholds(thresholds)
    if not isinstance(obs, torch.Tensor):
        obs = np.asarray(obs)
    if not isinstance(ens, torch.Tensor):
        ens = np.asarray(ens)
    elif not ens.is_cuda:
        raise ValueError("ens: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
    if len(ens.shape) < 4:
        raise ValueError("ens: expected an array or tensor of shape (S, ..., 24, ny, nx)")
    S = int(ens.shape[0])
    if not 1 <= S <= MAX_MEMBERS:
        raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {S}")
    if tuple(ens.shape[1:]) != tuple(obs.shape):
        raise ValueError(f"ens: expected shape (S,) + {tuple(obs.shape)}, got {tuple(ens.shape)}")
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
    S, step = int(n_scenarios), int(scenario_chunk)
    if not 1 <= S <= MAX_MEMBERS:
        raise ValueError(f"the number of scenarios must lie in 1 .. {MAX_MEMBERS}, got {S}")
    if step < 1:
        raise ValueError("scenario_chunk must be at least 1")
    wd, n_bins, rank_seed = check_scales(scales, S), _check_bins(n_bins, S), _check_seed(rank_seed)
    dataset = hasattr(observed, "daily_plane")
    obs = observed.data if dataset else observed
    if isinstance(obs, torch.Tensor):
        if not (obs.is_cuda and obs.dtype == torch.float32):
            raise ValueError("observed: expected a numpy array, a float32 CUDA tensor or a DeviceDataset")
    else:
        obs = np.asarray(obs)
    shape = _check_obs_shape(obs.shape, "observed")
    if len(shape) not in (3, 4):
        raise ValueError(f"observed must have shape (24, ny, nx) or (n_days, 24, ny, nx), got {shape}")
    day_shape = shape[:-3] + shape[-2:]
    if daily is not None and not isinstance(daily, torch.Tensor):
        daily = np.asarray(daily)
    if daily is not None and tuple(daily.shape) != day_shape:
        raise ValueError(f"daily: expected shape {day_shape}, got {tuple(daily.shape)}")
    # the checks of disaggregate on a stand-in of the daily map's shape: nothing has touched the device so far
    _, squeeze_day, D, ny, nx, plan, z_shape = F._check_request(gen, np.broadcast_to(np.float32(0), day_shape), S, overlap, latent_mode,
                                                                latent, chunk, norm_scale)
    ver = EnsembleVerifier(obs, thr)
    dev = ver.obs.device
    with torch.cuda.device(dev):
        if daily is None:
            daily = observed.daily_plane() if dataset else ver.obs.sum(dim=-3)
        dd, info, _ = F._scan_request(daily, D, ny, nx, plan)
        # (without a wet tile disaggregate draws nothing)
        z_all = F._draw_latent(latent, seed, z_shape, dev) if info.n_active else None
        buf = torch.empty((min(step, S),) + shape, dtype=torch.float32, device=dev)
        cond = dd[0] if squeeze_day else dd
        for s0 in range(0, S, step):
            n = min(step, S - s0)
            F.disaggregate(gen, cond, n, overlap=overlap, latent_mode=latent_mode, latent=None if z_all is None else z_all[s0:s0 + n],
                           chunk=chunk, norm_scale=norm_scale, out=buf[:n])
            ver.add(buf[:n])
    return ver.result(scales=wd, n_bins=n_bins, seed=rank_seed)
