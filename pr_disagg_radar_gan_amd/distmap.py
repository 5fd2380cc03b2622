"""Distance-map verification of hourly fields against the observed hours (csrc/rdgan_distmap.hip.h): how far
is the member's rain from the observed rain, in pixels -- the binary-image distance measures built on the Euclidean distance
transform (Baddeley 1992; Gilleland 2011, 2017): Hausdorff distance, mean error distance, Baddeley's Delta, Zhu's measure.

For a threshold u the set of a plane is its pixels with a finite value v > u (fp32 compare): A the member's, B the observation's.
d2(x, S) = min over a in S of dy^2 + dx^2 is an exact integer, D(x, S) = isqrt(256 d2) the distance in 1/16 pixel (0xFFFF: S is
empty), w(x, S) = min(D(x, S), C) with the cutoff C in 1/16 pixel.  The device work is distance_maps (the observation's D(., B),
kept) and the record of every pair (member plane, observed plane of the same day and hour) and threshold: twelve integers,

    0 n_valid   1 nA   2 nB   3 nAB          over the pixels finite on both sides (the valid ones)
    4 sum over valid x in B of D(x, A)      5 sum over valid x in A of D(x, B)      6, 7 the maxima of the same two
    8 sum |wA - wB|   9 sum (wA - wB)^2   10 max |wA - wB|    over the valid pixels
    11 flags: 1 the bad-pixel masks differ, 2 A empty, 4 B empty (the whole sets)

4 .. 7 being 0 when the other set is empty.  Every record is bitwise the same however the members are grouped into calls or the
planes into passes.  measures_from_records is host code on numpy and needs no GPU.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._hourly import (MAX_ELEMS, MAX_MEMBERS, NHOURS, ObservedRequest, ObservedVerifier, admit, admit_array, check_pair, div,
                      grow_workspace, quantile_summary, summary_differences, to_state_device)
from .engine import require_gpu
from .verification import check_event_thresholds

MAX_SIDE = 2048                                                              # RD_DM_MAXSIDE
MAX_PASS = 1 << 20                                                           # RD_DM_MAXPASS
NREC = 12                                                                    # RD_DM_NREC
EMPTY = 0xFFFF                                                               # RD_DM_EMPTY
UNIT = 16                                                                    # distances are integers in 1 / UNIT pixel
MIN_CUTOFF, MAX_CUTOFF = 16, 65534                                           # RD_DM_CMIN, RD_DM_CMAX
_DEFAULT_PASS_BYTES = 1 << 28                                                # workspace the default pass takes at most
MEASURES = ("hausdorff", "med_model_to_obs", "med_obs_to_model", "baddeley_1", "baddeley_2", "baddeley_inf", "zhu", "csi")


def check_plane(ny, nx, what="hourly"):
    """ValueError for a plane the entries refuse: a side above 2048"""
    if ny > MAX_SIDE or nx > MAX_SIDE:
        raise ValueError(f"{what}: a plane of {ny} x {nx} pixels has a side above {MAX_SIDE}")


def check_planes_per_pass(planes_per_pass):
    return None if planes_per_pass is None else whole_number(planes_per_pass, 1, MAX_PASS, "planes_per_pass")


def cutoff16(cutoff_px, ny, nx):
    """-> C, the cutoff in 1/16 pixel: rint(16 cutoff_px), 16 .. 65534; None: the plane's diagonal, ceil(16 hypot(ny - 1, nx - 1))
    (at least 16), formed in integers"""
    if cutoff_px is None:
        v = 256 * ((ny - 1) ** 2 + (nx - 1) ** 2)
        r = math.isqrt(v)
        return max(MIN_CUTOFF, r + (r * r != v))
    if isinstance(cutoff_px, bool) or not isinstance(cutoff_px, (int, float, np.integer, np.floating)) or not math.isfinite(cutoff_px):
        raise ValueError(f"cutoff_px must be a finite number of pixels or None, got {cutoff_px!r}")
    C = round(UNIT * float(cutoff_px))
    if not MIN_CUTOFF <= C <= MAX_CUTOFF:
        raise ValueError(f"cutoff_px must lie in 1 .. {MAX_CUTOFF / UNIT} pixels, got {cutoff_px!r}")
    return int(C)


def _pass_bytes(lib, ny, nx, planes_per_pass, n_planes):
    one = workspace_bytes(lib, "rdgan_dm_workspace_bytes", ny, nx, 1)
    per_pass = planes_per_pass or max(1, min(n_planes, _DEFAULT_PASS_BYTES // one, MAX_PASS))
    return workspace_bytes(lib, "rdgan_dm_workspace_bytes", ny, nx, per_pass)


def _maps(lib, hourly, n, stride, shape, thr, planes_per_pass):
    """the library call of distance_maps on a device tensor -> (maps, set_sizes, workspace)"""
    ny, nx = shape[-2:]
    T, dev = len(thr), hourly.device
    with torch.cuda.device(dev):
        maps = torch.empty(shape[:-2] + (T, ny, nx), dtype=torch.uint16, device=dev)
        sizes = torch.empty(shape[:-2] + (T,), dtype=torch.int64, device=dev)
        nbytes = _pass_bytes(lib, ny, nx, planes_per_pass, n * NHOURS)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        rc = lib.rdgan_dm_maps(_p(hourly), n, stride, ny, nx, _hp(thr), T, _p(maps), _p(sizes), _p(ws), nbytes, _stream(maps))
    _lib.check(rc, None, "rdgan_dm_maps")
    return maps, sizes, ws


def distance_maps(hourly, thresholds, planes_per_pass=None):
    """The quantised distance transform of every plane of hourly (..., 24, ny, nx) float32: a CUDA tensor, whose leading axis may
    have any stride (a view of a wider buffer; _hourly.tensor_layout has the rule), or a numpy array; ny, nx <= 2048.  thresholds:
    the events in the unit of the data; planes_per_pass: how many planes the workspace holds at a time, 72 bytes per 64 pixels of a
    row -- None: up to 256 MB.  The result does not depend on it.
    -> (maps uint16 (..., 24, T, ny, nx): D(x, S_t) in 1/16 pixel, 0xFFFF where the set is empty; set_sizes int64 (..., 24, T): the
    pixels of each set), on the device"""
    thr, planes_per_pass = check_event_thresholds(thresholds), check_planes_per_pass(planes_per_pass)
    hourly, from_host, shape, n, stride = admit(hourly)
    check_plane(shape[-2], shape[-1])
    require_gpu()
    lib = _lib.load()
    device = torch.device("cuda", torch.cuda.current_device()) if from_host else hourly.device
    hourly = to_state_device(hourly, from_host, device)
    maps, sizes, _ = _maps(lib, hourly, n, stride, shape, thr, planes_per_pass)
    return maps, sizes


@dataclass
class PairRecords:
    """What DistanceMapVerifier.records returns, numpy on the host: records (S, n_days, 24, T, 12) int64, the twelve fields of the
    module's head per member, day, hour and threshold; cutoff16: C in 1/16 pixel."""
    records: np.ndarray
    thresholds: tuple
    cutoff16: int
    ny: int
    nx: int


@dataclass
class DistanceMeasures:
    """What measures_from_records returns, numpy on the host, each (S, n_days, 24, T) float64 in pixels unless said otherwise:
    hausdorff = max(rec6, rec7) / 16; med_model_to_obs = MED(A, B) = rec4 / nB, the mean distance to the model's set over the
    observed pixels; med_obs_to_model = MED(B, A) = rec5 / nA; zhu = lambda sqrt((nA + nB - 2 nAB) / n_valid) + (1 - lambda)
    MED(A, B); csi = nAB / (nA + nB - nAB), no unit; flags int64.  MED and Hausdorff are NaN where a set is empty or the dividing
    count is 0, Delta only at n_valid = 0, Zhu where its MED is, csi at 0 / 0."""
    records: PairRecords
    zhu_lambda: float
    hausdorff: np.ndarray
    med_model_to_obs: np.ndarray
    med_obs_to_model: np.ndarray
    zhu: np.ndarray
    csi: np.ndarray
    flags: np.ndarray

    def baddeley(self, p):
        """Baddeley's Delta_p with the cutoff of the records, p in 1, 2, inf: rec8 / n_valid, sqrt(rec9 / n_valid), rec10, in
        pixels; NaN at n_valid = 0"""
        r = self.records.records
        n = r[..., 0]
        if p == 1:
            return div(r[..., 8], UNIT * n)
        if p == 2:
            return np.sqrt(div(r[..., 9], UNIT * UNIT * n))
        if p in (np.inf, "inf"):
            return np.where(n != 0, r[..., 10] / float(UNIT), np.nan)
        raise ValueError(f"p must be 1, 2 or inf, got {p!r}")

    baddeley_1 = property(lambda self: self.baddeley(1))
    baddeley_2 = property(lambda self: self.baddeley(2))
    baddeley_inf = property(lambda self: self.baddeley(np.inf))

    def summary(self):
        """dict: thresholds, cutoff_px, mask_mismatch (the share of pairs with flag bit 0), and per measure in MEASURES a dict of
        median, q25, q75 and undefined (the share of pairs where it is NaN), each (24, T): per hour and threshold over the members
        and days; NaN where nothing is defined"""
        out = dict(thresholds=self.records.thresholds, cutoff_px=self.records.cutoff16 / UNIT, mask_mismatch=float(np.mean(self.flags & 1)))
        for name in MEASURES:
            a = getattr(self, name)
            out[name] = quantile_summary(np.moveaxis(a, -2, 0).reshape(NHOURS, -1, a.shape[-1]), 1)
        return out


def measures_from_records(records, zhu_lambda=0.5):
    """The measures of PairRecords, host code: each reported number takes one division and one root.  zhu_lambda in 0 .. 1 weighs
    the frequency term of Zhu's measure against its distance term.  -> DistanceMeasures"""
    if not isinstance(records, PairRecords):
        raise ValueError("measures_from_records takes PairRecords")
    if isinstance(zhu_lambda, bool) or not isinstance(zhu_lambda, (int, float, np.integer, np.floating)) or not 0 <= zhu_lambda <= 1:
        raise ValueError(f"zhu_lambda must lie in 0 .. 1, got {zhu_lambda!r}")
    r = np.asarray(records.records)
    if r.dtype != np.int64 or r.ndim < 1 or r.shape[-1] != NREC:
        raise ValueError(f"records: expected int64 (..., {NREC}), got {r.dtype} {r.shape}")
    lam = float(zhu_lambda)
    n, nA, nB, nAB, flags = r[..., 0], r[..., 1], r[..., 2], r[..., 3], r[..., 11]
    both = (flags & 6) == 0                                                  # neither whole set is empty
    med_ab = np.where(both, div(r[..., 4], UNIT * nB), np.nan)
    med_ba = np.where(both, div(r[..., 5], UNIT * nA), np.nan)
    haus = np.where(both & (nA > 0) & (nB > 0), np.maximum(r[..., 6], r[..., 7]) / float(UNIT), np.nan)
    zhu = lam * np.sqrt(div(nA + nB - 2 * nAB, n)) + (1.0 - lam) * med_ab
    return DistanceMeasures(records, lam, hausdorff=haus, med_model_to_obs=med_ab, med_obs_to_model=med_ba, zhu=zhu,
                            csi=div(nAB, nA + nB - nAB), flags=flags.copy())


def compare(a, b):
    """Two DistanceMeasures (or two of their summaries) with the same thresholds and cutoff -- two generators against the same
    observation -> dict: per measure the differences a - b of median, q25, q75 and undefined, each (24, T)"""
    a, b = (m.summary() if isinstance(m, DistanceMeasures) else m for m in (a, b))
    if not (isinstance(a, dict) and isinstance(b, dict) and "thresholds" in a and "thresholds" in b):
        raise ValueError("compare takes two DistanceMeasures or two summaries")
    if tuple(a["thresholds"]) != tuple(b["thresholds"]) or a["cutoff_px"] != b["cutoff_px"]:
        raise ValueError(f"the two summaries differ in thresholds or cutoff: {a['thresholds']}, {a['cutoff_px']} and {b['thresholds']}, {b['cutoff_px']}")
    return dict(thresholds=tuple(a["thresholds"]), cutoff_px=a["cutoff_px"], **summary_differences(a, b, MEASURES))


def _check_obs(shape, n_thresholds, max_map_bytes, what="obs"):
    """the checks of an observation (..., 24, ny, nx) before the device -> the bytes of its maps"""
    ny, nx = shape[-2:]
    check_plane(ny, nx, what)
    if int(np.prod(shape, dtype=np.int64)) > MAX_ELEMS:
        raise ValueError(f"{what}: more than {MAX_ELEMS} values")
    most = whole_number(max_map_bytes, 1, 1 << 62, "max_map_bytes")
    nbytes = 2 * n_thresholds * int(np.prod(shape, dtype=np.int64))
    if nbytes > most:
        raise ValueError(f"{what}: the distance maps of {n_thresholds} thresholds would take {nbytes} bytes, max_map_bytes is {most}")
    return nbytes


class DistanceMapVerifier(ObservedVerifier):
    """The observation and its distance maps on the device.  obs (..., 24, ny, nx), ny, nx <= 2048: a numpy array or a float32 CUDA
    tensor (used where it lies); thresholds: the events, in the unit of obs; cutoff_px: Baddeley's cutoff in pixels, 1 .. 4095.875
    -- None: the plane's diagonal, so that an empty set is "everything is a diagonal away"; planes_per_pass: how many planes the
    workspace holds at a time -- None: up to 256 MB, the records do not depend on it; max_map_bytes: a ValueError, before the
    device, if the maps (2 bytes per pixel and threshold) would exceed it."""

    def __init__(self, obs, thresholds, cutoff_px=None, planes_per_pass=None, max_map_bytes=2 << 30):
        self.thr = check_event_thresholds(thresholds)

        def check_obs(shape):
            _check_obs(shape, len(self.thr), max_map_bytes)
            self.cutoff16 = cutoff16(cutoff_px, shape[-2], shape[-1])
            self.planes_per_pass = check_planes_per_pass(planes_per_pass)

        self._admit_obs(obs, check_obs)
        self.maps, self.set_sizes, self._ws = _maps(self.lib, self.obs, self.n_days, NHOURS * self.ny * self.nx, self.shape, self.thr,
                                                    self.planes_per_pass)
        self._parts = []

    def add(self, members):
        """members (s, *obs.shape) float32, s <= 4096: a CUDA tensor, whose member axis may have any stride >= prod(obs.shape) (a
        view of a wider buffer), or a numpy array.  Appends the records of these members; returns self."""
        members, s, stride = self._admit_members(members)
        T, dev = len(self.thr), self.obs.device
        with torch.cuda.device(dev):
            rec = torch.empty((s, self.n_days, NHOURS, T, NREC), dtype=torch.int64, device=dev)
            nbytes = _pass_bytes(self.lib, self.ny, self.nx, self.planes_per_pass, s * self.n_days * NHOURS)
            ws = grow_workspace(self, nbytes, dev)
            rc = self.lib.rdgan_dm_records(_p(members), s, stride, _p(self.obs), _p(self.maps), self.n_days, self.ny, self.nx,
                                           _hp(self.thr), T, self.cutoff16, _p(rec), _p(ws), nbytes, _stream(rec))
        _lib.check(rc, None, "rdgan_dm_records")
        self._parts.append(rec)
        return self

    def records(self):
        """-> PairRecords of the members added so far, in the order they were added"""
        if not self._parts:
            raise ValueError("no member has been added")
        return PairRecords(torch.cat(self._parts, dim=0).cpu().numpy(), tuple(float(t) for t in self.thr), self.cutoff16, self.ny, self.nx)


def distmap_hourly(ens, obs, thresholds, cutoff_px=None, planes_per_pass=None, max_map_bytes=2 << 30, zhu_lambda=0.5):
    """One call for an ensemble that is held: ens (S, *obs.shape), obs (..., 24, ny, nx), each a float32 CUDA tensor or a numpy
    array.  -> DistanceMeasures of shape (S, n_days, 24, T); its .records are the PairRecords"""
    thr, planes_per_pass = check_event_thresholds(thresholds), check_planes_per_pass(planes_per_pass)
    obs, ens = admit_array(obs, "obs")[0], admit_array(ens, "ens")[0]
    check_pair(ens.shape, obs.shape)
    _check_obs(tuple(obs.shape), len(thr), max_map_bytes)
    cutoff16(cutoff_px, obs.shape[-2], obs.shape[-1])
    measures_from_records(PairRecords(np.zeros((0, NREC), np.int64), (), MIN_CUTOFF, 1, 1), zhu_lambda)        # (zhu_lambda, before the device)
    return measures_from_records(DistanceMapVerifier(obs, thr, cutoff_px, planes_per_pass, max_map_bytes).add(ens).records(), zhu_lambda)


def distmap_field(gen, observed, n_scenarios, thresholds, cutoff_px=None, planes_per_pass=None, max_map_bytes=2 << 30, zhu_lambda=0.5,
                  daily=None, scenario_chunk=16, overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024,
                  norm_scale=W.NORM_SCALE):
    """Disaggregate a day and take the distance measures of every scenario against its observed hours without holding the
    scenarios.  observed ([D,] 24, ny, nx): a numpy array, a float32 CUDA tensor or a DeviceDataset; daily: the condition, ([D,] ny,
    nx), by default the sum of the observed hours.  The latent array is drawn once for all n_scenarios (<= 4096) scenarios, exactly
    as field.disaggregate draws it for the same seed, latent and numpy RNG state; disaggregate then runs for scenario_chunk
    scenarios at a time into one reused buffer, and only the records of each chunk are kept.  The records equal those of
    distmap_hourly(disaggregate(...all scenarios...)[0], observed, ...) where the hourly values are the same
    (_hourly.evaluate_field says when they are).  -> DistanceMeasures of shape (S, D, 24, T)"""
    thr, planes_per_pass = check_event_thresholds(thresholds), check_planes_per_pass(planes_per_pass)
    S, step = F._check_scenarios(n_scenarios, scenario_chunk, MAX_MEMBERS)
    measures_from_records(PairRecords(np.zeros((0, NREC), np.int64), (), MIN_CUTOFF, 1, 1), zhu_lambda)

    def check_obs(shape):
        _check_obs(shape, len(thr), max_map_bytes, "observed")
        cutoff16(cutoff_px, shape[-2], shape[-1])

    request = ObservedRequest(gen, observed, daily, check_obs, S, overlap, latent_mode, latent, chunk, norm_scale)
    ver = DistanceMapVerifier(request.obs, thr, cutoff_px, planes_per_pass, max_map_bytes)
    request.stream(ver.obs, step, ver.add, seed)
    return measures_from_records(ver.records(), zhu_lambda)
