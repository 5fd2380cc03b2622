"""Scale-separation verification of hourly fields against the observed hours (csrc/rdgan_iss.hip.h): the
intensity-scale skill score of Casati, Ross and Stephenson (2004), with the bias-corrected reference of Casati (2010).  For each
threshold the binary error field member - observation is split by Haar wavelets into components of 1, 2, 4 ... 2^(L-1) pixels and
the means of the 2^L tiles; the MSE, the skill and the energy of either side are reported per component: at which spatial scale do
the errors sit.

The ensemble is never held: an IntensityScaleVerifier accumulates, over any number of add() calls, the integer state

    counts[t][h][l] = (QX, QO, QXO) = sum over the blocks b of side 2^l of the valid tiles of (SX_l(b)^2, SO_l(b)^2, SX_l(b) SO_l(b))
    tiles[h] = (valid, void)

SX and SO being the events (v > thr[t], v finite) of the member and of the observation in a block.  A tile of side 2^L of the centred
crop is void for a pair (member plane, observed plane) when any of its pixels is NaN or +-inf on either side.  Every accumulated
value is an integer, so the result does not depend on how the members were split into calls.  result() is host code on numpy and
Python integers and needs no GPU.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from . import field as F
from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._hourly import (MAX_ELEMS, MAX_MEMBERS, MAX_PLANE, NHOURS, ObservedRequest, ObservedVerifier, admit_array, check_pair,
                      grow_workspace)
from .verification import check_event_thresholds

MAX_LEVELS = 10                                                              # RD_ISS_MAXL
MAX_COUNT = 1 << 62                                                          # accumulated pixel-pairs * 4^L stay at or below it
MAX_PAIRS_PER_PASS = 1 << 30
_DEFAULT_PASS_BYTES = 1 << 28                                                # workspace the default pass takes at most (L > 6)


def check_levels(levels, ny, nx):
    """-> L: 1 .. 10 with 2^L <= min(ny, nx); None: the largest such"""
    most = min(MAX_LEVELS, int(min(ny, nx)).bit_length() - 1)
    if most < 1:
        raise ValueError(f"a plane of {ny} x {nx} pixels holds no tile of 2 x 2")
    if levels is None:
        return most
    L = whole_number(levels, 1, MAX_LEVELS, "levels")
    if L > most:
        raise ValueError(f"levels: a tile of 2^{L} pixels does not fit a plane of {ny} x {nx}")
    return L


def crop(ny, nx, levels):
    """(oy, ox, cy, cx): offset and size of the centred crop to whole tiles of side 2^levels"""
    side = 1 << levels
    return (ny % side) // 2, (nx % side) // 2, ny // side * side, nx // side * side


def _exact_ratio(num, den):
    """num / den elementwise for arrays of Python integers: one correctly rounded division each, NaN where den is 0"""
    return np.frompyfunc(lambda n, d: n / d if d else float("nan"), 2, 1)(num, den).astype(np.float64)


@dataclass
class IntensityScale:
    """What IntensityScaleVerifier.result returns, numpy on the host.  counts (T, 24, L + 1, 3) int64 = (QX, QO, QXO) per threshold,
    hour and level; tiles (24, 2) int64 = (valid, void) tile-pairs.  Component j = 0 .. L - 1 is the mother wavelet of features of 2^j
    pixels, component L the father (the tile means)."""
    thresholds: tuple
    levels: int
    ny: int
    nx: int
    counts: np.ndarray
    tiles: np.ndarray

    @property
    def scales_px(self):
        """the feature size of each component in pixels, (L + 1,): 1, 2, 4 ... 2^L (the last is the tile)"""
        return tuple(1 << j for j in range(self.levels + 1))

    def _q(self, by_hour):
        """(q (T, [24,] L + 1, 3), N ([24,] 1)) as arrays of Python integers; N = valid tiles * 4^L pixel-pairs"""
        q = np.asarray(self.counts).astype(object)
        n = np.asarray(self.tiles)[:, 0].astype(object) * (4 ** self.levels)
        if not by_hour:
            return q.sum(axis=1), np.asarray(n.sum(), dtype=object).reshape(1)
        return q, n.reshape(NHOURS, 1)

    def _components(self, z, n):
        """(numerators, denominators) of the L + 1 components of z (..., L + 1): 4 z_j - z_{j+1} over 4^(j+1) n, the father z_L
        over 4^L n; exact integers"""
        L = self.levels
        num = np.concatenate([4 * z[..., :-1] - z[..., 1:], z[..., -1:]], axis=-1)
        den = np.array([4 ** (j + 1) for j in range(L)] + [4 ** L], dtype=object) * n
        return num, np.broadcast_to(den, num.shape)

    def mse(self, by_hour=False):
        """the MSE of the binary error field per component, (T, L + 1) -- or (T, 24, L + 1); the components sum to the binary MSE
        QZ_0 / N; NaN without a valid tile"""
        q, n = self._q(by_hour)
        return _exact_ratio(*self._components(q[..., 0] - 2 * q[..., 2] + q[..., 1], n))

    def skill(self, by_hour=False, bias_corrected=False):
        """ISS_j = 1 - (L + 1) MSE_j / MSE_random, (T, L + 1) -- or (T, 24, L + 1).  MSE_random = 2 e (1 - e) with the base rate
        e = QO_0 / N; bias_corrected (Casati 2010): B e (1 - e) + e (1 - B e) with the frequency bias B = QX_0 / QO_0.  NaN where
        MSE_random is 0 (or B undefined).  Formed as one quotient of exact integers."""
        q, n = self._q(by_hour)
        num, den = self._components(q[..., 0] - 2 * q[..., 2] + q[..., 1], n)
        x0, o0 = q[..., 0, 0][..., None], q[..., 0, 1][..., None]
        # MSE_random = r / n^2
        r = x0 * (n - o0) + o0 * (n - x0) if bias_corrected else 2 * o0 * (n - o0)
        if bias_corrected:
            r = np.where(o0 == 0, 0, r)
        d = den * r
        return _exact_ratio(d - (self.levels + 1) * num * n * n, d)

    def energy(self, by_hour=False):
        """(En^X, En^O, relative difference), each (T, L + 1) -- or (T, 24, L + 1): the components' mean squares of the member's and
        of the observation's binary field, and (En^X - En^O) / (En^X + En^O), NaN at 0 / 0"""
        q, n = self._q(by_hour)
        nx_, den = self._components(q[..., 0], n)
        no_, _ = self._components(q[..., 1], n)
        return _exact_ratio(nx_, den), _exact_ratio(no_, den), _exact_ratio(nx_ - no_, np.where(n == 0, 0, nx_ + no_))

    def contingency(self, by_hour=False):
        """(hits, false alarms, misses, correct negatives) over the pixel-pairs of the valid tiles, (T, 4) -- or (T, 24, 4) int64"""
        q, n = self._q(by_hour)
        x0, o0, xo = q[..., 0, 0], q[..., 0, 1], q[..., 0, 2]
        return np.stack([xo, x0 - xo, o0 - xo, n[..., 0] - x0 - o0 + xo], axis=-1).astype(np.int64)

    def summary(self):
        """dict: thresholds, levels, scales_px, valid_tiles, void_tiles, base_rate and bias (T,), mse, skill, skill_bias_corrected,
        energy_model, energy_obs, energy_rel_diff (T, L + 1), skill_by_hour (T, 24, L + 1)"""
        q, n = self._q(False)
        enx, eno, rel = self.energy()
        return dict(thresholds=self.thresholds, levels=self.levels, scales_px=self.scales_px, valid_tiles=int(self.tiles[:, 0].sum()),
                    void_tiles=int(self.tiles[:, 1].sum()), base_rate=_exact_ratio(q[..., 0, 1], n), bias=_exact_ratio(q[..., 0, 0], q[..., 0, 1]),
                    mse=self.mse(), skill=self.skill(), skill_bias_corrected=self.skill(bias_corrected=True), energy_model=enx,
                    energy_obs=eno, energy_rel_diff=rel, skill_by_hour=self.skill(by_hour=True))


def compare(a, b):
    """Two IntensityScale with the same thresholds and levels -- two generators against the same observation -> dict: the
    differences a - b of skill, skill_bias_corrected, energy_model and energy_rel_diff, each (T, L + 1)"""
    if not (isinstance(a, IntensityScale) and isinstance(b, IntensityScale)):
        raise ValueError("compare takes two IntensityScale")
    if tuple(a.thresholds) != tuple(b.thresholds) or a.levels != b.levels:
        raise ValueError(f"the two results differ in thresholds or levels: {a.thresholds}, {a.levels} and {b.thresholds}, {b.levels}")
    ea, eb = a.energy(), b.energy()
    return dict(thresholds=tuple(a.thresholds), levels=a.levels, skill=a.skill() - b.skill(),
                skill_bias_corrected=a.skill(bias_corrected=True) - b.skill(bias_corrected=True), energy_model=ea[0] - eb[0],
                energy_rel_diff=ea[2] - eb[2])


def _check_pairs_per_pass(pairs_per_pass):
    return None if pairs_per_pass is None else whole_number(pairs_per_pass, 1, MAX_PAIRS_PER_PASS, "pairs_per_pass")


def _check_obs(shape, levels, what="obs"):
    ny, nx = shape[-2:]
    if ny * nx > MAX_PLANE:
        raise ValueError(f"{what}: a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
    if int(np.prod(shape, dtype=np.int64)) > MAX_ELEMS:
        raise ValueError(f"{what}: more than {MAX_ELEMS} values")
    return check_levels(levels, ny, nx)


class IntensityScaleVerifier(ObservedVerifier):
    """The state of an intensity-scale verification on the device.  obs (..., 24, ny, nx): a numpy array or a float32 CUDA tensor
    (used where it lies); thresholds: the events, in the unit of obs; levels: L, the tile is 2^L pixels wide -- None:
    min(10, floor(log2(min(ny, nx)))); pairs_per_pass: how many (member plane, observed plane) pairs the workspace of L > 6 holds at
    a time -- None: up to 256 MB.  The state does not depend on it."""

    def __init__(self, obs, thresholds, levels=None, pairs_per_pass=None):
        self.thr = check_event_thresholds(thresholds)

        def check_obs(shape):
            self.levels = _check_obs(shape, levels)
            self.pairs_per_pass = _check_pairs_per_pass(pairs_per_pass)

        self._admit_obs(obs, check_obs)
        dev = self.obs.device
        _, _, cy, cx = crop(self.ny, self.nx, self.levels)
        self._pairs_of_a_member = self.n_days * NHOURS * cy * cx                # pixel-pairs one member adds
        self.n_members = 0
        self.counts = torch.zeros((len(self.thr), NHOURS, self.levels + 1, 3), dtype=torch.int64, device=dev)
        self.tiles = torch.zeros((NHOURS, 2), dtype=torch.int64, device=dev)

    def _check_members(self, s):
        if (self.n_members + s) * self._pairs_of_a_member * 4 ** self.levels > MAX_COUNT:
            raise ValueError(f"{self.n_members + s} members of {self._pairs_of_a_member} pixel-pairs each at levels={self.levels} could "
                             "overflow the 64-bit state (pixel-pairs * 4^levels must stay at or below 2^62)")

    def add(self, members):
        """members (s, *obs.shape) float32, s <= 4096: a CUDA tensor, whose member axis may have any stride >= prod(obs.shape) (a
        view of a wider buffer), or a numpy array.  Returns self."""
        members, s, stride = self._admit_members(members)
        L = self.levels
        with torch.cuda.device(self.obs.device):
            one = workspace_bytes(self.lib, "rdgan_iss_workspace_bytes", self.ny, self.nx, L, 1)
            pairs = self.pairs_per_pass or max(1, min(s * self.n_days * NHOURS, _DEFAULT_PASS_BYTES // one))
            nbytes = workspace_bytes(self.lib, "rdgan_iss_workspace_bytes", self.ny, self.nx, L, pairs)
            ws = grow_workspace(self, nbytes, self.obs.device)
            rc = self.lib.rdgan_iss_accumulate(_p(members), s, stride, _p(self.obs), self.n_days, self.ny, self.nx, _hp(self.thr),
                                               len(self.thr), L, _p(self.counts), _p(self.tiles), _p(ws), nbytes,
                                               _stream(self.obs))
        _lib.check(rc, None, "rdgan_iss_accumulate")
        self.n_members += s
        return self

    def state(self):
        """(counts (T, 24, L + 1, 3) int64, tiles (24, 2) int64): the tensors themselves, on the device"""
        return self.counts, self.tiles

    def result(self):
        """-> IntensityScale of the members added so far"""
        if self.n_members < 1:
            raise ValueError("no member has been added")
        return IntensityScale(tuple(float(t) for t in self.thr), self.levels, self.ny, self.nx, self.counts.cpu().numpy(),
                              self.tiles.cpu().numpy())


def intensity_scale_hourly(ens, obs, thresholds, levels=None):
    """One call for an ensemble that is held: ens (S, *obs.shape), obs (..., 24, ny, nx), each a float32 CUDA tensor or a numpy
    array.  -> IntensityScale"""
    thr = check_event_thresholds(thresholds)
    obs, ens = admit_array(obs, "obs")[0], admit_array(ens, "ens")[0]
    check_pair(ens.shape, obs.shape)
    levels = _check_obs(tuple(obs.shape), levels)
    return IntensityScaleVerifier(obs, thr, levels).add(ens).result()


def intensity_scale_field(gen, observed, n_scenarios, thresholds, levels=None, daily=None, scenario_chunk=16, overlap=4,
                          latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a day and take the intensity-scale state of the scenarios against its observed hours without holding them.
    observed ([D,] 24, ny, nx): a numpy array, a float32 CUDA tensor or a DeviceDataset; daily: the condition, ([D,] ny, nx), by
    default the sum of the observed hours.  The latent array is drawn once for all n_scenarios (<= 4096) scenarios, exactly as
    field.disaggregate draws it for the same seed, latent and numpy RNG state; disaggregate then runs for scenario_chunk scenarios at
    a time into one reused buffer and each result is added to an IntensityScaleVerifier.  The state equals that of
    intensity_scale_hourly(disaggregate(...all scenarios...)[0], observed, ...) where the hourly values are the same
    (_hourly.evaluate_field says when they are).  -> IntensityScale"""
    thr = check_event_thresholds(thresholds)
    S, step = F._check_scenarios(n_scenarios, scenario_chunk, MAX_MEMBERS)
    request = ObservedRequest(gen, observed, daily, lambda shape: _check_obs(shape, levels, "observed"), S, overlap, latent_mode, latent,
                              chunk, norm_scale)
    ver = IntensityScaleVerifier(request.obs, thr, levels)
    request.stream(ver.obs, step, ver.add, seed)
    return ver.result()
