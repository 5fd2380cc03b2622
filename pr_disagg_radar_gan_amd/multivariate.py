"""Joint-field scores (csrc/rdgan_mvscore.hip.h): an ensemble of whole hourly days against the observed day
taken as ONE vector of 24 ny nx components -- the energy score (Gneiting et al. 2008) and the variogram score of order p (Scheuerer
& Hamill 2015).  The per-pixel CRPS is blind to the dependence between pixels and hours, which is where the climatological day,
RainFARM, the analog baseline and the GAN differ; these two scores are not.

A NaN of the observation leaves its position out of every sum of that day; a day without a valid position scores NaN.  The members
must be finite.  ES = obs_sum / m - pair_sum / m^2, or pair_sum / (m (m - 1)) with fair=True (0 spread at m = 1).  VS = sum over
the displacements (l, di, dj) of w * sq, by default w = 1 / sqrt(l^2 + di^2 + dj^2).

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass, field
from typing import Dict

import numpy as np
import torch

from . import _lib, crps_experiment, ensemble, rainfarm
from . import weights as W
from ._dev import device_f32, ptr as _p, stream as _stream, whole_number, workspace_bytes
from .analog import AnalogLibrary
from ._hourly import MAX_PLANE, NHOURS
from .cascade import CascadeModel
from .engine import require_gpu

MAX_MEMBERS = crps_experiment.MAX_MEMBERS                                    # RD_MV_MAXM
MAX_DAYS = 1 << 20                                                           # RD_MV_MAXDAYS
MAX_RADIUS = 4                                                               # RD_MV_MAXR
MAX_LAG = 3                                                                  # RD_MV_MAXLAG
ORDERS = (0.5, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# host: arguments, displacements, weights
# ---------------------------------------------------------------------------------------------------------------------------------
def in_half_space(l, di, dj):
    """the displacements that count each unordered pair once"""
    return l > 0 or (l == 0 and (di > 0 or (di == 0 and dj > 0)))


def displacements(radius, max_lag):
    """[(l, di, dj)] of the half-space in table order: ((2r + 1)^2 - 1) / 2 + max_lag (2r + 1)^2 of them"""
    r, L = check_radius(radius), check_max_lag(max_lag)
    return [(l, di, dj) for l in range(L + 1) for di in range(-r, r + 1) for dj in range(-r, r + 1) if in_half_space(l, di, dj)]


def default_weights(radius, max_lag):
    """(max_lag + 1, 2r + 1, 2r + 1) float64: 1 / sqrt(l^2 + di^2 + dj^2) in the half-space, 0 outside"""
    r, L = check_radius(radius), check_max_lag(max_lag)
    w = np.zeros((L + 1, 2 * r + 1, 2 * r + 1))
    for l, di, dj in displacements(r, L):
        w[l, di + r, dj + r] = 1.0 / np.sqrt(float(l * l + di * di + dj * dj))
    return w


def check_radius(radius):
    return whole_number(radius, 0, MAX_RADIUS, "radius")


def check_max_lag(max_lag):
    return whole_number(max_lag, 0, MAX_LAG, "max_lag")


def check_order(p):
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or float(p) not in ORDERS:
        raise ValueError(f"p must be one of {ORDERS}, got {p!r}")
    return float(p)


def check_weights(weights, radius, max_lag):
    """None -> default_weights; else a table of the same shape, finite; entries outside the half-space are ignored"""
    r, L = check_radius(radius), check_max_lag(max_lag)
    if weights is None:
        return default_weights(r, L)
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.asarray(weights)
    if w.shape != (L + 1, 2 * r + 1, 2 * r + 1) or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
        raise ValueError(f"weights: expected a table of numbers of shape {(L + 1, 2 * r + 1, 2 * r + 1)}, got {w.dtype} {w.shape}")
    w = w.astype(np.float64)
    if not np.isfinite(w).all():
        raise ValueError("weights: every weight must be finite")
    return w * (default_weights(r, L) > 0)


def _shape_of(a, name):
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError(f"{name}: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
        if not a.dtype.is_floating_point:
            raise ValueError(f"{name}: expected floating-point values")
        return tuple(int(v) for v in a.shape)
    a = np.asarray(a)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{name}: expected an array of numbers")
    return tuple(int(v) for v in a.shape)


def admit(ens, obs):
    """The shapes of a call, host code: ens (m, 24, ny, nx) with obs (24, ny, nx) or (D, 24, ny, nx) -- one shared ensemble -- or
    ens (D, m, 24, ny, nx) with obs (D, 24, ny, nx).  -> (m, D, ny, nx, shared)"""
    es, os_ = _shape_of(ens, "ens"), _shape_of(obs, "obs")
    if len(es) not in (4, 5) or es[-3] != NHOURS or min(es) < 1:
        raise ValueError(f"ens: expected shape (m, {NHOURS}, ny, nx) or (D, m, {NHOURS}, ny, nx) with no empty axis, got {es}")
    if len(os_) not in (3, 4) or min(os_) < 1 or os_[-3:] != es[-3:]:
        raise ValueError(f"obs: expected shape ({NHOURS}, {es[-2]}, {es[-1]}) or (D, {NHOURS}, {es[-2]}, {es[-1]}), got {os_}")
    m, ny, nx = es[-4], es[-2], es[-1]
    D = os_[0] if len(os_) == 4 else 1
    shared = len(es) == 4
    if not shared and (len(os_) != 4 or es[0] != D):
        raise ValueError(f"ens holds {es[0]} days, obs must have shape ({es[0]}, {NHOURS}, {ny}, {nx}), got {os_}")
    if m > MAX_MEMBERS:
        raise ValueError(f"at most {MAX_MEMBERS} members, got {m}")
    if ny * nx > MAX_PLANE:
        raise ValueError(f"a plane has {ny * nx} pixels, the limit is {MAX_PLANE}")
    if D > MAX_DAYS:
        raise ValueError(f"at most {MAX_DAYS} days per call, got {D}")
    return m, D, ny, nx, shared


def _on_device(ens, obs):
    require_gpu()
    ens = device_f32(ens, "ens", obs.device if isinstance(obs, torch.Tensor) else None)
    obs = device_f32(obs, "obs", ens.device)
    if obs.device != ens.device:
        raise ValueError(f"ens lies on {ens.device}, obs on {obs.device}")
    return ens, obs


def _workspace(lib, dev, entry, *args):
    nbytes = workspace_bytes(lib, entry, *args)
    return torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=dev), nbytes


# ---------------------------------------------------------------------------------------------------------------------------------
# the two scores
# ---------------------------------------------------------------------------------------------------------------------------------
def energy_terms(ens, obs):
    """(obs_sum, pair_sum), float64 CUDA tensors (D,): the sum over the members of |x_i - y| and the sum over i < j of
    |x_i - x_j|, Euclidean over the day's valid positions, differences and sums in fp64.  ens (m, 24, ny, nx) -- one ensemble for
    every day of obs, its member distances computed once -- or (D, m, 24, ny, nx); obs (24, ny, nx) or (D, 24, ny, nx); numpy or
    CUDA.  Two calls agree bit for bit; a day's sums do not depend on the other days of the call."""
    m, D, ny, nx, shared = admit(ens, obs)
    ens, obs = _on_device(ens, obs)
    lib, dev = _lib.load(), ens.device
    obs_sum = torch.empty(D, dtype=torch.float64, device=dev)
    pair_sum = torch.empty(D, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _workspace(lib, dev, "rdgan_mv_energy_workspace_bytes", m, D, int(shared))
        rc = lib.rdgan_mv_energy(_p(ens), _p(obs), m, D, ny, nx, int(shared), _p(obs_sum), _p(pair_sum), _p(ws), nbytes, _stream(ens))
    _lib.check(rc, None, "rdgan_mv_energy")
    return obs_sum, pair_sum


def energy_from_terms(obs_sum, pair_sum, m, fair=False):
    """ES = obs_sum / m - pair_sum / m^2, or - pair_sum / (m (m - 1)) for the fair score, whose spread term is 0 at m = 1"""
    if fair:
        return obs_sum / m - (pair_sum / (m * (m - 1)) if m > 1 else pair_sum * 0.0)
    return obs_sum / m - pair_sum / (m * m)


def energy_score(ens, obs, fair=False):
    """The energy score per day, a float64 CUDA tensor (D,); arguments as energy_terms.  NaN for a day without a valid position."""
    if not isinstance(fair, (bool, np.bool_)):
        raise ValueError(f"fair must be True or False, got {fair!r}")
    m = admit(ens, obs)[0]
    obs_sum, pair_sum = energy_terms(ens, obs)
    return energy_from_terms(obs_sum, pair_sum, m, bool(fair))


def variogram_score(ens, obs, p=0.5, radius=2, max_lag=1, weights=None, normalised=False, return_tables=False):
    """The variogram score of order p (0.5 or 1) per day, a float64 CUDA tensor (D,): the sum over the displacements (l, di, dj), 0
    <= l <= max_lag <= 3 hours and |di|, |dj| <= radius <= 4 pixels, each unordered pair once, of w times the sum over the valid
    pairs of (|y_a - y_b|^p - mean over the members of |x_a - x_b|^p)^2.  weights: None for 1 / sqrt(l^2 + di^2 + dj^2), or a table
    (max_lag + 1, 2 radius + 1, 2 radius + 1).  normalised: divided by the sum of w * count.  return_tables: also sq (float64) and
    count (int64), CUDA tensors (D, max_lag + 1, 2 radius + 1, 2 radius + 1), 0 outside the half-space.  ens and obs as
    energy_terms; a shared ensemble's member means are computed once."""
    p, r, L = check_order(p), check_radius(radius), check_max_lag(max_lag)
    w = check_weights(weights, r, L)
    m, D, ny, nx, shared = admit(ens, obs)
    ens, obs = _on_device(ens, obs)
    lib, dev = _lib.load(), ens.device
    side = 2 * r + 1
    sq = torch.empty((D, L + 1, side, side), dtype=torch.float64, device=dev)
    count = torch.empty((D, L + 1, side, side), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _workspace(lib, dev, "rdgan_mv_variogram_workspace_bytes", D, ny, nx, r, L, int(shared))
        rc = lib.rdgan_mv_variogram(_p(ens), _p(obs), m, D, ny, nx, int(shared), p, r, L, _p(sq), _p(count), _p(ws), nbytes, _stream(ens))
    _lib.check(rc, None, "rdgan_mv_variogram")
    wd = torch.from_numpy(w).to(dev)
    keep = wd != 0                                                         # (a NaN sq under a zero weight stays out)
    vs = (torch.where(keep, sq, torch.zeros_like(sq)) * wd).sum(dim=(1, 2, 3))
    if normalised:
        vs = vs / (count.to(torch.float64) * wd).sum(dim=(1, 2, 3))
    return (vs, sq, count) if return_tables else vs


# ---------------------------------------------------------------------------------------------------------------------------------
# many days, one ensemble in memory at a time
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_reals(reals, name="reals"):
    shape = _shape_of(reals, name)
    if len(shape) != 4 or shape[1] != NHOURS or min(shape) < 1:
        raise ValueError(f"{name}: expected shape (D, {NHOURS}, ny, nx) with no empty axis, got {shape}")
    return shape


def scores_for_days(make_ensemble, reals, fair=False, p=0.5, radius=2, max_lag=1, weights=None, normalised=False):
    """reals (D, 24, ny, nx), numpy or CUDA; make_ensemble(d) -> day d's (m, 24, ny, nx) ensemble, which is scored against
    reals[d] and dropped before the next one is made: the m 24 ny nx floats exist for one day at a time.  -> (es, vs), numpy
    float64 (D,)."""
    if not callable(make_ensemble):
        raise ValueError("make_ensemble must be callable")
    if not isinstance(fair, (bool, np.bool_)):
        raise ValueError(f"fair must be True or False, got {fair!r}")
    shape = _check_reals(reals)
    p, r, L = check_order(p), check_radius(radius), check_max_lag(max_lag)
    w = check_weights(weights, r, L)
    require_gpu()
    reals = device_f32(reals, "reals")
    es, vs = [], []
    for d in range(shape[0]):
        ens = make_ensemble(d)
        es.append(energy_score(ens, reals[d], fair=fair))
        vs.append(variogram_score(ens, reals[d], p=p, radius=r, max_lag=L, weights=w, normalised=normalised))
        del ens
    return torch.cat(es).cpu().numpy(), torch.cat(vs).cpu().numpy()


@dataclass
class MultivariateExperimentResult:
    """Per-day scores, numpy float64 (D,), by method: es["gan"], es["random"] (the fixed climatological ensemble), and es["rainfarm"]
    / es["analog"] where the experiment had slopes / a library; vs likewise."""
    es: Dict[str, np.ndarray] = field(default_factory=dict)
    vs: Dict[str, np.ndarray] = field(default_factory=dict)

    def summary(self, perc=1, N=10000, seed=0):
        """{"es": {...}, "vs": {...}}; each holds the mean score per method under its name and, per baseline b, "gan-b" =
        {"ttest_p": crps_experiment.ttest_1samp(gan - b)[1], "bootstrap": [mean, lower, upper] of gan - b
        (crps_experiment.bootstrapped_difference_onesample)}"""
        out = {}
        for name, table in (("es", self.es), ("vs", self.vs)):
            s = {k: float(np.mean(v, dtype=np.float64)) for k, v in table.items()}
            for k, v in table.items():
                if k != "gan":
                    diff = (table["gan"] - v).astype(np.float64)
                    s[f"gan-{k}"] = {"ttest_p": crps_experiment.ttest_1samp(diff)[1],
                                     "bootstrap": crps_experiment.bootstrapped_difference_onesample(diff, perc=perc, N=N, seed=seed)}
            out[name] = s
        return out


def gan_ensemble(gen, real, n_members, seed=None, norm_scale=W.NORM_SCALE):
    """The generator's ensemble for one real day (24, nd, nd) on the host, in mm/h: the fractions of
    ensemble.generate_ensemble_device times the condition, as crps_experiment.crps_for_days scales them"""
    dsum = real.sum(0)
    fractions = ensemble.generate_ensemble_device(gen, (dsum / norm_scale).numpy()[..., None], n_members, seed=seed)
    return fractions * (dsum / norm_scale * norm_scale).to(fractions.device)


def multivariate_experiment(gen, reals_precip, climatology, slopes=None, library=None, n_members=1000, seed=0, fair=False, p=0.5,
                            radius=2, max_lag=1, weights=None, normalised=False, k=10, analog_weights="rank", query_groups=None, cascade=None,
                            cascade_patch=1):
    """Energy and variogram score per real day for the competing methods.  reals_precip (D, 24, nd, nd) mm/h; climatology
    (n, 24, nd, nd), e.g. crps_experiment.climatology_sample(dataset), scored in the shared form.  Seed rules, those of the CRPS
    experiment: the GAN's day d uses the device generator seeded seed + d (crps_experiment.crps_for_days); RainFARM, with slopes =
    (alpha, beta), draws the members d n_members .. (d + 1) n_members - 1 of the counter RNG (rainfarm_crps_for_days); the analog
    baseline, with library = an AnalogLibrary, is library.generate(daily sum of day d, n_members, k, seed, analog_weights,
    first_query=d), query_groups (D,) leaving the library's days of the same group out; the random cascade, with cascade = a
    cascade.CascadeModel, is cascade.generate(daily sum of day d, n_members, seed, first_query=d, patch=cascade_patch) and adds
    es["cascade"] and vs["cascade"].  -> MultivariateExperimentResult."""
    shape = _check_reals(reals_precip, "reals_precip")
    cs = _check_reals(climatology, "climatology")
    if shape[2] != shape[3] or cs[1:] != shape[1:] or cs[0] > MAX_MEMBERS:
        raise ValueError(f"reals_precip (D, {NHOURS}, nd, nd) and climatology (n <= {MAX_MEMBERS}, {NHOURS}, nd, nd) expected, got {shape} and {cs}")
    if slopes is not None:
        if len(slopes) != 2:
            raise ValueError("slopes must be (alpha, beta)")
        rainfarm._check_nd(shape[2])
    if library is not None and (not isinstance(library, AnalogLibrary) or tuple(library.plane_shape) != shape[2:]):
        raise ValueError(f"library: expected an AnalogLibrary of planes {shape[2:]}")
    if query_groups is not None and (library is None or len(query_groups) != shape[0]):
        raise ValueError(f"query_groups: {shape[0]} groups and a library expected")
    if cascade is not None and not isinstance(cascade, CascadeModel):
        raise ValueError("cascade: expected a cascade.CascadeModel")
    cascade_patch = whole_number(cascade_patch, 1, MAX_PLANE, "cascade_patch")
    m = whole_number(n_members, 1, MAX_MEMBERS, "n_members")
    seed = whole_number(seed, 0, (1 << 62), "seed")
    score = dict(fair=fair, p=check_order(p), radius=check_radius(radius), max_lag=check_max_lag(max_lag),
                 weights=check_weights(weights, radius, max_lag), normalised=normalised)
    if not isinstance(fair, (bool, np.bool_)):
        raise ValueError(f"fair must be True or False, got {fair!r}")
    require_gpu()
    reals = device_f32(reals_precip, "reals_precip")
    reals_host = reals.cpu()                                                 # the GAN's daily sums are taken on the host, as crps_for_days does
    res = MultivariateExperimentResult()
    res.es["gan"], res.vs["gan"] = scores_for_days(lambda d: gan_ensemble(gen, reals_host[d], m, seed=seed + d), reals, **score)
    clim = device_f32(climatology, "climatology", reals.device)
    vs_score = {key: v for key, v in score.items() if key != "fair"}
    res.es["random"] = energy_score(clim, reals, fair=fair).cpu().numpy()
    res.vs["random"] = variogram_score(clim, reals, **vs_score).cpu().numpy()
    if slopes is not None:
        alpha, beta = float(slopes[0]), float(slopes[1])
        res.es["rainfarm"], res.vs["rainfarm"] = scores_for_days(
            lambda d: rainfarm.downscale_device(reals[d].sum(0), alpha, beta, n_members=m, seed=seed, first_member=d * m), reals, **score)
    if library is not None:
        groups = None if query_groups is None else np.asarray(query_groups)
        res.es["analog"], res.vs["analog"] = scores_for_days(
            lambda d: library.generate(reals[d:d + 1].sum(1), m, k=k, seed=seed, weights=analog_weights, first_query=d,
                                       query_groups=None if groups is None else groups[d:d + 1])[0], reals, **score)
    if cascade is not None:
        res.es["cascade"], res.vs["cascade"] = scores_for_days(
            lambda d: cascade.generate(reals[d:d + 1].sum(1), m, seed=seed, first_query=d, patch=cascade_patch)[0], reals, **score)
    return res
