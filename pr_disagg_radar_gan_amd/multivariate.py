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

from . import _lib, crps_experiment
from ._dev import flag, ptr as _p, stream as _stream, whole_number, workspace_bytes
from ._experiment import competing_methods, for_each_day, gan_ensemble     # noqa: F401 (gan_ensemble is public here)
from ._hourly import MAX_PLANE, NHOURS, admit_ensemble, ensemble_on_device  # noqa: F401 (the two limits are public here)

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


def admit(ens, obs):
    """_hourly.admit_ensemble with the limits of the scores: at most 8192 members, 2^20 days.  -> (m, D, ny, nx, shared)"""
    return admit_ensemble(ens, obs, MAX_MEMBERS, MAX_DAYS)


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
    ens, obs = ensemble_on_device(ens, obs)
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
    fair, m = flag(fair, "fair"), admit(ens, obs)[0]
    obs_sum, pair_sum = energy_terms(ens, obs)
    return energy_from_terms(obs_sum, pair_sum, m, fair)


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
    ens, obs = ensemble_on_device(ens, obs)
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
def scores_for_days(make_ensemble, reals, fair=False, p=0.5, radius=2, max_lag=1, weights=None, normalised=False):
    """reals (D, 24, ny, nx), numpy or CUDA; make_ensemble(d) -> day d's (m, 24, ny, nx) ensemble, which is scored against
    reals[d] and dropped before the next one is made: the m 24 ny nx floats exist for one day at a time.  -> (es, vs), numpy
    float64 (D,)."""
    fair, p, r, L = flag(fair, "fair"), check_order(p), check_radius(radius), check_max_lag(max_lag)
    w = check_weights(weights, r, L)
    days = for_each_day(make_ensemble, reals, lambda d, ens, real: (
        energy_score(ens, real, fair=fair), variogram_score(ens, real, p=p, radius=r, max_lag=L, weights=w, normalised=normalised)))
    return tuple(torch.cat(part).cpu().numpy() for part in zip(*days))


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


def multivariate_experiment(gen, reals_precip, climatology, slopes=None, library=None, n_members=1000, seed=0, fair=False, p=0.5,
                            radius=2, max_lag=1, weights=None, normalised=False, k=10, analog_weights="rank", query_groups=None, cascade=None,
                            cascade_patch=1):
    """Energy and variogram score per real day for the competing methods.  reals_precip (D, 24, nd, nd) mm/h; climatology
    (n, 24, nd, nd), e.g. crps_experiment.climatology_sample(dataset), scored in the shared form as es["random"]; es["gan"] always,
    es["rainfarm"] / es["analog"] / es["cascade"] with slopes / a library / a cascade model; vs likewise.  The methods' arguments
    and the seed rules that make day d's ensemble are _experiment.competing_methods'.  -> MultivariateExperimentResult."""
    fair, p, r, L = flag(fair, "fair"), check_order(p), check_radius(radius), check_max_lag(max_lag)
    score = dict(p=p, radius=r, max_lag=L, weights=check_weights(weights, r, L), normalised=normalised)
    roster = competing_methods(gen, reals_precip, climatology, max_members=MAX_MEMBERS, slopes=slopes, library=library, n_members=n_members,
                               seed=seed, k=k, analog_weights=analog_weights, query_groups=query_groups, cascade=cascade, cascade_patch=cascade_patch)
    both = roster.run(lambda make: scores_for_days(make, roster.reals, fair=fair, **score),
                      lambda clim, reals: (energy_score(clim, reals, fair=fair).cpu().numpy(), variogram_score(clim, reals, **score).cpu().numpy()))
    return MultivariateExperimentResult({name: es for name, (es, _) in both.items()}, {name: vs for name, (_, vs) in both.items()})
