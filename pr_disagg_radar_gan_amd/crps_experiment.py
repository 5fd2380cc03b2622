"""The CRPS experiment of the paper's skill table (reference generate_and_evaluate_crps.py:164-203, C below; analyze_crps_results.py,
A below) on the device (csrc/rdgan_crps.hip.h): the CRPS of the GAN, of the "random" climatological baseline
(every real day against ONE fixed ensemble of training tiles, C:164, 193-194) and of RainFARM for a set of real days, then the
one-sample t-test on gan - random (A:14) and the bootstrapped interval of its mean (A:25-42).

The fixed ensemble is sorted once per call and every day costs one binary search per grid point; the bootstrap draws its indices
from the project's counter RNG on the device; the t statistic comes from device moments and its p-value from the regularised
incomplete beta function on the host (own continued fraction: the package does not depend on scipy).  No CPU fallback: without a
visible MI355X every device entry point raises RdganError; argument errors are ValueErrors raised before any device call."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, ensemble, rainfarm
from . import weights as W
from ._dev import device_f32, ptr as _p, stream as _stream
from .engine import require_gpu

NHOURS = 24
MAX_MEMBERS = 8192              # RD_CRPS_MAXN of csrc/rdgan_crps.hip.h


def _check_days(a, name):
    shape = tuple(a.shape)
    if len(shape) != 4 or shape[1] != NHOURS or shape[2] != shape[3] or shape[0] < 1 or shape[2] < 1:
        raise ValueError(f"{name} must have shape (n, {NHOURS}, nd, nd), got {shape}")
    return shape


def _device_f64_vector(x, name):
    shape = tuple(x.shape)
    if len(shape) != 1 or shape[0] < 1:
        raise ValueError(f"{name} must be a non-empty 1-D array, got shape {shape}")
    if shape[0] >= 2 ** 32:
        raise ValueError(f"{name}: fewer than 2^32 values, got {shape[0]}")
    require_gpu()
    if isinstance(x, torch.Tensor):
        return x.to(device="cuda" if not x.is_cuda else x.device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------
# the "random" baseline
# ---------------------------------------------------------------------------------------------------------------------------------
def climatology_sample(dataset, n=5000):
    """The ensemble of the "random" baseline: rainfarm_calibrate.py:76-83 / 96-97 (rainfarm_calibration_data.npy) on a
    DeviceDataset: n indices from np.random.randint(n_samples, size=n) (the global numpy RNG) and their raw mm/h tiles
    (n, 24, nd, nd), a float32 CUDA tensor."""
    if not 1 <= int(n) <= MAX_MEMBERS:
        raise ValueError(f"1 .. {MAX_MEMBERS} members, got {n}")
    return rainfarm.random_tiles(dataset, int(n))


def crps_fixed_ensemble_device(ens, obs, per_position=False):
    """properscoring.crps_ensemble(obs[d], ens, axis=0) for every day d against ONE ensemble (C:193-194).  ens (n, 24, nd, nd) mm/h,
    1 <= n <= 8192, obs (D, 24, nd, nd), numpy or CUDA -> the hourly area means (D, 24), a float32 CUDA tensor; with per_position
    also the CRPS per grid point: (hourly, (D, 24, nd, nd)).  The members must be finite; a NaN observation gives NaN at its grid
    point and in that hour's mean.  Two calls on the same inputs agree bit for bit."""
    es, os_ = _check_days(ens, "ens"), _check_days(obs, "obs")
    if es[2] != os_[2]:
        raise ValueError(f"ens and obs differ in ndomain: {es[2]} and {os_[2]}")
    n, D, nd = es[0], os_[0], es[2]
    if n > MAX_MEMBERS:
        raise ValueError(f"at most {MAX_MEMBERS} members, got {n}")
    if D * NHOURS * nd * nd >= 2 ** 31:
        raise ValueError(f"obs: fewer than 2^31 values per call, got {D * NHOURS * nd * nd}")
    require_gpu()
    lib = _lib.load()
    ens = device_f32(ens, "ens")
    obs = device_f32(obs, "obs").to(ens.device)
    hourly = torch.empty((D, NHOURS), dtype=torch.float32, device=ens.device)
    crps = torch.empty((D, NHOURS, nd, nd), dtype=torch.float32, device=ens.device) if per_position else None
    _lib.check(lib.rdgan_crps_fixed_ensemble(_p(ens), _p(obs), _p(crps), _p(hourly), n, D, nd, _stream(ens)), None,
               "rdgan_crps_fixed_ensemble")
    return (hourly, crps) if per_position else hourly


# ---------------------------------------------------------------------------------------------------------------------------------
# the two generated ensembles, many days, one copy
# ---------------------------------------------------------------------------------------------------------------------------------
def crps_for_days(gen, reals_precip, n_fake_per_real=1000, seed=None, norm_scale=W.NORM_SCALE):
    """The loop C:177-192 for many real days: reals_precip (D, 24, nd, nd) mm/h -> the hourly area-mean CRPS of the generator's
    ensembles, numpy (D, 24).  The body is ensemble.crps_for_day's; the per-day results stay on the device and are copied once.
    Seed rule: with a seed, day d uses the device generator seeded seed + d, and its row equals
    ensemble.crps_for_day(gen, reals_precip[d], n_fake_per_real, seed=seed + d) bit for bit; without one the latent noise comes from
    the global numpy RNG in the reference's order (C:184).  As in crps_for_day the daily sums are taken on the host (:168): a CUDA
    input is copied there once."""
    _check_days(reals_precip, "reals_precip")
    if int(n_fake_per_real) < 1 or int(n_fake_per_real) > MAX_MEMBERS:
        raise ValueError(f"1 .. {MAX_MEMBERS} members per day, got {n_fake_per_real}")
    require_gpu()
    if isinstance(reals_precip, torch.Tensor):
        reals = reals_precip.detach().to(device="cpu", dtype=torch.float32).contiguous()
    else:
        reals = torch.from_numpy(np.ascontiguousarray(reals_precip, dtype=np.float32))
    reals_dev = None
    rows = []
    for d in range(reals.shape[0]):
        real = reals[d]
        dsum = real.sum(0)                                            # reals_dsum, :168
        cond = (dsum / norm_scale).numpy()[..., None]
        ens = ensemble.generate_ensemble_device(gen, cond, int(n_fake_per_real), seed=None if seed is None else int(seed) + d)
        if reals_dev is None:
            reals_dev = reals.to(ens.device)
        scale = (dsum / norm_scale * norm_scale).to(ens.device)       # generated * cond * norm_scale, :186
        scale = scale.unsqueeze(0).expand(W.NHOURS, -1, -1).contiguous()
        rows.append(ensemble.crps_ensemble_device(ens, reals_dev[d], scale).mean(dim=(1, 2)))
    return torch.stack(rows).cpu().numpy()


def rainfarm_crps_for_days(reals_precip, alpha, beta, n_members=1000, seed=None):
    """rainfarm_generate_crps.py:27-35 for many real days: reals_precip (D, 24, nd, nd) mm/h, numpy or CUDA -> the hourly area-mean
    CRPS of n_members RainFARM days per real day, numpy (D, 24).  The body is rainfarm.crps_for_day's, everything on the device, one
    copy at the end.  Seed rule: with a seed, day d draws the members d n_members .. (d + 1) n_members - 1 of the seeded counter
    RNG (downscale_device(first_member=d * n_members)), so no two days share a member and day 0 equals
    rainfarm.crps_for_day(reals_precip[0], alpha, beta, n_members, seed) bit for bit; without one the phases come from the global
    numpy RNG in R's order."""
    shape = _check_days(reals_precip, "reals_precip")
    rainfarm.check_nd(shape[2])
    if int(n_members) < 1 or int(n_members) > MAX_MEMBERS:
        raise ValueError(f"1 .. {MAX_MEMBERS} members per day, got {n_members}")
    require_gpu()
    reals = device_f32(reals_precip, "reals_precip")
    rows = []
    for d in range(shape[0]):
        real = reals[d]
        ens = rainfarm.downscale_device(real.sum(0), alpha, beta, n_members=int(n_members), seed=seed,
                                        first_member=0 if seed is None else d * int(n_members))
        rows.append(ensemble.crps_ensemble_device(ens, real).mean(dim=(1, 2)))
    return torch.stack(rows).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def moments_device(x):
    """(n, mean, variance with ddof = 1) of a 1-D array in fp64 on the device (two passes, fixed order)."""
    xd = _device_f64_vector(x, "x")
    out = torch.empty(3, dtype=torch.float64, device=xd.device)
    _lib.check(_lib.load().rdgan_moments_f64(_p(xd), xd.numel(), _p(out), _stream(xd)), None, "rdgan_moments_f64")
    n, mean, var = out.cpu().tolist()
    return int(n), mean, var


def bootstrap_means_device(x, n_resamples, seed=0, first_resample=0):
    """n_resamples means of len(x) draws with replacement from x -> float64 CUDA tensor.  Resample r = first_resample + j draws
    x[idx], idx = (bits * n) >> 32 with the 32 bits of the counter RNG for (seed, r, draw) (csrc/rdgan_rng.h, stream 7): an entry
    depends on (seed, r) only, so first_resample continues a run exactly, and repeated calls agree bit for bit."""
    if int(n_resamples) < 1 or int(n_resamples) >= 2 ** 31:
        raise ValueError(f"1 .. 2^31 - 1 resamples per call, got {n_resamples}")
    if int(first_resample) < 0:
        raise ValueError("first_resample must be >= 0")
    xd = _device_f64_vector(x, "x")
    out = torch.empty(int(n_resamples), dtype=torch.float64, device=xd.device)
    _lib.check(_lib.load().rdgan_bootstrap_means(_p(xd), xd.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_resample),
                                                 int(n_resamples), _p(out), _stream(xd)), None, "rdgan_bootstrap_means")
    return out


def _stirling_tail(z):
    z2 = z * z
    return (1 / 12 - (1 / 360 - (1 / 1260 - (1 / 1680 - 1 / (1188 * z2)) / z2) / z2) / z2) / z


def _log_beta(a, b):
    """ln B(a, b).  For a large argument lgamma(a) - lgamma(a + b) is taken from the Stirling series directly (the lgamma values
    themselves are ~1e6 at a = 120 000 and their difference would lose ten digits)."""
    if a < b:
        a, b = b, a
    if a < 30.0:
        return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)
    return math.lgamma(b) - (a - 0.5) * math.log1p(b / a) - b * math.log(a + b) + b + _stirling_tail(a) - _stirling_tail(a + b)


def _betacf(a, b, x):
    """continued fraction of the incomplete beta function, modified Lentz"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = 1.0
    d = 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 100000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = 1.0 + aa / c
        c = c if abs(c) > tiny else tiny
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-16:
            return h
    raise ArithmeticError(f"incomplete beta continued fraction did not converge (a={a}, b={b}, x={x})")


def _betainc(a, b, x, xc):
    """regularised incomplete beta function I_x(a, b); xc = 1 - x, passed in so that neither end loses digits"""
    if x <= 0.0:
        return 0.0
    if xc <= 0.0:
        return 1.0
    lnx = math.log1p(-xc) if xc < 0.5 else math.log(x)
    lnxc = math.log1p(-x) if x < 0.5 else math.log(xc)
    front = math.exp(a * lnx + b * lnxc - _log_beta(a, b))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, xc) / b


def t_two_sided_p(t, df):
    """P(|T| >= |t|) for Student's t with df degrees of freedom = I_{df / (df + t^2)}(df / 2, 1 / 2), in fp64 on the host."""
    t, df = float(t), float(df)
    if math.isnan(t) or not df > 0:
        return float("nan")
    t2 = t * t
    if math.isinf(t2):
        return 0.0
    den = df + t2
    return min(1.0, _betainc(0.5 * df, 0.5, df / den, t2 / den))


def ttest_1samp(x, popmean=0.0):
    """scipy.stats.ttest_1samp(x, popmean) of A:14 -> (t, p), two-sided: count, mean and unbiased variance from the device
    (rdgan_moments_f64), t = (mean - popmean) / sqrt(var / n), p = t_two_sided_p(t, n - 1)."""
    n, mean, var = moments_device(x)
    if n < 2:
        return float("nan"), float("nan")
    se = math.sqrt(var / n)
    num = mean - float(popmean)
    t = num / se if se > 0 else (float("nan") if num == 0 else math.copysign(math.inf, num))
    return t, t_two_sided_p(t, n - 1)


def bootstrapped_difference_onesample(x1, perc=1, N=10000, seed=0):
    """A:25-42 with the resampling on the device: np.array([mean(x1), lower, upper]), lower / upper the perc / 100 - perc
    percentiles (np.percentile, the reference's last step) of N means of len(x1) draws with replacement.  The reference draws
    np.random.choice from the global numpy RNG; here the indices come from the counter RNG under `seed`, so a call is reproducible
    and its interval agrees with the reference's to the sampling error of N resamples."""
    if not 0 < perc < 50:
        raise ValueError(f"perc must lie in (0, 50), got {perc}")
    if int(N) < 1:
        raise ValueError(f"N must be >= 1, got {N}")
    means = bootstrap_means_device(x1, int(N), seed=seed).cpu().numpy()
    _, mmean, _ = moments_device(x1)
    upper = np.percentile(means, q=100 - perc)
    lower = np.percentile(means, q=perc)
    return np.array([mmean, lower, upper])


# ---------------------------------------------------------------------------------------------------------------------------------
# the experiment
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class CRPSExperimentResult:
    """Hourly area-mean CRPS per real day, numpy (D, 24): gan (crps_amean_all, C:197), random (crps_baseline_amean_all, C:198),
    rainfarm (crps_amean_all_rainfarm; None when no slopes were given)."""
    gan: np.ndarray
    random: np.ndarray
    rainfarm: Optional[np.ndarray] = None

    def summary(self, perc=1, N=10000, seed=0):
        """The numbers of analyze_crps_results.py: the means under the keys of crps_results.json (A:17-22), "ttest_p" (A:14) and
        "bootstrap" = [mean, lower, upper] (A:45) of (gan - random).flatten()."""
        diff = (self.gan.astype(np.float64) - self.random.astype(np.float64)).ravel()
        return {"gan": float(self.gan.mean(dtype=np.float64)), "random": float(self.random.mean(dtype=np.float64)),
                "rainfarm": None if self.rainfarm is None else float(self.rainfarm.mean(dtype=np.float64)),
                "ttest_p": ttest_1samp(diff)[1], "bootstrap": bootstrapped_difference_onesample(diff, perc=perc, N=N, seed=seed)}


def crps_experiment(gen, reals_precip, climatology, slopes=None, n_fake_per_real=1000, seed=0):
    """C:164-203 and rainfarm_generate_crps.py for the real days reals_precip (D, 24, nd, nd) mm/h: the generator's ensembles
    (crps_for_days), the fixed climatological ensemble `climatology` (n, 24, nd, nd), e.g. climatology_sample(dataset), and with
    slopes = (alpha, beta) RainFARM (rainfarm_crps_for_days, n_fake_per_real members).  Returns a CRPSExperimentResult."""
    shape = _check_days(reals_precip, "reals_precip")
    cs = _check_days(climatology, "climatology")
    if cs[2] != shape[2] or cs[0] > MAX_MEMBERS:
        raise ValueError(f"climatology must have shape (n <= {MAX_MEMBERS}, {NHOURS}, {shape[2]}, {shape[2]}), got {cs}")
    if slopes is not None and len(slopes) != 2:
        raise ValueError("slopes must be (alpha, beta)")
    require_gpu()
    gan = crps_for_days(gen, reals_precip, n_fake_per_real=n_fake_per_real, seed=seed)
    random = crps_fixed_ensemble_device(climatology, reals_precip).cpu().numpy()
    rf = None
    if slopes is not None:
        rf = rainfarm_crps_for_days(reals_precip, float(slopes[0]), float(slopes[1]), n_members=n_fake_per_real, seed=seed)
    return CRPSExperimentResult(gan=gan, random=random, rainfarm=rf)
