"""RainFARM, the paper's baseline (reference rainfarm/*.py, R = rainfarm_temporal_downscaling.py): spectral-slope calibration and
stochastic generation of hourly days from daily sums, on the device (csrc/rdgan_rainfarm.hip.h).

The log-power statistics of the calibration run in fp64 on the device, reduced per frequency class; the straight-line fit
(R:6-19) runs on the host over the classes with the reference's own abscissae, so the points it keeps are R's.  Generation is
fp32 on the device; its phases come from a caller's uniforms (np.random.rand, as R:103 draws them) or from the project's counter
RNG.  No CPU fallback: without a visible MI355X every device entry point raises RdganError."""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._dev import device_f32, ptr as _p, stream as _stream
from .engine import require_gpu
from .ensemble import crps_ensemble_device

NHOURS = 24
ND_SUPPORTED = (8, 16, 24, 32, 48, 64)
N_TCLASS = 13                   # |m| = 0 .. 12 of the 24-point DFT
MAX_N = 1 << 24                 # samples / members per kernel call


def check_nd(nd):
    if int(nd) not in ND_SUPPORTED:
        raise ValueError(f"ndomain {nd} is not covered by the RainFARM kernels {ND_SUPPORTED}")
    return int(nd)


# ---------------------------------------------------------------------------------------------------------------------------------
# host: amplitude table, class abscissae, fit
# ---------------------------------------------------------------------------------------------------------------------------------
def spectral_amplitudes(alpha, beta, nd, ds_t_factor=NHOURS):
    """(24, nd, nd) complex128: R:94-113's sqrt(om^-beta * k_sqr^-alpha/2) with om = 2 pi fftfreq(24) taken as complex (negative
    om, Nyquist included, on numpy's principal branch: phase wrap(-pi beta) / 2), zero on the om = 0 plane and at k = 0."""
    nd = check_nd(nd)
    if ds_t_factor != NHOURS:
        raise ValueError(f"ds_t_factor must be {NHOURS}, got {ds_t_factor}")
    ki = np.fft.fftfreq(nd)
    kj = np.fft.fftfreq(nd)
    k_sqr = ki[:, None] ** 2 + kj[None, :] ** 2
    om = (2 * np.pi * np.fft.fftfreq(ds_t_factor)).astype(complex)
    with np.errstate(all="ignore"):
        fg = np.sqrt((om[:, None, None] ** (-beta)) * k_sqr[None, :, :] ** (-alpha / 2))
    fg[0] = 0
    fg[:, 0, 0] = 0
    assert np.all(np.isfinite(fg))
    return fg


def class_abscissae(nd):
    """(x_spatial (nd/2+1, nd/2+1), x_temporal (13,)): log of R's wavenumber for every class, by R's own float64 expressions
    (R:68-72 and R:39-41), so every point of a class has exactly the x R gives it.  Class (0, 0) and m = 0 are -inf (never kept)."""
    nd = check_nd(nd)
    h = nd // 2 + 1
    ki = np.fft.fftfreq(nd)
    k = np.sqrt(ki[:h, None] ** 2 + ki[None, :h] ** 2)     # index |a| of fftfreq: +|a|/nd, or -1/2 at nd/2 (same square)
    om = 2 * np.pi * np.fft.fftfreq(NHOURS)
    om = np.sqrt(om ** 2)
    with np.errstate(divide="ignore"):
        return np.log(k), np.log(om[:N_TCLASS])


def fit_classes(x, counts, sums):
    """_log_slope (R:6-19) over classes: x the class abscissae, counts the kept points per class, sums their summed log power.
    Trims 1/6 of [min x, max x] over the populated classes at each end (inclusive bounds, R's float expressions) and returns minus
    the least-squares slope of the expanded points, in closed form (centred sums, fp64)."""
    x = np.asarray(x, dtype=np.float64).ravel()
    cnt = np.asarray(counts, dtype=np.float64).ravel()
    s = np.asarray(sums, dtype=np.float64).ravel()
    present = cnt > 0
    if not present.any():
        raise ValueError("no kept points: every series / plane is dry or constant")
    lk_min = x[present].min()
    lk_max = x[present].max()
    lk_range = lk_max - lk_min
    lk_min += (1 / 6) * lk_range
    lk_max -= (1 / 6) * lk_range
    sel = present & (lk_min <= x) & (x <= lk_max)
    xs, w, ys = x[sel], cnt[sel], s[sel]
    n = w.sum()
    xbar = (w * xs).sum() / n
    ybar = ys.sum() / n
    sxx = (w * (xs - xbar) ** 2).sum()
    if not sxx > 0:
        raise ValueError("fewer than two distinct wavenumbers survive the trim: the slope is undefined")
    return -((xs - xbar) * (ys - w * ybar)).sum() / sxx


# ---------------------------------------------------------------------------------------------------------------------------------
# device: calibration
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class SlopeStatistics:
    """Per-class statistics of a calibration batch.  spatial_* are (nd/2+1, nd/2+1), indexed by (|a|, |b|) of the integer fftfreq
    indices; temporal_* are (13,), indexed by |m|.  counts: kept points (power > 0, frequency != 0); sums: fp64 sum of log power.
    alpha / beta: the fits (estimate_alpha / estimate_beta)."""
    spatial_counts: np.ndarray
    spatial_sums: np.ndarray
    temporal_counts: np.ndarray
    temporal_sums: np.ndarray
    alpha: float
    beta: float


def slope_statistics(p_samples):
    """p_samples (n, 24, nd, nd), numpy or CUDA, mm/h -> SlopeStatistics.  The DFTs, logs and class sums run on the device in fp64
    (R:22-81 on fp32 inputs); only the fits run on the host."""
    x = p_samples
    shape = tuple(x.shape)
    if len(shape) != 4 or shape[1] != NHOURS or shape[2] != shape[3]:
        raise ValueError(f"p_samples must have shape (n, {NHOURS}, nd, nd), got {shape}")
    nd = check_nd(shape[2])
    n = shape[0]
    if not 1 <= n <= MAX_N:
        raise ValueError(f"p_samples: 1 .. {MAX_N} samples per call, got {n}")
    require_gpu()
    lib = _lib.load()
    x = device_f32(x, "p_samples")
    if x.data_ptr() % 16:
        x = x.clone()
    nc = int(lib.rdgan_rainfarm_classes(nd))
    counts = torch.empty(nc, dtype=torch.int64, device=x.device)
    sums = torch.empty(nc, dtype=torch.float64, device=x.device)
    wsb = int(lib.rdgan_rainfarm_stats_workspace_bytes(n, nd))
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    _lib.check(lib.rdgan_rainfarm_slope_stats(_p(x), n, nd, _p(counts), _p(sums), _p(ws), wsb, _stream(x)), None,
               "rdgan_rainfarm_slope_stats")
    c = counts.cpu().numpy()
    s = sums.cpu().numpy()
    h = nd // 2 + 1
    xs, xt = class_abscissae(nd)
    sc, ss = c[:h * h].reshape(h, h), s[:h * h].reshape(h, h)
    tc, ts = c[h * h:], s[h * h:]
    return SlopeStatistics(spatial_counts=sc, spatial_sums=ss, temporal_counts=tc, temporal_sums=ts,
                           alpha=float(fit_classes(xs, sc, ss)), beta=float(fit_classes(xt, tc, ts)))


def estimate_slopes(p_samples):
    """(alpha, beta) = (estimate_alpha, estimate_beta) of R for p_samples (n, 24, nd, nd), from one device pass."""
    st = slope_statistics(p_samples)
    return st.alpha, st.beta


def estimate_alpha(p_samples):
    """R:54-81: spatial spectral slope of p_samples (n, 24, nd, nd)."""
    return slope_statistics(p_samples).alpha


def estimate_beta(p_samples):
    """R:22-51: temporal spectral slope of p_samples (n, 24, nd, nd)."""
    return slope_statistics(p_samples).beta


def random_tiles(dataset, n):
    """rainfarm_calibrate.py:76-81 on a DeviceDataset: n indices drawn with np.random.randint(n_samples, size=n) (:76, the global
    numpy RNG) and their raw mm/h tiles (n, 24, nd, nd) gathered from dataset.data on the device (:80-81)."""
    if dataset.indices is None:
        raise ValueError("dataset has no valid-tile indices (set_indices)")
    nd = check_nd(dataset.ndomain)
    dev = dataset.data.device
    ar = torch.arange(nd, device=dev)
    hours = torch.arange(NHOURS, device=dev)
    ixs = np.random.randint(dataset.n_samples, size=n)
    idx = dataset.indices[torch.from_numpy(ixs).to(dev)].long()
    days, ys, xs = idx[:, 0], idx[:, 1:2] + ar, idx[:, 2:3] + ar
    batch = dataset.data[days[:, None, None, None], hours[None, :, None, None], ys[:, None, :, None], xs[:, None, None, :]]
    return batch.contiguous()


def calibrate(dataset, n_calib=5000, n_repeat=10):
    """rainfarm_calibrate.py:67-93 on a DeviceDataset: n_repeat times, n_calib indices drawn with
    np.random.randint(n_samples, size=n_calib) (:76, the global numpy RNG), their raw mm/h tiles (n_calib, 24, nd, nd) gathered
    from dataset.data on the device (:80-81), and (alpha, beta) estimated.  Returns the list of (alpha, beta)."""
    if dataset.indices is None:
        raise ValueError("dataset has no valid-tile indices (set_indices)")
    check_nd(dataset.ndomain)
    return [estimate_slopes(random_tiles(dataset, n_calib)) for _ in range(n_repeat)]


# ---------------------------------------------------------------------------------------------------------------------------------
# device: generation
# ---------------------------------------------------------------------------------------------------------------------------------
def downscale_device(precip, alpha, beta, n_members=None, seed=None, uniforms=None, first_member=0):
    """downscale_spatiotemporal (R:84-125) for many members at once -> (n, 24, nd, nd) float32 CUDA tensor, hourly mm/h whose hourly
    sums are precip.  precip (nd, nd) is used for all n_members members, precip (n, nd, nd) gives one member each.
    Phases: uniforms (n, 24, nd, nd) float32 or float64 (numpy or CUDA), e.g. np.random.rand draws; else with a seed the counter
    RNG, members first_member .. first_member + n - 1 (a member's phases depend on (seed, member) only); else n draws of
    np.random.rand(24, nd, nd) from the global numpy RNG, in R's order."""
    pr = precip
    shape = tuple(pr.shape)
    if len(shape) == 2:
        per_member = False
        if n_members is None:
            n_members = 1 if uniforms is None else int(uniforms.shape[0])
    elif len(shape) == 3:
        per_member = True
        if n_members is not None and int(n_members) != shape[0]:
            raise ValueError(f"n_members {n_members} != the {shape[0]} precip fields")
        n_members = shape[0]
    else:
        raise ValueError(f"precip must have shape (nd, nd) or (n, nd, nd), got {shape}")
    if shape[-1] != shape[-2]:
        raise ValueError(f"precip fields must be square, got {shape}")
    nd = check_nd(shape[-1])
    n = int(n_members)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"1 .. {MAX_N} members per call, got {n}")
    if int(first_member) < 0:
        raise ValueError("first_member must be >= 0")
    require_gpu()
    lib = _lib.load()
    pr = device_f32(pr, "precip")
    dev = pr.device
    amp = torch.from_numpy(spectral_amplitudes(alpha, beta, nd).astype(np.complex64).view(np.float32)).to(dev)
    u = None
    fp64 = 0
    if uniforms is None and seed is None:
        uniforms = np.random.rand(n, NHOURS, nd, nd)
    if uniforms is not None:
        if tuple(uniforms.shape) != (n, NHOURS, nd, nd):
            raise ValueError(f"uniforms must have shape ({n}, {NHOURS}, {nd}, {nd}), got {tuple(uniforms.shape)}")
        u = uniforms if isinstance(uniforms, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uniforms))
        if u.dtype not in (torch.float32, torch.float64):
            u = u.to(torch.float64)
        fp64 = 1 if u.dtype == torch.float64 else 0
        u = u.to(dev).contiguous()
    out = torch.empty((n, NHOURS, nd, nd), dtype=torch.float32, device=dev)
    wsb = int(lib.rdgan_rainfarm_gen_workspace_bytes(n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    _lib.check(lib.rdgan_rainfarm_generate(_p(amp), _p(pr), 1 if per_member else 0, _p(u), fp64,
                                           int(seed or 0) & 0xFFFFFFFFFFFFFFFF, int(first_member), _p(out), n, nd, _p(ws), wsb,
                                           _stream(out)), None, "rdgan_rainfarm_generate")
    return out


def downscale_spatiotemporal(precip, alpha, beta, ds_t_factor):
    """Drop-in for R:84-125: precip (nd, nd) daily sum -> (24, nd, nd) numpy float32 day.  Draws np.random.rand(24, nd, nd) from the
    global numpy RNG exactly as R:103 does, so np.random.seed(s) reproduces R's day to fp32 accuracy."""
    if ds_t_factor != NHOURS:
        raise ValueError(f"ds_t_factor must be {NHOURS}, got {ds_t_factor}")
    pr = np.asarray(precip)
    if pr.ndim != 2 or pr.shape[0] != pr.shape[1]:
        raise ValueError(f"precip must have shape (nd, nd), got {pr.shape}")
    check_nd(pr.shape[0])
    require_gpu()
    u = np.random.rand(NHOURS, pr.shape[0], pr.shape[1])
    return downscale_device(pr, alpha, beta, uniforms=u[None]).cpu().numpy()[0]


def generate_one_per_day(real_precip, alpha, beta, seed=None):
    """rainfarm_generate.py:18-23: one RainFARM day per real day from its daily sum.  real_precip (n, 24, nd, nd) mm/h, numpy or
    CUDA -> (n, 24, nd, nd) CUDA tensor, the layout spectral.lsd_evaluation takes.  Phases from the global numpy RNG in R's order,
    or from the counter RNG (member i = day i) when a seed is given."""
    real = _check_days(real_precip)
    require_gpu()
    real = device_f32(real, "real_precip")
    return downscale_device(real.sum(1), alpha, beta, seed=seed)


def crps_for_day(real_precip, alpha, beta, n_members=1000, seed=None):
    """rainfarm_generate_crps.py:27-33: n_members RainFARM days from one real day's daily sum, their CRPS against the real hourly
    fields per grid point (already mm/h: no scale), the area mean per hour.  real_precip (24, nd, nd) -> numpy (24,)."""
    shape = tuple(real_precip.shape)
    if len(shape) != 3 or shape[0] != NHOURS or shape[1] != shape[2]:
        raise ValueError(f"real_precip must have shape ({NHOURS}, nd, nd), got {shape}")
    check_nd(shape[1])
    require_gpu()
    real = device_f32(real_precip, "real_precip")
    ens = downscale_device(real.sum(0), alpha, beta, n_members=n_members, seed=seed)
    crps = crps_ensemble_device(ens, real)
    return crps.mean(dim=(1, 2)).cpu().numpy()


def _check_days(real_precip):
    shape = tuple(real_precip.shape)
    if len(shape) != 4 or shape[1] != NHOURS or shape[2] != shape[3]:
        raise ValueError(f"real_precip must have shape (n, {NHOURS}, nd, nd), got {shape}")
    check_nd(shape[2])
    return real_precip
