"""Log-spectral distance on the device (reference log_spectral_distance.py): radial power spectra of the hourly fields and the
distance of every ordered pair of them, reduced to a histogram and moments so that the N x M distances never need to exist.
No CPU fallback: without a visible MI355X every entry point raises RdganError."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._dev import device_f32, ptr as _p, stream as _stream
from .engine import require_gpu

DEFAULT_BINS = 512
DEFAULT_RANGE = (0.0, 20.0)          # dB; the evaluation's distances lie well inside (the reference plots a KDE of them)
MATRIX_LIMIT_BYTES = 1 << 31         # matrix=True refuses an N x M fp32 output above 2 GiB: use the histogram instead


def spectra_bins(nd):
    """K, the number of radial bins the spectrum of an (nd, nd) field keeps (nd 8/16/24/32/48/64: 3/9/15/20/32/43)."""
    k = _lib.load().rdgan_spectra_bins(int(nd))
    if k < 1:
        raise ValueError(f"ndomain {nd} is not covered by the spectra kernel (8, 16, 24, 32, 48 or 64)")
    return k


def radial_spectra_device(fields, log=False):
    """fields (N, nd, nd) float32 CUDA -> (N, K): compute_radial_spectrum (reference :59-65), the mean of |fftshift(fft2)|^2 over
    the radial bins 1..K; log=True returns 10 log10 of it (dB, -inf for a bin without power)."""
    require_gpu()
    lib = _lib.load()
    if not (isinstance(fields, torch.Tensor) and fields.is_cuda and fields.dtype == torch.float32):
        raise ValueError("fields: expected a float32 CUDA tensor")
    if fields.dim() != 3 or fields.shape[1] != fields.shape[2]:
        raise ValueError(f"fields: expected shape (N, nd, nd), got {tuple(fields.shape)}")
    fields = fields.contiguous()
    n, nd = fields.shape[0], fields.shape[1]
    out = torch.empty((n, spectra_bins(nd)), dtype=torch.float32, device=fields.device)
    if n == 0:
        return out
    _lib.check(lib.rdgan_radial_spectra(_p(fields), _p(out), n, nd, 1 if log else 0, _stream(fields)), None,
               "rdgan_radial_spectra")
    return out


@dataclass
class LSDResult:
    """Distribution of the pairwise log-spectral distances.  hist[b] counts the finite d with
    b = int(floor((d - lo) * float32(bins) / (hi - lo))) in float32 arithmetic, clamped to bins - 1; under / over count d < lo
    and d >= hi; nan and inf the pairs of two dry spectra and of one; total = every pair counted.  mean, std (population), min
    and max are over the finite distances (NaN when there are none)."""
    hist: np.ndarray
    edges: np.ndarray
    total: int
    nan: int
    inf: int
    under: int
    over: int
    count: int
    mean: float
    std: float
    min: float
    max: float
    matrix: Optional[torch.Tensor] = None


def log_spectral_distance_device(spec_a, spec_b=None, *, bins=DEFAULT_BINS, range=DEFAULT_RANGE, exclude_diagonal=True,
                                 matrix=False):
    """log_spectral_distance (reference :68-77) of every ordered pair (spec_a[i], spec_b[j]), as compute_dists (:104-118) pairs
    them; spec_a (N, K) and spec_b (M, K) are log-spectra in dB (radial_spectra_device(..., log=True)), spec_b=None compares
    spec_a with itself.  exclude_diagonal leaves the pairs i == j out (the reference skips and then removes them, :123-130).
    matrix=True also returns the (N, M) distances (0 on an excluded diagonal) and raises ValueError above MATRIX_LIMIT_BYTES."""
    require_gpu()
    lib = _lib.load()
    a = device_f32(spec_a, "spec_a")
    b = a if spec_b is None else device_f32(spec_b, "spec_b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"spec_a (N, K) and spec_b (M, K) expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    if b.device != a.device:
        raise ValueError("spec_a and spec_b must be on the same device")
    n, k = a.shape
    m = b.shape[0]
    lo, hi = (float(np.float32(r)) for r in range)
    bins = int(bins)
    dev = a.device
    dist = None
    if matrix:
        nbytes = 4 * n * m
        if nbytes > MATRIX_LIMIT_BYTES:
            raise ValueError(f"matrix=True: a {n} x {m} fp32 matrix is {nbytes} bytes, above MATRIX_LIMIT_BYTES = "
                             f"{MATRIX_LIMIT_BYTES}; use the histogram and moments, or fewer rows per call")
        dist = torch.empty((n, m), dtype=torch.float32, device=dev)
    hist = torch.empty(bins + 4, dtype=torch.int64, device=dev)
    moments = torch.empty(5, dtype=torch.float64, device=dev)
    wsb = int(lib.rdgan_lsd_workspace_bytes(n, m))
    if wsb < 0:
        raise ValueError(f"spec_a / spec_b: {n} x {m} pairs exceed the kernel's limits (rows <= 2^22)")
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.rdgan_lsd_pairwise(_p(a), _p(b), n, m, k, 1 if exclude_diagonal else 0, _p(dist), _p(hist), bins, lo, hi,
                                      _p(moments), _p(ws), wsb, _stream(a)), None, "rdgan_lsd_pairwise")
    h = hist.cpu().numpy()
    cnt, s, sq, mn, mx = moments.cpu().numpy().tolist()
    count = int(cnt)
    mean = s / count if count else float("nan")
    std = float(np.sqrt(max(sq / count - mean * mean, 0.0))) if count else float("nan")
    return LSDResult(hist=h[:bins], edges=np.linspace(lo, hi, bins + 1), total=int(h.sum()), under=int(h[bins]),
                     over=int(h[bins + 1]), nan=int(h[bins + 2]), inf=int(h[bins + 3]), count=count, mean=mean, std=std,
                     min=mn if count else float("nan"), max=mx if count else float("nan"), matrix=dist)


def lsd_evaluation(real_precip, generated_precip, **hist_kw):
    """The reference's three GAN comparisons (log_spectral_distance.py:88-130): real_precip and generated_precip (n, 24, nd, nd)
    mm/h, host or device, flattened to (24 n, nd, nd) with the hour fastest; returns {"real": real vs real, "gen": generated vs
    generated, "gen_real": generated (rows) vs real (columns)} as LSDResult, the diagonal excluded in all three."""
    require_gpu()
    real = device_f32(real_precip, "real_precip")
    gen = device_f32(generated_precip, "generated_precip")
    if real.dim() != 4 or tuple(real.shape) != tuple(gen.shape) or real.shape[2] != real.shape[3]:
        raise ValueError(f"real and generated precipitation of one shape (n, 24, nd, nd) expected, got {tuple(real.shape)} "
                         f"and {tuple(gen.shape)}")
    nd = real.shape[2]
    s_real = radial_spectra_device(real.reshape(-1, nd, nd), log=True)
    s_gen = radial_spectra_device(gen.reshape(-1, nd, nd), log=True)
    return {"real": log_spectral_distance_device(s_real, **hist_kw),
            "gen": log_spectral_distance_device(s_gen, **hist_kw),
            "gen_real": log_spectral_distance_device(s_gen, s_real, **hist_kw)}
