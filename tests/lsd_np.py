"""fp64 numpy restatement of the log-spectral distance, written from its definition, for the tests.

Radial bins about the centre ((nd-1)/2, (nd-1)/2) of the fftshifted spectrum: pixel (i, j) has 2 r = sqrt(p^2 + q^2) with
p = 2 j - (nd-1), q = 2 i - (nd-1) odd, so floor(r) = isqrt((p^2 + q^2) // 4) exactly.  Bins 1..K are kept, K = max bin - 1."""
import numpy as np

K_TABLE = {8: 3, 16: 9, 24: 15, 32: 20, 48: 32, 64: 43}


def bin_map(nd):
    c = 2 * np.arange(nd) - (nd - 1)
    s = (c[:, None] ** 2 + c[None, :] ** 2) // 4
    b = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    b -= (b * b > s)                        # exact integer square root (the float guess is at most one off here)
    b += ((b + 1) * (b + 1) <= s)
    return b


def n_bins(nd):
    return int(bin_map(nd).max()) - 1


def radial_spectrum(x):
    """(nd, nd) -> (K,) mean of |fftshift(fft2(x))|^2 over radial bins 1..K, in fp64."""
    nd = x.shape[-1]
    P = np.abs(np.fft.fftshift(np.fft.fft2(np.asarray(x, dtype=np.float64)))) ** 2
    b = bin_map(nd)
    return np.array([P[b == k].mean() for k in range(1, n_bins(nd) + 1)])


def radial_spectra(fields):
    return np.array([radial_spectrum(f) for f in fields])


def to_db(spec):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(spec, dtype=np.float64))


def lsd_matrix_db(la, lb, exclude_diagonal=True):
    """la (N, K), lb (M, K) log-spectra in dB -> (N, M) sqrt(sum_k (la_i - lb_j)^2) / K; NaN for two empty spectra, +inf for
    one; 0 on the diagonal when it is excluded (the reference never writes it)."""
    la = np.asarray(la, dtype=np.float64)
    lb = np.asarray(lb, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(((la[:, None, :] - lb[None, :, :]) ** 2).sum(-1)) / la.shape[1]
    if exclude_diagonal:
        n = min(d.shape)
        d[np.arange(n), np.arange(n)] = 0.0
    return d


def lsd_matrix(spec_a, spec_b, exclude_diagonal=True):
    return lsd_matrix_db(to_db(spec_a), to_db(spec_b), exclude_diagonal)


def hist_rule(d, nbins, lo, hi):
    """The documented fp32 bin rule applied to fp32 distances d: (bins, under, over, nan, inf)."""
    d = np.asarray(d, dtype=np.float32).ravel()
    lo32, hi32 = np.float32(lo), np.float32(hi)
    scale = np.float32(nbins) / (hi32 - lo32)
    nan = np.isnan(d)
    inf = np.isinf(d)
    fin = d[~nan & ~inf]
    under = fin < lo32
    over = fin >= hi32
    mid = fin[~under & ~over]
    b = np.minimum(np.floor((mid - lo32) * scale).astype(np.int64), nbins - 1)
    return (np.bincount(b, minlength=nbins).astype(np.int64), int(under.sum()), int(over.sum()), int(nan.sum()), int(inf.sum()))
