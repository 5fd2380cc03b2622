"""fp64 numpy restatement of RainFARM, written from its definition, for the tests.

Calibration: log power of the 2-D DFT of every hour plane and of the 24-point DFT of every pixel series; a point is kept when its
power is > 0 and its frequency is not 0; per class ((|a|, |b|) of the integer fftfreq indices, or |m|) the count and the sum of the
log powers; the slope is minus the least-squares slope of log power on log wavenumber over the kept points whose log wavenumber lies
in the middle 2/3 of its range (bounds included).  Generation: g = Re ifftn(A e^{2 pi i u}), z = g / std(g) (population),
out = exp(z) precip / sum_t exp(z)."""
import numpy as np

NHOURS = 24


def class_index(nd):
    """(nd,) |integer fftfreq index| of every DFT position"""
    i = np.arange(nd)
    return np.minimum(i, nd - i)


def class_statistics(p):
    """p (n, 24, nd, nd) -> (spatial counts (h, h), spatial sums (h, h), temporal counts (13,), temporal sums (13,)), h = nd/2 + 1"""
    p = np.asarray(p, dtype=np.float64)
    nd = p.shape[-1]
    h = nd // 2 + 1
    ci = class_index(nd)
    cls = (ci[:, None] * h + ci[None, :]).ravel()
    P = np.abs(np.fft.fft2(p)) ** 2                                   # (n, 24, nd, nd)
    keep = P > 0
    keep[..., 0, 0] = False
    lp = np.zeros_like(P)
    lp[keep] = np.log(P[keep])
    full = np.broadcast_to(cls.reshape(nd, nd), P.shape)
    sc = np.bincount(full[keep], minlength=h * h).reshape(h, h)
    ss = np.bincount(full[keep], weights=lp[keep], minlength=h * h).reshape(h, h)
    Pt = np.abs(np.fft.fft(p, axis=1)) ** 2
    keep_t = Pt > 0
    keep_t[:, 0] = False
    lpt = np.zeros_like(Pt)
    lpt[keep_t] = np.log(Pt[keep_t])
    m = np.broadcast_to(class_index(NHOURS)[None, :, None, None], Pt.shape)
    tc = np.bincount(m[keep_t], minlength=13)
    ts = np.bincount(m[keep_t], weights=lpt[keep_t], minlength=13)
    return sc, ss, tc, ts


def abscissae(nd):
    """log wavenumber per class: log sqrt((|a|/nd)^2 + (|b|/nd)^2) and log(2 pi |m| / 24), as float64 numpy computes them"""
    h = nd // 2 + 1
    f = np.fft.fftfreq(nd)[:h]
    om = 2 * np.pi * np.fft.fftfreq(NHOURS)
    with np.errstate(divide="ignore"):
        return np.log(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)), np.log(np.sqrt(om ** 2)[:13])


def fit(x, counts, sums):
    """minus the least-squares slope over the expanded points of the populated classes in the trimmed range"""
    x, c, s = (np.asarray(a, dtype=np.float64).ravel() for a in (x, counts, sums))
    pres = c > 0
    lo, hi = x[pres].min(), x[pres].max()
    r = hi - lo
    lo, hi = lo + r / 6, hi - r / 6
    sel = pres & (x >= lo) & (x <= hi)
    x, c, s = x[sel], c[sel], s[sel]
    n = c.sum()
    xm = (c * x).sum() / n
    ym = s.sum() / n
    return -((x - xm) * (s - c * ym)).sum() / (c * (x - xm) ** 2).sum()


def slopes(p):
    """(alpha, beta) of a calibration batch"""
    nd = np.asarray(p).shape[-1]
    sc, ss, tc, ts = class_statistics(p)
    xs, xt = abscissae(nd)
    return fit(xs, sc, ss), fit(xt, tc, ts)


def expand_points(p):
    """every kept point as (x, log power), spatial and temporal, for a direct np.polyfit"""
    p = np.asarray(p, dtype=np.float64)
    nd = p.shape[-1]
    xs, xt = abscissae(nd)
    ci = class_index(nd)
    P = np.abs(np.fft.fft2(p)) ** 2
    keep = P > 0
    keep[..., 0, 0] = False
    xsf = np.broadcast_to(xs[ci[:, None], ci[None, :]], P.shape)
    Pt = np.abs(np.fft.fft(p, axis=1)) ** 2
    keep_t = Pt > 0
    keep_t[:, 0] = False
    xtf = np.broadcast_to(xt[class_index(NHOURS)][None, :, None, None], Pt.shape)
    return (xsf[keep], np.log(P[keep])), (xtf[keep_t], np.log(Pt[keep_t]))


def amplitudes(alpha, beta, nd):
    """closed form of the (24, nd, nd) amplitude table: |om|^(-beta/2) k^(-alpha/2), with the phase wrap(-pi beta) / 2 where om < 0
    (om = 2 pi fftfreq(24), the Nyquist -pi included); 0 where om = 0 or k = 0"""
    f = np.fft.fftfreq(nd)
    k = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    om = 2 * np.pi * np.fft.fftfreq(NHOURS)
    phase = np.angle(np.exp(-1j * np.pi * beta)) / 2                 # wrap(-pi beta) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.abs(om)[:, None, None] ** (-beta / 2) * k[None] ** (-alpha / 2)
        a = mag * np.where(om < 0, np.exp(1j * phase), 1.0)[:, None, None]
    a[0] = 0
    a[:, 0, 0] = 0
    return a


def generate(precip, amp, u):
    """precip (nd, nd) or (n, nd, nd), amp (24, nd, nd) complex, u (n, 24, nd, nd) -> (n, 24, nd, nd) fp64"""
    u = np.asarray(u, dtype=np.float64)
    g = np.fft.ifftn(amp[None] * np.exp(2j * np.pi * u), axes=(1, 2, 3)).real
    g /= g.std(axis=(1, 2, 3), keepdims=True)
    r = np.exp(g)
    pr = np.asarray(precip, dtype=np.float64)
    pr = pr[None] if pr.ndim == 2 else pr
    return r * pr[:, None] / r.sum(axis=1, keepdims=True)


def crps_ensemble(obs, ens):
    """properscoring.crps_ensemble(obs, ens, axis=0) in fp64: mean |x - y| - 0.5 mean |x - x'|"""
    ens = np.asarray(ens, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    t1 = np.abs(ens - obs[None]).mean(0)
    s = np.sort(ens, axis=0)
    n = ens.shape[0]
    w = (2 * np.arange(1, n + 1) - n - 1).reshape((n,) + (1,) * (ens.ndim - 1))
    t2 = (w * s).sum(0) / (n * n)                                   # 0.5 mean |x - x'| = sum_i (2i - n - 1) x_(i) / n^2
    return t1 - t2
