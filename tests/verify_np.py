"""numpy restatement of the verification of field ensembles (pr_disagg_radar_gan_amd/verification.py, csrc/rdgan_verify.hip.h), written
from the definitions and not from the product code: the state (exceed, below, equal, bad), the tie-breaking ranks with the hash of
csrc/rdgan_rng.h restated, the reliability and Brier sums, and the FSS sums by cumulative sums.  int64 and fp64 throughout."""
import numpy as np

NHOURS = 24
STREAM_VERIFY = 8
M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def make_key(seed, stream):
    seed = int(seed)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    return (mix32(lo ^ mix32(hi ^ np.uint64(0x9E3779B9))) + np.uint64((stream * 0x85EBCA6B) & 0xFFFFFFFF)) & M32


def member_key(base, member):
    m = np.asarray(member, dtype=np.uint64)
    return mix32(base ^ mix32((m & M32) ^ mix32((m >> np.uint64(32)) ^ np.uint64(0x9E3779B9))))


def bits(key, idx):
    return mix32(mix32(np.uint64(idx)) ^ key)


def b24(seed, p):
    """the 24 random bits of position p (64-bit index in the whole array)"""
    return (bits(member_key(make_key(seed, STREAM_VERIFY), p), 0) >> np.uint64(8)).astype(np.int64)


def thresholds_f32(thresholds):
    return np.asarray(thresholds, dtype=np.float64).astype(np.float32)


def state(members, obs, thresholds):
    """members (S, *shape), obs (*shape) -> (exceed (T, *shape) int32, below, equal (*shape) int32, bad (*shape) uint8)"""
    x, o, thr = np.asarray(members, dtype=np.float32), np.asarray(obs, dtype=np.float32), thresholds_f32(thresholds)
    assert x.shape[1:] == o.shape
    with np.errstate(invalid="ignore"):
        exceed = np.stack([(x > t).sum(axis=0) for t in thr]).astype(np.int32)
        below = (x < o[None]).sum(axis=0).astype(np.int32)
        equal = (x == o[None]).sum(axis=0).astype(np.int32)
    bad = (np.isnan(o) | np.isnan(x).any(axis=0)).astype(np.uint8)
    return exceed, below, equal, bad


def add_states(a, b):
    return a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] | b[3]


def hours(shape):
    """the hour of every position of an array of shape ([D,] 24, ny, nx), flat"""
    plane = shape[-2] * shape[-1]
    p = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (p // plane) % NHOURS


def ranks(below, equal, seed, first=0):
    """flat int64 ranks; first: the index of the array's first position in the whole array"""
    b, e = below.reshape(-1).astype(np.int64), equal.reshape(-1).astype(np.int64)
    p = first + np.arange(b.shape[0], dtype=np.int64)
    return b + ((b24(seed, p) * (e + 1)) >> 24)


def reduce(obs, st, n_members, thresholds, n_bins, seed):
    """-> (rank_hist (24, S + 1), reliability (T, 24, n_bins, 3), brier_sums (T, 24, 4)) int64"""
    exceed, below, equal, bad = st
    o, thr, S = np.asarray(obs, dtype=np.float32), thresholds_f32(thresholds), int(n_members)
    T = len(thr)
    hr = hours(o.shape)
    valid = (bad.reshape(-1) == 0) & ~np.isnan(o.reshape(-1))
    r = ranks(below, equal, seed)
    rank_hist = np.zeros((NHOURS, S + 1), dtype=np.int64)
    np.add.at(rank_hist, (hr[valid], r[valid]), 1)
    rel = np.zeros((T, NHOURS, n_bins, 3), dtype=np.int64)
    brier = np.zeros((T, NHOURS, 4), dtype=np.int64)
    for t in range(T):
        c = exceed[t].reshape(-1).astype(np.int64)[valid]
        with np.errstate(invalid="ignore"):
            e = (o.reshape(-1) > thr[t]).astype(np.int64)[valid]
        h = hr[valid]
        b = (c * n_bins) // (S + 1)
        for k, v in enumerate((np.ones_like(c), e, c)):
            np.add.at(rel[t, :, :, k], (h, b), v)
        for k, v in enumerate((np.ones_like(c), e, c * e, c * c)):
            np.add.at(brier[t, :, k], h, v)
    return rank_hist, rel, brier


def box_sums(a, w):
    """a (..., ny, nx) int64 -> the sums over the w x w box centred at each pixel, clipped at the edge, by cumulative sums"""
    a = np.asarray(a, dtype=np.int64)
    ny, nx, r = a.shape[-2], a.shape[-1], w // 2
    sat = np.zeros(a.shape[:-2] + (ny + 1, nx + 1), dtype=np.int64)
    sat[..., 1:, 1:] = a.cumsum(axis=-2).cumsum(axis=-1)
    y0, y1 = np.maximum(np.arange(ny) - r, 0), np.minimum(np.arange(ny) + r, ny - 1) + 1
    x0, x1 = np.maximum(np.arange(nx) - r, 0), np.minimum(np.arange(nx) + r, nx - 1) + 1
    return (sat[..., y1[:, None], x1[None, :]] - sat[..., y0[:, None], x1[None, :]] - sat[..., y1[:, None], x0[None, :]]
            + sat[..., y0[:, None], x0[None, :]])


def fss_sums(obs, exceed, bad, n_members, thresholds, widths):
    """obs ([D,] 24, ny, nx) -> (T, W, 24, 2) float64 = (num, den) summed over days and pixels"""
    o, thr, S = np.asarray(obs, dtype=np.float32), thresholds_f32(thresholds), int(n_members)
    ny, nx = o.shape[-2:]
    o = o.reshape(-1, NHOURS, ny, nx)
    ok = (bad.reshape(o.shape) == 0) & ~np.isnan(o)
    out = np.zeros((len(thr), len(widths), NHOURS, 2), dtype=np.float64)
    for t in range(len(thr)):
        C = np.where(ok, exceed[t].reshape(o.shape).astype(np.int64), 0)
        with np.errstate(invalid="ignore"):
            E = np.where(ok, (o > thr[t]).astype(np.int64), 0)
        for i, w in enumerate(widths):
            bc, be = box_sums(C, int(w)), S * box_sums(E, int(w))
            num, den = (bc - be) ** 2, bc ** 2 + be ** 2
            assert int(den.sum()) < 2 ** 53
            out[t, i, :, 0] = num.sum(axis=(0, 2, 3)).astype(np.float64)
            out[t, i, :, 1] = den.sum(axis=(0, 2, 3)).astype(np.float64)
    return out


def fss(sums):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sums[..., 1] > 0, 1.0 - sums[..., 0] / sums[..., 1], np.nan)


def brier_score(brier, n_members):
    """(BS, base rate, BSS) from (N, sum e, sum c e, sum c^2) along the last axis"""
    b = np.asarray(brier, dtype=np.float64)
    n, se, sce, sc2 = (b[..., k] for k in range(4))
    S = float(n_members)
    with np.errstate(divide="ignore", invalid="ignore"):
        bs = (sc2 - 2 * S * sce + S * S * se) / (S * S * n)
        base = se / n
        bss = np.where(base * (1 - base) > 0, 1 - bs / (base * (1 - base)), np.nan)
    return bs, base, bss


def verify(members, obs, thresholds, widths, n_bins, seed):
    """everything at once -> (state, rank_hist, reliability, brier_sums, fss_sums)"""
    st = state(members, obs, thresholds)
    S = np.asarray(members).shape[0]
    return (st,) + reduce(obs, st, S, thresholds, n_bins, seed) + (fss_sums(obs, st[0], st[3], S, thresholds, widths),)
