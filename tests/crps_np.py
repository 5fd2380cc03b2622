"""fp64 numpy mirrors of the CRPS experiment's kernels, written from their definitions, for the tests.

Fixed-ensemble CRPS by the sorted-prefix identity: with the members sorted, P_k the sum of the k smallest and k = #{x_i <= y},
mean_i |x_i - y| = (y (2k - n) - 2 P_k + P_n) / n, and 0.5 mean_{i,j} |x_i - x_j| = sum_i (2i - n - 1) x_(i) / n^2, i = 1..n.
Bootstrap indices from the counter RNG of oracle/rng.py with the member key of csrc/rdgan_rng.h (stream 7 is defined here: it
belongs to this feature).  Moments in two passes."""
import numpy as np

from oracle import rng as orng

STREAM_BOOTSTRAP = 7                # RD_STREAM_BOOTSTRAP of csrc/rdgan_rng.h


def crps_fixed(ens, obs):
    """ens (n, ...), obs (D, ...) -> crps (D, ...) in fp64; a NaN observation gives NaN"""
    ens = np.asarray(ens)
    obs = np.asarray(obs, dtype=np.float64)
    n, D = ens.shape[0], obs.shape[0]
    # sorted in the input's own type (the order is the same) along contiguous rows, then widened
    s = np.sort(np.ascontiguousarray(ens.reshape(n, -1).T), axis=1).T.astype(np.float64)
    y = obs.reshape(D, -1)
    npos = s.shape[1]
    pre = np.concatenate([np.zeros((1, npos)), np.cumsum(s, axis=0)])
    w = (2 * np.arange(1, n + 1) - n - 1).astype(np.float64)
    spread = (w[:, None] * s).sum(0) / (float(n) * n)
    k = np.empty((D, npos), dtype=np.int64)
    for p in range(npos):
        k[:, p] = np.searchsorted(s[:, p], y[:, p], side="right")
    nan = np.isnan(y)
    k[nan] = 0
    mabs = (y * (2 * k - n) - 2 * np.take_along_axis(pre, k, axis=0) + pre[n][None]) / n
    return (mabs - spread[None]).reshape(obs.shape)


def hourly_mean(crps):
    """(D, 24, nd, nd) -> (D, 24) area means in fp64"""
    return np.asarray(crps, dtype=np.float64).mean(axis=(2, 3))


def member_key(seed, stream, member):
    base = np.uint32(orng.make_key(seed, stream))
    lo, hi = np.uint32(member & 0xFFFFFFFF), np.uint32(member >> 32)
    return orng.mix32(base ^ orng.mix32(lo ^ orng.mix32(hi ^ np.uint32(0x9E3779B9))))


def bootstrap_indices(seed, resample, n):
    """(n,) indices of resample `resample`: (uint64(bits(key, i)) * n) >> 32, i = 0 .. n - 1"""
    key = member_key(seed, STREAM_BOOTSTRAP, int(resample))
    bits = orng.mix32(orng.mix32(np.arange(n, dtype=np.uint64).astype(np.uint32)) ^ key)
    return ((bits.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def bootstrap_means(x, seed, first, count):
    x = np.asarray(x, dtype=np.float64)
    return np.array([x[bootstrap_indices(seed, r, len(x))].mean() for r in range(first, first + count)])


def moments(x):
    """(n, mean, variance with ddof = 1), two passes"""
    x = np.asarray(x, dtype=np.float64)
    m = x.mean()
    with np.errstate(invalid="ignore", divide="ignore"):             # n = 1: 0 / 0 = NaN, as np.var(ddof=1)
        return len(x), m, ((x - m) ** 2).sum() / (len(x) - 1)
