"""The definitions of pr_disagg_radar_gan_amd/multivariate_ranks.py restated in numpy, each piece with its
own code: mid-ranks by searchsorted on a sorted column, the band depth from lt and gt, Prim's algorithm on a dense matrix, the
integer features of the MST route, the observation's rank and its histogram.  Test infrastructure only."""
import numpy as np

UNIT = 32
FEATMAX = 65535
MAX_DEPTH = 2048


def stack(ens, obs):
    """ens (m, ...), obs (...) -> z (N, P) float32, index 0 the observation"""
    ens, obs = np.asarray(ens, dtype=np.float32), np.asarray(obs, dtype=np.float32)
    return np.concatenate([obs.reshape(1, -1), ens.reshape(ens.shape[0], -1)], axis=0)


def lt_gt(z):
    """z (N, P) of finite values -> (lt, gt) int64 (N, P): per column, how many values lie strictly below / above each one"""
    s = np.sort(z, axis=0)
    lt, gt = np.empty(z.shape, np.int64), np.empty(z.shape, np.int64)
    for p in range(z.shape[1]):
        lt[:, p] = np.searchsorted(s[:, p], z[:, p], side="left")
        gt[:, p] = z.shape[0] - np.searchsorted(s[:, p], z[:, p], side="right")
    return lt, gt


def prerank_sums(ens, obs):
    """One case -> (sums (N, 2) int64: avg, depth; n_valid).  A position is valid when the observation and every member are finite."""
    z = stack(ens, obs)
    N = z.shape[0]
    z = z[:, np.isfinite(z).all(axis=0)] + np.float32(0)                                  # (-0.0 + 0.0 = +0.0: one zero for the sort)
    lt, gt = lt_gt(z)
    avg = (lt - gt + N + 1).sum(axis=1)
    depth = ((N - 1) * (N - 2) - lt * (lt - 1) - gt * (gt - 1)).sum(axis=1)
    return np.stack([avg, depth], axis=1).astype(np.int64), int(z.shape[1])


def prerank_sums_by_hour(ens, obs):
    """ens (m, 24, ny, nx), obs (24, ny, nx) -> (sums (24, N, 2), n_valid (24,))"""
    out = [prerank_sums(np.asarray(ens)[:, h], np.asarray(obs)[h]) for h in range(np.asarray(obs).shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64)


def prim(dist):
    """the length of the minimum spanning tree of a dense symmetric matrix, python integers; 0 for fewer than two vertices"""
    d = np.asarray(dist)
    n = len(d)
    if n < 2:
        return 0
    key, inside, total = d[0].astype(object), np.zeros(n, bool), 0
    inside[0] = True
    for _ in range(n - 1):
        cand = np.where(inside, None, key)
        u = min((j for j in range(n) if not inside[j]), key=lambda j: cand[j])
        total += int(key[u])
        inside[u] = True
        key = np.minimum(key, d[u].astype(object))
    return total


def prim_fast(dist):
    """prim() in int64 arithmetic, for the sizes at which python integers are too slow"""
    d = np.asarray(dist, dtype=np.int64)
    n = len(d)
    if n < 2:
        return 0
    big = np.iinfo(np.int64).max
    key, inside, total = d[0].copy(), np.zeros(n, bool), 0
    inside[0] = True
    for _ in range(n - 1):
        u = int(np.argmin(np.where(inside, big, key)))
        total += int(key[u])
        inside[u] = True
        key = np.minimum(key, d[u])
    return total


def mst_leave_one_out(dist, fast=True):
    """(N,) int64: the MST length of the vertices other than i"""
    d = np.asarray(dist)
    f = prim_fast if fast else prim
    return np.array([f(np.delete(np.delete(d, i, axis=0), i, axis=1)) for i in range(len(d))], np.int64)


def pixel_features(x):
    """x fp32 -> (e int64, bad bool): e = min(rint(32 x), 65535), the fp32 product, rint to even; bad: not finite, < 0 or >= 2048"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(x) & (x >= 0) & (x < np.float32(MAX_DEPTH))
        q = np.rint(np.where(good, x, np.float32(0)) * np.float32(UNIT))
    return np.minimum(q, FEATMAX).astype(np.int64), ~good


def features(z, pool):
    """z (N, 24, ny, nx) -> (feat (N, Pf) int64, bad (Pf,) bool): p x p blocks of a plane, rim blocks with their own pixel count,
    (sum + n // 2) // n; a position is bad when any pixel of any vector is"""
    e, bad = pixel_features(z)
    N, H, ny, nx = e.shape
    by, bx = -(-ny // pool), -(-nx // pool)
    feat, fbad = np.zeros((N, H, by, bx), np.int64), np.zeros((H, by, bx), bool)
    for yb in range(by):
        for xb in range(bx):
            ys, xs = slice(yb * pool, min((yb + 1) * pool, ny)), slice(xb * pool, min((xb + 1) * pool, nx))
            n = (ys.stop - ys.start) * (xs.stop - xs.start)
            feat[:, :, yb, xb] = (e[:, :, ys, xs].sum(axis=(2, 3)) + n // 2) // n
            fbad[:, yb, xb] = bad[:, :, ys, xs].any(axis=(0, 2, 3))
    return feat.reshape(N, -1), fbad.reshape(-1)


def l1_distances(feat, bad):
    f = feat[:, ~bad]
    return np.stack([np.abs(f - f[i]).sum(axis=1) for i in range(len(f))]).astype(np.int64)


def mst_preranks(ens, obs, pool=1):
    """One case -> (lengths (N,) int64, n_valid): index 0 the observation"""
    z = np.concatenate([np.asarray(obs, np.float32)[None], np.asarray(ens, np.float32)], axis=0)
    feat, bad = features(z, pool)
    return mst_leave_one_out(l1_distances(feat, bad)), int((~bad).sum())


def observation_ranks(preranks):
    """preranks (..., N) -> (below, equal): the members whose pre-rank lies below / equals the observation's"""
    r = np.asarray(preranks)
    return (r[..., 1:] < r[..., :1]).sum(axis=-1), (r[..., 1:] == r[..., :1]).sum(axis=-1)


def histogram(below, equal, n_members, seed=0):
    """the rank below + U, U uniform on 0 .. equal from default_rng(seed), counted over the cases: (n_members + 1,) int64"""
    below, equal = np.asarray(below).reshape(-1), np.asarray(equal).reshape(-1)
    u = np.random.default_rng(seed).integers(0, equal + 1)
    return np.bincount(below + u, minlength=n_members + 1).astype(np.int64)


def chi_square(counts):
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() / len(counts)
    return float(((counts - e) ** 2 / e).sum())
