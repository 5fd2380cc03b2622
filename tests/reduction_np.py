"""The definitions of pr_disagg_radar_gan_amd/reduction.py restated in numpy, as plainly as they read: pooled
integer features and their bad bits, the order-free mask, the all-pairs L1 distances (a double loop), fast forward selection with
its tie rule and explicit skip of selected members, and the assignment.  Test infrastructure only."""
import numpy as np

UNIT = 32
FEATMAX = 65535
MAX_DEPTH = 2048
MAX_MEMBERS = 4096


def pixel_features(x):
    """x (...) fp32 -> (e int64, bad bool): e = min(rint(32 x), 65535), the fp32 product, rint to even; 0 where bad"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(x) & (x >= 0) & (x < np.float32(MAX_DEPTH))
        q = np.rint(np.where(good, x, np.float32(0)) * np.float32(UNIT))
    return np.minimum(q, FEATMAX).astype(np.int64), ~good


def features(members, pool=1):
    """members (S, [D,] 24, ny, nx) -> (feat (S, Pf) uint16, bad (S, Pf) bool): position f = (plane, block row, block column)"""
    e, bad = pixel_features(members)
    S, ny, nx = e.shape[0], e.shape[-2], e.shape[-1]
    e, bad = e.reshape(S, -1, ny, nx), bad.reshape(S, -1, ny, nx)
    by, bx = -(-ny // pool), -(-nx // pool)
    feat, fbad = np.zeros((S, e.shape[1], by, bx), np.int64), np.zeros((S, e.shape[1], by, bx), bool)
    for yb in range(by):
        for xb in range(bx):
            blk = (slice(None), slice(None), slice(yb * pool, min((yb + 1) * pool, ny)), slice(xb * pool, min((xb + 1) * pool, nx)))
            n = e[blk].shape[2] * e[blk].shape[3]                                     # a rim block's own pixel count
            any_bad = bad[blk].any(axis=(2, 3))
            feat[:, :, yb, xb] = np.where(any_bad, 0, (e[blk].sum(axis=(2, 3)) + n // 2) // n)
            fbad[:, :, yb, xb] = any_bad
    return feat.reshape(S, -1).astype(np.uint16), fbad.reshape(S, -1)


def distances(feat, bad):
    """feat (S, Pf), bad (S, Pf) or (Pf,) -> (Dist (S, S) int64, n_valid): a position is masked when any member is bad there"""
    mask = np.asarray(bad).reshape(-1, feat.shape[1]).any(axis=0)
    f = feat.astype(np.int64)[:, ~mask]
    S = f.shape[0]
    dist = np.zeros((S, S), np.int64)
    for i in range(S):
        for j in range(S):
            dist[i, j] = np.abs(f[i] - f[j]).sum()
    return dist, int((~mask).sum())


def distances_fast(feat, bad):
    """the same numbers, a row at a time: for the sizes at which the double loop is too slow"""
    mask = np.asarray(bad).reshape(-1, feat.shape[1]).any(axis=0)
    f = feat.astype(np.int64)[:, ~mask]
    return np.stack([np.abs(f - f[i]).sum(axis=1) for i in range(f.shape[0])]), int((~mask).sum())


def select(dist, k):
    """-> (chosen (k,) int32, cost (k,) int64): python integers throughout, so no width is assumed"""
    S = len(dist)
    assert 1 <= k <= S <= MAX_MEMBERS
    rows = [[int(v) for v in row] for row in np.asarray(dist)]
    m, selected, chosen, cost = [None] * S, [False] * S, [], []                            # None: +inf
    for _ in range(k):
        best = None
        for u in range(S):
            if selected[u]:
                continue
            z = sum(rows[u][j] if m[j] is None else min(m[j], rows[u][j]) for j in range(S))
            if best is None or (z << 12 | u) < best:
                best = z << 12 | u
        u = best & 0xFFF
        chosen.append(u), cost.append(best >> 12)
        selected[u] = True
        m = [rows[u][j] if m[j] is None else min(m[j], rows[u][j]) for j in range(S)]
    return np.array(chosen, np.int32), np.array(cost, np.int64)


def select_fast(dist, k):
    """select() with numpy rows: for the sizes at which python integers are too slow; entries < 2^52 / S"""
    d = np.asarray(dist, dtype=np.int64)
    S = len(d)
    m, selected, chosen, cost = None, np.zeros(S, bool), [], []
    for _ in range(k):
        z = (d if m is None else np.minimum(d, m[None, :])).sum(axis=1)
        key = np.where(selected, np.iinfo(np.uint64).max, (z.astype(np.uint64) << np.uint64(12)) | np.arange(S, dtype=np.uint64))
        u = int(np.argmin(key))
        chosen.append(u), cost.append(int(z[u]))
        selected[u] = True
        m = d[u].copy() if m is None else np.minimum(m, d[u])
    return np.array(chosen, np.int32), np.array(cost, np.int64)


def assign(dist, chosen):
    """-> (assign (S,) int32, counts (k,) int32): the chosen u of the smallest Dist[u][j] << 12 | u"""
    S = len(dist)
    out, counts = np.zeros(S, np.int32), np.zeros(len(chosen), np.int32)
    for j in range(S):
        keys = [(int(dist[u][j]) << 12 | int(u), t) for t, u in enumerate(chosen)]
        key, t = min(keys)
        out[j] = key & 0xFFF
        counts[t] += 1
    return out, counts


def reduce(members, k, pool=1):
    """features, mask, distances, selection and assignment in one: -> dict"""
    feat, bad = features(members, pool)
    dist, n_valid = distances_fast(feat, bad)
    chosen, cost = select_fast(dist, k)
    a, counts = assign(dist, chosen)
    return dict(feat=feat, bad=bad.any(axis=0), dist=dist, n_valid=n_valid, chosen=chosen, cost=cost, assign=a, counts=counts)
