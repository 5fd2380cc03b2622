"""The yardstick of the space-time tests: the definitions of DESIGN.md section 19 restated in numpy with shifted slices, and once
more in plain Python loops for small arrays.  No bit masks, no packing of tie-break keys.  The reference project has no such code."""
import numpy as np


def days_of(x):
    """(..., 24, ny, nx) -> (n, 24, ny, nx) float32"""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim >= 3 and x.shape[-3] == 24
    return x.reshape((-1,) + x.shape[-3:])


def masks_of(x, thresholds):
    """-> finite (n, 24, ny, nx) bool, wet (T, n, 24, ny, nx) bool"""
    thr = np.asarray(thresholds, np.float64).astype(np.float32)
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        wet = np.stack([fin & (x > t) for t in thr])
    return fin, wet


def empty_state(T, R, K):
    s = 2 * R + 1
    return dict(n_days=0, n_bad_pixels=0, pairs=np.zeros((K + 1, s, s), np.int64), wet_first=np.zeros((T, K + 1, s, s), np.int64),
                wet_second=np.zeros((T, K + 1, s, s), np.int64), joint=np.zeros((T, K + 1, s, s), np.int64),
                shift_hist=np.zeros((T, K, s, s), np.int64), no_shift=np.zeros((T, K), np.int64), dist_best=np.zeros((T, K), np.int64),
                dist_zero=np.zeros((T, K), np.int64))


def tie_order(R):
    """the displacements (dy, dx) in the order in which a tie is decided: dy^2 + dx^2, then dy, then dx"""
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda d: (d[0] ** 2 + d[1] ** 2, d[0], d[1]))


def spacetime_np(x, thresholds, radius, max_lag):
    """-> the state as a dict of int64 arrays"""
    x = days_of(x)
    n, _, ny, nx = x.shape
    R, K, T = radius, max_lag, len(thresholds)
    assert min(ny, nx) >= 2 * R + 1
    fin, wet = masks_of(x, thresholds)
    o = empty_state(T, R, K)
    o["n_days"], o["n_bad_pixels"] = n, int((~fin).sum())
    order = tie_order(R)
    for k in range(K + 1):
        first, second = slice(0, 24 - k), slice(k, 24)
        for dy in range(-R, R + 1):
            ya, yb = slice(max(0, -dy), ny - max(0, dy)), slice(max(0, dy), ny - max(0, -dy))
            for dx in range(-R, R + 1):
                xa, xb = slice(max(0, -dx), nx - max(0, dx)), slice(max(0, dx), nx - max(0, -dx))
                ok = fin[:, first, ya, xa] & fin[:, second, yb, xb]
                o["pairs"][k, dy + R, dx + R] = ok.sum()
                for t in range(T):
                    a, b = wet[t][:, first, ya, xa], wet[t][:, second, yb, xb]
                    o["wet_first"][t, k, dy + R, dx + R] = (ok & a).sum()
                    o["wet_second"][t, k, dy + R, dx + R] = (ok & b).sum()
                    o["joint"][t, k, dy + R, dx + R] = (ok & a & b).sum()
        if k == 0:
            continue
        for t in range(T):
            a = wet[t][:, first, R:ny - R, R:nx - R]
            dist = np.stack([(a != wet[t][:, second, R + dy:ny - R + dy, R + dx:nx - R + dx]).sum(axis=(-1, -2)) for dy, dx in order])
            informative = a.any(axis=(-1, -2)) & wet[t][:, second].any(axis=(-1, -2))
            best = dist.argmin(axis=0)                                   # (the first of the smallest, in the order of the ties)
            for i, h in zip(*np.nonzero(informative)):
                dy, dx = order[best[i, h]]
                o["shift_hist"][t, k - 1, dy + R, dx + R] += 1
                o["dist_best"][t, k - 1] += dist[best[i, h], i, h]
                o["dist_zero"][t, k - 1] += dist[0, i, h]                  # (order[0] is (0, 0))
            o["no_shift"][t, k - 1] = (~informative).sum()
    return o


def spacetime_loops(x, thresholds, radius, max_lag):
    """the same in plain Python loops over pixels, for small arrays"""
    x = days_of(x)
    n, _, ny, nx = x.shape
    R, K, T = radius, max_lag, len(thresholds)
    thr = [np.float32(np.float64(t)) for t in thresholds]
    o = empty_state(T, R, K)
    o["n_days"] = n
    bad = [[[[not np.isfinite(x[i, h, y, c]) for c in range(nx)] for y in range(ny)] for h in range(24)] for i in range(n)]
    o["n_bad_pixels"] = sum(bad[i][h][y][c] for i in range(n) for h in range(24) for y in range(ny) for c in range(nx))
    wet = [[[[[(not bad[i][h][y][c]) and bool(x[i, h, y, c] > thr[t]) for c in range(nx)] for y in range(ny)] for h in range(24)]
            for i in range(n)] for t in range(T)]
    for i in range(n):
        for k in range(K + 1):
            for h in range(24 - k):
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        for y in range(ny):
                            for c in range(nx):
                                if not (0 <= y + dy < ny and 0 <= c + dx < nx) or bad[i][h][y][c] or bad[i][h + k][y + dy][c + dx]:
                                    continue
                                o["pairs"][k, dy + R, dx + R] += 1
                                for t in range(T):
                                    a, b = wet[t][i][h][y][c], wet[t][i][h + k][y + dy][c + dx]
                                    o["wet_first"][t, k, dy + R, dx + R] += a
                                    o["wet_second"][t, k, dy + R, dx + R] += b
                                    o["joint"][t, k, dy + R, dx + R] += a and b
                if k == 0:
                    continue
                for t in range(T):
                    A, B = wet[t][i][h], wet[t][i][h + k]
                    core = [(y, c) for y in range(R, ny - R) for c in range(R, nx - R)]
                    if not any(A[y][c] for y, c in core) or not any(any(row) for row in B):
                        o["no_shift"][t, k - 1] += 1
                        continue
                    best = None
                    for dy in range(-R, R + 1):
                        for dx in range(-R, R + 1):
                            dist = sum(A[y][c] != B[y + dy][c + dx] for y, c in core)
                            cand = (dist, dy * dy + dx * dx, dy, dx)
                            best = cand if best is None or cand < best else best
                            if (dy, dx) == (0, 0):
                                o["dist_zero"][t, k - 1] += dist
                    o["shift_hist"][t, k - 1, best[2] + R, best[3] + R] += 1
                    o["dist_best"][t, k - 1] += best[0]
    return o


def flat_state(o):
    """the dict -> the flat int64 state in the order of include/rdgan.h"""
    T = o["wet_first"].shape[0]
    per = [np.concatenate([o[name][t].ravel() for name in ("wet_first", "wet_second", "joint", "shift_hist", "no_shift", "dist_best", "dist_zero")])
           for t in range(T)]
    return np.concatenate([o["pairs"].ravel()] + per + [np.array([o["n_days"], o["n_bad_pixels"]], np.int64)]).astype(np.int64)


def check_identities(o):
    K = o["pairs"].shape[0] - 1
    assert np.all(o["joint"] <= np.minimum(o["wet_first"], o["wet_second"]))
    assert np.all(np.maximum(o["wet_first"], o["wet_second"]) <= o["pairs"][None])
    # k = 0: the pair (p, p + d) is the pair (q, q - d) with q = p + d, first and second swapped
    assert np.array_equal(o["pairs"][0], o["pairs"][0, ::-1, ::-1])
    assert np.array_equal(o["joint"][:, 0], o["joint"][:, 0, ::-1, ::-1])
    assert np.array_equal(o["wet_first"][:, 0], o["wet_second"][:, 0, ::-1, ::-1])
    for k in range(1, K + 1):
        assert np.all(o["shift_hist"][:, k - 1].sum(axis=(1, 2)) + o["no_shift"][:, k - 1] == o["n_days"] * (24 - k))
    assert np.all(o["dist_best"] <= o["dist_zero"])


# ---------------------------------------------------------------------------------------------------------------------------------
def rain_like(shape, seed, wet=0.15):
    """float32 of `shape`: about `wet` of the pixels wet, in blobs of a few pixels, amounts on multiples of 1/8"""
    rng = np.random.default_rng(seed)
    f = rng.random(shape)
    for axis in (-1, -2):                                                 # a short moving average makes the wet pixels clump
        f = (f + np.roll(f, 1, axis) + np.roll(f, -1, axis)) / 3
    cut = np.quantile(f, 1 - wet)
    return (np.where(f > cut, np.ceil(rng.gamma(1.0, 2.0, shape) * 8) / 8, 0.0)).astype(np.float32)


L_BLOB = ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2))                          # an L of 5 pixels: no translate of it equals it


def moving_blob(n, ny, nx, start, step, amount=2.0):
    """(n, 24, ny, nx): the L, its corner at start + h step in hour h, dry elsewhere"""
    x = np.zeros((n, 24, ny, nx), np.float32)
    for h in range(24):
        for by, bx in L_BLOB:
            x[:, h, start[0] + h * step[0] + by, start[1] + h * step[1] + bx] = amount
    return x


def tie_day(a, b, ny=9, nx=9):
    """(1, 24, ny, nx): wet pixels `a` in hour 0, `b` in hour 1, every other hour dry"""
    x = np.zeros((1, 24, ny, nx), np.float32)
    for y, c in a:
        x[0, 0, y, c] = 1.0
    for y, c in b:
        x[0, 1, y, c] = 1.0
    return x


# 9 x 9 with R = 2: the core is rows and columns 2 .. 6, so every candidate below keeps the other pixel of B inside the core
TIES = [
    # one wet pixel at (4, 4), then two at equal distance: dy^2 + dx^2 decides nothing, the smaller dy wins
    (((4, 4),), ((3, 4), (5, 4)), (-1, 0)),
    # the same along a row: dy equal, the smaller dx wins
    (((4, 4),), ((4, 3), (4, 5)), (0, -1)),
    # (1, 0) and (0, 1) tie on dist and on dy^2 + dx^2: the smaller dy, (0, 1)
    (((4, 4),), ((5, 4), (4, 5)), (0, 1)),
    # a near and a far candidate with equal dist: the smaller dy^2 + dx^2 wins over the smaller dy
    (((4, 4),), ((2, 4), (4, 5)), (0, 1)),
    # the pixel stays and a second appears: dist(0) = 1 = dist(to the second), "did not move" wins
    (((4, 4),), ((4, 4), (2, 2)), (0, 0)),
]
