"""The joint-field scores of DESIGN.md section 23 in plain numpy, written from the definitions: brute-force loops over pairs of
members and over displacements (the pairs of positions of one displacement are array slices).  Energy score: everything in float64.  Variogram score: differences and powers in float32, sums
and the rest in float64.  A NaN of the observation leaves its position out; a day without a valid position gives NaN."""
import numpy as np


def energy_terms(x, y):
    """x (m, 24, ny, nx), y (24, ny, nx) -> (obs_sum, pair_sum): sum_i |x_i - y|, sum_{i<j} |x_i - x_j| over the valid positions"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = x.shape[0]
    valid = ~np.isnan(y).ravel()
    if not valid.any():
        return np.nan, np.nan
    xs, ys = x.reshape(m, -1)[:, valid], y.ravel()[valid]
    obs_sum = 0.0
    for i in range(m):
        obs_sum += np.sqrt(np.sum((xs[i] - ys) ** 2))
    pair_sum = 0.0
    for i in range(m):
        for j in range(i + 1, m):
            pair_sum += np.sqrt(np.sum((xs[i] - xs[j]) ** 2))
    return obs_sum, pair_sum


def energy_score(x, y, fair=False):
    m = np.asarray(x).shape[0]
    obs_sum, pair_sum = energy_terms(x, y)
    if fair:
        return obs_sum / m - (pair_sum / (m * (m - 1)) if m > 1 else 0.0)
    return obs_sum / m - pair_sum / (m * m)


def in_half_space(l, di, dj):
    return l > 0 or (l == 0 and di > 0) or (l == 0 and di == 0 and dj > 0)


def displacements(radius, max_lag):
    return [(l, di, dj) for l in range(max_lag + 1) for di in range(-radius, radius + 1) for dj in range(-radius, radius + 1)
            if in_half_space(l, di, dj)]


def _power(a, p):
    a = np.abs(a).astype(np.float32)
    return np.sqrt(a) if p == 0.5 else a


def variogram_tables(x, y, p=0.5, radius=2, max_lag=1, return_norm=False):
    """x (m, 24, ny, nx), y (24, ny, nx) -> (sq float64, count int64) of shape (max_lag + 1, 2r + 1, 2r + 1); with return_norm also
    the sum over the pairs of o^2 + mean^2, what the comparison's tolerance scales with"""
    assert p in (0.5, 1)
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    m, nh, ny, nx = x.shape
    side = 2 * radius + 1
    sq, count, norm = np.zeros((max_lag + 1, side, side)), np.zeros((max_lag + 1, side, side), np.int64), np.zeros((max_lag + 1, side, side))
    for l, di, dj in displacements(radius, max_lag):
        # every pair (a, b) of this displacement that lies inside the day and the plane: a = (h, i, j), b = (h + l, i + di, j + dj)
        i0, i1, j0, j1 = max(0, -di), min(ny, ny - di), max(0, -dj), min(nx, nx - dj)
        if i1 <= i0 or j1 <= j0:
            continue
        ya, yb = y[:nh - l, i0:i1, j0:j1], y[l:, i0 + di:i1 + di, j0 + dj:j1 + dj]
        xa, xb = x[:, :nh - l, i0:i1, j0:j1], x[:, l:, i0 + di:i1 + di, j0 + dj:j1 + dj]
        valid = ~(np.isnan(ya) | np.isnan(yb))
        mean = _power(xa - xb, p).astype(np.float64).sum(axis=0) / m
        o = _power(np.where(valid, ya - yb, np.float32(0)), p).astype(np.float64)
        sq[l, di + radius, dj + radius] = np.sum(((o - mean) ** 2)[valid])
        norm[l, di + radius, dj + radius] = np.sum((o * o + mean * mean)[valid])
        count[l, di + radius, dj + radius] = valid.sum()
    if np.isnan(y).all():
        sq[default_weights(radius, max_lag) > 0] = np.nan
    return (sq, count, norm) if return_norm else (sq, count)


def default_weights(radius, max_lag):
    side = 2 * radius + 1
    w = np.zeros((max_lag + 1, side, side))
    for l, di, dj in displacements(radius, max_lag):
        w[l, di + radius, dj + radius] = 1.0 / np.sqrt(l * l + di * di + dj * dj)
    return w


def variogram_score(x, y, p=0.5, radius=2, max_lag=1, weights=None, normalised=False):
    sq, count = variogram_tables(x, y, p, radius, max_lag)
    w = default_weights(radius, max_lag) if weights is None else np.asarray(weights, dtype=np.float64)
    keep = default_weights(radius, max_lag) > 0
    vs = float(np.sum(w[keep] * sq[keep]))
    return vs / float(np.sum(w[keep] * count[keep])) if normalised else vs


def crps_ensemble(x, y):
    """the closed form of the ensemble CRPS at one position, float64: mean |x_i - y| - sum_{i,j} |x_i - x_j| / (2 m^2)"""
    x = np.asarray(x, dtype=np.float64)
    m = len(x)
    return np.abs(x - y).mean() - np.abs(x[:, None] - x[None, :]).sum() / (2.0 * m * m)
