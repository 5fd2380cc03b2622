"""The yardstick of the areal-extremes tests: the definitions of DESIGN.md section 21 restated in numpy, twice -- a brute-force
loop over every start hour and box corner that sums the quantised values of the box directly, and a cumulative-sum form that is
fast enough for the larger test planes.  They share only the quantisation and the per-day statistics; tests/test_areal_host.py
checks them against each other and against answers worked out by hand.  No code is shared with the module, and the reference
project has no such code, so this file is the definition."""
import numpy as np

from tests.hourly_np import levels_q as level_q, quantise

NHOURS, NARF = 24, 21
ORDER = ("level_count", "start_hour", "arf_hist", "sum_A", "sum_A1", "sum_A_all", "max_A", "n_days", "n_void", "n_dry")


def days_of(x):
    """(..., 24, ny, nx) -> (n, 24, ny, nx) float32"""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim >= 3 and x.shape[-3] == NHOURS
    return x.reshape((-1,) + x.shape[-3:])


def day_maxima_brute(day, windows, widths):
    """day (24, ny, nx) -> (A, h): int64 (K, W) each, the largest box sum and the smallest start hour attaining it; A = -1 where
    no (window, box) is free of bad pixel-hours.  The sums are taken box by box."""
    q, bad = quantise(day)
    _, ny, nx = q.shape
    A = np.full((len(windows), len(widths)), -1, np.int64)
    H = np.full(A.shape, -1, np.int64)
    for ki, k in enumerate(windows):
        for wi, w in enumerate(widths):
            for h0 in range(NHOURS - k + 1):
                for y0 in range(ny - w + 1):
                    for x0 in range(nx - w + 1):
                        box = (slice(h0, h0 + k), slice(y0, y0 + w), slice(x0, x0 + w))
                        if bad[box].any():
                            continue
                        a = int(q[box].sum())
                        if a > A[ki, wi]:                                               # strictly: the smallest h0 keeps a tie
                            A[ki, wi], H[ki, wi] = a, h0
    return A, H


def _box_sums(plane, w):
    """(ny, nx) int64 -> (ny - w + 1, nx - w + 1): the sum of every w x w box, by a summed-area table"""
    t = np.zeros((plane.shape[0] + 1, plane.shape[1] + 1), np.int64)
    t[1:, 1:] = plane.cumsum(axis=0).cumsum(axis=1)
    return t[w:, w:] - t[:-w, w:] - t[w:, :-w] + t[:-w, :-w]


def day_maxima(day, windows, widths):
    """day_maxima_brute by cumulative sums over the hours and summed-area tables over the plane"""
    q, bad = quantise(day)
    cq = np.concatenate([np.zeros((1,) + q.shape[1:], np.int64), q.cumsum(axis=0)])
    cb = np.concatenate([np.zeros((1,) + q.shape[1:], np.int64), bad.astype(np.int64).cumsum(axis=0)])
    A = np.full((len(windows), len(widths)), -1, np.int64)
    H = np.full(A.shape, -1, np.int64)
    for ki, k in enumerate(windows):
        for h0 in range(NHOURS - k + 1):
            wq, wb = cq[h0 + k] - cq[h0], cb[h0 + k] - cb[h0]
            for wi, w in enumerate(widths):
                if w > min(wq.shape):
                    continue
                a = np.where(_box_sums(wb, w) == 0, _box_sums(wq, w), -1).max()
                if a > A[ki, wi]:
                    A[ki, wi], H[ki, wi] = a, h0
    return A, H


def empty_state(K, W, L):
    z = lambda *s: np.zeros((K, W) + s, np.int64)
    return dict(level_count=z(L + 1), start_hour=z(NHOURS), arf_hist=z(NARF), sum_A=z(), sum_A1=z(), sum_A_all=z(), max_A=z(), n_days=z(),
                n_void=z(), n_dry=z(), n_days_total=0, n_bad=0)


def areal_np(x, windows, widths, levels, maxima=day_maxima):
    """x (..., 24, ny, nx) -> (state dict, depths (n, K, W) int64 with -1 for a void day)"""
    x = days_of(x)
    K, W, L = len(windows), len(widths), len(levels)
    lq = level_q(levels)
    o = empty_state(K, W, L)
    depths = np.zeros((len(x), K, W), np.int64)
    for u, day in enumerate(x):
        A, H = maxima(day, windows, widths)
        A1 = A[:, 0] if widths[0] == 1 else maxima(day, windows, (1,))[0][:, 0]
        depths[u] = A
        o["n_days_total"] += 1
        o["n_bad"] += int(quantise(day)[1].sum())
        for ki in range(K):
            for wi, w in enumerate(widths):
                a, a1 = int(A[ki, wi]), int(A1[ki])
                if a < 0:
                    o["n_void"][ki, wi] += 1
                    continue
                o["n_days"][ki, wi] += 1
                o["level_count"][ki, wi, sum(a >= l * w * w for l in lq)] += 1
                o["start_hour"][ki, wi, H[ki, wi]] += 1
                o["sum_A_all"][ki, wi] += a
                o["max_A"][ki, wi] = max(o["max_A"][ki, wi], a)
                if a1 > 0:
                    o["arf_hist"][ki, wi, min(20, (20 * a) // (w * w * a1))] += 1
                    o["sum_A"][ki, wi] += a
                    o["sum_A1"][ki, wi] += a1
                else:
                    o["n_dry"][ki, wi] += 1
    return o, depths


def flat_state(o):
    """the state dict -> the flat int64 array in the order of include/rdgan.h"""
    K, W = o["n_days"].shape
    per = np.concatenate([np.asarray(o[name], np.int64).reshape(K, W, -1) for name in ORDER], axis=2)
    return np.concatenate([per.ravel(), np.array([o["n_days_total"], o["n_bad"]], np.int64)])


def check_identities(o):
    """what holds for every state"""
    assert np.array_equal(o["level_count"].sum(axis=2), o["n_days"]) and np.array_equal(o["start_hour"].sum(axis=2), o["n_days"])
    assert np.array_equal(o["arf_hist"].sum(axis=2) + o["n_dry"], o["n_days"])
    assert np.all(o["n_days"] + o["n_void"] == o["n_days_total"])
    assert np.all(o["sum_A"] <= o["sum_A_all"]) and np.all(o["max_A"] * np.maximum(o["n_days"], 1) >= o["sum_A_all"])


def only_nonzero(a):
    """{index: value} of the non-zero entries of an integer array"""
    a = np.asarray(a)
    return {tuple(int(i) for i in idx): int(a[tuple(idx)]) for idx in np.argwhere(a != 0)}
