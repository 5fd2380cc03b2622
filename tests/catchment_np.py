"""The yardstick of the catchment-rainfall tests: the definitions of DESIGN.md section 25 restated in numpy, a loop over the
catchments, days and windows that sums the quantised values of each catchment's pixels directly.  tests/test_catchment_host.py
checks it against answers worked out by hand.  No code is shared with the module, and the reference project has no such code, so
this file is the definition."""
import numpy as np

from tests.hourly_np import levels_q as level_q, quantise

NHOURS = 24
ORDER = ("level_count", "start_hour", "sum_A", "max_A", "n_days", "n_void", "n_dry")


def days_of(x):
    """(..., 24, ny, nx) -> (n, 24, ny, nx) float32"""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim >= 3 and x.shape[-3] == NHOURS
    return x.reshape((-1,) + x.shape[-3:])


def members_of(regions=None, masks=None, valid=None):
    """-> a list of C arrays of flat pixel indices y * nx + x, ascending: the pixels of each catchment, those with valid False
    dropped.  regions (ny, nx) labels, -1 for none; or masks (C, ny, nx) booleans."""
    assert (regions is None) != (masks is None)
    if regions is not None:
        regions = np.asarray(regions)
        masks = np.stack([regions == c for c in range(int(regions.max()) + 1)])
    ok = np.ones(masks.shape[1:], bool) if valid is None else np.asarray(valid, bool)
    return [np.flatnonzero(m & ok) for m in np.asarray(masks, bool)]


def window_maximum(P, B, k):
    """P, B (24,) -> (A, h0): the largest sum of k consecutive clean hours and the smallest start hour attaining it; (-1, -1)
    with no clean window"""
    A, H = -1, -1
    for h0 in range(NHOURS - k + 1):
        if B[h0:h0 + k].any():
            continue
        a = int(P[h0:h0 + k].sum())
        if a > A:                                                               # strictly: the smallest h0 keeps a tie
            A, H = a, h0
    return A, H


def empty_state(C, K, L):
    z = lambda *s: np.zeros((C, K) + s, np.int64)
    return dict(level_count=z(L + 1), start_hour=z(NHOURS), sum_A=z(), max_A=z(), n_days=z(), n_void=z(), n_dry=z(), n_days_total=0, n_bad=0)


def catchment_np(x, members, windows, levels):
    """x (..., 24, ny, nx), members as members_of gives them -> (state dict, series (n, C, 24) int64 with -1 at a void
    catchment-hour, depths (n, C, K) int64 with -1 for a void day)"""
    x = days_of(x)
    C, K, L = len(members), len(windows), len(levels)
    lq = level_q(levels)
    o = empty_state(C, K, L)
    series = np.zeros((len(x), C, NHOURS), np.int64)
    depths = np.zeros((len(x), C, K), np.int64)
    for u, day in enumerate(x):
        q, bad = quantise(day.reshape(NHOURS, -1))
        o["n_days_total"] += 1
        for c, pix in enumerate(members):
            P, B = q[:, pix].sum(axis=1), bad[:, pix].sum(axis=1)
            o["n_bad"] += int(B.sum())
            series[u, c] = np.where(B > 0, -1, P)
            for ki, k in enumerate(windows):
                a, h0 = window_maximum(P, B, k)
                depths[u, c, ki] = a
                if a < 0:
                    o["n_void"][c, ki] += 1
                    continue
                o["n_days"][c, ki] += 1
                o["level_count"][c, ki, sum(a >= l * len(pix) for l in lq)] += 1
                o["sum_A"][c, ki] += a
                o["max_A"][c, ki] = max(o["max_A"][c, ki], a)
                if a > 0:
                    o["start_hour"][c, ki, h0] += 1
                else:
                    o["n_dry"][c, ki] += 1
    return o, series, depths


def flat_state(o):
    """the state dict -> the flat int64 array in the order of include/rdgan.h"""
    C, K = o["n_days"].shape
    per = np.concatenate([np.asarray(o[name], np.int64).reshape(C, K, -1) for name in ORDER], axis=2)
    return np.concatenate([per.ravel(), np.array([o["n_days_total"], o["n_bad"]], np.int64)])


def check_identities(o):
    """what holds for every state"""
    assert np.array_equal(o["level_count"].sum(axis=2), o["n_days"])
    assert np.array_equal(o["start_hour"].sum(axis=2) + o["n_dry"], o["n_days"])
    assert np.all(o["n_days"] + o["n_void"] == o["n_days_total"])
    assert np.all(o["max_A"] * np.maximum(o["n_days"], 1) >= o["sum_A"])
