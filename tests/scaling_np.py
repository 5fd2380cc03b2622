"""The scaling structure of hourly fields restated in numpy from the definition: quantise, reshape and sum per
level, Python-int second moments.  The yardstick of tests/test_hip_scaling.py and tests/test_scaling_host.py; it shares no code with
pr_disagg_radar_gan_amd/scaling.py."""
import numpy as np

from tests import hourly_np

DURATIONS = (1, 2, 4, 8, 24)
BINS = 288
ORDER = ("n_boxes", "n_void", "n_wet", "sum1", "sum2_hh", "sum2_hl", "sum2_ll", "max_R")
RECORD = len(ORDER) + BINS
LOW = (1 << 19) - 1


def bin_of(R):
    """the bin of one box sum, a Python int"""
    R = int(R)
    if R < 8:
        return R
    e = R.bit_length() - 1
    return 8 + 8 * (e - 3) + ((R >> (e - 3)) & 7)


def bins_of(R):
    """the same for an int64 array: floor(log2 R) is the exponent of the fp64, exact below 2^53"""
    R = np.asarray(R, dtype=np.int64)
    e = np.frexp(np.maximum(R, 8).astype(np.float64))[1].astype(np.int64) - 1
    return np.where(R < 8, R, 8 + 8 * (e - 3) + ((R >> (e - 3)) & 7))


def box_sums(x, a, b):
    """x (n, 24, ny, nx) -> (R int64, void bool), each (n, 24 / T, ny >> a, nx >> a): the sums of q over the boxes of side 2^a wholly
    inside the plane and the aligned windows of T = DURATIONS[b] hours, and where one holds a bad pixel-hour"""
    q, bad = hourly_np.quantise(x)
    n, _, ny, nx = q.shape
    s, T = 1 << a, DURATIONS[b]
    my, mx = ny // s, nx // s
    fold = lambda v: v[:, :, :my * s, :mx * s].reshape(n, 24 // T, T, my, s, mx, s)
    return fold(q).sum(axis=(2, 4, 6)), fold(bad).any(axis=(2, 4, 6))


def empty_state(A):
    o = {name: np.zeros((A + 1, 5), np.int64) for name in ORDER}
    o.update(hist=np.zeros((A + 1, 5, BINS), np.int64), n_days_total=0, n_bad=0)
    return o


def scaling_np(x, A):
    """x (..., 24, ny, nx) float32, space levels 0 .. A -> the state as a dict of named int64 arrays"""
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape((-1,) + x.shape[-3:])
    assert x.shape[1] == 24 and (1 << A) <= min(x.shape[2:])
    o = empty_state(A)
    o["n_days_total"], o["n_bad"] = x.shape[0], int(hourly_np.quantise(x)[1].sum())
    for a in range(A + 1):
        for b in range(5):
            R, void = box_sums(x, a, b)
            v = R[~void]
            o["n_boxes"][a, b], o["n_void"][a, b], o["n_wet"][a, b] = v.size, int(void.sum()), int((v > 0).sum())
            h, l = v >> 19, v & LOW                                              # both below 2^19: a product fits an int64, a sum may not
            total = lambda t: int(t.astype(object).sum()) if t.size else 0       # Python ints
            o["sum1"][a, b] = total(v)
            o["sum2_hh"][a, b], o["sum2_hl"][a, b], o["sum2_ll"][a, b] = total(h * h), total(h * l), total(l * l)
            o["max_R"][a, b] = int(v.max()) if v.size else 0
            o["hist"][a, b] = np.bincount(bins_of(v), minlength=BINS)
    return o


def flat_state(o):
    """the flat order of include/rdgan.h: per (a, b) the eight words and the histogram, then n_days_total and n_bad"""
    per = np.concatenate([np.stack([np.asarray(o[name], np.int64) for name in ORDER], axis=2), np.asarray(o["hist"], np.int64)], axis=2)
    return np.concatenate([per.ravel(), np.array([o["n_days_total"], o["n_bad"]], np.int64)])


def sum2(o):
    """(A + 1, 5) Python ints: the exact sum of R^2"""
    return [[(int(o["sum2_hh"][a, b]) << 38) + (int(o["sum2_hl"][a, b]) << 20) + int(o["sum2_ll"][a, b]) for b in range(5)]
            for a in range(o["sum1"].shape[0])]


def exact_moment(x, A, q):
    """(A + 1, 5) float64: the mean over the valid box-windows of (box-mean intensity in mm/h)^q, 0^0 = 0, from the box sums themselves"""
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape((-1,) + x.shape[-3:])
    out = np.full((A + 1, 5), np.nan)
    for a in range(A + 1):
        for b in range(5):
            R, void = box_sums(x, a, b)
            v = R[~void].astype(np.float64) / (4.0 ** a * DURATIONS[b] * 1024.0)
            if v.size:
                out[a, b] = (v[v > 0] ** q).sum() / v.size
    return out
