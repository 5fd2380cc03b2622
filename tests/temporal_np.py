"""The definitions of DESIGN.md section 17 (include/rdgan.h, rdgan_temporal_accumulate) restated in vectorised numpy: the yardstick of
tests/test_hip_temporal.py, itself checked in tests/test_temporal_host.py against plain loops and closed forms."""
import numpy as np

NH = 24


def series_of(x):
    """x (..., 24, ny, nx) -> (N, 24) float32, series i * plane + q in order"""
    x = np.asarray(x, dtype=np.float32)
    ny, nx = x.shape[-2:]
    return np.ascontiguousarray(x.reshape(-1, NH, ny * nx).transpose(0, 2, 1)).reshape(-1, NH)


def _runs(w):
    """w (N, 24) bool -> (spell (2, 24) int64 = [edge class][L - 1], longest (N,) int64)"""
    pad = np.zeros((w.shape[0], 1), dtype=bool)
    start = w & ~np.concatenate([pad, w[:, :-1]], axis=1)
    end = w & ~np.concatenate([w[:, 1:], pad], axis=1)
    rs, s = np.nonzero(start)                                  # row-major: the k-th start of a row pairs with its k-th end
    _, e = np.nonzero(end)
    L = e - s + 1
    c = ((s == 0) | (e == NH - 1)).astype(np.int64)
    spell = np.bincount(c * NH + L - 1, minlength=2 * NH).reshape(2, NH).astype(np.int64)
    longest = np.zeros(w.shape[0], dtype=np.int64)
    np.maximum.at(longest, rs, L)
    return spell, longest


def temporal_np(x, thresholds, max_lag=6):
    """-> dict with the arrays of temporal.split_state"""
    s = series_of(x)
    thr = np.asarray(thresholds, dtype=np.float64).astype(np.float32)
    T, K = len(thr), int(max_lag)
    good = np.isfinite(s).all(axis=1)
    v = s[good]
    N = v.shape[0]
    out = dict(n_valid=int(N), n_bad=int(s.shape[0] - N),
               wet_hours=np.zeros((T, NH + 1), np.int64), longest_wet=np.zeros((T, NH + 1), np.int64),
               wet_spell=np.zeros((T, 2, NH), np.int64), dry_spell=np.zeros((T, 2, NH), np.int64),
               first_wet=np.zeros((T, NH), np.int64), last_wet=np.zeros((T, NH), np.int64),
               trans=np.zeros((T, NH - 1, 2, 2), np.int64), wet_amount=np.zeros((T, NH), np.float64))
    d = v.astype(np.float64)
    out["moments"] = np.stack([d.sum(axis=0), (d * d).sum(axis=0)], axis=1) if N else np.zeros((NH, 2))
    out["lag"] = np.array([(d[:, :NH - k] * d[:, k:]).sum() for k in range(1, K + 1)], dtype=np.float64)
    for t in range(T):
        w = v > thr[t]
        out["wet_hours"][t] = np.bincount(w.sum(axis=1), minlength=NH + 1)
        out["wet_spell"][t], longest = _runs(w)
        out["dry_spell"][t], _ = _runs(~w)
        out["longest_wet"][t] = np.bincount(longest, minlength=NH + 1)
        some = w.any(axis=1)
        out["first_wet"][t] = np.bincount(np.argmax(w[some], axis=1), minlength=NH)
        out["last_wet"][t] = np.bincount(NH - 1 - np.argmax(w[some][:, ::-1], axis=1), minlength=NH)
        code = w[:, :-1].astype(np.int64) * 2 + w[:, 1:]
        out["trans"][t] = (code[:, :, None] == np.arange(4)).sum(axis=0).reshape(NH - 1, 2, 2)
        out["wet_amount"][t] = (d * w).sum(axis=0)
    return out


def terms(out, T, K):
    """the number of terms of every fp64 sum, in the shapes of moments, lag and wet_amount: the N of the bound N 2^-52"""
    n = out["n_valid"]
    return dict(moments=np.full((NH, 2), n), lag=np.array([n * (NH - k) for k in range(1, K + 1)]), wet_amount=np.full((T, NH), n))


def single_run_days():
    """the 300 days with one wet run (start, length), then an all-dry, an all-wet and the two alternating days; wet = 1.0
    -> (x (304, 24, 1, 1) float32, list of (start, length))"""
    runs = [(s, L) for L in range(1, NH + 1) for s in range(0, NH - L + 1)]
    x = np.zeros((len(runs) + 4, NH), dtype=np.float32)
    for i, (s, L) in enumerate(runs):
        x[i, s:s + L] = 1.0
    x[len(runs) + 1] = 1.0
    x[len(runs) + 2, 0::2] = 1.0
    x[len(runs) + 3, 1::2] = 1.0
    return x.reshape(-1, NH, 1, 1), runs


def single_run_closed_form(runs):
    """the counts of single_run_days for one threshold in (0, 1), from the definitions by hand"""
    o = dict(wet_hours=np.zeros(NH + 1, np.int64), longest_wet=np.zeros(NH + 1, np.int64), wet_spell=np.zeros((2, NH), np.int64),
             dry_spell=np.zeros((2, NH), np.int64), first_wet=np.zeros(NH, np.int64), last_wet=np.zeros(NH, np.int64),
             trans=np.zeros((NH - 1, 2, 2), np.int64))
    for s, L in runs:
        e = s + L - 1
        o["wet_hours"][L] += 1
        o["longest_wet"][L] += 1
        o["wet_spell"][int(s == 0 or e == NH - 1), L - 1] += 1
        if s > 0:
            o["dry_spell"][1, s - 1] += 1                      # hours 0 .. s - 1: holds hour 0
        if e < NH - 1:
            o["dry_spell"][1, NH - 1 - e - 1] += 1             # hours e + 1 .. 23: holds hour 23
        o["first_wet"][s] += 1
        o["last_wet"][e] += 1
        for h in range(NH - 1):
            o["trans"][h, int(s <= h <= e), int(s <= h + 1 <= e)] += 1
    # all dry
    o["wet_hours"][0] += 1; o["longest_wet"][0] += 1; o["dry_spell"][1, NH - 1] += 1; o["trans"][:, 0, 0] += 1
    # all wet
    o["wet_hours"][NH] += 1; o["longest_wet"][NH] += 1; o["wet_spell"][1, NH - 1] += 1; o["trans"][:, 1, 1] += 1
    o["first_wet"][0] += 1; o["last_wet"][NH - 1] += 1
    # wet at the even hours: 12 wet runs of 1 (the first holds hour 0), 12 dry runs of 1 (the last holds hour 23)
    o["wet_hours"][12] += 1; o["longest_wet"][1] += 1; o["wet_spell"][1, 0] += 1; o["wet_spell"][0, 0] += 11
    o["dry_spell"][1, 0] += 1; o["dry_spell"][0, 0] += 11; o["first_wet"][0] += 1; o["last_wet"][NH - 2] += 1
    o["trans"][0::2, 1, 0] += 1; o["trans"][1::2, 0, 1] += 1
    # wet at the odd hours
    o["wet_hours"][12] += 1; o["longest_wet"][1] += 1; o["wet_spell"][1, 0] += 1; o["wet_spell"][0, 0] += 11
    o["dry_spell"][1, 0] += 1; o["dry_spell"][0, 0] += 11; o["first_wet"][1] += 1; o["last_wet"][NH - 1] += 1
    o["trans"][0::2, 0, 1] += 1; o["trans"][1::2, 1, 0] += 1
    return o
