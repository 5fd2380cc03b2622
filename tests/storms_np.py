"""The yardstick of the storm tests: the definitions of DESIGN.md section 20 restated in numpy -- a union-find over the voxels of a
day whose unions are taken a whole list of links at a time.  It shares no code with the module, and uses no scipy.  The reference
project has no such code, so this file is the definition; tests/test_storms_host.py checks it against answers worked out by
hand."""
import numpy as np

NHOURS, NCLASS, NBINS, NSPD, NLONG = 24, 4, 28, 65, 25


def days_of(x):
    """(..., 24, ny, nx) -> (n, 24, ny, nx) float32"""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim >= 3 and x.shape[-3] == NHOURS
    return x.reshape((-1,) + x.shape[-3:])


def links(wet, connectivity, reach):
    """wet (24, ny, nx) bool -> (a, b): the day-local indices of every linked pair of wet voxels, a < b"""
    idx = np.arange(wet.size, dtype=np.int64).reshape(wet.shape)
    steps = [(0, 0, 1), (0, 1, 0)] + ([(0, 1, 1), (0, 1, -1)] if connectivity == 8 else [])
    steps += [(1, dy, dx) for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1)]
    ny, nx = wet.shape[1:]
    a, b = [], []
    for dh, dy, dx in steps:
        if abs(dy) >= ny or abs(dx) >= nx:
            continue
        # the voxels (h, y, x) with (h + dh, y + dy, x + dx) inside the day
        lo = (slice(0, NHOURS - dh), slice(max(0, -dy), ny - max(0, dy)), slice(max(0, -dx), nx - max(0, dx)))
        hi = (slice(dh, NHOURS), slice(max(0, dy), ny - max(0, -dy)), slice(max(0, dx), nx - max(0, -dx)))
        both = wet[lo] & wet[hi]
        a.append(idx[lo][both])
        b.append(idx[hi][both])
    return np.concatenate(a), np.concatenate(b)


def label_day(wet, connectivity, reach):
    """wet (24, ny, nx) bool -> int32 (24, ny, nx): the smallest day-local index of the voxel's storm, -1 where dry.  root[] is a
    forest with root[i] <= i that is kept flat; a round hangs, for every link between two trees, the larger root under the
    smaller, and flattens again.  Every tree that is not yet a whole storm has such a link, so a round at least halves their
    number."""
    a, b = links(wet, connectivity, reach)
    root = np.arange(wet.size, dtype=np.int64)
    while True:
        ra, rb = root[a], root[b]
        open_ = ra != rb
        if not open_.any():
            break
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]            # (a link inside a tree stays inside it)
        np.minimum.at(root, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            above = root[root]
            if np.array_equal(above, root):
                break
            root = above
    return np.where(wet.ravel(), root, -1).reshape(wet.shape).astype(np.int32)


def near_bad(bad):
    """bad (24, ny, nx) bool -> bool: a bad pixel in the 8-neighbourhood of the same hour (or the pixel itself)"""
    n, ny, nx = bad.shape
    pad = np.zeros((n, ny + 2, nx + 2), bool)
    pad[:, 1:-1, 1:-1] = bad
    out = np.zeros(bad.shape, bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + ny, dx:dx + nx]
    return out


def quantum(v):
    """q(x) = rint(min(x, 2^20) 2^16) as int64, the product exact in fp64, half to even"""
    return np.rint(np.minimum(v.astype(np.float64), 2.0 ** 20) * 2.0 ** 16).astype(np.int64)


def empty_state(T):
    z = lambda *s: np.zeros((T,) + s, np.int64)
    return dict(n_days=0, n_bad_pixels=0, wet_pixels=z(NHOURS), storms=z(NCLASS), duration_hist=z(NCLASS, NHOURS), start_hour=z(NCLASS, NHOURS),
                size_hist=z(NCLASS, NBINS), size_sum=z(NCLASS), size_sq_sum=z(NCLASS), size_by_duration=z(NCLASS, NHOURS),
                volume_by_duration=z(NCLASS, NHOURS), storms_per_day=z(NSPD), longest_duration=z(NLONG))


def storms_np(x, thresholds, connectivity=8, reach=1, want_labels=None):
    """-> the state as a dict of int64 arrays (and, with want_labels = t, the labels at threshold t as a second value)"""
    days = days_of(x)
    thr = np.asarray(thresholds, np.float64).astype(np.float32)
    T = len(thr)
    o = empty_state(T)
    labels = np.full(days.shape, -1, np.int32)
    ny, nx = days.shape[2:]
    plane = ny * nx
    rim = np.zeros((NHOURS, ny, nx), bool)
    rim[:, 0], rim[:, -1], rim[:, :, 0], rim[:, :, -1] = True, True, True, True
    hour = np.broadcast_to(np.arange(NHOURS)[:, None, None], rim.shape)
    for i, v in enumerate(days):
        fin = np.isfinite(v)
        o["n_days"] += 1
        o["n_bad_pixels"] += int((~fin).sum())
        cut = rim | near_bad(~fin)
        for t in range(T):
            with np.errstate(invalid="ignore"):
                wet = fin & (v > thr[t])
            o["wet_pixels"][t] += wet.sum(axis=(1, 2))
            if not wet.any():
                o["storms_per_day"][t, 0] += 1
                o["longest_duration"][t, 0] += 1
                continue
            lab = label_day(wet, connectivity, reach)
            if want_labels == t:
                labels[i] = lab
            names, inv, size = np.unique(lab[wet].astype(np.int64), return_inverse=True, return_counts=True)
            vol = np.zeros(len(names), np.int64)
            np.add.at(vol, inv, quantum(v[wet]))
            space = np.zeros(len(names), np.int64)
            np.maximum.at(space, inv, cut[wet].astype(np.int64))
            last = np.zeros(len(names), np.int64)
            np.maximum.at(last, inv, hour[wet])
            start = names // plane
            dur = last - start + 1
            c = space + 2 * ((start == 0) | (last == NHOURS - 1))
            b = np.floor(np.log2(size)).astype(np.int64)                  # (exact: size < 2^53 and log2 of a power of two is exact)
            assert np.all((1 << b) <= size) and np.all(size < (2 << b)) and np.all(dur >= 1)
            np.add.at(o["storms"][t], c, 1)
            np.add.at(o["duration_hist"][t], (c, dur - 1), 1)
            np.add.at(o["start_hour"][t], (c, start), 1)
            np.add.at(o["size_hist"][t], (c, b), 1)
            np.add.at(o["size_sum"][t], c, size)
            np.add.at(o["size_sq_sum"][t], c, size * size)
            np.add.at(o["size_by_duration"][t], (c, dur - 1), size)
            np.add.at(o["volume_by_duration"][t], (c, dur - 1), vol)
            o["storms_per_day"][t, min(len(names), NSPD - 1)] += 1
            o["longest_duration"][t, dur.max()] += 1
    return (o, labels.reshape(np.shape(x))) if want_labels is not None else o


def labels_np(x, threshold, connectivity=8, reach=1):
    """int32 of x's shape"""
    days = days_of(x)
    with np.errstate(invalid="ignore"):
        wet = np.isfinite(days) & (days > np.float32(threshold))
    return np.stack([label_day(w, connectivity, reach) for w in wet]).reshape(np.shape(x))


ORDER = ("wet_pixels", "storms", "duration_hist", "start_hour", "size_hist", "size_sum", "size_sq_sum", "size_by_duration",
         "volume_by_duration", "storms_per_day", "longest_duration")


def flat_state(o):
    """the dict -> the flat int64 state in the order of include/rdgan.h"""
    T = o["wet_pixels"].shape[0]
    per = [np.concatenate([np.asarray(o[k][t]).ravel() for k in ORDER]) for t in range(T)]
    return np.concatenate(per + [np.array([o["n_days"], o["n_bad_pixels"]], np.int64)]).astype(np.int64)


def only_nonzero(a):
    """the indices of the non-zero entries with their values"""
    return {tuple(int(i) for i in ix): int(a[tuple(ix)]) for ix in np.argwhere(a)}


def check_identities(o):
    for t in range(o["wet_pixels"].shape[0]):
        assert o["size_sum"][t].sum() == o["wet_pixels"][t].sum() == o["size_by_duration"][t].sum()
        assert np.array_equal(o["duration_hist"][t].sum(axis=-1), o["storms"][t])
        assert np.array_equal(o["start_hour"][t].sum(axis=-1), o["storms"][t])
        assert np.array_equal(o["size_hist"][t].sum(axis=-1), o["storms"][t])
        assert o["storms_per_day"][t].sum() == o["n_days"] == o["longest_duration"][t].sum()
        assert o["storms_per_day"][t, 0] == o["longest_duration"][t, 0]
        assert o["size_sq_sum"][t].sum() >= o["size_sum"][t].sum()
        # a storm without time_edge starts after hour 0 and ends before hour 23
        assert o["start_hour"][t, :2, 0].sum() == 0 and o["duration_hist"][t, :2, 22:].sum() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# patterns, (24, ny, nx) float32 with 1.0 on the figure and 0.0 elsewhere
def stepping_pixel(ny, nx, row=None, col=0):
    """one wet pixel per hour that steps one column per hour along a row (the middle one unless given), from column col"""
    a = np.zeros((NHOURS, ny, nx), np.float32)
    a[np.arange(NHOURS), ny // 2 if row is None else row, col + np.arange(NHOURS)] = 1
    return a


def inverting_checkerboard(ny, nx):
    """a checkerboard whose colours swap every hour: no wet pixel is wet in the next hour"""
    h, y, x = np.indices((NHOURS, ny, nx))
    return ((h + y + x) % 2 == 0).astype(np.float32)


def staircase(first, ny, nx):
    """`first` (ny, nx) in hour 0, then its last wet pixel alone, stepping one pixel per hour back along the flat order (a
    one-pixel step in a row; the row changes with a jump, so the stairs break there unless the reach bridges it)"""
    a = np.zeros((NHOURS, ny, nx), np.float32)
    a[0] = first
    p = int(np.flatnonzero(first.ravel())[-1])
    for h in range(1, NHOURS):
        a[h].ravel()[max(p - h, 0)] = 1
    return a
