"""The yardstick of the cell tests: the definitions of DESIGN.md section 18 restated in numpy and plain Python -- a flood fill per
plane, no scipy.  The reference project has no such code."""
import numpy as np

NBINS, NKPP = 25, 65


def planes_of(x):
    """(..., 24, ny, nx) -> (n * 24, ny, nx) float32"""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim >= 3 and x.shape[-3] == 24
    return x.reshape((-1,) + x.shape[-2:])


def label_plane(wet, connectivity):
    """wet (ny, nx) bool -> int32 (ny, nx): the smallest flat index of the pixel's cell, -1 where dry.  Pixels are visited in flat
    order, so the seed of a fill is the smallest index of its cell."""
    ny, nx = wet.shape
    lab = np.full((ny + 2) * (nx + 2), -1, np.int64)
    pad = np.zeros((ny + 2, nx + 2), bool)
    pad[1:-1, 1:-1] = wet
    todo = pad.ravel().copy()
    w = nx + 2
    steps = (-w, -1, 1, w) if connectivity == 4 else (-w - 1, -w, -w + 1, -1, 1, w - 1, w, w + 1)
    for seed in np.flatnonzero(todo):
        if not todo[seed]:
            continue
        name = (seed // w - 1) * nx + seed % w - 1
        todo[seed] = False
        stack = [seed]
        while stack:
            p = stack.pop()
            lab[p] = name
            for s in steps:
                if todo[p + s]:
                    todo[p + s] = False
                    stack.append(p + s)
    return lab.reshape(ny + 2, nx + 2)[1:-1, 1:-1].astype(np.int32)


def near_bad(bad):
    """bad (ny, nx) bool -> bool: a bad pixel in the 8-neighbourhood (or the pixel itself)"""
    ny, nx = bad.shape
    pad = np.zeros((ny + 2, nx + 2), bool)
    pad[1:-1, 1:-1] = bad
    out = np.zeros((ny, nx), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + ny, dx:dx + nx]
    return out


def quantum(v):
    """q(x) = rint(min(x, 2^20) 2^16) as int64, the product exact in fp64, half to even"""
    return np.rint(np.minimum(v.astype(np.float64), 2.0 ** 20) * 2.0 ** 16).astype(np.int64)


def labels_np(x, threshold, connectivity=8):
    """int32 of x's shape"""
    p = planes_of(x)
    thr = np.float32(threshold)
    out = np.full(p.shape, -1, np.int32)
    for i, v in enumerate(p):
        with np.errstate(invalid="ignore"):
            wet = np.isfinite(v) & (v > thr)
        if wet.any():
            out[i] = label_plane(wet, connectivity)
    return out.reshape(np.shape(x))


def empty_state(T):
    return dict(n_planes=0, n_bad_pixels=0, wet_pixels=np.zeros((T, 24), np.int64), cells=np.zeros((T, 2, 24), np.int64),
                area_hist=np.zeros((T, 2, NBINS), np.int64), area_sum=np.zeros((T, 2), np.int64), area_sq_sum=np.zeros((T, 2), np.int64),
                volume_by_area=np.zeros((T, 2, NBINS), np.int64), cells_per_plane=np.zeros((T, NKPP), np.int64),
                largest_area=np.zeros((T, NBINS), np.int64), dry_planes=np.zeros(T, np.int64), area_by_area=np.zeros((T, 2, NBINS), np.int64))


def cells_np(x, thresholds, connectivity=8, want_labels=None):
    """-> the state as a dict of int64 arrays (and, with want_labels = t, the labels at threshold t as a second value)"""
    p = planes_of(x)
    thr = np.asarray(thresholds, np.float64).astype(np.float32)
    T = len(thr)
    o = empty_state(T)
    labels = np.full(p.shape, -1, np.int32)
    ny, nx = p.shape[1:]
    rim = np.zeros((ny, nx), bool)
    rim[0], rim[-1], rim[:, 0], rim[:, -1] = True, True, True, True
    for i, v in enumerate(p):
        h = i % 24
        fin = np.isfinite(v)
        o["n_planes"] += 1
        o["n_bad_pixels"] += int((~fin).sum())
        cut = rim | near_bad(~fin)
        for t in range(T):
            with np.errstate(invalid="ignore"):
                wet = fin & (v > thr[t])
            o["wet_pixels"][t, h] += int(wet.sum())
            if not wet.any():
                o["cells_per_plane"][t, 0] += 1
                o["dry_planes"][t] += 1
                continue
            lab = label_plane(wet, connectivity)
            if want_labels == t:
                labels[i] = lab
            flat = lab[wet].astype(np.int64)
            names, inv, area = np.unique(flat, return_inverse=True, return_counts=True)
            vol = np.zeros(len(names), np.int64)
            np.add.at(vol, inv, quantum(v[wet]))
            c = np.zeros(len(names), np.int64)
            np.maximum.at(c, inv, cut[wet].astype(np.int64))
            b = np.floor(np.log2(area)).astype(np.int64)                  # (exact: area < 2^53 and log2 of a power of two is exact)
            assert np.all((1 << b) <= area) and np.all(area < (2 << b))
            np.add.at(o["cells"][t, :, h], c, 1)
            np.add.at(o["area_hist"][t], (c, b), 1)
            np.add.at(o["area_sum"][t], c, area)
            np.add.at(o["area_sq_sum"][t], c, area * area)
            np.add.at(o["volume_by_area"][t], (c, b), vol)
            np.add.at(o["area_by_area"][t], (c, b), area)
            o["cells_per_plane"][t, min(len(names), NKPP - 1)] += 1
            o["largest_area"][t, b.max()] += 1
    return (o, labels.reshape(np.shape(x))) if want_labels is not None else o


def flat_state(o):
    """the dict -> the flat int64 state in the order of include/rdgan.h"""
    T = o["wet_pixels"].shape[0]
    per = [np.concatenate([o["wet_pixels"][t].ravel(), o["cells"][t].ravel(), o["area_hist"][t].ravel(), o["area_sum"][t].ravel(),
                           o["area_sq_sum"][t].ravel(), o["volume_by_area"][t].ravel(), o["cells_per_plane"][t].ravel(),
                           o["largest_area"][t].ravel(), o["dry_planes"][t:t + 1], o["area_by_area"][t].ravel()]) for t in range(T)]
    return np.concatenate(per + [np.array([o["n_planes"], o["n_bad_pixels"]], np.int64)]).astype(np.int64)


def check_identities(o):
    for t in range(o["wet_pixels"].shape[0]):
        assert o["area_sum"][t].sum() == o["wet_pixels"][t].sum() == o["area_by_area"][t].sum()
        assert o["area_hist"][t].sum() == o["cells"][t].sum()
        assert np.array_equal(o["area_hist"][t].sum(axis=1), o["cells"][t].sum(axis=1))
        assert o["cells_per_plane"][t].sum() == o["n_planes"]
        assert o["largest_area"][t].sum() + o["dry_planes"][t] == o["n_planes"]
        assert o["cells_per_plane"][t, 0] == o["dry_planes"][t]
        k = np.arange(NKPP - 1)
        assert (o["cells_per_plane"][t, :-1] * k).sum() + 64 * o["cells_per_plane"][t, -1] <= o["cells"][t].sum()
        assert o["area_sq_sum"][t].sum() >= o["area_sum"][t].sum()


# ---------------------------------------------------------------------------------------------------------------------------------
# patterns, (ny, nx) float32 with 1.0 on the figure and 0.0 elsewhere
def spiral(ny, nx):
    """a one-pixel-wide path that winds inwards from (0, 0), turning right where the pixel ahead or the one behind it is taken or
    outside: one long cell with a dry pixel between its turns"""
    a = np.zeros((ny, nx), np.float32)
    inside = lambda y, x: 0 <= y < ny and 0 <= x < nx
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = 1
    while True:
        for _ in range(2):
            y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(y1, x1) and a[y1, x1] == 0 and (not inside(y2, x2) or a[y2, x2] == 0):
                y, x = y1, x1
                a[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return a


def serpentine(ny, nx):
    """wet even rows joined at alternating ends: one cell that runs through every row"""
    a = np.zeros((ny, nx), np.float32)
    a[0::2] = 1
    for k, y in enumerate(range(1, ny - 1, 2)):
        a[y, nx - 1 if k % 2 == 0 else 0] = 1
    return a


def checkerboard(ny, nx):
    yy, xx = np.indices((ny, nx))
    return ((yy + xx) % 2 == 0).astype(np.float32)
