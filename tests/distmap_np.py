"""The yardstick of the distance-map verification (pr_disagg_radar_gan_amd/distmap.py, csrc/rdgan_distmap.hip.h), written from the
definition of DESIGN.md section 30 in explicit numpy.  d2 by brute force over every pair (pixel, set pixel) for planes up to
BRUTE_PIXELS pixels, by a separable min over rows above (checked against the brute force on the small ones by
tests/test_distmap_host.py); D by math.isqrt; the records by plain masked sums."""
import math

import numpy as np

BRUTE_PIXELS = 9000
EMPTY = 0xFFFF
NREC = 12


def events(a, u):
    """the set of threshold u: finite and above the fp32 rounding of u"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (a.astype(np.float32) > np.float32(u))


def d2_brute(mask):
    """(ny, nx) bool -> int64 (ny, nx): min over the set pixels of dy^2 + dx^2; None for an empty set"""
    ny, nx = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return None
    dy2 = (np.arange(ny, dtype=np.int64)[:, None] - ys[None, :]) ** 2          # (ny, K)
    dx2 = (np.arange(nx, dtype=np.int64)[:, None] - xs[None, :]) ** 2          # (nx, K)
    out = np.empty((ny, nx), np.int64)
    for y in range(ny):
        out[y] = (dx2 + dy2[y][None, :]).min(axis=1)
    return out


def d2_separable(mask):
    """the same by rows: g(y, x) the distance to the nearest set pixel of row y, then min over y' of (y - y')^2 + g(y', x)^2"""
    ny, nx = mask.shape
    if not mask.any():
        return None
    big = 1 << 20                                                           # "no set pixel in this row": its square dwarfs any d2
    col = np.arange(nx, dtype=np.int64)
    g = np.where(mask[:, None, :], np.abs(col[:, None] - col[None, :])[None], big).min(axis=2)      # (ny, nx)
    g2 = g * g
    rows = np.arange(ny, dtype=np.int64)
    out = np.empty((ny, nx), np.int64)
    for y0 in range(0, ny, 64):
        dy2 = (rows[y0:y0 + 64, None] - rows[None, :]) ** 2                   # (chunk, ny)
        out[y0:y0 + 64] = (dy2[:, :, None] + g2[None]).min(axis=1)
    return out


def d2_np(mask):
    return d2_brute(mask) if mask.size <= BRUTE_PIXELS else d2_separable(mask)


def quantise(d2):
    """D = isqrt(256 d2) elementwise through Python integers; None -> None"""
    if d2 is None:
        return None
    u, inv = np.unique(d2, return_inverse=True)
    table = np.array([math.isqrt(256 * int(v)) for v in u], np.int64)
    return table[inv].reshape(d2.shape)


def plane_maps(plane, thresholds):
    """(ny, nx) -> (D (T, ny, nx) int64 with EMPTY for an empty set, sizes (T,))"""
    out = np.full((len(thresholds),) + plane.shape, EMPTY, np.int64)
    sizes = np.zeros(len(thresholds), np.int64)
    for t, u in enumerate(thresholds):
        m = events(plane, u)
        sizes[t] = m.sum()
        if sizes[t]:
            out[t] = quantise(d2_np(m))
    return out, sizes


def maps_np(hourly, thresholds):
    """hourly (..., 24, ny, nx) -> (maps uint16 (..., 24, T, ny, nx), set_sizes int64 (..., 24, T))"""
    hourly = np.asarray(hourly, np.float32)
    lead, (ny, nx), T = hourly.shape[:-2], hourly.shape[-2:], len(thresholds)
    flat = hourly.reshape(-1, ny, nx)
    maps, sizes = np.empty((flat.shape[0], T, ny, nx), np.uint16), np.empty((flat.shape[0], T), np.int64)
    for i, plane in enumerate(flat):
        m, sizes[i] = plane_maps(plane, thresholds)
        assert m.max() <= EMPTY
        maps[i] = m
    return maps.reshape(lead + (T, ny, nx)), sizes.reshape(lead + (T,))


def default_cutoff16(ny, nx):
    """ceil(16 hypot(ny - 1, nx - 1)), at least 16, in integers"""
    v = 256 * ((ny - 1) ** 2 + (nx - 1) ** 2)
    r = math.isqrt(v)
    return max(16, r + (r * r != v))


def pair_record(x, o, DA, DB, u, C):
    """the twelve fields of one pair at one threshold; DA, DB int64 (ny, nx) with EMPTY for an empty set"""
    badx, bado = ~np.isfinite(x), ~np.isfinite(o)
    valid = ~badx & ~bado
    A, B = events(x, u), events(o, u)
    emptyA, emptyB = not A.any(), not B.any()
    rec = np.zeros(NREC, np.int64)
    rec[0], rec[1], rec[2], rec[3] = valid.sum(), (A & valid).sum(), (B & valid).sum(), (A & B & valid).sum()
    if not emptyA and (B & valid).any():
        rec[4], rec[6] = DA[B & valid].sum(), DA[B & valid].max()
    if not emptyB and (A & valid).any():
        rec[5], rec[7] = DB[A & valid].sum(), DB[A & valid].max()
    if valid.any():
        d = np.abs(np.minimum(DA, C) - np.minimum(DB, C))[valid]
        rec[8], rec[9], rec[10] = d.sum(), (d * d).sum(), d.max()
    rec[11] = int(np.any(badx != bado)) | (2 if emptyA else 0) | (4 if emptyB else 0)
    return rec


def records_np(members, obs, thresholds, C=None):
    """members (s, [D,] 24, ny, nx), obs ([D,] 24, ny, nx) -> records (s, D, 24, T, 12) int64; C: the cutoff in 1/16 pixel, None:
    the diagonal"""
    members, obs = np.asarray(members, np.float32), np.asarray(obs, np.float32)
    ny, nx = obs.shape[-2:]
    C = default_cutoff16(ny, nx) if C is None else C
    o = obs.reshape(-1, 24, ny, nx)
    m = members.reshape(members.shape[0], -1, 24, ny, nx)
    T = len(thresholds)
    out = np.zeros((m.shape[0], o.shape[0], 24, T, NREC), np.int64)
    for d in range(o.shape[0]):
        for h in range(24):
            DB, _ = plane_maps(o[d, h], thresholds)
            for s in range(m.shape[0]):
                DA, _ = plane_maps(m[s, d, h], thresholds)
                for t, u in enumerate(thresholds):
                    out[s, d, h, t] = pair_record(m[s, d, h], o[d, h], DA[t], DB[t], u, C)
    return out
