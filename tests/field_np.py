"""numpy restatement of whole-field disaggregation (pr_disagg_radar_gan_amd/field.py, csrc/rdgan_field.hip.h), written from the
rules and not from the product code: the tile plan, the blending weights, the tile scan, the condition batch and the blend, all in
fp64 (the product stores the weights as fp32; the restatement keeps them in fp64, so its weights sum to 1 to fp64 rounding)."""
import numpy as np

NHOURS = 24


def origins_1d(L, nd, overlap):
    """0, s, 2s, ... while o + nd <= L; if the last of those ends before L, one more at L - nd"""
    if L < nd or not 0 <= overlap <= nd // 2:
        raise ValueError((L, nd, overlap))
    s = nd - overlap
    out, o = [], 0
    while o + nd <= L:
        out.append(o)
        o += s
    if out[-1] + nd < L:
        out.append(L - nd)
    return out


def cover_1d(L, nd, origins):
    """per coordinate the list of (tile index, weight): p = min(y - o + 1, o + nd - y), w = p / sum p, fp64"""
    table = []
    for y in range(L):
        ent = [(i, float(min(y - o + 1, o + nd - y))) for i, o in enumerate(origins) if o <= y < o + nd]
        tot = sum(p for _, p in ent)
        table.append([(i, np.float64(p) / np.float64(tot)) for i, p in ent])
    return table


class Plan:
    def __init__(self, ny, nx, nd, overlap):
        self.ny, self.nx, self.nd, self.overlap = ny, nx, nd, overlap
        self.yo, self.xo = origins_1d(ny, nd, overlap), origins_1d(nx, nd, overlap)
        self.ycov, self.xcov = cover_1d(ny, nd, self.yo), cover_1d(nx, nd, self.xo)
        self.n_ty, self.n_tx = len(self.yo), len(self.xo)
        self.n_tiles = self.n_ty * self.n_tx

    def origin(self, tile):
        return self.yo[tile // self.n_tx], self.xo[tile % self.n_tx]


def scan(daily, plan):
    """counts (D, T, 3): wet (finite and > 0), NaN, bad (negative or infinite) pixels per (day, tile)"""
    D, nd = daily.shape[0], plan.nd
    counts = np.zeros((D, plan.n_tiles, 3), dtype=np.int32)
    for d in range(D):
        for t in range(plan.n_tiles):
            oy, ox = plan.origin(t)
            v = daily[d, oy:oy + nd, ox:ox + nd]
            with np.errstate(invalid="ignore"):
                counts[d, t] = (np.sum(np.isfinite(v) & (v > 0)), np.sum(np.isnan(v)), np.sum((v < 0) | np.isinf(v)))
    return counts


def active_entries(daily, plan):
    """the (day, tile) pairs holding at least one finite pixel > 0, as day * T + tile, ascending"""
    return np.flatnonzero(scan(daily, plan)[..., 0].reshape(-1) > 0).astype(np.int32)


def cond_batch(daily, plan, entries, norm_scale):
    """(m, nd, nd, 1) float32: daily / norm_scale as generate_scenarios forms it (fp64 quotient, then the cast to fp32 predict
    applies), NaN entering as 0"""
    nd = plan.nd
    out = np.empty((len(entries), nd, nd, 1), dtype=np.float32)
    for k, e in enumerate(entries):
        d, t = divmod(int(e), plan.n_tiles)
        oy, ox = plan.origin(t)
        v = daily[d, oy:oy + nd, ox:ox + nd].astype(np.float64) / np.float64(norm_scale)
        out[k, :, :, 0] = np.where(np.isnan(v), 0.0, v).astype(np.float32)
    return out


def blend(frac, slots, plan, daily, first_unit=0):
    """out (units, 24, ny, nx) float64 = daily * sum over the covering tiles of wy * wx * frac[slot, :, y - oy, x - ox];
    a slot of -1 adds nothing; a dry pixel gives 0 and a NaN pixel NaN whatever frac holds.  Unit u is day (first_unit + u) % D."""
    frac = np.asarray(frac, dtype=np.float64).reshape(-1, NHOURS, plan.nd, plan.nd)
    units, D = slots.shape[0], daily.shape[0]
    out = np.zeros((units, NHOURS, plan.ny, plan.nx), dtype=np.float64)
    for u in range(units):
        day = daily[(first_unit + u) % D].astype(np.float64)
        for y in range(plan.ny):
            for x in range(plan.nx):
                dv = day[y, x]
                if np.isnan(dv):
                    out[u, :, y, x] = np.nan
                    continue
                if dv == 0:
                    continue
                acc = np.zeros(NHOURS)
                for iy, wy in plan.ycov[y]:
                    for ix, wx in plan.xcov[x]:
                        s = slots[u, iy * plan.n_tx + ix]
                        if s >= 0:
                            acc += (wy * wx) * frac[s, :, y - plan.yo[iy], x - plan.xo[ix]]
                out[u, :, y, x] = dv * acc
    return out


def disaggregate(predict, daily, latent, plan, norm_scale, latent_mode="shared"):
    """The whole path around a generator `predict([latent (n, 100), cond (n, nd, nd, 1)]) -> (n, 24, nd, nd, 1)`: daily (D, ny, nx),
    latent (S, D, 100) or (S, D, T, 100).  Every active (scenario, day, tile) goes through predict in ONE batch in plan order
    (scenario, day, tile).  -> (out (S, D, 24, ny, nx) fp64, n_active)"""
    D, T = daily.shape[0], plan.n_tiles
    S = latent.shape[0]
    entries = active_entries(daily, plan)
    by_day = [[int(e) % T for e in entries if int(e) // T == d] for d in range(D)]
    slots = np.full((S * D, T), -1, dtype=np.int64)
    z, ent = [], []
    for u in range(S * D):
        s, d = divmod(u, D)
        for t in by_day[d]:
            slots[u, t] = len(ent)
            ent.append(d * T + t)
            z.append(latent[s, d] if latent_mode == "shared" else latent[s, d, t])
    if not ent:
        frac = np.zeros((1, NHOURS, plan.nd, plan.nd))
    else:
        frac = predict([np.asarray(z, dtype=np.float32), cond_batch(daily, plan, ent, norm_scale)])
    out = blend(frac, slots, plan, daily)
    return out.reshape(S, D, NHOURS, plan.ny, plan.nx), len(entries)


def example_field(rng, D=2, ny=20, nx=30):
    """(D, 20, 30) float32 for nd 16, overlap 4 (y origins 0, 4; x origins 0, 12, 14; tile = iy * 3 + ix): a dry region that swallows
    whole tiles, a NaN block across a tile border and one wet pixel alone in an otherwise dry tile"""
    daily = rng.gamma(0.6, 8.0, (D, ny, nx)).astype(np.float32) + np.float32(0.01)
    daily[0, :, 12:] = 0.0                   # day 0: the four tiles at x origin 12 and 14 are dry
    daily[0, 2:7, 10:14] = np.nan            # a NaN block across y = 4 and x = 12, partly inside the dry tiles
    daily[1, :, :16] = 0.0                   # day 1: the two tiles at x origin 0 are dry ...
    daily[1, 2, 3] = 7.5                     # ... but for one wet pixel, which tile 0 (rows 0 .. 15) holds and tile 3 (rows 4 .. 19) does not
    return daily
