"""Disaggregate whole daily fields (csrc/rdgan_field.hip.h): a daily precipitation map of any size
ny, nx >= ndomain is cut into overlapping ndomain x ndomain tiles, every tile that holds rain goes through the generator, and the
tiles' hourly fractions are blended across the overlaps on the device.  Each tile's fractions sum to 1 over the hours and the
blending weights sum to 1 at every pixel, so every pixel's 24 values sum to its daily value: mass is conserved by construction.

No CPU fallback: without a visible MI355X disaggregate and blend_device raise RdganError; argument errors are ValueErrors raised
before any device call."""
from dataclasses import dataclass, field as _dc_field

import numpy as np
import torch

from . import _lib, models
from . import weights as W
from ._dev import host_ptr as _hp, ptr as _p, stream as _stream
from .engine import require_gpu

MAX_COVER = 3                   # RD_FIELD_COVER of csrc/rdgan_field.hip.h: tiles covering a coordinate per axis
LATENT_MODES = ("shared", "independent")


def axis_origins(L, ndomain, overlap):
    """Tile origins along an axis of length L: 0, s, 2s, ... (s = ndomain - overlap) while the tile fits, plus one tile flush with
    the end when the last of those stops short of it."""
    L, nd, overlap = int(L), int(ndomain), int(overlap)
    if nd < 1 or L < nd:
        raise ValueError(f"the field must be at least one tile wide: axis length {L} < ndomain {nd}")
    if not 0 <= overlap <= nd // 2:
        raise ValueError(f"overlap must lie in 0 .. ndomain / 2 = {nd // 2}, got {overlap}")
    s = nd - overlap
    origins = list(range(0, L - nd + 1, s))
    if origins[-1] + nd < L:
        origins.append(L - nd)
    return np.asarray(origins, dtype=np.int32)


def axis_table(L, ndomain, origins):
    """(idx, w): idx (L, 3) int32, the tiles covering each coordinate in ascending order (-1: fewer than 3), and w (L, 3) float32,
    their weights: the profile p = min(y - o + 1, o + ndomain - y) of each covering tile over the sum of the profiles, taken in fp64
    and stored as fp32.  One covering tile gives exactly 1."""
    nd = int(ndomain)
    idx = np.full((L, MAX_COVER), -1, dtype=np.int32)
    w = np.zeros((L, MAX_COVER), dtype=np.float32)
    for y in range(L):
        cover = [i for i, o in enumerate(origins) if o <= y < o + nd]
        if not 1 <= len(cover) <= MAX_COVER:
            raise ValueError(f"coordinate {y} is covered by {len(cover)} tiles")           # (cannot happen for overlap <= nd / 2)
        p = np.array([min(y - int(origins[i]) + 1, int(origins[i]) + nd - y) for i in cover], dtype=np.float64)
        idx[y, :len(cover)] = cover
        w[y, :len(cover)] = (p / p.sum()).astype(np.float32)
    return idx, w


@dataclass
class TilePlan:
    """The tiling of an (ny, nx) field: origins per axis, tiles numbered y-major (tile = iy * n_tx + ix), and the per-axis tables
    of (covering tile, weight) the blend kernel reads.  The tables are uploaded once per device (device_tables)."""
    ny: int
    nx: int
    ndomain: int
    overlap: int
    y_origins: np.ndarray
    x_origins: np.ndarray
    ytab_idx: np.ndarray
    ytab_w: np.ndarray
    xtab_idx: np.ndarray
    xtab_w: np.ndarray
    _device: dict = _dc_field(default_factory=dict, repr=False, compare=False)

    @property
    def n_ty(self):
        return len(self.y_origins)

    @property
    def n_tx(self):
        return len(self.x_origins)

    @property
    def n_tiles(self):
        return self.n_ty * self.n_tx

    def origins(self):
        """(n_tiles, 2) int32: (oy, ox) of every tile in plan order"""
        oy, ox = np.meshgrid(self.y_origins, self.x_origins, indexing="ij")
        return np.stack([oy.ravel(), ox.ravel()], axis=1).astype(np.int32)

    def device_tables(self, device):
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                                      for a in (self.ytab_idx, self.ytab_w, self.xtab_idx, self.xtab_w))
        return self._device[key]


def tile_plan(ny, nx, ndomain, overlap):
    """The tile plan of an (ny, nx) field for a generator of `ndomain`: host code, no device call.  ValueError for ny or nx <
    ndomain and for an overlap outside 0 .. ndomain / 2."""
    ny, nx, nd, overlap = int(ny), int(nx), int(ndomain), int(overlap)
    yo, xo = axis_origins(ny, nd, overlap), axis_origins(nx, nd, overlap)
    yi, yw = axis_table(ny, nd, yo)
    xi, xw = axis_table(nx, nd, xo)
    return TilePlan(ny, nx, nd, overlap, yo, xo, yi, yw, xi, xw)


@dataclass
class FieldInfo:
    """What disaggregate met: tiles per day, (day, tile) pairs that held rain and went through the generator, NaN pixels of the
    input (their 24 output values are NaN)."""
    n_tiles: int
    n_active: int
    n_nan_pixels: int


def _check_f32_cuda(t, shape, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous float32 CUDA tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def blend_device(frac, slots, plan, daily, first_unit=0, out=None):
    """The blend kernel alone.  frac (m, 24, nd, nd) float32 CUDA (a trailing axis of 1 is accepted: the generator's output as it
    stands); slots (units, n_tiles) integers, numpy: the row of frac holding each (unit, tile), -1 for a skipped tile; daily
    (n_days, ny, nx) float32 CUDA; unit u is day (first_unit + u) % n_days.  Returns out (units, 24, ny, nx) float32 CUDA:
    out[u, h, y, x] = daily[day, y, x] * sum over the covering tiles of wy * wx * frac[slot, h, y - oy, x - ox]."""
    nd = plan.ndomain
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    if slots.ndim != 2 or slots.shape[0] < 1 or slots.shape[1] != plan.n_tiles:
        raise ValueError(f"slots must have shape (units, {plan.n_tiles}), got {slots.shape}")
    if isinstance(frac, torch.Tensor) and frac.dim() == 5 and frac.shape[-1] == 1:
        frac = frac.view(frac.shape[:-1])
    m = int(frac.shape[0]) if hasattr(frac, "shape") and len(frac.shape) else 0
    if slots.min() < -1 or slots.max() >= m:
        raise ValueError(f"slots must lie in -1 .. {m - 1}")
    require_gpu()
    lib = _lib.load()
    _check_f32_cuda(frac, (m, W.NHOURS, nd, nd), "frac")
    if not (isinstance(daily, torch.Tensor) and daily.dim() == 3):
        raise ValueError("daily: expected a (n_days, ny, nx) CUDA tensor")
    _check_f32_cuda(daily, (daily.shape[0], plan.ny, plan.nx), "daily")
    units = slots.shape[0]
    if out is None:
        out = torch.empty((units, W.NHOURS, plan.ny, plan.nx), dtype=torch.float32, device=frac.device)
    _check_f32_cuda(out, (units, W.NHOURS, plan.ny, plan.nx), "out")
    yi, yw, xi, xw = plan.device_tables(frac.device)
    rc = lib.rdgan_field_blend(_p(frac), m, _hp(slots), units, int(first_unit), _p(yi), _p(yw), _p(xi), _p(xw), _p(daily),
                               int(daily.shape[0]), plan.ny, plan.nx, nd, plan.overlap, _p(out), _stream(frac))
    _lib.check(rc, None, "rdgan_field_blend")
    return out


def scan_device(daily, plan):
    """counts (n_days, n_tiles, 3) int32 CUDA: wet (finite, > 0), NaN and bad (negative or infinite) pixels per (day, tile)."""
    require_gpu()
    lib = _lib.load()
    _check_f32_cuda(daily, (daily.shape[0], plan.ny, plan.nx), "daily")
    counts = torch.empty((daily.shape[0], plan.n_tiles, 3), dtype=torch.int32, device=daily.device)
    rc = lib.rdgan_field_scan(_p(daily), int(daily.shape[0]), plan.ny, plan.nx, plan.ndomain, plan.overlap, _p(counts), _stream(daily))
    _lib.check(rc, None, "rdgan_field_scan")
    return counts


def cond_device(daily, plan, entries, norm_scale=W.NORM_SCALE, out=None):
    """The normalised condition batch (m, nd, nd, 1) float32 CUDA of the (day, tile) pairs entries[i] = day * n_tiles + tile:
    daily / norm_scale (the fp64 quotient rounded to fp32, as generate_scenarios forms it), NaN entering as 0."""
    entries = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1)
    m, nd = entries.shape[0], plan.ndomain
    if m < 1 or entries.min() < 0 or entries.max() >= daily.shape[0] * plan.n_tiles:
        raise ValueError("entries must be a non-empty list of day * n_tiles + tile")
    require_gpu()
    lib = _lib.load()
    _check_f32_cuda(daily, (daily.shape[0], plan.ny, plan.nx), "daily")
    if out is None:
        out = torch.empty((m, nd, nd, 1), dtype=torch.float32, device=daily.device)
    _check_f32_cuda(out, (m, nd, nd, 1), "cond out")
    rc = lib.rdgan_field_cond(_p(daily), int(daily.shape[0]), plan.ny, plan.nx, nd, plan.overlap, _hp(entries), m,
                              float(norm_scale), _p(out), _stream(daily))
    _lib.check(rc, None, "rdgan_field_cond")
    return out


def _group_units(rows_per_unit, chunk):
    """Consecutive units grouped so that a group holds at most `chunk` generator rows -- but at least one whole unit.
    -> [(u0, u1)], every unit in exactly one group, in order."""
    groups, u0, rows = [], 0, 0
    for u, r in enumerate(rows_per_unit):
        if u > u0 and rows + r > chunk:
            groups.append((u0, u))
            u0, rows = u, 0
        rows += r
    groups.append((u0, len(rows_per_unit)))
    return groups


def _check_request(gen, daily, n_scenarios, overlap, latent_mode, latent, chunk, norm_scale):
    """The argument checks of disaggregate (and of field_products.disaggregate_peaks), host code only.
    -> (daily, squeeze_day, D, ny, nx, plan, z_shape)"""
    nd = int(gen.ndomain)
    n_scenarios, chunk = int(n_scenarios), int(chunk)
    if int(getattr(gen, "n_cond_channels", 1)) != 1:
        raise ValueError("disaggregate takes a generator with one condition channel (extra channels have no field form)")
    if latent_mode not in LATENT_MODES:
        raise ValueError(f"latent_mode must be one of {LATENT_MODES}, got {latent_mode!r}")
    if n_scenarios < 1 or chunk < 1:
        raise ValueError("n_scenarios and chunk must be at least 1")
    if not float(norm_scale) > 0:
        raise ValueError("norm_scale must be positive")
    if hasattr(daily, "daily_plane"):
        daily = daily.daily_plane()
    if isinstance(daily, torch.Tensor) and not daily.is_cuda:
        raise ValueError("daily: expected a numpy array, a CUDA tensor or a DeviceDataset")
    shape = tuple(daily.shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"daily must have shape (ny, nx) or (n_days, ny, nx), got {shape}")
    squeeze_day = len(shape) == 2
    D, ny, nx = (1,) + shape if squeeze_day else shape
    if D < 1:
        raise ValueError("daily holds no day")
    plan = tile_plan(ny, nx, nd, overlap)
    T, S = plan.n_tiles, n_scenarios
    z_shape = (S, D, W.LATENT_DIM) if latent_mode == "shared" else (S, D, T, W.LATENT_DIM)
    if latent is not None and tuple(np.shape(latent)) != z_shape:
        raise ValueError(f"latent must have shape {z_shape} for latent_mode {latent_mode!r}, got {tuple(np.shape(latent))}")
    return daily, squeeze_day, D, ny, nx, plan, z_shape


def _scan_request(daily, D, ny, nx, plan):
    """The daily plane on the device and what the tile scan found.  -> (dd (D, ny, nx) float32 CUDA, info, active_tiles per day)"""
    require_gpu()
    if isinstance(daily, torch.Tensor):
        dd = daily.detach().to(torch.float32).contiguous().view(D, ny, nx)
    else:
        dd = torch.from_numpy(np.ascontiguousarray(daily, dtype=np.float32).reshape(D, ny, nx)).cuda()
    T = plan.n_tiles
    # which tiles hold rain: D * T * 3 counts and the number of NaN pixels, in one copy
    with torch.cuda.device(dd.device):
        counts = scan_device(dd, plan)
        n_nan = torch.isnan(dd).sum().to(torch.int32).view(1)
        host = torch.cat([counts.view(-1), n_nan]).cpu().numpy()
    counts_h, n_nan_pixels = host[:-1].reshape(D, T, 3), int(host[-1])
    if counts_h[..., 2].any():
        raise ValueError("daily holds negative or infinite values")
    active = counts_h[..., 0] > 0                                   # (D, T)
    info = FieldInfo(n_tiles=T, n_active=int(active.sum()), n_nan_pixels=n_nan_pixels)
    return dd, info, [np.flatnonzero(active[d]).astype(np.int32) for d in range(D)]


def _draw_latent(latent, seed, z_shape, dev):
    """The latent array of a request, on the device: `latent` as given, else z_shape draws from the global numpy RNG (as
    generate_scenarios draws them), or from a device generator when `seed` is given.  Called with the device current."""
    if latent is not None:
        return torch.as_tensor(latent, dtype=torch.float32).to(dev)
    if seed is None:
        return torch.from_numpy(np.random.normal(size=z_shape).astype(np.float32)).to(dev)
    g = torch.Generator(device=dev); g.manual_seed(int(seed))
    return torch.randn(z_shape, generator=g, device=dev)


def _run_groups(gen, dd, plan, S, active_tiles, latent_mode, seed, latent, z_shape, chunk, norm_scale, blend, dry):
    """The group loop disaggregate and field_products.disaggregate_peaks share: units u = scenario * D + day in order, grouped by
    _group_units; per group the condition batch, the latent rows and the generator in batches of at most `chunk` tiles, then
    blend(frac (m, 24, nd, nd, 1), slots (u1 - u0, T), u0, u1) -- or dry(u0, u1) for a group without a wet tile."""
    nd, T, D, dev = plan.ndomain, plan.n_tiles, int(dd.shape[0]), dd.device
    rows_per_unit = [len(active_tiles[u % D]) for u in range(S * D)]            # unit u = scenario * D + day
    with torch.cuda.device(dev):
        z_all = _draw_latent(latent, seed, z_shape, dev).reshape(-1, W.LATENT_DIM).contiguous()      # row u (shared) or u * T + tile (independent)

        groups = _group_units(rows_per_unit, chunk)
        max_rows = max(sum(rows_per_unit[u0:u1]) for u0, u1 in groups)
        eng = models.get_engine(nd, min(chunk, max_rows))           # (grows only when a bigger batch is asked for)
        slab = gen.device_slab(eng)
        version = getattr(gen, "_version", 0)
        frac = torch.empty((max_rows, W.NHOURS, nd, nd, 1), dtype=torch.float32, device=dev)
        cond = torch.empty((max_rows, nd, nd, 1), dtype=torch.float32, device=dev)
        for u0, u1 in groups:
            slots = np.full((u1 - u0, T), -1, dtype=np.int32)
            entries, zrows, m = [], [], 0
            for u in range(u0, u1):
                d, tiles = u % D, active_tiles[u % D]
                slots[u - u0, tiles] = np.arange(m, m + len(tiles), dtype=np.int32)
                entries.append(d * T + tiles)
                zrows.append(np.full(len(tiles), u, dtype=np.int64) if latent_mode == "shared" else u * T + tiles.astype(np.int64))
                m += len(tiles)
            if m == 0:                                              # a run of dry days
                dry(u0, u1)
                continue
            cond_device(dd, plan, np.concatenate(entries), norm_scale, out=cond[:m])
            z = z_all.index_select(0, torch.from_numpy(np.concatenate(zrows)).to(dev))
            for i in range(0, m, eng.max_batch):
                k = min(eng.max_batch, m - i)
                eng.gen_forward(slab, z[i:i + k].contiguous(), cond[i:i + k], out=frac[i:i + k], gen_version=version)
                eng.check_numerics()             # reference T:349-350
            blend(frac[:m], slots, u0, u1)


def _check_scenarios(n_scenarios, scenario_chunk, max_scenarios=None):
    """The counts of a scenario stream, host code.  -> (S, scenario_chunk) as ints"""
    S, step = int(n_scenarios), int(scenario_chunk)
    if S < 1 or (max_scenarios is not None and S > max_scenarios):
        raise ValueError(f"the number of scenarios must be at least 1{f' and at most {max_scenarios}' if max_scenarios else ''}, got {S}")
    if step < 1:
        raise ValueError("scenario_chunk must be at least 1")
    return S, step


def _stream_scenarios(gen, request, daily, S, scenario_chunk, sink, overlap, latent_mode, seed, latent, chunk, norm_scale):
    """The scenario stream the *_field evaluations share.  request: what _check_request returned for S scenarios; daily: the plane
    to scan (request[0], unless the request was checked on a stand-in).  The latent array is drawn once for all S scenarios, exactly
    as disaggregate draws it -- and, as there, not at all without a wet tile; disaggregate then runs for scenario_chunk scenarios at
    a time into one reused buffer, and sink(buf[:n]) takes each chunk ([D,] 24, ny, nx per scenario) before the next overwrites it."""
    _, squeeze_day, D, ny, nx, plan, z_shape = request
    dd, info, _ = _scan_request(daily, D, ny, nx, plan)
    dev = dd.device
    with torch.cuda.device(dev):
        z_all = _draw_latent(latent, seed, z_shape, dev) if info.n_active else None
        shape = (W.NHOURS, ny, nx) if squeeze_day else (D, W.NHOURS, ny, nx)
        buf = torch.empty((min(scenario_chunk, S),) + shape, dtype=torch.float32, device=dev)
        cond = dd[0] if squeeze_day else dd
        for s0 in range(0, S, scenario_chunk):
            n = min(scenario_chunk, S - s0)
            disaggregate(gen, cond, n, overlap=overlap, latent_mode=latent_mode, latent=None if z_all is None else z_all[s0:s0 + n],
                         chunk=chunk, norm_scale=norm_scale, out=buf[:n])
            sink(buf[:n])


def disaggregate(gen, daily, n_scenarios, overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024,
                 norm_scale=W.NORM_SCALE, out=None):
    """Hourly scenarios for whole daily fields.  daily: (ny, nx) or (n_days, ny, nx) daily sums in mm/day, a numpy array, a CUDA
    tensor or a DeviceDataset (its daily plane is used where it lies); ny, nx >= gen.ndomain.  Returns (fields, info): fields
    (n_scenarios, [n_days,] 24, ny, nx) float32 CUDA in mm/h, whose 24 values sum to the daily value at every pixel, and a FieldInfo.

    The field is tiled by tile_plan(ny, nx, gen.ndomain, overlap).  A tile without a finite pixel > 0 never reaches the generator (a
    dry pixel's output is 0 whatever the fractions are).  A NaN pixel enters the condition as 0 and its 24 output values are NaN.
    A negative or infinite daily value raises ValueError.
    latent_mode "shared": one latent vector per (scenario, day) serves every tile of that day (the reference's same-noise device,
    generate_and_evaluate.py:519-528), so neighbouring tiles do not time their rain independently; "independent": one per
    (scenario, day, tile).  The noise comes from the global numpy RNG, as generate_scenarios draws it, from a device generator
    when `seed` is given, or from `latent`: (n_scenarios, n_days, 100), or (n_scenarios, n_days, n_tiles, 100) for "independent".
    The generator runs in batches of at most `chunk` tiles; whole (scenario, day) units are blended as soon as their tiles are
    there, so the fraction buffer holds a few units, never the ensemble.  out: the tensor to write, of the returned shape."""
    n_scenarios, chunk = int(n_scenarios), int(chunk)
    daily, squeeze_day, D, ny, nx, plan, z_shape = _check_request(gen, daily, n_scenarios, overlap, latent_mode, latent, chunk, norm_scale)
    S = n_scenarios
    out_shape = (S, W.NHOURS, ny, nx) if squeeze_day else (S, D, W.NHOURS, ny, nx)
    if out is not None:
        _check_f32_cuda(out, out_shape, "out")

    dd, info, active_tiles = _scan_request(daily, D, ny, nx, plan)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=dd.device)
    out_units = out.view(S * D, W.NHOURS, ny, nx)
    if info.n_active == 0:                                          # nothing to generate: zeros and NaNs straight from the plane
        out_units.copy_((dd * 0.0)[None, :, None].expand(S, D, W.NHOURS, ny, nx).reshape(S * D, W.NHOURS, ny, nx))
        return out, info

    def blend(frac, slots, u0, u1):
        blend_device(frac, slots, plan, dd, first_unit=u0, out=out_units[u0:u1])

    def dry(u0, u1):
        out_units[u0:u1].copy_(torch.stack([dd[u % D] * 0.0 for u in range(u0, u1)])[:, None].expand(-1, W.NHOURS, -1, -1))

    _run_groups(gen, dd, plan, S, active_tiles, latent_mode, seed, latent, z_shape, chunk, norm_scale, blend, dry)
    return out, info
