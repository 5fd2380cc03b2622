"""Catchment rainfall of hourly fields (csrc/rdgan_catchment.hip.h): what a rainfall-runoff model sees.  For
a map of basins and every day (or scenario) of an hourly array: the hyetograph of each basin -- its areal rainfall hour by hour --
the largest accumulation of each basin over any k consecutive hours and the hour it starts, and statistics of those maxima over
the days: their mean and maximum, the share of days at or above given levels, the start-hour distribution.  A generator whose peaks
are speckled gets the catchment maxima too low on every real basin although its pixel statistics are right.

A CatchmentMap is built from an integer label map (-1: no catchment) or a stack of boolean masks, where a pixel may lie in several
catchments (nested basins) or in none; an optional `valid` plane drops pixels from every catchment.  Everything is defined in
integers, with the conventions of areal.py: q = rint(x * 1024) in units of 2^-10 mm; a pixel-hour is bad when x is NaN, +-inf,
negative or >= 2048; a catchment-hour that holds a bad pixel-hour is void, and so is every window over it.  A CatchmentRainfall
accumulates, over any number of add() calls, the integer state include/rdgan.h lists for rdgan_catchment_accumulate; the array is
read on the device and never copied to the host, and the state does not depend on how the days were split into calls or on
workspace_days.

Out of scope: fractional pixel weights (a pixel is in a catchment or not), routing and unit hydrographs, plots, and scores of the
series against observations -- series_mm gives the form field_products.member_stats_device and the CRPS functions take.

No CPU fallback: without a visible MI355X the device functions raise RdganError; argument errors are ValueErrors raised before any
device call."""
from dataclasses import dataclass

import numpy as np
import torch

from . import field as F, weights as W
from ._dev import host_ptr as _hp, ptr as _p
from ._hourly import MAX_PLANE, NHOURS, UNIT, HourlyAccumulator, admit, check_out_tensor, div as _div, tv as _tv
from .areal import check_levels, check_windows, check_workspace_days
from .engine import require_gpu

CHUNK = 256                                                                  # RD_CT_CHUNK: list entries of a chunk
MAX_CATCHMENTS = 65535                                                       # RD_CT_MAXCATCH
MAX_ENTRIES = 1 << 26                                                        # RD_CT_MAXENTRIES
MAX_PASS = 65535                                                             # RD_CT_MAXPASS: days of a pass
MAX_GROUPS = (1 << 24) - 1                                                   # RD_CT_MAXGROUPS: workgroups of a launch
N_FIXED = 29                                                                 # RD_CT_FIXED: words of a record besides level_count
# offsets behind level_count[L + 1] in the record of one (c, k) (RD_CT_START ..)
_START, _SUM_A, _MAX_A, _NDAYS, _NVOID, _NDRY = 0, 24, 25, 26, 27, 28
_DEFAULT_PASS_BYTES = 1 << 26                                                # 64 MB of workspace at most by default
DEFAULT_LEVELS = (1.0, 2.0, 5.0, 10.0, 20.0, 50.0, 100.0)                    # mm, of raindisagg_gan_pretrained.catchment_rainfall_field


class CatchmentMap:
    """The catchments of a plane as lists of pixels.  Exactly one of
      regions (ny, nx) integers: -1 no catchment, 0 .. C - 1 the catchment of the pixel (C is the largest label + 1);
      masks (C, ny, nx) booleans: masks[c] the pixels of catchment c; a pixel may lie in several (nested basins) or in none.
    valid (ny, nx) booleans, optional: a pixel that is False there is dropped from every catchment (a permanently blind radar
    pixel must not void a basin for good).  names: C names for messages and for the user, optional.

    Pure numpy until first used on a device: n_catch; npix (C,) int32; offsets (C + 1,) int64 and pixels (E,) int32, the CSR list
    of flat indices y * nx + x, ascending within a catchment; chunks (n_chunks, 3) int32 = (catchment, first entry, count), runs of
    at most CHUNK consecutive entries of one catchment; plane_shape.  Limits: 1 <= C <= 65535, ny nx <= 2^24, E <= 2^26, and every
    catchment keeps at least one pixel -- an empty one is a ValueError that names it."""

    def __init__(self, regions=None, masks=None, valid=None, names=None):
        if (regions is None) == (masks is None):
            raise ValueError("a CatchmentMap takes exactly one of regions and masks")
        if regions is not None:
            regions = np.asarray(regions)
            if regions.ndim != 2 or regions.size < 1 or not np.issubdtype(regions.dtype, np.integer):
                raise ValueError(f"regions: expected a non-empty integer array (ny, nx), got {regions.dtype} {regions.shape}")
            plane_shape = regions.shape
        else:
            masks = np.asarray(masks)
            if masks.ndim != 3 or masks.size < 1 or masks.dtype != np.bool_:
                raise ValueError(f"masks: expected a non-empty boolean array (C, ny, nx), got {masks.dtype} {masks.shape}")
            plane_shape = masks.shape[1:]
        plane = int(plane_shape[0]) * int(plane_shape[1])
        if plane > MAX_PLANE:
            raise ValueError(f"a plane has {plane} pixels, the limit is {MAX_PLANE}")
        if valid is not None:
            valid = np.asarray(valid)
            if valid.dtype != np.bool_ or valid.shape != tuple(plane_shape):
                raise ValueError(f"valid: expected a boolean array of shape {tuple(plane_shape)}, got {valid.dtype} {valid.shape}")
            valid = valid.ravel()
        if regions is not None:
            flat = regions.ravel().astype(np.int64)
            if flat.min() < -1:
                raise ValueError(f"regions: the smallest label is {int(flat.min())}; -1 means no catchment, labels start at 0")
            C = int(flat.max()) + 1
            if C < 1:
                raise ValueError("regions holds no catchment: every label is -1")
            if C <= MAX_CATCHMENTS:
                keep = flat >= 0 if valid is None else (flat >= 0) & valid
                idx = np.flatnonzero(keep)
                labels = flat[idx]
                pixels = idx[np.argsort(labels, kind="stable")]                 # by catchment, ascending within one
                npix = np.bincount(labels, minlength=C)
        else:
            C = int(masks.shape[0])
            if C <= MAX_CATCHMENTS:
                m = masks.reshape(C, plane) if valid is None else masks.reshape(C, plane) & valid[None, :]
                if np.count_nonzero(m) > MAX_ENTRIES:
                    raise ValueError(f"the catchments list {np.count_nonzero(m)} pixels in all, the limit is {MAX_ENTRIES}")
                labels, pixels = np.nonzero(m)                                  # row-major: the same order
                npix = np.bincount(labels, minlength=C)
        if C > MAX_CATCHMENTS:
            raise ValueError(f"{C} catchments, the limit is {MAX_CATCHMENTS}")
        if names is not None:
            names = tuple(str(v) for v in names)
            if len(names) != C:
                raise ValueError(f"names: expected {C} names, got {len(names)}")
        self.names = names
        empty = np.flatnonzero(npix == 0)
        if empty.size:
            c = int(empty[0])
            what = "a gap in the labels" if regions is not None and valid is None else "no pixel is left"
            raise ValueError(f"catchment {c}{f' ({names[c]!r})' if names else ''} is empty: {what}")
        if pixels.size > MAX_ENTRIES:
            raise ValueError(f"the catchments list {pixels.size} pixels in all, the limit is {MAX_ENTRIES}")
        self.n_catch = C
        self.plane_shape = (int(plane_shape[0]), int(plane_shape[1]))
        self.npix = npix.astype(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(npix)]).astype(np.int64)
        self.pixels = pixels.astype(np.int32)
        self.chunks = make_chunks(self.offsets)
        self._device = {}

    @property
    def n_entries(self):
        return int(self.pixels.size)

    def on(self, device):
        """(chunks, pixels, npix) as int32 tensors on `device`, copied once per device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(a).to(device) for a in (self.chunks, self.pixels, self.npix))
        return self._device[device]


def make_chunks(offsets, chunk=CHUNK):
    """offsets (C + 1,) of a CSR list -> (n_chunks, 3) int32 = (catchment, first entry, count): every catchment cut into runs of at
    most `chunk` consecutive entries, in order"""
    offsets = np.asarray(offsets, dtype=np.int64)
    per = (np.diff(offsets) + chunk - 1) // chunk
    catch = np.repeat(np.arange(len(per), dtype=np.int64), per)
    within = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    first = offsets[catch] + within * chunk
    count = np.minimum(chunk, offsets[catch + 1] - first)
    return np.stack([catch, first, count], axis=1).astype(np.int32)


def check_chunks(chunks, offsets, pixels, plane, chunk=CHUNK):
    """What the kernels rely on, host code: the chunks cover every entry once and in order, none crosses a catchment, counts lie in
    1 .. chunk, and every entry is a pixel of the plane.  ValueError otherwise."""
    chunks, offsets, pixels = np.asarray(chunks, np.int64).reshape(-1, 3), np.asarray(offsets, np.int64), np.asarray(pixels, np.int64)
    c, first, count = chunks[:, 0], chunks[:, 1], chunks[:, 2]
    C = len(offsets) - 1
    if len(chunks) < 1 or c.min() < 0 or c.max() >= C:
        raise ValueError("chunks: a catchment index lies outside 0 .. C - 1")
    if count.min() < 1 or count.max() > chunk:
        raise ValueError(f"chunks: a count lies outside 1 .. {chunk}")
    if np.any(first < offsets[c]) or np.any(first + count > offsets[c + 1]):
        raise ValueError("chunks: a chunk crosses a catchment")
    if first[0] != 0 or np.any(first[1:] != first[:-1] + count[:-1]) or first[-1] + count[-1] != len(pixels):
        raise ValueError("chunks: the chunks do not cover the list once and in order")
    if len(pixels) and (pixels.min() < 0 or pixels.max() >= plane):
        raise ValueError(f"pixels: an entry lies outside 0 .. {plane - 1}")


def state_count(n_catch, n_windows, n_levels):
    return n_catch * n_windows * (n_levels + 1 + N_FIXED) + 2


def split_state(counts, n_catch, n_windows, n_levels):
    """the flat state of rdgan_catchment_accumulate (numpy) -> dict of named int64 arrays, (C, K, ...) each"""
    C, K, L = n_catch, n_windows, n_levels
    c = np.asarray(counts, dtype=np.int64)
    if c.shape != (state_count(C, K, L),):
        raise ValueError(f"expected {state_count(C, K, L)} counts, got {c.shape}")
    per = c[:-2].reshape(C, K, L + 1 + N_FIXED)
    fixed = per[:, :, L + 1:]
    word = lambda i: fixed[:, :, i].copy()
    return dict(level_count=per[:, :, :L + 1].copy(), start_hour=fixed[:, :, _START:_SUM_A].copy(), sum_A=word(_SUM_A), max_A=word(_MAX_A),
                n_days=word(_NDAYS), n_void=word(_NVOID), n_dry=word(_NDRY), n_days_total=int(c[-2]), n_bad=int(c[-1]))


@dataclass
class CatchmentStats:
    """What CatchmentRainfall.result returns, numpy on the host, int64; C catchments, K windows, L levels.  level_count
    (C, K, L + 1): counted days by the number of levels the day's maximum reaches; start_hour (C, K, 24): days with rain by the hour
    the wettest window starts; sum_A, max_A, n_days, n_void, n_dry (C, K), depths in 1/1024 mm summed over the catchment's npix
    pixels.  n_days_total and n_bad (bad pixel-hours of the lists) once."""
    windows: tuple
    levels: tuple
    npix: np.ndarray
    names: tuple
    n_days_total: int
    n_bad: int
    level_count: np.ndarray
    start_hour: np.ndarray
    sum_A: np.ndarray
    max_A: np.ndarray
    n_days: np.ndarray
    n_void: np.ndarray
    n_dry: np.ndarray

    def _area(self):
        return np.asarray(self.npix, dtype=np.int64)[:, None]

    def mean_depth(self):
        """(C, K): the mean over the counted days of the largest catchment-mean accumulation, mm; NaN without a counted day"""
        return _div(self.sum_A, self.n_days * self._area() * UNIT)

    def max_depth(self):
        """(C, K): the largest catchment-mean accumulation of any day, mm; NaN without a counted day"""
        return np.where(self.n_days > 0, self.max_A / (self._area() * float(UNIT)), np.nan)

    def exceedance(self):
        """(C, K, L): the share of counted days whose largest catchment-mean accumulation is at or above each level"""
        above = self.level_count[:, :, ::-1].cumsum(axis=2)[:, :, ::-1][:, :, 1:]          # days that reach at least l + 1 levels
        return _div(above, self.n_days[:, :, None])

    def start_hour_distribution(self):
        """(C, K, 24): the share of days with rain whose wettest window starts in hour h"""
        return _div(self.start_hour, self.start_hour.sum(axis=2, keepdims=True))


def compare(a, b):
    """Two CatchmentStats of the same map, windows and levels (real days against generated days) -> dict: the differences a - b of
    mean_depth (C, K) and of exceedance (C, K, L), and the total-variation distance of the start-hour distributions
    (tv_start_hour (C, K))"""
    if not (isinstance(a, CatchmentStats) and isinstance(b, CatchmentStats)):
        raise ValueError("compare takes two CatchmentStats")
    for name in ("windows", "levels"):
        if tuple(getattr(a, name)) != tuple(getattr(b, name)):
            raise ValueError(f"the two statistics have different {name}: {getattr(a, name)} and {getattr(b, name)}")
    if not np.array_equal(a.npix, b.npix):
        raise ValueError("the two statistics belong to different catchment maps")
    return dict(windows=tuple(a.windows), levels=tuple(a.levels), mean_depth=a.mean_depth() - b.mean_depth(),
                exceedance=a.exceedance() - b.exceedance(), tv_start_hour=_tv(a.start_hour_distribution(), b.start_hour_distribution()))


def stats_from_state(counts, npix, windows, levels, names=None):
    """the flat state (numpy) and the pixel counts of the catchments -> CatchmentStats"""
    k, lv = check_windows(windows), check_levels(levels)
    npix = np.asarray(npix, dtype=np.int64)
    if npix.ndim != 1 or npix.size < 1 or npix.min() < 1:
        raise ValueError("npix: expected one positive count per catchment")
    return CatchmentStats(windows=tuple(int(v) for v in k), levels=tuple(float(v) for v in lv), npix=npix,
                          names=None if names is None else tuple(names), **split_state(counts, len(npix), len(k), len(lv)))


def _check_map(cmap):
    if not isinstance(cmap, CatchmentMap):
        raise ValueError("cmap: expected a CatchmentMap")
    return cmap


class CatchmentRainfall(HourlyAccumulator):
    """The state of a catchment-rainfall evaluation on the device.  cmap: the CatchmentMap; windows: the durations k in hours;
    levels: depths in mm of catchment-MEAN accumulation whose exceedance is counted (may be empty); device: where a numpy input
    goes (None: "cuda"; a tensor input fixes it); workspace_days: how many days the workspace holds at a time, 288 bytes per
    catchment -- None: up to 64 MB.  The result does not depend on it.  state(): counts (C K (L + 30) + 2,) int64."""
    entry, workspace_entry, out_name = "rdgan_catchment_accumulate", "rdgan_catchment_workspace_bytes", "series_out"

    def __init__(self, cmap, windows, levels=(), device=None, workspace_days=None):
        self.cmap = _check_map(cmap)
        self.windows, self.levels = check_windows(windows), check_levels(levels)
        self.device = device
        self.workspace_days = check_workspace_days(workspace_days)
        self.reset()

    def add(self, hourly, series_out=None, depths_out=None):
        """hourly (..., 24, ny, nx) float32 in mm/h, (ny, nx) the map's plane: a CUDA tensor or a numpy array, admitted as
        HourlyAccumulator.add admits it.  series_out: None, or a contiguous int64 CUDA tensor (n, C, 24), n the days of hourly,
        that receives the catchment sums in 1/1024 mm, -1 at a void catchment-hour; depths_out: None, or (n, C, K) likewise for the
        days' maxima, -1 for a void day.  Returns self."""
        return super().add(hourly, series_out, depths_out)

    def _state_tensors(self, device):
        self.counts = torch.zeros(state_count(self.cmap.n_catch, len(self.windows), len(self.levels)), dtype=torch.int64, device=device)

    def _check_plane(self, ny, nx, what):
        if (ny, nx) != self.cmap.plane_shape:
            raise ValueError(f"{what}: the plane is {(ny, nx)}, the catchment map's is {self.cmap.plane_shape}")

    def _check_args(self, shape, n, series_out, depths_out=None):
        check_out_tensor(series_out, "series_out", torch.int64, (n, self.cmap.n_catch, NHOURS))
        check_out_tensor(depths_out, "depths_out", torch.int64, (n, self.cmap.n_catch, len(self.windows)))
        if series_out is not None and depths_out is not None and series_out.device != depths_out.device:
            raise ValueError(f"series_out lies on {series_out.device}, depths_out on {depths_out.device}")
        return (depths_out,)

    def _pass_units(self, n, ny, nx):
        per_pass = self.workspace_days or max(1, _DEFAULT_PASS_BYTES // (288 * self.cmap.n_catch))
        return min(per_pass, n, MAX_PASS, max(1, MAX_GROUPS // len(self.cmap.chunks)))

    def _workspace_args(self, n, ny, nx):
        return self.cmap.n_catch, self._pass_units(n, ny, nx)

    def _entry_args(self, ny, nx, series_out, depths_out):
        if depths_out is not None and depths_out.device != self.counts.device:
            raise ValueError(f"depths_out lies on {depths_out.device}, the state on {self.counts.device}")
        chunks, pixels, npix = self.cmap.on(self.counts.device)
        return (ny, nx, _p(chunks), len(self.cmap.chunks), _p(pixels), self.cmap.n_entries, _p(npix), self.cmap.n_catch, _hp(self.windows),
                len(self.windows), _hp(self.levels), len(self.levels), _p(self.counts), _p(series_out), _p(depths_out))

    def result(self):
        """-> CatchmentStats"""
        return stats_from_state(self.state().cpu().numpy(), self.cmap.npix, self.windows, self.levels, self.cmap.names)


def _outputs(cr, hourly, return_series, return_depths):
    """the tensors catchment_rainfall allocates for an admitted array, after every host check"""
    hourly, from_host, shape, n, _ = admit(hourly)
    cr._check_plane(shape[-2], shape[-1], "hourly")
    require_gpu()
    device = "cuda" if from_host else hourly.device
    new = lambda last: torch.empty((n, cr.cmap.n_catch, last), dtype=torch.int64, device=device)
    return hourly, (new(NHOURS) if return_series else None), (new(len(cr.windows)) if return_depths else None)


def catchment_rainfall(hourly, cmap, windows, levels=(), return_series=False, return_depths=False, workspace_days=None):
    """One call for an array that is held: hourly (..., 24, ny, nx).  -> CatchmentStats, followed by series (n, C, 24) with
    return_series and by depths (n, C, K) with return_depths: int64 CUDA tensors in 1/1024 mm summed over the catchment (-1: void),
    for return levels across days or members; series_mm turns the series into catchment-mean mm/h"""
    cr = CatchmentRainfall(cmap, windows, levels, workspace_days=workspace_days)
    if not (return_series or return_depths):
        return cr.add(hourly).result()
    hourly, series, depths = _outputs(cr, hourly, return_series, return_depths)
    stats = cr.add(hourly, series_out=series, depths_out=depths).result()
    return (stats,) + tuple(t for t in (series, depths) if t is not None)


def series_mm(series, cmap):
    """series (..., C, 24) int64 CUDA, as series_out or catchment_rainfall return it -> float32 CUDA of the same shape: the
    catchment-mean rainfall in mm/h, series / (1024 npix), NaN where the catchment-hour is void (-1).  The form
    field_products.member_stats_device takes for quantiles across members, and a runoff model as input."""
    cmap = _check_map(cmap)
    if not (isinstance(series, torch.Tensor) and series.is_cuda and series.dtype == torch.int64 and series.dim() >= 2
            and tuple(series.shape[-2:]) == (cmap.n_catch, NHOURS)):
        raise ValueError(f"series: expected an int64 CUDA tensor of shape (..., {cmap.n_catch}, {NHOURS})")
    area = cmap.on(series.device)[2].to(torch.float64)[:, None] * float(UNIT)
    mm = (series.to(torch.float64) / area).to(torch.float32)
    return torch.where(series < 0, torch.full_like(mm, float("nan")), mm)


def catchment_rainfall_field(gen, daily, n_scenarios, cmap, windows, levels=(), return_series=False, workspace_days=None, scenario_chunk=16,
                             overlap=4, latent_mode="shared", seed=None, latent=None, chunk=1024, norm_scale=W.NORM_SCALE):
    """Disaggregate a daily map ([D,] ny, nx) into n_scenarios scenarios and take their catchment rainfall without holding them:
    the scenario stream of _hourly.evaluate_field, which says how the scenarios are drawn and what the result equals, on a
    CatchmentRainfall.  -> CatchmentStats, or (CatchmentStats, series) with return_series: series (n_scenarios, [D,] C, 24) int64
    CUDA, every scenario's hyetographs (series_mm: in mm/h) -- a few MB where the hourly ensemble would be GB."""
    cr = CatchmentRainfall(cmap, windows, levels, workspace_days=workspace_days)
    S, step = F._check_scenarios(n_scenarios, scenario_chunk)
    req = F._check_request(gen, daily, S, overlap, latent_mode, latent, chunk, norm_scale)
    squeeze_day, D = req[1], req[2]
    cr._check_plane(req[3], req[4], "daily")
    series, done = None, 0

    def sink(buf):
        nonlocal series, done
        n = int(buf.shape[0])
        if return_series and series is None:
            series = torch.empty((S, D, cr.cmap.n_catch, NHOURS), dtype=torch.int64, device=buf.device)
        cr.add(buf, series_out=series[done:done + n].view(n * D, cr.cmap.n_catch, NHOURS) if return_series else None)
        done += n

    F._stream_scenarios(gen, req, req[0], S, step, sink, overlap, latent_mode, seed, latent, chunk, norm_scale)
    if not return_series:
        return cr.result()
    return cr.result(), (series[:, 0] if squeeze_day else series)
