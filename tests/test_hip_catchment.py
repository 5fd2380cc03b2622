"""-m gpu: catchment rainfall of hourly fields (csrc/rdgan_catchment.hip.h, pr_disagg_radar_gan_amd/catchments.py) against the numpy
restatement (tests/catchment_np.py, itself checked on the CPU by tests/test_catchment_host.py).  Everything is an integer: states,
series and depths are compared int64 against int64, with no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, catchments as CT, field as F, models, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import catchment_np as cn
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

WINDOWS = (1, 3, 6, 12, 24)
LEVELS = (0.0, 0.5, 2.0, 10.0, 50.0)


def check(x, cmap, members, windows=WINDOWS, levels=LEVELS, want=None, **kw):
    """state, series and depths of one add() of x against the yardstick -> the CatchmentRainfall"""
    want, series, depths = want or cn.catchment_np(x, members, windows, levels)
    n = int(np.prod(x.shape[:-3], dtype=np.int64))
    got_s = torch.full((n, cmap.n_catch, 24), -7, dtype=torch.int64, device="cuda")
    got_d = torch.full((n, cmap.n_catch, len(windows)), -7, dtype=torch.int64, device="cuda")
    cr = CT.CatchmentRainfall(cmap, windows, levels, **kw).add(dev(x), series_out=got_s, depths_out=got_d)
    assert torch.equal(got_s.cpu(), torch.from_numpy(series))
    assert torch.equal(got_d.cpu(), torch.from_numpy(depths))
    assert torch.equal(cr.state().cpu(), torch.from_numpy(cn.flat_state(want)))
    cn.check_identities(CT.split_state(cr.state().cpu().numpy(), cmap.n_catch, len(windows), len(levels)))
    return cr


@functools.lru_cache(maxsize=None)
def rain_like(ny, nx, days, seed):
    """(days, 24, ny, nx): gamma amounts where a smoothed noise field is above its 70 % quantile, so that the wet areas have a size;
    some values at quantisation ties.  Shared: copy before writing."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(days, 24, ny, nx))
    for _ in range(2):
        g = (g + np.roll(g, 1, 1) + np.roll(g, 1, 2) + np.roll(g, -1, 2) + np.roll(g, 1, 3) + np.roll(g, -1, 3)) / 6
    x = ((0.2 + rng.gamma(0.6, 3.0, g.shape)) * (g > np.quantile(g, 0.7))).astype(np.float32)
    ties = rng.random(g.shape) < 0.05
    x[ties] = ((rng.integers(0, 8192, g.shape) + 0.5) / 1024).astype(np.float32)[ties]
    return x


@functools.lru_cache(maxsize=None)
def striped_map():
    """40 x 40: catchments of 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 3 pixels -- a wave and a chunk, one less and one
    more -- dealt over the plane with a stride of 7 pixels, so that no list is a contiguous run; the remaining pixels lie in none"""
    sizes = (63, 64, 65, CT.CHUNK - 1, CT.CHUNK, CT.CHUNK + 1, 2 * CT.CHUNK + 3)
    labels = np.full(1600, -1)
    labels[:sum(sizes)] = np.repeat(np.arange(len(sizes)), sizes)
    regions = np.empty(1600, np.int64)
    regions[(np.arange(1600) * 7) % 1600] = labels
    regions = regions.reshape(40, 40)
    cmap = CT.CatchmentMap(regions=regions)
    assert cmap.npix.tolist() == list(sizes) and np.any(np.diff(cmap.pixels[:63]) > 1)
    assert cmap.chunks[:, 2].tolist() == [63, 64, 65, 255, 256, 256, 1, 256, 256, 3]
    return cmap, tuple(cn.members_of(regions=regions))


def test_odd_plane_one_pixel_one_row_and_the_rest():
    regions = np.full((5, 7), 2)
    regions[0, 0] = 0
    regions[3] = 1
    cmap = CT.CatchmentMap(regions=regions)
    assert cmap.npix.tolist() == [1, 7, 27]
    s = check(rain_like(5, 7, 3, 1), cmap, cn.members_of(regions=regions)).result()
    assert s.n_days_total == 3 and s.n_bad == 0 and np.all(s.n_days == 3)
    check(rain_like(5, 7, 3, 1), cmap, cn.members_of(regions=regions), windows=(24,), levels=())


def test_chunk_and_wave_boundaries_on_interleaved_stripes():
    cmap, members = striped_map()
    s = check(rain_like(40, 40, 2, 2), cmap, members).result()
    assert np.all(s.n_days == 2) and np.all(s.max_A[:, -1] > 0)
    # every pixel at one unit: the sums are the pixel counts, so a lane dropped or taken twice at a boundary shows as itself
    one = np.full((1, 24, 40, 40), 1 / 1024, np.float32)
    series = torch.empty((1, 7, 24), dtype=torch.int64, device="cuda")
    CT.CatchmentRainfall(cmap, (1,)).add(dev(one), series_out=series)
    assert torch.equal(series.cpu(), torch.from_numpy(cmap.npix.astype(np.int64))[None, :, None].expand(1, 7, 24))


def test_nested_masks_and_a_third_of_the_plane_in_no_catchment():
    masks = np.zeros((3, 30, 33), bool)
    masks[0, :, :22] = True                                            # the basin: the left two thirds
    masks[1, :14, :9] = True                                           # two sub-basins inside it
    masks[2, 10:, 5:22] = True
    cmap = CT.CatchmentMap(masks=masks, names=("gauge", "upper", "lower"))
    assert cmap.n_entries == 660 + 126 + 340 and not np.isin(np.arange(30 * 33).reshape(30, 33)[:, 22:], cmap.pixels).any()
    x = rain_like(30, 33, 3, 3).copy()
    x[1, 4, 12, 7] = np.nan                                            # in the basin and in both sub-basins: counted three times
    s = check(x, cmap, cn.members_of(masks=masks)).result()
    assert s.n_bad == 3 and s.names == ("gauge", "upper", "lower")
    assert np.all(s.sum_A[0] >= s.sum_A[1]) and np.all(s.max_A[0, -1] >= s.max_A[1:, -1])


def test_bad_pixel_hours():
    cmap, members = striped_map()
    x = rain_like(40, 40, 2, 4).copy()
    pix = members[4]                                                   # the catchment of exactly one chunk
    at = lambda p: (p // 40, p % 40)
    for v, p in zip((np.nan, -1.0, np.inf, 2048.0), pix[[0, 63, 64, 255]]):
        x[(0, 9) + at(p)] = v                                          # four bad values, one hour, one catchment
    outside = np.flatnonzero(cmap_regions(cmap) < 0)
    x[(0, 2) + at(outside[0])], x[(1, 9) + at(outside[-1])] = np.nan, -np.inf          # in no catchment: nothing changes
    x[(1, 3) + at(members[2][5])] = 2047.9999                          # admitted
    cr = check(x, cmap, members)
    s = cr.result()
    assert s.n_bad == 4 and s.n_void.sum() == 1 and s.n_void[4].tolist() == [0, 0, 0, 0, 1]       # only the 24-hour window holds hour 9 for sure
    series = torch.empty((2, 7, 24), dtype=torch.int64, device="cuda")
    depths = torch.empty((2, 7, 5), dtype=torch.int64, device="cuda")
    CT.CatchmentRainfall(cmap, WINDOWS).add(dev(x), series_out=series, depths_out=depths)
    assert (series == -1).nonzero().tolist() == [[0, 4, 9]] and (depths == -1).nonzero().tolist() == [[0, 4, 4]]
    assert int(series[1, 2, 3]) >= 2048 * 1024 - 1
    # hours 8 and 17 bad: the windows of 12 fit between them nowhere, those of 6 do
    x[(0, 17) + at(pix[100])] = np.nan
    x[(0, 8) + at(pix[100])] = np.nan
    s = check(x, cmap, members).result()
    assert s.n_void[4].tolist() == [0, 0, 0, 1, 1] and s.n_bad == 6
    # a bad pixel in every hour: void for every window, whatever the other pixels hold
    x = rain_like(40, 40, 2, 4).copy()
    x[(1, slice(None)) + at(members[0][62])] = np.nan
    s = check(x, cmap, members).result()
    assert s.n_void[0].tolist() == [1] * 5 and s.n_void[1:].sum() == 0 and s.n_bad == 24 and np.all(s.n_days[0] == 1)
    # an all-NaN day
    x = rain_like(5, 7, 3, 5).copy()
    x[1] = np.nan
    regions = np.arange(35).reshape(5, 7) % 3
    s = check(x, CT.CatchmentMap(regions=regions), cn.members_of(regions=regions)).result()
    assert np.all(s.n_void == 1) and np.all(s.n_days == 2) and s.n_bad == 24 * 35


def cmap_regions(cmap):
    """the label map of a CatchmentMap without overlap, -1 where no catchment lists the pixel"""
    regions = np.full(cmap.plane_shape[0] * cmap.plane_shape[1], -1)
    regions[cmap.pixels] = np.repeat(np.arange(cmap.n_catch), cmap.npix)
    return regions


def test_ties_and_dry_days():
    cmap, members = striped_map()
    x = np.full((3, 24, 40, 40), 0.75, np.float32)                     # every key ties: every start hour is 0
    x[1] = 0.0                                                         # a dry day: counted, in n_dry and in no start hour
    x[2, 23] = 9.0                                                     # the maximum only in the last window
    s = check(x, cmap, members, levels=(0.0, 0.75, 18.0, 26.25)).result()
    K = len(WINDOWS)
    want = {(c, k, 0): 1 for c in range(7) for k in range(K)} | {(c, k, 24 - WINDOWS[k]): 1 for c in range(7) for k in range(K - 1)}
    want |= {(c, K - 1, 0): 2 for c in range(7)}
    got = {tuple(int(i) for i in idx): int(s.start_hour[tuple(idx)]) for idx in np.argwhere(s.start_hour != 0)}
    assert got == want and np.all(s.n_dry == 1) and np.all(s.n_days == 3) and np.all(s.n_void == 0)
    # the dry day reaches the level 0 and no other; 0.75 mm a pixel sits exactly on the second level at k = 1, and the 24-hour
    # sums sit exactly on 18 and on 26.25 mm
    assert s.level_count[:, 0].tolist() == [[0, 1, 2, 0, 0]] * 7 and s.level_count[:, K - 1].tolist() == [[0, 1, 0, 1, 1]] * 7
    assert np.array_equal(s.max_A[:, 0], 9216 * cmap.npix) and np.allclose(s.max_depth()[:, K - 1], 0.75 * 23 + 9.0)


def test_sums_past_2_32():
    """one catchment over 512 x 512 pixels at 2047 mm/h: an hour sums to almost 2^39, the day to 2^43.6"""
    x = np.full((1, 24, 512, 512), 2047.0, np.float32)
    cmap = CT.CatchmentMap(regions=np.zeros((512, 512), np.int8))
    hour = 2047 * 1024 * 512 * 512
    want = cn.empty_state(1, 2, 2)
    want["n_days_total"] = 1
    want["n_days"][0], want["sum_A"][0], want["max_A"][0] = 1, (hour, 24 * hour), (hour, 24 * hour)
    want["start_hour"][0, :, 0] = 1
    want["level_count"][0, 0], want["level_count"][0, 1] = (0, 1, 0), (0, 0, 1)           # levels 2047 and 2047 * 24 mm, both met exactly
    series, depths = np.full((1, 1, 24), hour, np.int64), np.array([[[hour, 24 * hour]]], np.int64)
    assert hour > 2 ** 38 and cn.quantise(x[0, :1, :1, :4])[0].tolist() == [[[2047 * 1024] * 4]]
    check(x, cmap, None, windows=(1, 24), levels=(2047.0, 2047.0 * 24), want=(want, series, depths))


def test_grouping_strides_and_passes():
    cmap, members = striped_map()
    x = rain_like(40, 40, 7, 11).copy()
    x[3, 5, 20, 20] = np.nan
    xd = dev(x)
    whole = check(x, cmap, members)
    sa = torch.empty((7, 7, 24), dtype=torch.int64, device="cuda")
    da = torch.empty((7, 7, 5), dtype=torch.int64, device="cuda")
    whole.reset().add(xd, series_out=sa, depths_out=da)
    new = lambda **kw: CT.CatchmentRainfall(cmap, WINDOWS, LEVELS, **kw)
    sb, db = torch.empty_like(sa), torch.empty_like(da)
    assert torch.equal(new().add(xd[:3], sb[:3], db[:3]).add(xd[3:], sb[3:], db[3:]).state(), whole.state())
    assert torch.equal(sa, sb) and torch.equal(da, db)
    for days in (1, 3):                                                # 7 = 3 + 3 + 1: a short last pass
        sb, db = torch.empty_like(sa), torch.empty_like(da)
        assert torch.equal(new(workspace_days=days).add(xd, sb, db).state(), whole.state()) and torch.equal(sa, sb) and torch.equal(da, db)
    V = 24 * 1600
    for pad in (52, 3):                                                # the second: no day but the first is 16-byte aligned
        wide = torch.full((7, V + pad), float("nan"), dtype=torch.float32, device="cuda")
        view = wide[:, :V].view(7, 24, 40, 40)
        view.copy_(xd)
        assert view.stride(0) == V + pad
        sb = torch.empty_like(sa)
        assert torch.equal(new().add(view, series_out=sb).state(), whole.state()) and torch.equal(sa, sb)
    # a second accumulator on a workspace an earlier call left larger
    cr = new().add(xd)
    size = cr._ws.numel()
    sb, db = torch.empty_like(sa[:2]), torch.empty_like(da[:2])
    other = new()
    other._ws = cr._ws
    other.add(xd[:2], sb, db).add(xd[2:])
    assert other._ws.numel() == size and torch.equal(other.state(), whole.state()) and torch.equal(sb, sa[:2]) and torch.equal(db, da[:2])
    # numpy in, and the one-call form
    assert torch.equal(new().add(x).state(), whole.state())
    s, series, depths = CT.catchment_rainfall(x, cmap, WINDOWS, LEVELS, return_series=True, return_depths=True, workspace_days=2)
    assert np.array_equal(cn.flat_state(vars(s)), whole.state().cpu().numpy()) and torch.equal(series, sa) and torch.equal(depths, da)
    s, depths = CT.catchment_rainfall(xd.view(1, 7, 24, 40, 40), cmap, WINDOWS, LEVELS, return_depths=True)
    assert np.array_equal(cn.flat_state(vars(s)), whole.state().cpu().numpy()) and torch.equal(depths, da)
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2])


def test_series_mm():
    cmap, members = striped_map()
    x = rain_like(40, 40, 2, 4).copy()
    x[0, 9, 0, 0] = np.nan
    _, series = CT.catchment_rainfall(x, cmap, (1,), return_series=True)
    mm = CT.series_mm(series, cmap)
    s = series.cpu().numpy()
    want = np.where(s < 0, np.nan, s / (1024.0 * cmap.npix[None, :, None])).astype(np.float32)
    assert mm.dtype == torch.float32 and mm.is_cuda and np.isnan(want).sum() == 1
    assert np.array_equal(mm.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(CT.series_mm(series.view(2, 1, 7, 24), cmap).cpu().numpy(), want.reshape(2, 1, 7, 24), equal_nan=True)
    with pytest.raises(ValueError):
        CT.series_mm(series[:, :3], cmap)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_catchment_rainfall_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, one NaN pixel, a dry tile; `chunk` is one unit's wet tiles on both sides, as
    tests/test_hip_areal.py pins it, so that the hourly values the two sides see are the same"""
    S, levels = 5, (1.0, 5.0, 20.0)
    rng = np.random.default_rng(31)
    daily = (rng.gamma(0.8, 6.0, (40, 52)) * (rng.random((40, 52)) < 0.7)).astype(np.float32)
    daily[:16, :16] = 0.0
    daily[2, 50] = np.nan
    regions = np.full((40, 52), -1)
    regions[:16, :16] = 0                                              # the dry tile
    regions[20:, :30] = 1
    regions[:20, 30:] = 2                                              # holds the NaN pixel: void in every hour
    regions[25:, 35:] = 3
    cmap = CT.CatchmentMap(regions=regions)
    members = cn.members_of(regions=regions)
    dd = dev(daily)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, dd, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, dd, S, latent=z, chunk=unit_tiles)
    assert info.n_nan_pixels == 1 and hourly.shape == (S, 24, 40, 52)
    want, want_series = CT.catchment_rainfall(hourly, cmap, WINDOWS, levels, return_series=True)
    # the restatement of the returned fields: state and series, and in them every scenario's 24-hour sum of rint-quantised hours
    o, series_np, depths_np = cn.catchment_np(hourly.cpu().numpy(), members, WINDOWS, levels)
    assert np.array_equal(cn.flat_state(vars(want)), cn.flat_state(o)) and torch.equal(want_series.cpu(), torch.from_numpy(series_np))
    assert want.n_bad == S * 24 and np.all(want.n_void[2] == S) and np.all(want.n_dry[0] == S) and np.all(want.max_A[[1, 3]] > 0)
    q = cn.quantise(hourly.cpu().numpy().reshape(S, 24, -1))[0]
    for c in (0, 1, 3):
        assert np.array_equal(want_series[:, c].sum(dim=1).cpu().numpy(), q[:, :, members[c]].sum(axis=(1, 2)))
        assert np.array_equal(depths_np[:, c, -1], q[:, :, members[c]].sum(axis=(1, 2)))
    for scenario_chunk in (1, 3, 5):
        got, series = CT.catchment_rainfall_field(generator, dd if scenario_chunk == 3 else daily, S, cmap, WINDOWS, levels, return_series=True,
                                                  latent=z, scenario_chunk=scenario_chunk, chunk=unit_tiles)
        assert np.array_equal(cn.flat_state(vars(got)), cn.flat_state(vars(want))), scenario_chunk
        assert series.shape == (S, 4, 24) and torch.equal(series, want_series), scenario_chunk
    got = CT.catchment_rainfall_field(generator, daily[None], S, cmap, WINDOWS, levels, latent=z, chunk=unit_tiles)        # a day axis, no series
    assert np.array_equal(cn.flat_state(vars(got)), cn.flat_state(vars(want)))
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a, series = P.catchment_rainfall_field(daily, S, cmap, return_series=True, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert (a.windows, a.levels) == ((1, 3, 6, 12, 24), CT.DEFAULT_LEVELS)
    b, series2 = CT.catchment_rainfall(hourly2, cmap, a.windows, a.levels, return_series=True)
    assert np.array_equal(cn.flat_state(vars(a)), cn.flat_state(vars(b))) and torch.equal(series, series2)


def test_c_entries_refuse_bad_arguments_and_touch_nothing():
    lib = _lib.load()
    regions = np.arange(35).reshape(5, 7) % 3
    cmap = CT.CatchmentMap(regions=regions)
    chunks, pixels, npix = cmap.on("cuda")
    one = lib.rdgan_catchment_workspace_bytes(3, 1)
    n_state = lib.rdgan_catchment_state_count(3, 2, 2)
    assert one == 3 * 288 and n_state == 6 * 32 + 2
    x = dev(np.full((2, 24, 5, 7), 3.0, np.float32))
    counts = torch.zeros(n_state, dtype=torch.int64, device="cuda")
    series = torch.full((2, 3, 24), -7, dtype=torch.int64, device="cuda")
    depths = torch.full((2, 3, 2), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(2 * one // 8, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    null = ctypes.c_void_p(0)
    ints = lambda *v: np.array(v, np.int32)
    lv = np.array([1.0, 100.0])

    def acc(xp=p(x), n=2, stride=24 * 35, ny=5, nx=7, chp=p(chunks), n_chunks=3, pxp=p(pixels), E=35, npp=p(npix), C=3, k=ints(1, 24), K=2, lv=lv, L=2,
            cp=p(counts), sp=p(series), dp=p(depths), wp=p(ws), nbytes=2 * one):
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else null
        return lib.rdgan_catchment_accumulate(xp, n, stride, ny, nx, chp, n_chunks, pxp, E, npp, C, hp(k), K, hp(lv), L, cp, sp, dp, wp, nbytes,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    for kw in (dict(xp=null), dict(cp=null), dict(wp=null), dict(chp=null), dict(pxp=null), dict(npp=null), dict(k=None), dict(lv=None),
               dict(xp=off(x, 2)), dict(cp=off(counts, 4)), dict(sp=off(series, 4)), dict(dp=off(depths, 4)), dict(wp=off(ws, 4)), dict(chp=off(chunks, 2)),
               dict(n=0), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4096), dict(C=0), dict(C=65536), dict(E=2), dict(n_chunks=2), dict(n_chunks=36),
               dict(K=0), dict(K=9), dict(k=ints(24, 1)), dict(k=ints(1, 25)), dict(lv=np.array([100.0, 1.0])), dict(lv=np.array([np.nan, 1.0])),
               dict(L=-1), dict(L=17), dict(stride=24 * 35 - 1), dict(nbytes=one - 1), dict(nbytes=0)):
        assert acc(**kw) == -2, kw
    torch.cuda.synchronize()
    assert not counts.any() and torch.all(series == -7) and torch.all(depths == -7)
    assert acc(nbytes=one) == 0                                        # a workspace for one day: two passes
    want, s, d = cn.catchment_np(x.cpu().numpy(), cn.members_of(regions=regions), (1, 24), lv)
    assert torch.equal(counts.cpu(), torch.from_numpy(cn.flat_state(want)))
    assert torch.equal(series.cpu(), torch.from_numpy(s)) and torch.equal(depths.cpu(), torch.from_numpy(d))
    assert acc(sp=null, dp=null, L=0, lv=None, cp=p(torch.zeros(6 * 30 + 2, dtype=torch.int64, device="cuda"))) == 0      # no outputs, no levels
    torch.cuda.synchronize()
