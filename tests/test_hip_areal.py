"""-m gpu: areal extremes of hourly fields (csrc/rdgan_areal.hip.h, pr_disagg_radar_gan_amd/areal.py) against the numpy
restatement (tests/areal_np.py, itself checked on the CPU by tests/test_areal_host.py).  Everything is an integer: states and
depths are compared int64 against int64, with no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, areal as AR, field as F, field_products as FP, models, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import areal_np as an
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

# the smallest plane; w equal to ny; a single box covering the field; a halo wider than a tile and tiles cut by both edges
SHAPES = {"1x1": (1, 1, 3, (1,)), "5x7": (5, 7, 3, (1, 3, 5)), "64x64": (64, 64, 2, (1, 2, 63, 64)), "70x130": (70, 130, 2, (1, 7, 64))}
WINDOWS = (1, 3, 6, 12, 24)
LEVELS = (0.0, 0.5, 2.0, 10.0, 50.0)


def check(x, windows, widths, levels, want=None, **kw):
    """state and depths of one add() of x against the yardstick -> the ArealExtremes"""
    want, depths = want or an.areal_np(x, windows, widths, levels)
    n = int(np.prod(x.shape[:-3], dtype=np.int64))
    got = torch.full((n, len(windows), len(widths)), -7, dtype=torch.int64, device="cuda")
    ae = AR.ArealExtremes(windows, widths, levels, **kw).add(dev(x), depths_out=got)
    assert torch.equal(got.cpu(), torch.from_numpy(depths))
    assert torch.equal(ae.state().cpu(), torch.from_numpy(an.flat_state(want)))
    an.check_identities(AR.split_state(ae.state().cpu().numpy(), len(windows), len(widths), len(levels)))
    return ae


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


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_fields_against_restatement(name):
    ny, nx, days, widths = SHAPES[name]
    s = check(rain_like(ny, nx, days, len(name)), WINDOWS, widths, LEVELS).result()
    assert s.n_days_total == days and s.n_bad == 0 and np.all(s.n_days == days)


def test_widths_without_one_still_have_the_pixel_maximum():
    x = rain_like(70, 130, 2, 6)
    check(x, (2, 24), (7, 64), LEVELS)
    check(x, (2, 24), (64,), ())
    a = AR.areal_extremes(x, (2, 24), (1, 7, 64), LEVELS)
    b = AR.areal_extremes(x, (2, 24), (7, 64), LEVELS)
    assert np.array_equal(a.sum_A1[:, 1:], b.sum_A1) and np.array_equal(a.arf_hist[:, 1:], b.arf_hist)


@pytest.mark.parametrize("name", list(SHAPES))
def test_constant_field(name):
    """every key ties: every h* is 0 and the ARF is 1"""
    ny, nx, days, widths = SHAPES[name]
    s = check(np.full((days, 24, ny, nx), 0.75, np.float32), WINDOWS, widths, (0.75, 0.76, 18.0)).result()
    K, Wn = len(WINDOWS), len(widths)
    assert an.only_nonzero(s.start_hour) == {(k, w, 0): days for k in range(K) for w in range(Wn)}
    assert an.only_nonzero(s.arf_hist) == {(k, w, 20): days for k in range(K) for w in range(Wn)} and np.all(s.arf() == 1.0)
    assert np.array_equal(s.max_A, 768 * np.outer(WINDOWS, np.square(widths))) and s.exceedance()[:, 0].tolist() == [[1, 0, 0]] + [[1, 1, 0]] * 3 + [[1, 1, 1]]


def test_one_wet_pixel_hour():
    """the ARF is 1 / w^2"""
    x = np.zeros((2, 24, 70, 130), np.float32)
    x[0, 9, 66, 3] = 5.0
    x[1, 23, 69, 129] = 0.5                                            # the last hour, the last pixel
    s = check(x, WINDOWS, (1, 7, 64), LEVELS).result()
    assert np.array_equal(s.sum_A, np.full((5, 3), 5632)) and np.allclose(s.arf(), 1 / np.square((1, 7, 64)))
    assert s.start_hour[0, :, [9, 23]].tolist() == [[1] * 3] * 2 and s.start_hour[2, :, [4, 18]].tolist() == [[1] * 3] * 2


@pytest.mark.parametrize("name", ["5x7", "70x130"])
def test_maximum_only_in_the_last_window_and_the_last_corner(name):
    ny, nx, _, widths = SHAPES[name]
    x = np.full((1, 24, ny, nx), 0.25, np.float32)
    x[0, 23, ny - 1, nx - 1] = 9.0
    s = check(x, WINDOWS, widths, ()).result()
    assert an.only_nonzero(s.start_hour) == {(k, w, 24 - WINDOWS[k]): 1 for k in range(5) for w in range(len(widths))}


def test_quantisation_ties():
    rng = np.random.default_rng(8)
    x = ((rng.integers(0, 1 << 16, (2, 24, 5, 7)) + 0.5) / 1024).astype(np.float32)
    assert np.all(np.modf(x.astype(np.float64) * 1024)[0] == 0.5)
    check(x, WINDOWS, (1, 3, 5), LEVELS)


def test_box_sum_past_2_32():
    """every pixel-hour at the largest good value: 24 hours over 64 x 64 pixels sum to 2^37.6"""
    x = np.full((1, 24, 64, 64), 2047.9990234375, np.float32)
    q = 2048 * 1024 - 1
    want, depths = an.areal_np(x, (1, 24), (1, 64), (2047.0, 2048.0 * 24))
    assert depths[0].tolist() == [[q, q * 4096], [24 * q, 24 * q * 4096]] and depths[0, 1, 1] > 2 ** 37
    s = check(x, (1, 24), (1, 64), (2047.0, 2048.0 * 24), want=(want, depths)).result()
    assert s.level_count.tolist() == [[[0, 1, 0]] * 2, [[0, 1, 0]] * 2] and np.all(s.arf() == 1.0)


def test_bad_values():
    x = rain_like(70, 130, 2, 4).copy()
    x[0, 7, 69, 129] = np.nan                                          # a far corner: only the boxes and windows that cover it go
    s = check(x, WINDOWS, (1, 7, 64), LEVELS).result()
    assert s.n_bad == 1 and np.all(s.n_void == 0)
    x = rain_like(5, 7, 3, 5).copy()
    x[0, 3, 2, 2], x[1, 4, 0, 0], x[1, 5, 4, 6], x[2, 0, 1, 1] = -0.001, np.inf, 2048.0, -np.inf
    s = check(x, WINDOWS, (1, 3, 5), LEVELS).result()
    assert s.n_bad == 4
    # an all-NaN day is void for every (k, w), -1 in depths_out and in no count
    x = rain_like(5, 7, 3, 5).copy()
    x[1] = np.nan
    depths = torch.zeros((3, 5, 3), dtype=torch.int64, device="cuda")
    s = AR.ArealExtremes(WINDOWS, (1, 3, 5), LEVELS).add(dev(x), depths_out=depths).result()
    assert torch.all(depths[1] == -1) and torch.all(depths[0] >= 0) and np.all(s.n_void == 1) and np.all(s.n_days == 2) and s.n_bad == 24 * 35
    check(x, WINDOWS, (1, 3, 5), LEVELS)
    # a day whose only good pixels admit w = 1 but no larger box: a bad pixel in every 2 x 2 box, for all hours
    x = rain_like(64, 64, 2, 7).copy()
    x[0, :, 1::2, 1::2] = np.nan
    s = check(x, WINDOWS, (1, 2, 63, 64), LEVELS).result()
    assert s.n_void.tolist() == [[0, 1, 1, 1]] * 5 and s.n_bad == 24 * 32 * 32
    # bad in some hours only: the long windows are void, the short ones find the clean hours
    x = rain_like(64, 64, 2, 7).copy()
    x[1, 12, 1::2, 1::2] = np.nan
    s = check(x, WINDOWS, (1, 2, 63, 64), LEVELS).result()
    assert s.n_void[:, 1].tolist() == [0, 0, 0, 0, 1]


def test_grouping_strides_and_passes():
    x = rain_like(70, 130, 3, 11).copy()
    x[1, 5, 40, 100] = np.nan
    widths = (1, 7, 64)
    xd = dev(x)
    da = torch.empty((3, 5, 3), dtype=torch.int64, device="cuda")
    whole = check(x, WINDOWS, widths, LEVELS)
    whole.reset().add(xd, depths_out=da)
    new = lambda **kw: AR.ArealExtremes(WINDOWS, widths, LEVELS, **kw)
    assert torch.equal(new().add(xd[:1]).add(xd[1:2]).add(xd[2:]).state(), whole.state())
    for days in (1, 2):                                                # 3 = 2 + 1: a short last pass
        db = torch.empty_like(da)
        assert torch.equal(new(workspace_days=days).add(xd, depths_out=db).state(), whole.state()) and torch.equal(da, db)
    assert torch.equal(new().add(xd.view(1, 3, 24, 70, 130)).state(), whole.state())
    V = 24 * 70 * 130
    for pad in (52, 3):                                                # the second: no day but the first is 16-byte aligned
        wide = torch.full((3, V + pad), float("nan"), dtype=torch.float32, device="cuda")
        view = wide[:, :V].view(3, 24, 70, 130)
        view.copy_(xd)
        assert view.stride(0) == V + pad
        assert torch.equal(new().add(view).state(), whole.state())
    # numpy in: the same
    assert torch.equal(new().add(x).state(), whole.state())
    assert torch.equal(new().add(xd[:1]).add(x[1:]).state(), whole.state())                # numpy onto a state that exists
    s, depths = AR.areal_extremes(x, WINDOWS, widths, LEVELS, return_depths=True, workspace_days=1)
    assert np.array_equal(an.flat_state(vars(s)), whole.state().cpu().numpy()) and torch.equal(depths, da)
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2])
    # an odd plane takes the scalar prefix pass, an even one the vector pass: both against the yardstick
    check(rain_like(5, 7, 3, 5), (1, 24), (1, 5), ())
    check(rain_like(64, 64, 2, 7), (1, 24), (1, 64), ())


def test_pixel_maximum_equals_the_peaks_of_field_products():
    """multiples of 2^-10 mm below 64 mm: fp32 sums of 24 of them are exact, so both sides compute the same numbers"""
    rng = np.random.default_rng(12)
    x = (rng.integers(0, 1 << 16, (3, 24, 70, 130)) * (rng.random((3, 24, 70, 130)) < 0.4) / 1024).astype(np.float32)
    _, depths = AR.areal_extremes(x, WINDOWS, (1, 7), (), return_depths=True)
    peaks, _ = FP.peaks_device(dev(x), WINDOWS)
    assert torch.equal(depths[:, :, 0].double() / 1024, peaks.amax(dim=(2, 3)).double())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_extremes_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, one NaN pixel, a dry tile; `chunk` is one unit's wet tiles on both sides, as
    tests/test_hip_storms.py pins it, so that the hourly values the two sides see are the same"""
    S, widths, levels = 5, (1, 5, 15, 31), (1.0, 5.0, 20.0)
    rng = np.random.default_rng(31)
    daily = (rng.gamma(0.8, 6.0, (40, 52)) * (rng.random((40, 52)) < 0.7)).astype(np.float32)
    daily[:16, :16] = 0.0
    daily[2, 50] = np.nan                                              # (some boxes of width 31 stay clear of it)
    dd = dev(daily)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, dd, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, dd, S, latent=z, chunk=unit_tiles)
    assert info.n_nan_pixels == 1 and hourly.shape == (S, 24, 40, 52)
    want = AR.ArealExtremes(WINDOWS, widths, levels).add(hourly)
    assert torch.equal(want.state().cpu(), torch.from_numpy(an.flat_state(an.areal_np(hourly.cpu().numpy(), WINDOWS, widths, levels)[0])))
    ws = want.result()
    assert ws.n_bad == S * 24 and ws.n_days_total == S and np.all(ws.n_days == S) and np.all(ws.max_A > 0)
    for scenario_chunk in (1, 3, 5):
        got = AR.areal_extremes_field(generator, dd if scenario_chunk == 3 else daily, S, WINDOWS, widths, levels, latent=z,
                                      scenario_chunk=scenario_chunk, chunk=unit_tiles)
        assert np.array_equal(an.flat_state(vars(got)), want.state().cpu().numpy()), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.areal_extremes_field(daily, S, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert (a.windows, a.widths, a.levels) == ((1, 3, 6, 12, 24), (1, 5, 15, 31), AR.DEFAULT_LEVELS)
    assert np.array_equal(an.flat_state(vars(a)), AR.ArealExtremes(a.windows, a.widths, a.levels).add(hourly2).state().cpu().numpy())


def test_c_entries_refuse_bad_arguments_and_touch_nothing():
    lib = _lib.load()
    ny, nx = 5, 7
    one = lib.rdgan_areal_workspace_bytes(ny, nx, 1)
    assert one == 576 + 120 * 35 and lib.rdgan_areal_state_count(2, 2, 2) == 4 * 55 + 2
    x = dev(np.full((2, 24, ny, nx), 3.0, np.float32))
    counts = torch.zeros(4 * 55 + 2, dtype=torch.int64, device="cuda")
    depths = torch.full((2, 2, 2), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(2 * one // 8, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    null = ctypes.c_void_p(0)
    ints = lambda *v: np.array(v, np.int32)
    lv = np.array([1.0, 100.0])

    def acc(xp=p(x), n=2, stride=24 * 35, ny=ny, nx=nx, k=ints(1, 24), K=2, w=ints(1, 5), Wn=2, lv=lv, L=2, cp=p(counts), dp=p(depths), wp=p(ws),
            nbytes=2 * one):
        hp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else null
        return lib.rdgan_areal_accumulate(xp, n, stride, ny, nx, hp(k), K, hp(w), Wn, hp(lv), L, cp, dp, wp, nbytes,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    for kw in (dict(xp=null), dict(cp=null), dict(wp=null), dict(k=None), dict(w=None), dict(lv=None), dict(xp=off(x, 2)), dict(cp=off(counts, 4)),
               dict(dp=off(depths, 4)), dict(wp=off(ws, 4)), dict(n=0), dict(ny=0), dict(nx=0), dict(ny=-3), dict(ny=4097, nx=4096), dict(w=ints(1, 6)),
               dict(w=ints(5, 1)), dict(w=ints(0, 5)), dict(Wn=0), dict(Wn=9), dict(K=0), dict(K=9), dict(k=ints(24, 1)), dict(k=ints(1, 25)),
               dict(lv=np.array([100.0, 1.0])), dict(lv=np.array([np.nan, 1.0])), dict(L=-1), dict(L=17), dict(stride=24 * 35 - 1),
               dict(nbytes=one - 1), dict(nbytes=0)):
        assert acc(**kw) == -2, kw
    torch.cuda.synchronize()
    assert not counts.any() and torch.all(depths == -7)
    assert acc(nbytes=one) == 0                                        # a workspace for one day: two passes
    want, d = an.areal_np(x.cpu().numpy(), (1, 24), (1, 5), lv)
    assert torch.equal(counts.cpu(), torch.from_numpy(an.flat_state(want))) and torch.equal(depths.cpu(), torch.from_numpy(d))
    assert acc(dp=null, L=0, lv=None, cp=p(torch.zeros(4 * 53 + 2, dtype=torch.int64, device="cuda"))) == 0          # no depths, no levels
    torch.cuda.synchronize()
