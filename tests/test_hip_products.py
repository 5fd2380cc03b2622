"""-m gpu: ensemble products (csrc/rdgan_products.hip.h, pr_disagg_radar_gan_amd/field_products.py) against the numpy restatement
(tests/products_np.py): the k-hour peaks bit for bit, the blend fused with them against the two kernels it replaces, the member
statistics within one fp32 rounding, the whole path around a seeded generator, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, models
from pr_disagg_radar_gan_amd import field as F
from pr_disagg_radar_gan_amd import field_products as FP
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from pr_disagg_radar_gan_amd import weights as W
from tests import field_np as fn
from tests import products_np as pn
from tests.hip_util import dev, ptr, stream
from tests.test_hip_field import BLEND_RTOL, MASS_RTOL, _blend_case

pytestmark = pytest.mark.gpu

WINDOW_LISTS = [(1,), (24,), (1, 2, 3, 6, 12, 24), (1, 2, 3, 4, 6, 8, 12, 24)]
# quantiles and mean: the fp64 intermediates err far below an fp32 ulp, so only the final rounding to fp32 can differ, by one ulp
# (at most 2^-23 = 1.2e-7 of the value); 2.4e-7 grants that one ulp and no more than two, and atol 0 keeps zeros exactly 0
STATS_RTOL = 2.4e-7
PROBS, THRESHOLDS = (0.0, 0.1, 0.5, 0.99, 1.0), (0.0, 1.0, 10.0)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def np_same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                                       b.view(np.int32) if b.dtype == np.float32 else b)


def _hourly_case(units, ny, nx, seed):
    """gamma hours with many exact zeros; a plateau (equal maxima), an all-zero pixel and a pixel with one NaN hour"""
    rng = np.random.default_rng(seed)
    x = (rng.gamma(0.5, 3.0, (units, 24, ny, nx)) * (rng.random((units, 24, ny, nx)) > 0.4)).astype(np.float32)
    x[0, :, 0, 0] = 0.0
    x[0, 5:9, 0, 0] = 1.25                               # plateau: hours 5 .. 8 share the 1-hour maximum, the first wins
    x[-1, :, ny - 1, nx - 1] = 0.0
    if ny * nx > 2:
        x[units // 2, 13, ny // 2, nx // 2] = np.nan
    return x


@pytest.mark.parametrize("ny,nx", [(5, 67), (1, 1)])
@pytest.mark.parametrize("windows", WINDOW_LISTS)
def test_hourly_peaks_bit_for_bit(ny, nx, windows):
    x = _hourly_case(3, ny, nx, seed=ny + nx + len(windows))
    xd = dev(x)
    peaks, hour = FP.peaks_device(xd, windows)
    again = FP.peaks_device(xd, windows)
    assert peaks.shape == (3, len(windows), ny, nx) and hour.shape == (3, ny, nx) and hour.dtype == torch.uint8
    assert same_bits(peaks, again[0]) and same_bits(hour, again[1])
    ref, ref_hour = pn.hourly_peaks(x, windows)
    assert np_same_bits(peaks.cpu().numpy(), ref) and np.array_equal(hour.cpu().numpy(), ref_hour)
    assert ref_hour[0, 0, 0] == (5 if windows[0] == 1 else 0) and ref_hour[-1, ny - 1, nx - 1] == 0
    if ny * nx > 2:
        assert ref_hour[1, ny // 2, nx // 2] == 255 and np.isnan(ref[1, :, ny // 2, nx // 2]).all() and np.isnan(ref).sum() == len(windows)
    # any leading axes: (3, 24, ny, nx) seen as (3, 1, 24, ny, nx) and one unit alone as (24, ny, nx)
    p5, h5 = FP.peaks_device(xd.view(3, 1, 24, ny, nx), windows)
    p1, h1 = FP.peaks_device(xd[2], windows)
    assert same_bits(p5, peaks) and same_bits(h5, hour) and same_bits(p1, peaks[2:3]) and same_bits(h1, hour[2:3])


@pytest.mark.parametrize("h", [0, 23])
def test_hourly_peaks_one_hot_probes(h):
    windows = (1, 2, 3, 6, 12, 24)
    x = np.zeros((2, 24, 5, 67), np.float32)
    x[1, h, 3, 65] = 2.5
    peaks, hour = FP.peaks_device(dev(x), windows)
    peaks, hour = peaks.cpu().numpy(), hour.cpu().numpy()
    want = np.zeros(peaks.shape, np.float32)
    want[1, :, 3, 65] = 2.5
    assert np.array_equal(peaks, want)
    want_hour = np.zeros(hour.shape, np.uint8)
    want_hour[1, 3, 65] = h
    assert np.array_equal(hour, want_hour)


def test_hourly_peaks_offsets_past_2_31():
    units, ny, nx = 2100, 256, 256
    assert units * 24 * ny * nx > 2 ** 31
    x = torch.zeros((units, 24, ny, nx), device="cuda")
    x[0, 7, 2, 3] = 1.5
    x[0, 8, 2, 3] = 2.0
    x[-1, 22, 255, 254] = 4.0
    x[-1, 23, 255, 254] = 3.0
    peaks, hour = FP.peaks_device(x, (1, 2))
    for u in (0, units - 1):
        ref, ref_hour = pn.hourly_peaks(x[u:u + 1].cpu().numpy(), (1, 2))
        assert np_same_bits(peaks[u:u + 1].cpu().numpy(), ref) and np.array_equal(hour[u:u + 1].cpu().numpy(), ref_hour)
    assert peaks[0, :, 2, 3].tolist() == [2.0, 3.5] and peaks[-1, :, 255, 254].tolist() == [4.0, 7.0]
    assert int(hour[0, 2, 3]) == 8 and int(hour[-1, 255, 254]) == 22


@pytest.mark.parametrize("nd,ny,nx,overlap", [(8, 11, 19, 3), (16, 20, 30, 4)])
def test_blend_peaks_against_the_two_kernels_and_the_restatement(nd, ny, nx, overlap):
    """the cases of tests/test_hip_field.py (a dry pixel, a NaN pixel, a dry row, skipped slots), first_unit 0 and 1"""
    windows = (1, 3, 6, 12, 24)
    ref_plan, frac, slots, daily = _blend_case(nd, ny, nx, overlap, seed=nd + ny + nx)
    plan = F.tile_plan(ny, nx, nd, overlap)
    fd, dd = dev(frac), dev(daily)
    for first in (0, 1):
        peaks, hour = FP.blend_peaks_device(fd, slots, plan, dd, windows, first_unit=first)
        two_p, two_h = FP.peaks_device(F.blend_device(fd, slots, plan, dd, first_unit=first), windows)
        assert peaks.shape == (2, 5, ny, nx) and same_bits(peaks, two_p) and same_bits(hour, two_h)           # bit for bit
        again = FP.blend_peaks_device(fd, slots, plan, dd, windows, first_unit=first)
        assert same_bits(peaks, again[0]) and same_bits(hour, again[1])
        peaks, hour = peaks.cpu().numpy(), hour.cpu().numpy()
        ref, ref_hour, margin = pn.hourly_peaks_f64(fn.blend(frac, slots, ref_plan, daily, first_unit=first), windows)
        day = daily[[(first + u) % 2 for u in range(2)]]
        nan, dry = np.isnan(day), day == 0
        assert nan.sum() == 1 and dry.sum() > 1
        assert np.array_equal(np.isnan(peaks), np.broadcast_to(nan[:, None], peaks.shape))
        ok = ~np.isnan(ref)
        err = np.abs(peaks[ok] - ref[ok]) / np.where(ref[ok] == 0, 1.0, np.abs(ref[ok]))
        print(f"nd {nd} field {ny} x {nx} first_unit {first}: worst relative error of the peaks {err.max():.2e} (limit {BLEND_RTOL})")
        np.testing.assert_allclose(peaks, ref, rtol=BLEND_RTOL, atol=0, equal_nan=True)
        assert np.all(hour[nan] == 255) and np.all(hour[dry] == 0) and np.all(peaks[np.broadcast_to(dry[:, None], peaks.shape)] == 0)
        # the hour is decided where the fp64 maximum stands clear of every other hour by more than both sums can err together
        with np.errstate(invalid="ignore"):
            decided = margin > 2 * BLEND_RTOL * ref[:, 0]
        live = ~nan & ~dry
        left_out = 1.0 - decided[live].mean()
        print(f"  peak hour compared at {decided[live].sum()} of {live.sum()} wet pixels ({100 * left_out:.2f} % left out, limit 5 %)")
        assert left_out < 0.05
        assert np.array_equal(hour[live & decided], ref_hour[live & decided])


def _member_case(S, P, seed):
    """gamma values with about 60 % exact zeros: many ties"""
    rng = np.random.default_rng(seed)
    return (rng.gamma(0.5, 6.0, (S, P)) * (rng.random((S, P)) > 0.6)).astype(np.float32)


def _assert_stats(st, x, what):
    q, mean, ex, n_nan = pn.member_stats(x, PROBS, THRESHOLDS)
    gq, gm, ge = st.quantiles.cpu().numpy(), st.mean.cpu().numpy(), st.exceedance.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        eq = np.nanmax(np.where(q == 0, np.abs(gq), np.abs(gq - q) / np.abs(q)), initial=0.0)
        em = np.nanmax(np.where(mean == 0, np.abs(gm), np.abs(gm - mean) / np.abs(mean)), initial=0.0)
    print(f"{what}: worst relative error quantiles {eq:.2e}, mean {em:.2e} (limit {STATS_RTOL})")
    np.testing.assert_allclose(gq, q, rtol=STATS_RTOL, atol=0, equal_nan=True)
    np.testing.assert_allclose(gm, mean, rtol=STATS_RTOL, atol=0, equal_nan=True)
    assert np.array_equal(ge, ex, equal_nan=True)
    assert st.n_nan_positions == n_nan


@pytest.mark.parametrize("S", [1, 2, 7, 64, 100, 1000, 1024, 1025, 4096])
def test_member_stats_against_restatement(S):
    for P_ in (1, 15, 16, 17, 1000):
        x = _member_case(S, P_, seed=S + P_)
        xd = dev(x)
        st = FP.member_stats_device(xd, PROBS, THRESHOLDS)
        assert st.quantiles.shape == (5, P_) and st.mean.shape == (P_,) and st.exceedance.shape == (3, P_)
        _assert_stats(st, x, f"S {S} P {P_}")
        again = FP.member_stats_device(xd, PROBS, THRESHOLDS)
        assert same_bits(st.quantiles, again.quantiles) and same_bits(st.mean, again.mean) and same_bits(st.exceedance, again.exceedance)


def test_member_stats_nan_column_strided_view_and_shapes():
    x = _member_case(100, 70, seed=4)
    x[37, 5] = np.nan
    x[0, 69] = np.nan
    x[99, 69] = np.nan
    st = FP.member_stats_device(dev(x), PROBS, THRESHOLDS)
    assert st.n_nan_positions == 2
    got = st.quantiles.cpu().numpy()
    assert np.isnan(got[:, [5, 69]]).all() and np.isnan(got).sum() == 10
    _assert_stats(st, x, "two NaN columns")
    # a view into a wider buffer: member stride 100 > P = 70, and positions of any shape
    wide = torch.full((100, 100), -5.0, device="cuda")
    wide[:, :70] = dev(x)
    view = wide[:, :70]
    assert view.stride(0) == 100 and not view.is_contiguous()
    sv = FP.member_stats_device(view, PROBS, THRESHOLDS)
    assert same_bits(sv.quantiles, st.quantiles) and same_bits(sv.mean, st.mean) and same_bits(sv.exceedance, st.exceedance)
    s3 = FP.member_stats_device(dev(x).view(100, 7, 10), PROBS, THRESHOLDS)
    assert s3.quantiles.shape == (5, 7, 10) and s3.mean.shape == (7, 10) and s3.exceedance.shape == (3, 7, 10)
    assert same_bits(s3.quantiles.view(5, 70), st.quantiles)
    s0 = FP.member_stats_device(dev(x), (0.5,))                  # no thresholds
    assert s0.exceedance.shape == (0, 70) and same_bits(s0.quantiles[0], st.quantiles[2])


def test_member_stats_member_offsets_past_2_31():
    stride = 2 ** 30 + 5
    buf = torch.empty(3 * stride, device="cuda")
    x = _member_case(3, 33, seed=8)
    rows = buf.view(3, stride)
    rows[:, :33] = dev(x)
    view = rows[:, :33]
    assert (view.shape[0] - 1) * view.stride(0) > 2 ** 31
    _assert_stats(FP.member_stats_device(view, PROBS, THRESHOLDS), x, "member stride 2^30 + 5")


def test_cabi_bad_arguments_return_minus_2():
    lib = _lib.load()
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    S, P_ = 10, 40
    x = dev(_member_case(S, P_, seed=1))
    quant = torch.full((2, P_), -7.0, device="cuda")
    mean = torch.full((P_,), -7.0, device="cuda")
    exceed = torch.full((1, P_), -7.0, device="cuda")
    n_nan = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    probs, thr = np.array([0.25, 1.0]), np.array([1.0])

    def stats(x=ptr(x), S=S, stride=P_, P=P_, probs=hp(probs), Q=2, thr=hp(thr), T=1, quant=ptr(quant), mean=ptr(mean),
              exceed=ptr(exceed), n_nan=ptr(n_nan)):
        return lib.rdgan_member_stats(x, S, stride, P, probs, Q, thr, T, quant, mean, exceed, n_nan, stream())

    for kw in (dict(x=null), dict(probs=null), dict(quant=null), dict(mean=null), dict(n_nan=null), dict(thr=null), dict(exceed=null),
               dict(S=0), dict(S=4097), dict(S=-1), dict(stride=P_ - 1), dict(P=0), dict(Q=0), dict(Q=17), dict(T=-1), dict(T=17),
               dict(probs=hp(np.array([0.25, 1.5]))), dict(probs=hp(np.array([-0.1, 1.0]))), dict(probs=hp(np.array([np.nan, 1.0]))),
               dict(thr=hp(np.array([np.nan]))), dict(thr=hp(np.array([np.inf])))):
        assert stats(**kw) == -2, kw

    nd, ny, nx, ov = 16, 20, 30, 4
    plan = F.tile_plan(ny, nx, nd, ov)
    hourly = dev(np.ones((2, 24, ny, nx), np.float32))
    peaks = torch.full((2, 2, ny, nx), -7.0, device="cuda")
    hour = torch.full((2, ny, nx), 77, dtype=torch.uint8, device="cuda")
    win = np.array([1, 6], np.int32)

    def pk(hourly=ptr(hourly), units=2, ny=ny, nx=nx, win=hp(win), K=2, peaks=ptr(peaks), hour=ptr(hour)):
        return lib.rdgan_hourly_peaks(hourly, units, ny, nx, win, K, peaks, hour, stream())

    bad_windows = [dict(win=null), dict(K=0), dict(K=9), dict(win=hp(np.array([6, 1], np.int32))), dict(win=hp(np.array([3, 3], np.int32))),
                   dict(win=hp(np.array([0, 1], np.int32))), dict(win=hp(np.array([1, 25], np.int32)))]
    for kw in bad_windows + [dict(hourly=null), dict(peaks=null), dict(hour=null), dict(units=0), dict(ny=0), dict(nx=0)]:
        assert pk(**kw) == -2, kw

    daily = dev(np.ones((2, ny, nx), np.float32))
    frac = dev(np.ones((2, 24, nd, nd), np.float32))
    yi, yw, xi, xw = plan.device_tables(daily.device)
    slots = np.array([[0, 1, -1, 0, 1, -1]], np.int32)

    def blend(frac=ptr(frac), m=2, slots=hp(slots), units=1, first=0, yi=ptr(yi), yw=ptr(yw), xi=ptr(xi), xw=ptr(xw), daily=ptr(daily),
              n_days=2, ny=ny, nx=nx, nd=nd, ov=ov, win=hp(win), K=2, peaks=ptr(peaks), hour=ptr(hour)):
        return lib.rdgan_field_blend_peaks(frac, m, slots, units, first, yi, yw, xi, xw, daily, n_days, ny, nx, nd, ov, win, K, peaks,
                                           hour, stream())

    for kw in bad_windows + [dict(frac=null), dict(slots=null), dict(yi=null), dict(yw=null), dict(xi=null), dict(xw=null), dict(daily=null),
                             dict(peaks=null), dict(hour=null), dict(m=0), dict(units=0), dict(first=-1), dict(nd=12), dict(ov=-1),
                             dict(ov=nd // 2 + 1), dict(ny=nd - 1), dict(nx=nd - 1), dict(n_days=0),
                             dict(slots=hp(np.array([[0, 1, -1, 0, 2, -1]], np.int32))),
                             dict(slots=hp(np.array([[0, 1, -2, 0, 1, -1]], np.int32)))]:
        assert blend(**kw) == -2, kw
    torch.cuda.synchronize()
    for t, v in ((quant, -7), (mean, -7), (exceed, -7), (n_nan, -7), (peaks, -7), (hour, 77)):           # nothing was launched
        assert bool((t == v).all())
    assert stats() == 0 and pk() == 0
    torch.cuda.synchronize()
    assert int(n_nan) == 0 and not bool((quant == -7).any()) and not bool((mean == -7).any()) and not bool((exceed == -7).any())
    assert bool((peaks[:, 0] == 1).all()) and bool((peaks[:, 1] == 6).all()) and bool((hour == 0).all())
    peaks.fill_(-7.0)
    assert blend() == 0
    torch.cuda.synchronize()
    assert not bool((peaks[0] == -7).any()) and bool((peaks[1] == -7).all())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def _field(D, seed):
    """(D, 40, 52) for nd 16, overlap 4 (3 x 4 tiles): a dry corner that swallows whole tiles, a NaN block; with two days the
    second is dry"""
    rng = np.random.default_rng(seed)
    daily = rng.gamma(0.6, 8.0, (D, 40, 52)).astype(np.float32) + np.float32(0.01)
    daily[0, :18, 30:] = 0.0
    daily[0, 20:23, 10:14] = np.nan
    if D == 2:
        daily[1] = 0.0
    return daily


@pytest.mark.parametrize("mode", ["shared", "independent"])
@pytest.mark.parametrize("D", [1, 2])
def test_disaggregate_peaks_equals_peaks_of_disaggregate(generator, mode, D):
    S, windows, chunk = 5, (1, 3, 6, 12, 24), 8          # below one unit's 11 tiles: every unit its own group, dry days too
    daily = _field(D, seed=40 + D)
    plan = F.tile_plan(40, 52, 16, 4)
    assert plan.n_tiles == 12
    z = np.random.default_rng(50 + D).normal(size=(S, D, 100) if mode == "shared" else (S, D, 12, 100)).astype(np.float32)
    arg = daily[0] if D == 1 else daily                    # one day as (ny, nx): the day axis is squeezed
    peaks, hour, info = FP.disaggregate_peaks(generator, arg, S, windows, overlap=4, latent_mode=mode, latent=z, chunk=chunk)
    hourly, info2 = F.disaggregate(generator, arg, S, overlap=4, latent_mode=mode, latent=z, chunk=chunk)
    assert info == info2 and info.n_active == 11           # day 0: the tile in the dry corner is skipped; day 1 is dry
    two_p, two_h = FP.peaks_device(hourly, windows)
    lead = (S,) if D == 1 else (S, D)
    assert peaks.shape == lead + (5, 40, 52) and hour.shape == lead + (40, 52)
    assert same_bits(peaks.reshape(S * D, 5, 40, 52), two_p) and same_bits(hour.reshape(S * D, 40, 52), two_h)
    # the 24-hour window is the day's sum
    p24 = peaks.view(S, D, 5, 40, 52)[:, :, 4].cpu().numpy().astype(np.float64)
    want = np.broadcast_to(daily.astype(np.float64)[None], p24.shape)
    np.testing.assert_allclose(p24, want, rtol=MASS_RTOL, atol=0, equal_nan=True)
    hour = hour.view(S, D, 40, 52).cpu().numpy()
    assert np.all(hour[:, np.isnan(daily)] == 255) and np.all(hour[:, daily == 0] == 0)

    # ensemble_products = member_stats_device on those peaks, one launch per (day, window)
    thr = np.array([[0.5, 2.0], [1.0, 5.0], [1.0, 10.0], [2.0, 20.0], [5.0, 50.0]])
    prod = FP.ensemble_products(generator, arg, S, windows, probs=(0.1, 0.5, 0.9, 0.99), thresholds=thr, overlap=4, latent_mode=mode,
                                latent=z, chunk=chunk)
    dlead = () if D == 1 else (D,)
    assert prod.windows == windows and prod.probs == (0.1, 0.5, 0.9, 0.99) and prod.info == info
    assert prod.quantiles.shape == dlead + (5, 4, 40, 52) and prod.mean.shape == dlead + (5, 40, 52)
    assert prod.exceedance.shape == dlead + (5, 2, 40, 52) and np.array_equal(prod.peak_hour.view(S, D, 40, 52).cpu().numpy(), hour)
    pk = peaks.view(S, D, 5, 40, 52)
    for d in range(D):
        for k in range(5):
            st = FP.member_stats_device(pk[:, d, k], prod.probs, thr[k])
            assert same_bits(prod.quantiles.view(D, 5, 4, 40, 52)[d, k], st.quantiles)
            assert same_bits(prod.mean.view(D, 5, 40, 52)[d, k], st.mean)
            assert same_bits(prod.exceedance.view(D, 5, 2, 40, 52)[d, k], st.exceedance)
    q = prod.quantiles.view(D, 5, 4, 40, 52).cpu().numpy()
    finite = ~np.isnan(daily)
    assert np.array_equal(np.isnan(q), np.broadcast_to(~finite[:, None, None], q.shape))
    assert np.all(np.diff(q, axis=2)[np.broadcast_to(finite[:, None, None], (D, 5, 3, 40, 52))] >= 0)        # monotone in probs
    none = FP.ensemble_products(generator, arg, S, windows, latent_mode=mode, latent=z, chunk=chunk)
    assert none.exceedance is None and same_bits(none.quantiles, prod.quantiles)


def test_hourly_ensemble_is_never_allocated(generator):
    """64 scenarios of a 64 x 64 field in groups of two units.  The engine's workspace is a cache that outlives the call, so a first
    call with two scenarios (the same groups) creates it; the rise of the peak over the second call is then what the call itself
    holds: the fraction buffer of one group and the peaks, far below the hourly ensemble."""
    S, ny, nx = 64, 64, 64
    daily = np.random.default_rng(6).gamma(0.6, 8.0, (ny, nx)).astype(np.float32) + np.float32(0.01)
    dd = dev(daily)
    FP.disaggregate_peaks(generator, dd, 2, (1, 24), chunk=64, seed=1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    peaks, hour, info = FP.disaggregate_peaks(generator, dd, S, (1, 24), chunk=64, seed=1)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    ensemble = S * 24 * ny * nx * 4
    print(f"peak memory rose by {rise / 2 ** 20:.1f} MiB; the hourly ensemble would take {ensemble / 2 ** 20:.1f} MiB")
    assert info.n_active == 25 and peaks.shape == (S, 2, ny, nx) and rise < ensemble


def test_scenario_products_field_is_the_device_result(generator, monkeypatch):
    monkeypatch.setattr(P, "gen", generator)
    daily = _field(1, seed=41)[0]
    np.random.seed(5)
    got = P.scenario_products_field(daily[..., None], 3, windows=(1, 6), probs=(0.5, 0.9), thresholds=(1.0,))
    np.random.seed(5)
    want = FP.ensemble_products(generator, daily, 3, (1, 6), (0.5, 0.9), (1.0,), norm_scale=P.norm_scale)
    assert got.windows == (1, 6) and got.probs == (0.5, 0.9) and got.info == want.info
    for name in ("quantiles", "mean", "exceedance", "peak_hour"):
        a, b = getattr(got, name), getattr(want, name).cpu().numpy()
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name
    assert got.quantiles.shape == (2, 2, 40, 52) and got.peak_hour.shape == (3, 40, 52)


class _NoGenerator:
    """any use of the generator beyond its geometry raises AttributeError"""
    ndomain, n_cond_channels = 16, 1


def test_no_wet_tile_never_touches_the_generator():
    daily = np.zeros((2, 20, 30), np.float32)
    daily[1] = np.nan
    peaks, hour, info = FP.disaggregate_peaks(_NoGenerator(), daily, 2, (1, 24))
    assert (info.n_tiles, info.n_active, info.n_nan_pixels) == (6, 0, 600) and peaks.shape == (2, 2, 2, 20, 30)
    peaks, hour = peaks.cpu().numpy(), hour.cpu().numpy()
    assert np.all(peaks[:, 0] == 0) and np.isnan(peaks[:, 1]).all() and np.all(hour[:, 0] == 0) and np.all(hour[:, 1] == 255)
    prod = FP.ensemble_products(_NoGenerator(), daily, 2, (1, 24), thresholds=(1.0,))
    q, ex = prod.quantiles.cpu().numpy(), prod.exceedance.cpu().numpy()
    assert q.shape == (2, 2, 4, 20, 30) and np.all(q[0] == 0) and np.isnan(q[1]).all() and np.all(ex[0] == 0) and np.isnan(ex[1]).all()
    assert np.all(prod.mean[0].cpu().numpy() == 0) and np.array_equal(prod.peak_hour.cpu().numpy(), hour)
