"""-m gpu: extremes of hourly fields (csrc/rdgan_extremes.hip.h, pr_disagg_radar_gan_amd/extremes.py) against the numpy restatement
(tests/extremes_np.py, itself checked on the CPU by tests/test_extremes_host.py).  The block maxima and the L-moment sums are
integers and are compared with no tolerance; only the float64 formulas behind them have one, stated where it is used."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, areal as AR, catchments as CT, extremes as EX, field as F, field_products as FP, models, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import extremes_np as en
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

ALL_WINDOWS = (1, 2, 3, 6, 8, 12, 18, 24)
BLOCK11 = (2, 0, 2, 3, 0, 0, 3, 2, 2, 0, 3)                              # 11 days in 4 blocks, unsorted; block 1 has no day


@functools.lru_cache(maxsize=None)
def spells(days, ny, nx, seed):
    """shared: copy before writing"""
    return en.wet_spells(np.random.default_rng(seed), days, ny, nx)


def equal_state(bm, want):
    return all(torch.equal(g.cpu().view(-1), torch.from_numpy(w).view(-1)) for g, w in zip(bm.state(), want))


def check(x, block, n_blocks, windows, **kw):
    """one add() of x against the restatement -> (the BlockMaxima, the restatement's state)"""
    want = en.block_maxima_np(x, block, n_blocks, windows)
    bm = EX.BlockMaxima(windows, n_blocks, **kw).add(dev(x), block)
    for name, g, w in zip(("bmax", "ndays", "nvoid"), bm.result(), want):
        assert g.dtype == torch.from_numpy(w).dtype and torch.equal(g.cpu(), torch.from_numpy(w)), name
    return bm, want


@pytest.mark.parametrize("windows", [(1, 24), ALL_WINDOWS])
@pytest.mark.parametrize("plane", [(1, 1), (1, 7), (5, 7), (3, 67), (8, 64)])
def test_odd_planes_and_the_16_byte_route(plane, windows):
    x = spells(11, plane[0], plane[1], 1)
    bm, (bmax, ndays, nvoid) = check(x, BLOCK11, 4, windows)
    assert np.all(bmax[1] == -1) and not ndays[1].any() and ndays.sum() == 11 * plane[0] * plane[1] and not nvoid.any()
    assert bmax[[0, 2, 3], -1].max() > 0 and np.all(bmax[:, -1] >= bmax[:, 0])


def test_bad_values_void_the_pixel_day():
    x = spells(6, 5, 7, 2).copy()
    block = [0, 1, 0, 1, 2, 2]
    for day, (y, xx), hour, v in ((0, (0, 0), 3, np.nan), (1, (1, 2), 0, np.inf), (2, (2, 3), 23, -1.0), (3, (4, 6), 12, 2048.0)):
        x[day, hour, y, xx] = v
    x[0, 7, 3, 3] = 2047.999                                         # still good
    x[4, 5, 4, 0] = x[5, 9, 4, 0] = np.nan                            # pixel (4, 0) is void on both days of block 2
    x[1, 2, 1, 2] = -np.inf                                           # a second bad hour of a pixel-day that is void already
    bm, (bmax, ndays, nvoid) = check(x, block, 3, (1, 3, 24))
    want_void = np.zeros((3, 5, 7), np.int32)
    want_void[0, 0, 0] = want_void[1, 1, 2] = want_void[0, 2, 3] = want_void[1, 4, 6] = 1
    want_void[2, 4, 0] = 2
    assert np.array_equal(nvoid, want_void) and np.array_equal(ndays, 2 - want_void)
    assert np.all(bmax[2, :, 4, 0] == -1) and np.all(np.delete(bmax.reshape(3, 3, 35), 28, axis=2) >= 0)
    assert bmax[0, 0, 3, 3] == 2047 * 1024 + 1023
    q2, _ = en.quantise(x[2, :, 0, 0])                                # block 0 at pixel (0, 0): day 0 is void, the maxima are day 2's
    assert bmax[0, :, 0, 0].tolist() == [q2.max(), max(q2[h:h + 3].sum() for h in range(22)), q2.sum()]
    # an all-NaN array: every pixel-day void, nothing else
    bm, (bmax, ndays, nvoid) = check(np.full((3, 24, 5, 7), np.nan, np.float32), [0, 0, 1], 2, (1, 24))
    assert np.all(bmax == -1) and not ndays.any() and nvoid.sum() == 3 * 35


def test_ties_between_days_and_between_start_hours():
    x = np.zeros((4, 24, 1, 2), np.float32)
    x[0, 2:4, 0, 0] = x[0, 10:12, 0, 0] = 1.5                         # the same 2-hour sum at two start hours of one day
    x[1, 20:22, 0, 0] = 1.5                                           # and on a second day of the block
    x[2, 0, 0, 0] = 0.25
    x[3, 23, 0, 1] = 0.5 / 1024                                       # a quantisation tie: rint(0.5) = 0
    x[1, 5, 0, 1] = 1.5 / 1024                                        # rint(1.5) = 2
    bm, (bmax, _, _) = check(x, [0, 0, 1, 1], 2, (1, 2, 3, 24))
    assert bmax[:, :, 0, 0].tolist() == [[1536, 3072, 3072, 6144], [256, 256, 256, 256]] and bmax[:, 0, 0, 1].tolist() == [2, 0]


def test_grouping_order_strides_and_numpy():
    x = spells(11, 8, 64, 3).copy()
    x[4, 6, 3, 17] = np.nan
    xd = dev(x)
    whole, want = check(x, BLOCK11, 4, ALL_WINDOWS)
    new = lambda **kw: EX.BlockMaxima(ALL_WINDOWS, 4, **kw)
    by_day = new()
    for d in reversed(range(11)):
        by_day.add(xd[d:d + 1], BLOCK11[d:d + 1])
    assert equal_state(by_day, want)
    assert equal_state(new().add(xd[:4], BLOCK11[:4]).add(xd[4:], torch.tensor(BLOCK11[4:])), want)
    V = 24 * 512
    for pad in (52, 3):                                               # the second: no day but the first is 16-byte aligned
        wide = torch.full((11, V + pad), float("nan"), dtype=torch.float32, device="cuda")
        view = wide[:, :V].view(11, 24, 8, 64)
        view.copy_(xd)
        assert view.stride(0) == V + pad and equal_state(new().add(view, BLOCK11), want)
    assert equal_state(new().add(x, np.array(BLOCK11)), want)         # numpy in
    for run in (1, 3, 4096):
        assert equal_state(new(days_per_run=run).add(xd, BLOCK11), want), run
    # two leading axes (members, days, 24, ny, nx): the blocks in the order of the flattened axes
    x5 = spells(12, 5, 7, 4).reshape(3, 4, 24, 5, 7)
    block = (np.arange(3)[:, None] * 2 + np.array([0, 1, 1, 0])[None, :]).ravel()
    check(x5, block, 6, (1, 6, 24))
    again = whole.reset().add(xd, BLOCK11)
    assert again is whole and equal_state(whole, want)
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2], BLOCK11)
    with pytest.raises(ValueError):
        whole.add(xd[:, :, :4], BLOCK11)                              # the plane shape is pinned


def test_a_run_of_days_longer_than_a_workgroups_share():
    """300 days of an 8 x 8 plane in 3 blocks of 100: the library walks runs of 8 days, so the block changes inside the run of days
    96 .. 103 (and 200 falls on a boundary), and every run ends with a flush"""
    x = spells(300, 8, 8, 5).copy()
    x[150, 3, 2, 2] = np.nan
    block = np.repeat(np.arange(3), 100)
    bm, want = check(x, block, 3, (1, 3, 6, 12, 24))
    assert want[1].sum() == 300 * 64 - 1 and want[2].sum() == 1
    xd = dev(x)
    for run in (1, 7, 300):
        assert equal_state(EX.BlockMaxima((1, 3, 6, 12, 24), 3, days_per_run=run).add(xd, block), want), run
    shuffled = np.random.default_rng(6).permutation(300)
    assert equal_state(EX.BlockMaxima((1, 3, 6, 12, 24), 3).add(xd[torch.from_numpy(shuffled).cuda()].contiguous(), block[shuffled]), want)


# ---------------------------------------------------------------------------------------------------------------------------------
def check_sums(table, ndays=None, min_days=1):
    want_n, want_A, want_sorted = en.lmoment_sums_np(table, ndays, min_days)
    n, A, srt = EX.lmoment_sums(torch.from_numpy(table).cuda(), None if ndays is None else torch.from_numpy(ndays).cuda(), min_days, return_sorted=True)
    assert n.dtype == torch.int32 and A.dtype == torch.int64 and srt.dtype == torch.int64
    assert torch.equal(n.cpu(), torch.from_numpy(want_n)) and torch.equal(A.cpu(), torch.from_numpy(want_A))
    assert torch.equal(srt.cpu(), torch.from_numpy(want_sorted))
    n2, A2 = EX.lmoment_sums(table, ndays, min_days)                   # numpy in, no sorted output
    assert torch.equal(n2, n) and torch.equal(A2, A)
    return want_n, want_A


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M", [1, 63, 65, 1000])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 64, 128])
def test_lmoment_sums(B, M, S):
    rng = np.random.default_rng(1000 * B + 10 * M + S)
    table = rng.integers(0, 1 << 22, (S, B, M), dtype=np.int64)
    table[rng.random(table.shape) < 0.15] = -1                        # no maximum, at random places
    table[rng.random(table.shape) < 0.1] = 4096                       # ties
    table[S - 1, :, M // 2] = -1                                      # a whole series without a maximum
    table[0, :, M - 1] = rng.integers(-5, 0, B)                       # ... and every negative value counts as none
    n, A = check_sums(table)
    assert n[S - 1, M // 2] == 0 and not A[S - 1, M // 2].any() and (M == 1 or n[0, M - 1] == 0)


def test_lmoment_sums_equal_values_large_values_and_min_days():
    n, A = check_sums(np.full((2, 37, 70), 12345, np.int64))
    assert np.all(n == 37) and np.all(A[..., 0] == 37 * 12345) and np.all(A[..., 1] == 12345 * 36 * 37 // 2)
    big = np.full((1, 128, 66), (1 << 40) - 1, np.int64)              # A2 = (2^40 - 1) 127 126 128 / 3: near 2^62
    n, A = check_sums(big)
    assert A[0, 0, 2] == ((1 << 40) - 1) * (127 * 126 * 128 // 3) and A[0, 0, 2] > 1 << 59
    big[0, ::3, 5] = 7
    check_sums(big)
    rng = np.random.default_rng(8)
    table = rng.integers(-1, 50000, (2, 9, 130), dtype=np.int64)
    ndays = rng.integers(0, 6, table.shape).astype(np.int32)
    n, _ = check_sums(table, ndays, 3)
    assert 0 < n.sum() < (table >= 0).sum()
    check_sums(table, ndays, 0)
    check_sums(table, ndays.astype(np.int64), 6)                      # no block has six days
    with pytest.raises(ValueError):
        EX.lmoment_sums(torch.from_numpy(big + 1).cuda())             # a value of 2^40 on the device


# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ensemble():
    """3 members x 6 blocks x 4 days of a 5 x 7 plane, a void pixel-day and a block that is void at one pixel"""
    x = spells(72, 5, 7, 9).copy()
    x[5, 3, 2, 2] = np.nan
    x[24:28, 0, 4, 4] = np.nan                                        # member 1, block 0: all four days void at (4, 4)
    block = np.repeat(np.arange(18), 4)
    return x, block


REL_OBSERVED = 0.0                                                    # the largest relative deviation met against the restatement
# fp64 on both sides, the same handful of operations; they differ in the rounding of lgamma, exp, expm1 and log of two libraries.
# Largest deviation observed on the MI355X: 2.54e-13, in the GEV location (1.78e-13 in its return levels, 1.1e-15 in its scale,
# 3.5e-16 or less in everything Gumbel, 0 in the L-moments and the empirical levels); the bound is ten times it.  The GEV stands
# above the 1e-14 one would expect because lgamma(1 + k) is good to about 2^-53 in absolute terms and (1 - Gamma(1 + k)) / k
# divides that by a small k (extremes.gev_params).
REL_BOUND = 2.6e-12


def close(got, want, what):
    global REL_OBSERVED
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    dev_ = float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300), initial=0.0))
    REL_OBSERVED = max(REL_OBSERVED, dev_)
    print(f"{what}: largest relative deviation {dev_:.3e}")
    assert dev_ <= REL_BOUND, (what, dev_)


def test_end_to_end_against_the_restatement():
    x, block = ensemble()
    windows, T = (1, 3, 24), (2, 10, 50)
    st = EX.extremes(dev(x), block, 18, windows, series=3, return_sorted=True)
    bmax, ndays, _ = en.block_maxima_np(x, block, 18, windows)
    n, A, srt = en.lmoment_sums_np(bmax.reshape(3, 6, -1))
    assert st.windows == windows and st.shape == (3, 5, 7) and st.n_series == 3 and st.window_axis == 0
    assert torch.equal(st.n.cpu(), torch.from_numpy(n).view(3, 3, 5, 7)) and torch.equal(st.A.cpu(), torch.from_numpy(A).view(3, 3, 5, 7, 3))
    assert torch.equal(st.sorted.cpu(), torch.from_numpy(srt).view(3, 6, 3, 5, 7))
    assert n.reshape(3, 3, 5, 7)[1, :, 4, 4].tolist() == [5, 5, 5] and n.sum() == 3 * 3 * 35 * 6 - 3
    n, A, srt = n.reshape(3, 3, 5, 7), A.reshape(3, 3, 5, 7, 3), srt.reshape(3, 6, 3, 5, 7)
    l1, l2, t3 = en.lmoments_np(n, A)
    for name, got, want in zip(("l1", "l2", "t3"), st.lmoments(), (l1, l2, t3)):
        close(got, want, name)
    for name, got, want in zip(("gumbel loc", "gumbel scale"), st.gumbel(), en.gumbel_np(l1, l2)):
        close(got, want, name)
    for name, got, want in zip(("gev loc", "gev scale", "gev shape"), st.gev(), en.gev_np(l1, l2, t3)):
        close(got, want, name)
    for dist in EX.DISTS:
        close(st.return_levels(T, dist), en.return_levels_np(n, A, T, dist, srt), f"return levels {dist}")
    print(f"largest relative deviation of all: {REL_OBSERVED:.3e} (bound {REL_BOUND:.1e})")
    # min_days: with 4 a block counts only where all its days are good
    st4 = EX.extremes(dev(x), block, 18, windows, series=3, min_days=4)
    nd = np.broadcast_to(ndays.reshape(3, 6, 1, 35), (3, 6, 3, 35)).reshape(3, 6, -1)
    n4, A4, _ = en.lmoment_sums_np(bmax.reshape(3, 6, -1), nd, 4)
    assert torch.equal(st4.n.cpu().view(3, -1), torch.from_numpy(n4)) and torch.equal(st4.A.cpu().view(3, -1, 3), torch.from_numpy(A4))
    assert n4.reshape(3, 3, 5, 7)[0, :, 2, 2].tolist() == [5, 5, 5] and st4.sorted is None
    # the band is member_stats_device on the levels, applied by hand
    probs = (0.0, 0.25, 1.0)
    for dist in ("gumbel", "empirical"):
        levels = st.return_levels(T, dist)
        by_hand = FP.member_stats_device(levels.transpose(0, 1).to(torch.float32).contiguous(), probs).quantiles
        band = st.band(T, probs, dist)
        assert band.shape == (3, 3, 3, 5, 7) and band.dtype == torch.float32 and torch.equal(torch.nan_to_num(band, nan=-1.0), torch.nan_to_num(by_hand, nan=-1.0))
    # member 0 as the observation lies inside every band from the smallest member to the largest
    obs = EX.ExtremeStats(st.windows, st.n[:1], st.A[:1], st.unit, st.sorted[:1], 0)
    for dist in EX.DISTS:
        c = EX.compare(obs, st, T, probs, dist)
        valid = ~torch.isnan(c["obs"]) & ~torch.isnan(c["band"][0])
        assert c["inside"].shape == (3, 3, 5, 7) and torch.equal(c["inside"], valid) and c["share_inside"].shape == (3, 3)
        assert valid[:2].any() and torch.all(c["share_inside"][valid.flatten(2).any(dim=2)] == 1.0), dist
    c = EX.compare(obs, st, T, (0.4, 0.6), "gumbel")                   # a narrow band leaves a member outside somewhere
    assert float(c["share_inside"].max()) > 0.0 and float(c["share_inside"].min()) < 1.0


def test_depth_tables_of_areal_and_catchments():
    x = spells(12, 20, 24, 10).copy()
    x[[7, 8, 11], 4, 3, 3] = np.nan                                   # every day of block 3: no clean 24-hour window in basin 0
    xd, block = dev(x), [0, 0, 1, 1, 2, 2, 0, 3, 3, 1, 2, 3]
    regions = (np.arange(20)[:, None] // 10) * 2 + np.arange(24)[None, :] // 12
    _, by_box = AR.areal_extremes(xd, (1, 6, 24), (1, 5), return_depths=True)
    _, by_basin = CT.catchment_rainfall(xd, CT.CatchmentMap(regions=regions), (1, 6, 24), return_depths=True)
    assert by_box.shape == (12, 3, 2) and by_basin.shape == (12, 4, 3) and (by_basin == -1).nonzero().tolist() == [[7, 0, 2], [8, 0, 2], [11, 0, 2]]
    for depths, least in ((by_box, 4), (by_basin, 3)):
        table = EX.block_maxima_of_depths(depths, block, 5)            # block 4 has no day
        d = depths.cpu().numpy()
        want = np.full((5,) + d.shape[1:], -1, np.int64)
        for i, b in enumerate(block):
            want[b] = np.maximum(want[b], d[i])
        assert torch.equal(table.cpu(), torch.from_numpy(want)) and np.all(want[4] == -1)
        n, A, srt = EX.lmoment_sums(table.view(1, 5, -1), return_sorted=True)
        wn, wA, ws = en.lmoment_sums_np(want.reshape(1, 5, -1))
        assert torch.equal(n.cpu(), torch.from_numpy(wn)) and torch.equal(A.cpu(), torch.from_numpy(wA)) and torch.equal(srt.cpu(), torch.from_numpy(ws))
        assert wn.max() == 4 and wn.min() == least                     # the void block is left out of basin 0's 24-hour series


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_extremes_of_disaggregate(generator, monkeypatch):
    """4 wet days of a 20 x 24 plane at ndomain 16, overlap 4, in 2 blocks, 3 scenarios; `chunk` is one unit's tiles on both sides
    (every tile of every day is wet), so that the hourly values the two sides see are the same"""
    S, D, B, windows = 3, 4, 2, (1, 6, 24)
    rng = np.random.default_rng(41)
    daily = (0.1 + rng.gamma(0.8, 6.0, (D, 20, 24))).astype(np.float32)
    daily[1, 3, 5] = np.nan
    block = [0, 1, 1, 0]
    dd = dev(daily)
    z = np.random.default_rng(42).normal(size=(S, D, 100)).astype(np.float32)
    info = F.disaggregate(generator, dd, 1, latent=z[:1])[1]
    assert info.n_active == D * info.n_tiles and info.n_nan_pixels == 1
    hourly, _ = F.disaggregate(generator, dd, S, latent=z, chunk=info.n_tiles)
    assert hourly.shape == (S, D, 24, 20, 24)
    member_block = (np.arange(S)[:, None] * B + np.array(block)[None, :]).ravel()
    want = EX.extremes(hourly, member_block, S * B, windows, series=S, return_sorted=True)
    bmax, _, nvoid = en.block_maxima_np(hourly.cpu().numpy(), member_block, S * B, windows)
    n, A, _ = en.lmoment_sums_np(bmax.reshape(S, B, -1))
    assert torch.equal(want.n.cpu().view(S, -1), torch.from_numpy(n)) and torch.equal(want.A.cpu().view(S, -1, 3), torch.from_numpy(A))
    assert nvoid.sum() == S and np.all(nvoid[1::2, 3, 5] == 1) and n.min() == 2 and bmax[:, -1].min() > 0
    for scenario_chunk in (1, 2, 3):
        got = EX.extremes_field(generator, dd if scenario_chunk == 2 else daily, S, block, B, windows, return_sorted=True, latent=z,
                                scenario_chunk=scenario_chunk, chunk=info.n_tiles)
        assert got.windows == windows and got.shape == (3, 20, 24) and got.n_series == S
        assert torch.equal(got.n, want.n) and torch.equal(got.A, want.A) and torch.equal(got.sorted, want.sorted), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.extremes_field(daily, S, block, B, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    b = EX.extremes(hourly2, member_block, S * B, a.windows, series=S)
    assert a.windows == (1, 3, 6, 12, 24) and torch.equal(a.n, b.n) and torch.equal(a.A, b.A) and a.sorted is None


def test_c_entries_refuse_bad_arguments_and_touch_nothing():
    lib = _lib.load()
    x = dev(spells(3, 5, 7, 11))
    bmax = torch.full((2, 2, 35), -1, dtype=torch.int64, device="cuda")
    ndays = torch.zeros((2, 35), dtype=torch.int32, device="cuda")
    nvoid = torch.zeros((2, 35), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)
    null = ctypes.c_void_p(0)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mask = (1 << 0) | (1 << 23)

    def acc(xp=p(x), n=3, stride=24 * 35, ny=5, nx=7, block=(0, 1, 1), NB=2, mask=mask, run=0, bp=p(bmax), dp=p(ndays), vp=p(nvoid)):
        b = np.array(block, np.int32) if block is not None else None
        return lib.rdgan_block_maxima_accumulate(xp, n, stride, ny, nx, b.ctypes.data_as(ctypes.c_void_p) if b is not None else null, NB, mask, run,
                                                 bp, dp, vp, st())

    for kw in (dict(xp=null), dict(block=None), dict(bp=null), dict(dp=null), dict(vp=null), dict(xp=off(x, 2)), dict(bp=off(bmax, 4)),
               dict(dp=off(ndays, 2)), dict(vp=off(nvoid, 1)), dict(n=0), dict(n=-1), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4096),
               dict(stride=24 * 35 - 1), dict(NB=0), dict(NB=1 << 26), dict(NB=(1 << 31) + 1), dict(mask=0), dict(mask=1 << 24), dict(mask=0x1FF),
               dict(block=(0, 2, 1)), dict(block=(0, -1, 1)), dict(run=-1), dict(run=4097)):
        assert acc(**kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.all(bmax == -1) and not ndays.any() and not nvoid.any()
    assert acc() == 0 and acc(xp=p(x[:1]), n=1, block=(0,), run=1) == 0          # day 0 twice in block 0
    want = en.block_maxima_np(x.cpu().numpy()[[0, 1, 2, 0]], (0, 1, 1, 0), 2, (1, 24))
    assert all(torch.equal(g.cpu().view(-1), torch.from_numpy(w).view(-1)) for g, w in zip((bmax, ndays, nvoid), want))
    # the sums
    table = torch.from_numpy(np.random.default_rng(12).integers(-1, 1000, (2, 5, 9), dtype=np.int64)).cuda()
    nd = torch.ones((2, 5, 9), dtype=torch.int32, device="cuda")
    A = torch.full((2, 9, 3), -7, dtype=torch.int64, device="cuda")
    n = torch.full((2, 9), -7, dtype=torch.int32, device="cuda")
    srt = torch.full((2, 5, 9), -7, dtype=torch.int64, device="cuda")

    def sums(tp=p(table), ndp=p(nd), min_days=1, S=2, B=5, M=9, Ap=p(A), np_=p(n), sp=p(srt)):
        return lib.rdgan_lmoment_sums(tp, ndp, min_days, S, B, M, Ap, np_, sp, st())

    for kw in (dict(tp=null), dict(Ap=null), dict(np_=null), dict(tp=off(table, 4)), dict(Ap=off(A, 4)), dict(sp=off(srt, 4)), dict(np_=off(n, 2)),
               dict(ndp=off(nd, 2)), dict(S=0), dict(M=0), dict(B=0), dict(B=129), dict(S=1 << 40), dict(M=1 << 40)):
        assert sums(**kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.all(A == -7) and torch.all(n == -7) and torch.all(srt == -7)
    assert sums() == 0
    wn, wA, ws = en.lmoment_sums_np(table.cpu().numpy())
    assert torch.equal(n.cpu(), torch.from_numpy(wn)) and torch.equal(A.cpu(), torch.from_numpy(wA)) and torch.equal(srt.cpu(), torch.from_numpy(ws))
    assert sums(ndp=null, sp=null) == 0                                # no ndays, no sorted output
    torch.cuda.synchronize()
    assert torch.equal(A.cpu(), torch.from_numpy(wA))
