"""-m gpu: space-time structure of hourly fields (csrc/rdgan_spacetime.hip.h, pr_disagg_radar_gan_amd/spacetime.py) against the
numpy restatement (tests/spacetime_np.py, itself checked on the CPU by tests/test_spacetime_host.py).  Everything is an integer:
states are compared int64 against int64 with torch.equal, no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, models, spacetime as ST, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import spacetime_np as sn
from tests.hip_util import dev, ptr, stream

pytestmark = pytest.mark.gpu

THR2 = (0.5, 2.0)
THR8 = (0.0, 0.125, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)


def rain_days(n, ny, nx, R, seed):
    """(n, 24, ny, nx): rain-like, about 15 % wet, amounts on multiples of 1/8; a NaN in a corner of the core, an inf and a -inf
    on the rim, a value exactly at a threshold"""
    x = sn.rain_like((n, 24, ny, nx), seed)
    x[0, 3, R, R] = np.nan
    x[n - 1, 4, ny - 1 - R, nx - 1 - R] = np.nan
    x[0, 5, 0, nx // 2], x[n - 1, 6, ny // 2, nx - 1] = np.inf, -np.inf
    x[0, 7, ny // 2, nx // 2] = np.float32(0.5)
    return x


def check(x, thresholds, R, K, xd=None, **kw):
    """the state of one add() of x against the yardstick -> the SpaceTimeStructure"""
    want = sn.spacetime_np(x, thresholds, R, K)
    st = ST.SpaceTimeStructure(thresholds, R, K, **kw).add(dev(x) if xd is None else xd)
    got = st.state().cpu()
    assert got.shape == (ST.state_count(len(thresholds), R, K),)
    assert torch.equal(got, torch.from_numpy(sn.flat_state(want)))
    sn.check_identities(ST.split_state(got.numpy(), len(thresholds), R, K))
    return st


# name: (ny, nx, R, n, K).  3x3: the core is one pixel; 17x17 at R = 8 likewise; nx = 63, 64, 65, 129: the word boundaries, the funnel
# shift across words and the pad bits (64 takes the 16-byte loads, the others the scalar path); 520x17: two row bands of 260 rows;
# 9x600: 10 words, two column bands; 120x520: two row bands and two column bands, 16-byte loads
SHAPES = {"3x3": (3, 3, 1, 2, 2), "17x17": (17, 17, 8, 2, 2), "9x63": (9, 63, 4, 2, 2), "9x64": (9, 64, 4, 2, 2), "9x65": (9, 65, 4, 2, 2),
          "9x129": (9, 129, 4, 2, 2), "520x17": (520, 17, 1, 2, 2), "9x600": (9, 600, 4, 2, 1), "120x520": (120, 520, 2, 1, 1)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_rain_like_days_against_restatement(name):
    ny, nx, R, n, K = SHAPES[name]
    bh, cw = ST.tile_shape(ny, nx, R)
    assert (bh < ny) == (name in ("520x17", "120x520")) and (cw < (nx + 63) // 64) == (name in ("9x600", "120x520"))
    s = check(rain_days(n, ny, nx, R, len(name) + 7), THR2, R, K).result()
    assert s.n_days == n and s.n_bad_pixels == 4


@pytest.mark.parametrize("T,K,n", [(1, 1, 1), (8, 6, 3), (8, 1, 1), (1, 6, 3)])
def test_thresholds_lags_and_days(T, K, n):
    s = check(rain_days(n, 9, 65, 2, 10 * T + K), THR8[1:2] if T == 1 else THR8, 2, K).result()
    assert s.shift_hist.shape == (T, K, 5, 5) and s.n_days == n and s.shift_hist.sum() > 0


def test_grouping_passes_strides_and_input_kinds():
    ny, nx, R, K = 12, 64, 3, 2                                        # nx % 4 == 0: a dense tensor takes the 16-byte loads
    x = rain_days(3, ny, nx, R, 77)
    xd = dev(x)
    whole = check(x, THR2, R, K, xd=xd)

    def state(*parts, **kw):
        st = ST.SpaceTimeStructure(THR2, R, K, **kw)
        for part in parts:
            st.add(part)
        return st.state()

    assert torch.equal(state(xd[0], xd[1], xd[2]), whole.state())     # one call per day
    assert torch.equal(state(xd[:1], xd[1:]), whole.state())
    assert torch.equal(state(xd, planes_per_pass=24), whole.state())  # one day per pass
    assert torch.equal(state(xd, planes_per_pass=48), whole.state())  # two days, then a short pass
    assert torch.equal(state(xd, planes_per_pass=71), whole.state())  # taken in whole days: two again
    wide = torch.full((3, 24 * ny * nx + 52), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :24 * ny * nx].view(3, 24, ny, nx)
    view.copy_(xd)
    assert view.stride(0) == 24 * ny * nx + 52
    assert torch.equal(state(view), whole.state())
    odd = torch.full((3, 24 * ny * nx + 3), float("nan"), dtype=torch.float32, device="cuda")      # a stride that is no multiple of 4
    view = odd[:, :24 * ny * nx].view(3, 24, ny, nx)
    view.copy_(xd)
    assert torch.equal(state(view), whole.state())
    shifted = torch.full((3 * 24 * ny * nx + 1,), float("nan"), dtype=torch.float32, device="cuda")   # 4 bytes off a 16-byte boundary
    view = shifted[1:].view(3, 24, ny, nx)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4
    assert torch.equal(state(view), whole.state())
    assert torch.equal(state(x), whole.state())                       # numpy in
    assert torch.equal(state(xd[:1], x[1:]), whole.state())           # numpy onto a state that exists
    for t, thr in enumerate(THR2):                                    # a threshold's block does not depend on the others
        single = ST.SpaceTimeStructure((thr,), R, K).add(xd).result()
        assert np.array_equal(single.joint[0], whole.result().joint[t]) and np.array_equal(single.shift_hist[0], whole.result().shift_hist[t])
        assert np.array_equal(single.pairs, whole.result().pairs)
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2])
    with pytest.raises(ValueError):
        whole.add(xd[..., :60])                                       # another plane shape


@pytest.mark.parametrize("step", [(1, 0), (0, -1), (1, -1)])
def test_moving_blob_on_the_device(step):
    R, K, ny, nx = 2, 3, 32, 31
    start = (R + (0 if step[0] >= 0 else 23), R + (0 if step[1] >= 0 else 23))
    x = sn.moving_blob(2, ny, nx, start, step)
    s = check(x, (1.0,), R, K).result()
    for k in range(1, K + 1):
        dy, dx = k * step[0], k * step[1]
        if max(abs(dy), abs(dx)) <= R:
            assert s.shift_hist[0, k - 1, dy + R, dx + R] == 2 * (24 - k) == s.shift_hist[0, k - 1].sum() and s.dist_best[0, k - 1] == 0
    assert np.array_equal(s.mean_shift()[0, 0], np.array(step, np.float64)) and s.shift_gain()[0, 0] == 1.0
    assert s.indicator_correlation()[0, 1, step[0] + R, step[1] + R] == 1.0


@pytest.mark.parametrize("a,b,want", sn.TIES)
def test_tie_break_on_the_device(a, b, want):
    R = 2
    s = check(sn.tie_day(a, b), (0.5,), R, 1).result()
    assert s.shift_hist[0, 0, want[0] + R, want[1] + R] == 1 == s.shift_hist.sum() and s.no_shift[0, 0] == 22 and s.dist_best[0, 0] == 1


def test_all_wet_and_all_dry_on_the_device():
    x = np.zeros((2, 24, 9, 70), np.float32)
    x[1] = 3.0
    s = check(x, (1.0,), 4, 2).result()
    assert s.no_shift[0].tolist() == [23, 22] and s.shift_hist[0, :, 4, 4].tolist() == [23, 22] and s.dist_zero.sum() == 0
    assert s.pairs[1, 0, 8] == 2 * 23 * 5 * 66 and s.joint[0, 1, 0, 8] == 23 * 5 * 66


def test_bad_arguments_leave_the_state_untouched():
    lib = _lib.load()
    ny, nx, R, K = 5, 7, 2, 1
    x = dev(np.ones((1, 24, ny, nx), np.float32))
    counts = torch.full((ST.state_count(2, R, K),), -7, dtype=torch.int64, device="cuda")
    day = lib.rdgan_spacetime_workspace_bytes(ny, nx, 2, 24)
    ws = torch.full((day // 8,), -7, dtype=torch.int64, device="cuda")
    thr = np.array([0.1, 1.0])
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)

    def acc(x=ptr(x), n=1, stride=24 * ny * nx, ny=ny, nx=nx, th=hp(thr), T=2, R=R, K=K, counts=ptr(counts), ws=ptr(ws), nbytes=day):
        return lib.rdgan_spacetime_accumulate(x, n, stride, ny, nx, th, T, R, K, counts, ws, nbytes, stream())

    for kw in (dict(x=null), dict(counts=null), dict(ws=null), dict(th=null), dict(x=ctypes.c_void_p(x.data_ptr() + 2)),
               dict(counts=ctypes.c_void_p(counts.data_ptr() + 4)), dict(ws=ctypes.c_void_p(ws.data_ptr() + 4)), dict(n=0), dict(ny=4), dict(nx=4),
               dict(R=3), dict(R=0), dict(R=9), dict(K=0), dict(K=7), dict(T=0), dict(T=9), dict(th=hp(np.array([1.0, 0.1]))),
               dict(th=hp(np.array([np.nan, 1.0]))), dict(stride=24 * ny * nx - 1), dict(nbytes=day - 1), dict(nbytes=0), dict(n=2 ** 40)):
        assert acc(**kw) == -2, kw
    torch.cuda.synchronize()
    assert torch.all(counts == -7) and torch.all(ws == -7)
    counts.zero_()
    assert acc() == 0
    assert torch.equal(counts.cpu(), torch.from_numpy(sn.flat_state(sn.spacetime_np(np.ones((1, 24, ny, nx), np.float32), (0.1, 1.0), R, K))))


def test_library_exports_the_three_entries():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rdgan_spacetime_state_count", "rdgan_spacetime_workspace_bytes", "rdgan_spacetime_accumulate"):
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr) and name in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_structure_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, one NaN pixel, a dry tile; `chunk` is one unit's wet tiles on both sides, as
    tests/test_hip_cells.py pins it, so that the hourly values the two sides see are the same"""
    S, thr, R, K = 5, (0.1, 0.5, 2.0), 3, 2
    rng = np.random.default_rng(31)
    daily = (rng.gamma(0.8, 6.0, (40, 52)) * (rng.random((40, 52)) < 0.7)).astype(np.float32)
    daily[:16, :16] = 0.0
    daily[20, 30] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, dd, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, dd, S, latent=z, chunk=unit_tiles)
    assert info.n_nan_pixels == 1 and hourly.shape == (S, 24, 40, 52)
    want = check(hourly.cpu().numpy(), thr, R, K, xd=hourly)
    ws = want.result()
    assert ws.n_bad_pixels == S * 24 and ws.n_days == S and ws.shift_hist.sum() > 0
    for scenario_chunk in (1, 3, 5):
        got = ST.spacetime_structure_field(generator, dd if scenario_chunk == 3 else daily, S, thr, radius=R, max_lag=K, latent=z,
                                           scenario_chunk=scenario_chunk, chunk=unit_tiles)
        assert np.array_equal(sn.flat_state(vars(got)), want.state().cpu().numpy()), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.spacetime_structure_field(daily, S, thr, radius=R, max_lag=K, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert np.array_equal(sn.flat_state(vars(a)), ST.SpaceTimeStructure(thr, R, K).add(hourly2).state().cpu().numpy())


def test_field_on_a_dry_day_draws_nothing():
    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    s = ST.spacetime_structure_field(NoGenerator(), np.zeros((20, 30), np.float32), 3, (0.1,), radius=2, max_lag=2)
    assert np.array_equal(np.random.get_state()[1], before)
    assert s.n_days == 3 and s.no_shift[0].tolist() == [69, 66] and s.shift_hist.sum() == 0 and s.joint.sum() == 0
    assert s.pairs[0, 2, 2] == 72 * 600 and np.all(np.isnan(s.mean_speed()))
