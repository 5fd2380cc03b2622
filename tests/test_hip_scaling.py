"""-m gpu: the scaling structure of hourly fields (csrc/rdgan_scaling.hip.h, pr_disagg_radar_gan_amd/scaling.py) against the numpy
restatement (tests/scaling_np.py, itself checked on the CPU by tests/test_scaling_host.py).  Everything is an integer: the whole
state is compared int64 against int64, with no tolerance."""
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import field as F, models, scaling as SC, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import scaling_np as sn
from tests.hip_util import dev

pytestmark = pytest.mark.gpu


def check(x, A=None, **kw):
    """the state of one add() of x against the yardstick -> the ScalingStructure"""
    sc = SC.ScalingStructure(A, **kw).add(dev(x) if isinstance(x, np.ndarray) else x)
    want = sn.flat_state(sn.scaling_np(x if isinstance(x, np.ndarray) else x.cpu().numpy(), sc.space_levels))
    got = sc.state().cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    return sc


@functools.lru_cache(maxsize=None)
def rain_like(ny, nx, days, seed):
    """(days, 24, ny, nx): gamma amounts where a smoothed noise field is above its 75 % quantile -- mostly zeros, the wet areas have a
    size; some values at quantisation ties.  Shared: copy before writing."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(days, 24, ny, nx))
    for _ in range(2):
        g = (g + np.roll(g, 1, 1) + np.roll(g, 1, 2) + np.roll(g, -1, 2) + np.roll(g, 1, 3) + np.roll(g, -1, 3)) / 6
    x = ((0.2 + rng.gamma(0.6, 3.0, g.shape)) * (g > np.quantile(g, 0.75))).astype(np.float32)
    ties = rng.random(g.shape) < 0.03
    x[ties] = ((rng.integers(0, 8192, g.shape) + 0.5) / 1024).astype(np.float32)[ties]
    return x


def test_one_full_tile():
    s = check(rain_like(64, 64, 1, 1)).result()
    assert s.space_levels == 6 and s.n_days_total == 1 and s.n_bad == 0 and not s.n_void.any()
    assert s.n_boxes.tolist() == [[4096 // 4 ** a * 24 // T for T in SC.DURATIONS] for a in range(7)]
    assert np.all(s.sum1 == s.sum1[0, 0]) and 0 < s.wet_fraction()[0, 0] < 0.5


@pytest.mark.parametrize("days", [1, 5, 16, 17])
def test_collage_of_16x16(days):
    """a partly filled collage, exactly one, and one plane that spills into a second workgroup"""
    s = check(rain_like(16, 16, 17, 2)[:days]).result()
    assert s.space_levels == 4 and s.n_days_total == days and s.n_boxes[4].tolist() == [days * 24 // T for T in SC.DURATIONS]


@pytest.mark.parametrize("shape", [(8, 8), (1, 1), (2, 64), (3, 4)])
def test_collage_of_other_shapes(shape):
    ny, nx = shape
    s = check(rain_like(ny, nx, 70, 3))
    assert s.space_levels == {(8, 8): 3, (1, 1): 0, (2, 64): 1, (3, 4): 1}[shape]
    check(rain_like(ny, nx, 4097 if shape == (1, 1) else 70, 3))              # (1 x 1: 4096 days fill a collage)


@pytest.mark.parametrize("shape", [(70, 67), (33, 130)])
def test_rims(shape):
    """rim tiles, boxes dropped per level, a single box of the top level in a row or a column"""
    ny, nx = shape
    s = check(rain_like(ny, nx, 3, 4)).result()
    assert s.space_levels == (6 if shape == (70, 67) else 5)
    assert s.n_boxes[:, 0].tolist() == [3 * 24 * (ny >> a) * (nx >> a) for a in range(s.space_levels + 1)]
    x = rain_like(ny, nx, 3, 4).copy()
    x[1, 4, ny - 1, nx - 1] = np.nan                                         # in the rim of every level above 0
    s = check(x).result()
    assert s.n_bad == 1 and s.n_void.tolist() == [[1] * 5] + [[0] * 5] * s.space_levels


def test_bad_values_void_exactly_their_boxes_and_windows():
    x = rain_like(64, 64, 1, 5).copy()
    x[0, 0, 0, 0], x[0, 7, 13, 50], x[0, 16, 63, 63], x[0, 23, 40, 9] = np.nan, np.inf, -0.5, 2048.0
    s = check(x).result()
    assert s.n_bad == 4
    # the four lie in four boxes up to level 4 (16 x 16: (0, 0), (0, 3), (3, 3), (2, 0)), and level 5 keeps them apart; hours 0, 7, 16, 23 share two 8-hour windows
    assert s.n_void[:5].tolist() == [[4, 4, 4, 4, 4]] * 5 and s.n_void[5].tolist() == [4, 4, 4, 4, 4] and s.n_void[6].tolist() == [4, 4, 4, 2, 1]
    x = rain_like(64, 64, 1, 5).copy()
    x[0, 2, 5, 5], x[0, 3, 6, 6] = np.nan, np.nan                           # one 2-hour window, two pixels of one 4 x 4 box
    s = check(x).result()
    assert s.n_bad == 2 and s.n_void[:, 0].tolist() == [2] * 7 and s.n_void[:, 1].tolist() == [2, 2] + [1] * 5


def test_box_sums_past_2_32():
    """every pixel-hour at the largest good value, 2048 - 2^-13, whose 1024-fold rounds up to 2^21: the day's sum over 64 x 64 pixels is
    24 * 2^33 = 1.5 * 2^37, the largest R there is"""
    x = np.full((1, 24, 64, 64), np.nextafter(np.float32(2048), np.float32(0)), np.float32)
    q = 2048 * 1024
    s = check(x).result()
    assert s.max_R.tolist() == [[q * 4 ** a * T for T in SC.DURATIONS] for a in range(7)] and s.max_R[6, 4] > 2 ** 37
    assert [[int(v) for v in row] for row in s.sum2()] == [[(q * 4 ** a * T) ** 2 * (4096 // 4 ** a) * (24 // T) for T in SC.DURATIONS] for a in range(7)]
    # the last bin that can be hit: the largest R has e = 37 and the bits 100 below its leading one
    assert sn.bin_of(q * 4096 * 24) == 284 and s.hist[6, 4, 284] == 1 and s.hist[6, 4].sum() == 1


def test_rounding_ties_go_to_even():
    rng = np.random.default_rng(8)
    x = ((2 * rng.integers(0, 1 << 15, (2, 24, 16, 16)) + 1) / 2048).astype(np.float32)
    assert np.all(np.modf(x.astype(np.float64) * 1024)[0] == 0.5)
    s = check(x).result()
    assert s.sum1[0, 0] == int((np.rint(x.astype(np.float64) * 1024)).sum()) and s.sum1[0, 0] % 2 == 0


def test_all_dry():
    s = check(np.zeros((2, 24, 32, 32), np.float32)).result()
    assert s.space_levels == 5 and not s.n_wet.any() and np.array_equal(s.hist[:, :, 0], s.n_boxes) and not s.sum1.any() and not s.max_R.any()
    assert np.all(s.wet_fraction() == 0) and np.all(np.isnan(s.exponents((1, 2)).slopes))


def test_grouping_strides_and_load_route():
    x = rain_like(16, 16, 7, 6).copy()
    x[3, 11, 4, 9] = np.nan
    xd = dev(x)
    whole = check(x)
    new = lambda: SC.ScalingStructure()
    assert torch.equal(new().add(xd[:3]).add(xd[3:]).state(), whole.state())
    assert torch.equal(new().add(xd[:3]).add(x[3:]).state(), whole.state())                # numpy onto a state that exists
    assert torch.equal(new().add(xd.view(1, 7, 24, 16, 16)).state(), whole.state())
    V = 24 * 256
    for pad in (52, 3):                                                     # the second: no day but the first is 16-byte aligned
        wide = torch.full((7, V + pad), float("nan"), dtype=torch.float32, device="cuda")
        view = wide[:, :V].view(7, 24, 16, 16)
        view.copy_(xd)
        assert view.stride(0) == V + pad
        assert torch.equal(new().add(view).state(), whole.state())
    # the same data behind a pointer offset by one float: the scalar route
    flat = torch.empty(7 * V + 1, dtype=torch.float32, device="cuda")
    shifted = flat[1:].view(7, 24, 16, 16)
    shifted.copy_(xd)
    assert shifted.data_ptr() % 16 == 4 and xd.data_ptr() % 16 == 0
    assert torch.equal(new().add(shifted).state(), whole.state())
    y = rain_like(70, 67, 3, 4)                                              # (an odd nx: the scalar route in any case)
    big = torch.empty(y.size + 1, dtype=torch.float32, device="cuda")
    big[1:].view(y.shape).copy_(dev(y))
    assert torch.equal(new().add(big[1:].view(y.shape)).state(), new().add(dev(y)).state())
    z = rain_like(64, 64, 1, 1)
    big = torch.empty(z.size + 1, dtype=torch.float32, device="cuda")
    big[1:].view(z.shape).copy_(dev(z))
    assert torch.equal(new().add(big[1:].view(z.shape)).state(), new().add(dev(z)).state())
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2])


def test_smaller_space_levels_give_a_prefix():
    x = rain_like(70, 67, 3, 4)
    full = check(x).state().cpu().numpy()
    for A in (0, 2, 5):
        part = check(x, A).state().cpu().numpy()
        assert np.array_equal(part[:-2], full[:SC.state_count(A) - 2]) and np.array_equal(part[-2:], full[-2:])
    with pytest.raises(ValueError):
        SC.ScalingStructure(5).add(dev(rain_like(16, 16, 17, 2)))


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_structure_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, one NaN pixel, a dry tile; `chunk` is one unit's wet tiles on both sides, the batch
    condition evaluate_field documents, so that the hourly values the two sides see are the same.  (A real generator at its initial
    weights: tests/fake_engine.py stands in for the training engine and has no generator forward for fields.)"""
    S = 5
    rng = np.random.default_rng(31)
    daily = (rng.gamma(0.8, 6.0, (40, 52)) * (rng.random((40, 52)) < 0.7)).astype(np.float32)
    daily[:16, :16] = 0.0
    daily[2, 50] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, dd, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, dd, S, latent=z, chunk=unit_tiles)
    assert info.n_nan_pixels == 1 and hourly.shape == (S, 24, 40, 52)
    want = check(hourly)
    ws = want.result()
    assert ws.space_levels == 5 and ws.n_bad == S * 24 and ws.n_days_total == S and np.all(ws.max_R > 0)
    for scenario_chunk in (1, 3, 5):
        got = SC.scaling_structure_field(generator, dd if scenario_chunk == 3 else daily, S, latent=z, scenario_chunk=scenario_chunk, chunk=unit_tiles)
        assert np.array_equal(sn.flat_state(vars(got)), want.state().cpu().numpy()), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.scaling_scenarios_field(daily, S, space_levels=3, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert a.space_levels == 3 and np.array_equal(sn.flat_state(vars(a)), SC.ScalingStructure(3).add(hourly2).state().cpu().numpy())
