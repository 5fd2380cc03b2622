"""-m gpu: the integer state of the intensity-scale verification (csrc/rdgan_iss.hip.h, pr_disagg_radar_gan_amd/intensity_scale.py)
against the numpy restatement (tests/iss_np.py, itself checked on the CPU by tests/test_iss_host.py).  Every comparison of state is
an equality of int64 arrays."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import field as F, intensity_scale as IS, models, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import iss_np as yn
from tests.hip_util import dev, lib

pytestmark = pytest.mark.gpu

THR8 = (0.0, 0.1, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0)
THR2 = (0.1, 1.0)
# name: (members, leading shape, ny, nx, L, thresholds)
CASES = {
    "64x64-L6-T1": (3, (), 64, 64, 6, (0.5,)),
    "64x64-L6-T8": (3, (), 64, 64, 6, THR8),
    "65x67-L6": (2, (), 65, 67, 6, THR2),                            # crop offsets (0, 1); rows off 16 bytes
    "130x70-L6": (2, (), 130, 70, 6, THR2),                          # 2 x 1 tiles, offsets (1, 3)
    "8x8-L3": (3, (5,), 8, 8, 3, THR2),                              # 64 days side by side in a block: 5 of them there
    "16x16-L4": (2, (2,), 16, 16, 4, THR2),
    "16x16-L2": (2, (2,), 16, 16, 2, THR2),
    "16x16-L1": (2, (2,), 16, 16, 1, THR2),
    "32x32-L5": (2, (3,), 32, 32, 5, THR2),
    "24x40-L3": (2, (3,), 24, 40, 3, THR2),                          # 24 rows in a share of 32; 40 columns: one day across
    "70x130-L4": (2, (), 70, 130, 4, THR2),                          # partial blocks at both edges
    "131x140-L7": (2, (), 131, 140, 7, THR2),
    "256x256-L8": (2, (), 256, 256, 8, THR2),
    "300x270-L8": (2, (), 300, 270, 8, THR2),                        # one tile and a crop (22, 7), through the upper kernel
    "256x384-L7": (2, (), 256, 384, 7, THR2),                        # 2 x 3 tiles of four blocks
}


@functools.lru_cache(maxsize=None)
def data(name):
    """(members (s, *lead, 24, ny, nx), obs): blobs of 0 .. 12 mm/h, some values exactly at a threshold, negative values, and
    NaN, +inf and -inf pixels on either side, in the crop margin and at block corners"""
    s, lead, ny, nx, L, thr = CASES[name]
    rng = np.random.default_rng(ny * 1000 + nx + L)
    shape = lead + (24, ny, nx)

    def blobs(shape):
        f = rng.random(shape)
        f = sum(np.roll(np.roll(f, dy, -2), dx, -1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9
        a = np.where(f > 0.52, 12.0 * rng.random(shape), 0.0)
        a = np.where(rng.random(shape) < 0.05, rng.choice(np.asarray(thr), shape), a)        # at a threshold: no event
        return np.where(rng.random(shape) < 0.02, -1.0, a).astype(np.float32)

    obs, ens = blobs(shape), blobs((s,) + shape)
    oy, ox, cy, cx = yn.crop(ny, nx, L)
    bads = (np.nan, np.inf, -np.inf)
    flat_o, flat_e = obs.reshape(-1, 24, ny, nx), ens.reshape(s, -1, 24, ny, nx)
    for k in range(6):                                              # hours 0 .. 5: a bad pixel in the crop, member then observation
        y, x = oy + int(rng.integers(cy)), ox + int(rng.integers(cx))
        if k < 3:
            flat_e[k % s, -1, k, y, x] = bads[k]
        else:
            flat_o[0, k, y, x] = bads[k - 3]
    if oy or ox:                                                    # the margin: no effect
        flat_e[0, 0, 7, 0, 0], flat_o[0, 8, ny - 1, nx - 1] = np.nan, np.inf
    if cy >= 128:                                                   # the corner where four blocks meet
        flat_e[-1, 0, 9, oy + 64, ox + 63] = np.nan
    return ens, obs


@functools.lru_cache(maxsize=None)
def reference(name):
    ens, obs = data(name)
    return yn.state_np(ens, obs, CASES[name][5], CASES[name][4])


def state_of(ver):
    counts, tiles = ver.state()
    return counts.cpu().numpy(), tiles.cpu().numpy()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", list(CASES))
def test_state_against_restatement(name):
    s, lead, ny, nx, L, thr = CASES[name]
    ens, obs = data(name)
    want = reference(name)
    assert want[1][:, 1].sum() >= 6 and want[1][:, 0].sum() > 0       # void and valid tiles both occur
    ver = IS.IntensityScaleVerifier(dev(obs), thr, L).add(dev(ens))
    got = state_of(ver)
    assert got[0].shape == (len(thr), 24, L + 1, 3) and got[1].shape == (24, 2)
    assert np.array_equal(got[1], want[1]), name
    assert np.array_equal(got[0], want[0]), name
    r = ver.result()
    assert r.levels == L and np.isclose(np.nansum(r.mse(), axis=-1), (r.contingency()[:, 1] + r.contingency()[:, 2]) / r.contingency().sum(axis=-1)).all()


def test_default_levels_and_leading_shapes():
    ens, obs = data("16x16-L4")
    ver = IS.IntensityScaleVerifier(obs, THR2).add(ens)               # numpy in, (D, 24, ny, nx), levels by default
    assert ver.levels == 4 and same(state_of(ver), reference("16x16-L4"))
    one = IS.IntensityScaleVerifier(dev(obs[1]), THR2, 4).add(dev(ens[:, 1]))                        # (24, ny, nx)
    assert same(state_of(one), yn.state_np(ens[:, 1], obs[1], THR2, 4))


def test_void_rule():
    L, thr = 3, (0.5,)
    rng = np.random.default_rng(4)
    obs = (rng.random((24, 19, 18)) * 2).astype(np.float32)          # crop (1, 1): 2 x 2 tiles of 8
    ens = (rng.random((2, 24, 19, 18)) * 2).astype(np.float32)
    clean = state_of(IS.IntensityScaleVerifier(obs, thr, L).add(ens))
    assert clean[1].tolist() == [[8, 0]] * 24 and same(clean, yn.state_np(ens, obs, thr, L))
    for h, bad in enumerate((np.nan, np.inf, -np.inf)):
        e, o = ens.copy(), obs.copy()
        e[1, h, 3, 4] = bad                                          # a member tile only: one pair's tile (0, 0)
        o[h + 3, 12, 12] = bad                                       # the observed tile (1, 1): void for both members
        e[0, h + 6, 0, 5], o[h + 6, 18, 3], e[0, h + 6, 17, 17] = bad, bad, bad       # the margin: no effect
        got = state_of(IS.IntensityScaleVerifier(o, thr, L).add(e))
        assert got[1][h].tolist() == [7, 1] and got[1][h + 3].tolist() == [6, 2] and got[1][h + 6].tolist() == [8, 0]
        assert same(got, yn.state_np(e, o, thr, L)) and np.array_equal(got[0][:, h + 6], clean[0][:, h + 6])
    e = ens.copy()
    e[0, 0] = -np.abs(e[0, 0])                                       # negative and finite: not bad, no event
    got = state_of(IS.IntensityScaleVerifier(obs, thr, L).add(e))
    assert got[1].tolist() == [[8, 0]] * 24 and same(got, yn.state_np(e, obs, thr, L)) and got[0][0, 0, 0, 2] < clean[0][0, 0, 0, 2]
    # L = 7: a NaN in one 64-block voids the whole 128 tile for that pair and no other
    obs = (rng.random((24, 128, 256)) * 2).astype(np.float32)
    ens = (rng.random((2, 24, 128, 256)) * 2).astype(np.float32)
    ens[1, 2, 70, 200] = np.nan                                      # member 1, hour 2, tile (0, 1), its block (1, 1)
    got = state_of(IS.IntensityScaleVerifier(obs, thr, 7).add(ens))
    assert got[1][2].tolist() == [3, 1] and got[1][:, 1].sum() == 1 and same(got, yn.state_np(ens, obs, thr, 7))
    other = state_of(IS.IntensityScaleVerifier(obs[:, :, :128], thr, 7).add(ens[:, :, :, :128]))    # the left tiles alone
    left = yn.events(ens[0, 2, :, 128:], 0.5).sum() ** 2             # hour 2, level 7: member 0's right tile is all that is added
    assert got[0][0, 2, 7, 0] - other[0][0, 2, 7, 0] == left


def test_a_value_equal_to_the_threshold_is_no_event():
    thr = (0.1, 1.0)
    t32 = np.asarray(thr, np.float32)
    obs = np.zeros((24, 8, 8), np.float32)
    ens = np.zeros((1, 24, 8, 8), np.float32)
    ens[0, 0], ens[0, 1], ens[0, 2] = t32[0], np.nextafter(t32[0], np.float32(1)), t32[1]
    got = state_of(IS.IntensityScaleVerifier(obs, thr, 3).add(ens))
    assert got[0][:, 0, 0, 0].tolist() == [0, 0] and got[0][:, 1, 0, 0].tolist() == [64, 0] and got[0][:, 2, 0, 0].tolist() == [64, 0]
    assert got[0][0, 1, :, 0].tolist() == [64, 64 * 4, 64 * 16, 64 * 64]


@pytest.mark.parametrize("name", ["70x130-L4", "131x140-L7"])
def test_grouping_does_not_change_the_state(name):
    s, lead, ny, nx, L, thr = CASES[name]
    rng = np.random.default_rng(11)
    _, obs = data(name)
    ens = np.concatenate([data(name)[0], (rng.random((3, 24, ny, nx)) * 3).astype(np.float32)])      # 5 members
    ens[3, 4, ny // 2, nx // 2] = np.nan
    want = yn.state_np(ens, obs, thr, L)
    od, ed = dev(obs), dev(ens)
    whole = state_of(IS.IntensityScaleVerifier(od, thr, L).add(ed))
    assert same(whole, want)
    for cut in (1, 2):
        assert same(state_of(IS.IntensityScaleVerifier(od, thr, L).add(ed[:cut]).add(ed[cut:])), whole), cut
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    assert same(state_of(IS.IntensityScaleVerifier(od, thr, L).add(ed[perm])), whole)
    for ppp in (1, 3, 7, 24):                                       # 1 pair a pass; the members cut 3 + 2; one unit a pass; four
        assert same(state_of(IS.IntensityScaleVerifier(od, thr, L, pairs_per_pass=ppp).add(ed)), whole), ppp
    Pn = 24 * ny * nx
    wide = torch.full((5, Pn + 52), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :Pn].view(5, 24, ny, nx)
    view.copy_(ed)
    assert view.stride(0) == Pn + 52 and same(state_of(IS.IntensityScaleVerifier(od, thr, L).add(view)), whole)
    assert same(state_of(IS.IntensityScaleVerifier(obs, thr, L).add(ens)), whole)                    # numpy in
    r = IS.intensity_scale_hourly(ed, od, thr, L)
    assert np.array_equal(r.counts, whole[0]) and np.array_equal(r.tiles, whole[1])
    with pytest.raises(ValueError):
        IS.IntensityScaleVerifier(od, thr, L).add(ed[:, :, :-1])


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_the_held_ensemble(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, a dry tile and a NaN pixel in the observation; `chunk` is one unit's wet tiles on both
    sides, the batch condition _hourly.evaluate_field states, so that the hourly values the two sides see are the same"""
    S, thr, L = 8, (0.01, 0.05, 0.2), 3
    rng = np.random.default_rng(31)
    obs = (rng.gamma(0.8, 0.6, (24, 40, 52)) * (rng.random((24, 40, 52)) < 0.5)).astype(np.float32)
    obs[:, :16, :16] = 0.0
    obs[3, 20, 30] = np.nan
    od = dev(obs)
    daily = od.sum(dim=0)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, daily, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, daily, S, latent=z, chunk=unit_tiles)
    want = IS.intensity_scale_hourly(hourly, od, thr, L)
    ref = yn.state_np(hourly.cpu().numpy(), obs, thr, L)
    assert np.array_equal(want.counts, ref[0]) and np.array_equal(want.tiles, ref[1]) and want.tiles[3, 1] == S and want.counts[0, :, 0, 0].min() > 0
    for scenario_chunk in (1, 7, S):
        got = IS.intensity_scale_field(generator, od if scenario_chunk == 7 else obs, S, thr, L, latent=z, scenario_chunk=scenario_chunk,
                                       chunk=unit_tiles)
        assert np.array_equal(got.counts, want.counts) and np.array_equal(got.tiles, want.tiles), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    # the daily sum is NaN at (20, 30), so every hour of every scenario is: at L = 4 one void tile of 2 x 3 per pair
    a = P.intensity_scale_scenarios_field(obs, 3, thr, scenario_chunk=2, levels=4)
    np.random.seed(5)
    b = P.intensity_scale_scenarios_field(obs, 3, thr, scenario_chunk=3, levels=4)
    assert a.levels == 4 and a.counts.shape == (3, 24, 5, 3) and a.tiles.tolist() == [[15, 3]] * 24
    assert np.array_equal(a.counts[:, :, :, 1], b.counts[:, :, :, 1]) and np.array_equal(a.tiles, b.tiles)
    stand_in = np.zeros((3,) + obs.shape, np.float32)
    stand_in[:, :, 20, 30] = np.nan
    assert np.array_equal(a.counts[:, :, :, 1], yn.state_np(stand_in, obs, thr, 4)[0][:, :, :, 1])     # the observation's side
    c = P.intensity_scale_scenarios_field(obs, 1, thr)
    assert c.levels == 5 and c.counts.shape == (3, 24, 6, 3) and c.tiles.tolist() == [[0, 1]] * 24


def test_library_exports_and_device_pointer_checks():
    L = lib()
    assert hasattr(L, "rdgan_iss_workspace_bytes") and hasattr(L, "rdgan_iss_accumulate")
    ny, nx, lv = 16, 20, 4
    x = torch.zeros((2, 24, ny, nx), dtype=torch.float32, device="cuda")
    o = torch.zeros((24, ny, nx), dtype=torch.float32, device="cuda")
    counts = torch.full((2 * 24 * 5 * 3 + 1,), -7, dtype=torch.int64, device="cuda")
    tiles = torch.full((24 * 2 + 1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(4, dtype=torch.int64, device="cuda")
    thr = np.array([0.1, 1.0])
    p = lambda t, k=0: ctypes.c_void_p(t.data_ptr() + k)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def acc(m=p(x), s=2, stride=24 * ny * nx, obs=p(o), th=thr.ctypes.data_as(ctypes.c_void_p), T=2, lv=lv, c=p(counts), t=p(tiles), w=p(ws), nbytes=8):
        return L.rdgan_iss_accumulate(m, s, stride, obs, 1, ny, nx, th, T, lv, c, t, w, nbytes, st)

    for kw in (dict(m=p(x, 2)), dict(obs=p(o, 2)), dict(c=p(counts, 4)), dict(t=p(tiles, 4)), dict(w=p(ws, 4)), dict(s=0), dict(s=4097), dict(T=9),
               dict(lv=5), dict(lv=0), dict(nbytes=7), dict(stride=24 * ny * nx - 1)):
        assert acc(**kw) == -2, kw
    torch.cuda.synchronize()
    assert (counts == -7).all() and (tiles == -7).all()              # no output touched
    counts[:-1], tiles[:-1] = 0, 0
    assert acc() == 0
    torch.cuda.synchronize()
    assert (counts[:-1] == 0).all() and counts[-1] == -7 and tiles[:-1].view(24, 2).tolist() == [[2, 0]] * 24 and tiles[-1] == -7
