"""-m gpu: the distance maps and the pair records of the distance-map verification (csrc/rdgan_distmap.hip.h,
pr_disagg_radar_gan_amd/distmap.py) against the numpy restatement (tests/distmap_np.py, itself checked on the CPU by
tests/test_distmap_host.py).  Every comparison is an equality of integer arrays."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import distmap as DM, field as F, models, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import distmap_np as yn
from tests.hip_util import dev, lib

pytestmark = pytest.mark.gpu

THR8 = (0.0, 0.1, 0.3, 0.5, 1.0, 2.0, 5.0, 10.0)
THR2 = (0.1, 1.0)
# name: (ny, nx, thresholds); the first seven also carry the records tests
CASES = {
    "8x8": (8, 8, THR2),
    "16x16": (16, 16, THR2),                                         # the collage: four planes side by side in a strip
    "24x40": (24, 40, THR2),
    "64x64-T1": (64, 64, (0.5,)),
    "64x64-T8": (64, 64, THR8),
    "65x67": (65, 67, THR2),                                         # a word boundary and a strip boundary one pixel in
    "70x130": (70, 130, THR2),
    "1x200": (1, 200, THR2),
    "200x1": (200, 1, THR2),                                         # 64 planes side by side, one lane each
    "256x256": (256, 256, (1.0,)),
    "1100x40": (1100, 40, (1.0,)),                                   # the 32-column strips of ny > 1024
}
RECORD_CASES = list(CASES)[:7]


def spells(rng, shape, thr, wet_hours=0.6):
    """rain-like spells: some hours dry, wet pixels in areas of 0 .. 12 mm/h, some values exactly at a threshold, negative
    values, and NaN, +inf and -inf pixels"""
    f = rng.random(shape)
    f = sum(np.roll(np.roll(f, dy, -2), dx, -1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9
    a = np.where(f > 0.56, 12.0 * rng.random(shape), 0.0)
    a = a * (rng.random(shape[:-2] + (1, 1)) < wet_hours)
    a = np.where(rng.random(shape) < 0.03, rng.choice(np.asarray(thr), shape), a)               # at a threshold: not in the set
    a = np.where(rng.random(shape) < 0.02, -1.0, a).astype(np.float32)
    flat = a.reshape(-1, shape[-2], shape[-1])
    for k, bad in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        flat[k % flat.shape[0], int(rng.integers(shape[-2])), int(rng.integers(shape[-1]))] = bad
    return a


@functools.lru_cache(maxsize=None)
def hourly(name):
    ny, nx, thr = CASES[name]
    return spells(np.random.default_rng(ny * 1000 + nx), (24, ny, nx), thr)


@functools.lru_cache(maxsize=None)
def maps_reference(name):
    return yn.maps_np(hourly(name), CASES[name][2])


@functools.lru_cache(maxsize=None)
def pairs(name):
    """(members (3, 2, 24, ny, nx), obs (2, 24, ny, nx)): hour 0 has an empty A for member 0, hour 1 an empty B, hour 2 both"""
    ny, nx, thr = CASES[name]
    rng = np.random.default_rng(ny * 1000 + nx + 7)
    obs, ens = spells(rng, (2, 24, ny, nx), thr), spells(rng, (3, 2, 24, ny, nx), thr)
    ens[0, :, 0], obs[:, 1], ens[:, :, 2], obs[:, 2] = 0.0, 0.0, 0.0, 0.0
    obs[:, 0, 0, 0], ens[1, :, 1, ny - 1, 0] = 11.0, 11.0                                       # the other side of hours 0 and 1 is not empty
    ens[1, 0, 3, 0, 0], obs[1, 4, ny - 1, nx - 1] = np.nan, np.inf                              # bad on one side only: flag bit 0
    ens[2, 1, 5, ny // 2, nx // 2], obs[1, 5, ny // 2, nx // 2] = np.nan, np.nan                # bad on both
    return ens, obs


@functools.lru_cache(maxsize=None)
def records_reference(name):
    ens, obs = pairs(name)
    return yn.records_np(ens, obs, CASES[name][2])


def maps_of(x, thr, **kw):
    maps, sizes = DM.distance_maps(x, thr, **kw)
    return maps.cpu().numpy(), sizes.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_maps_against_restatement(name):
    ny, nx, thr = CASES[name]
    want_maps, want_sizes = maps_reference(name)
    assert (want_sizes == 0).any() and (want_sizes > 0).any()         # empty and non-empty sets both occur
    got_maps, got_sizes = maps_of(dev(hourly(name)), thr)
    assert got_maps.dtype == np.uint16 and got_maps.shape == (24, len(thr), ny, nx) and got_sizes.shape == (24, len(thr))
    assert np.array_equal(got_sizes, want_sizes), name
    assert np.array_equal(got_maps, want_maps), name


def adversarial():
    ny, nx = 65, 67
    z = np.zeros((ny, nx), np.float32)
    planes = []
    for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (30, nx - 1)):       # the corners; the last column of the second word
        p = z.copy()
        p[y, x] = 1.0
        planes.append(p)
    yy, xx = np.indices((ny, nx))
    row = z.copy()
    row[40] = 1.0
    planes += [z, z + 1.0, ((yy + xx) % 2).astype(np.float32), row]
    planes += [z] * (24 - len(planes))
    return np.stack(planes)


def test_adversarial_masks():
    x = adversarial()
    want_maps, want_sizes = yn.maps_np(x, (0.5,))
    assert want_sizes[:9, 0].tolist() == [1, 1, 1, 1, 1, 0, 65 * 67, 65 * 67 // 2, 67]
    got_maps, got_sizes = maps_of(x, (0.5,))                          # numpy in
    assert np.array_equal(got_sizes, want_sizes) and np.array_equal(got_maps, want_maps)
    assert (got_maps[5] == 0xFFFF).all() and (got_maps[6] == 0).all() and got_maps[7].max() == 16 and got_maps[8, 0, 0, 5] == 16 * 40


def test_leading_shapes_strides_and_pass_size():
    name = "24x40"
    ny, nx, thr = CASES[name]
    _, obs = pairs(name)                                              # (2, 24, ny, nx)
    want = yn.maps_np(obs, thr)
    whole = maps_of(dev(obs), thr)
    assert whole[0].shape == (2, 24, 2, ny, nx) and np.array_equal(whole[0], want[0]) and np.array_equal(whole[1], want[1])
    for ppp in (1, 5, 48):
        got = maps_of(dev(obs), thr, planes_per_pass=ppp)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]), ppp
    Pn = 24 * ny * nx
    wide = torch.full((2, Pn + 20), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :Pn].view(2, 24, ny, nx)
    view.copy_(dev(obs))
    got = maps_of(view, thr)
    assert view.stride(0) == Pn + 20 and np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


def records_of(ens, obs, thr, **kw):
    return DM.DistanceMapVerifier(obs, thr, **kw).add(ens).records().records


@pytest.mark.parametrize("name", RECORD_CASES)
def test_records_against_restatement(name):
    ny, nx, thr = CASES[name]
    ens, obs = pairs(name)
    want = records_reference(name)
    assert want.shape == (3, 2, 24, len(thr), 12)
    f = want[..., 11]
    assert (f & 1).any() and ((f & 6) == 2).any() and ((f & 6) == 4).any() and ((f & 6) == 6).any() and ((f & 6) == 0).any()
    ver = DM.DistanceMapVerifier(dev(obs), thr).add(dev(ens))
    assert ver.cutoff16 == yn.default_cutoff16(ny, nx)
    got = ver.records()
    assert got.records.dtype == np.int64 and got.cutoff16 == ver.cutoff16 and (got.ny, got.nx) == (ny, nx)
    bad = np.argwhere(got.records != want)
    assert bad.size == 0, (name, bad[:5], got.records[tuple(bad[0][:-1])] if bad.size else None, want[tuple(bad[0][:-1])] if bad.size else None)
    m = DM.measures_from_records(got)
    assert np.isnan(m.hausdorff[0, :, 0]).all() and np.isfinite(m.baddeley(2)).all() and np.isfinite(m.hausdorff[:, :, 6:]).any()


def test_cutoff_below_at_and_above_the_largest_distance():
    name = "24x40"
    ny, nx, thr = CASES[name]
    ens, obs = pairs(name)
    full = records_reference(name)
    largest = int(max(full[..., 6].max(), full[..., 7].max()))        # the largest directed distance present, in 1/16 pixel
    assert 32 <= largest < yn.default_cutoff16(ny, nx)
    od, ed = dev(obs), dev(ens)
    for C in (largest - 16, largest, largest + 16):
        got = records_of(ed, od, thr, cutoff_px=C / 16)
        assert np.array_equal(got, yn.records_np(ens, obs, thr, C)), C
        assert np.array_equal(got[..., :8], full[..., :8]) and np.array_equal(got[..., 11], full[..., 11])       # only Delta sees the cutoff


@pytest.mark.parametrize("name", ["16x16", "70x130"])
def test_grouping_does_not_change_the_records(name):
    ny, nx, thr = CASES[name]
    ens, obs = pairs(name)
    want = records_reference(name)
    od, ed = dev(obs), dev(ens)
    whole = records_of(ed, od, thr)
    assert np.array_equal(whole, want)
    assert np.array_equal(DM.DistanceMapVerifier(od, thr).add(ed[:1]).add(ed[1:]).records().records, whole)     # 1 + 2 against 3
    assert np.array_equal(records_of(ed, od, thr, planes_per_pass=1), whole)
    assert np.array_equal(records_of(ed, od, thr, planes_per_pass=7), whole)
    Pn = 2 * 24 * ny * nx
    wide = torch.full((3, Pn + 52), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :Pn].view(3, 2, 24, ny, nx)
    view.copy_(ed)
    assert view.stride(0) == Pn + 52 and np.array_equal(records_of(view, od, thr), whole)                        # a strided member view
    assert np.array_equal(records_of(ens, obs, thr), whole)                                                      # numpy in
    m = DM.distmap_hourly(ed, od, thr)
    assert np.array_equal(m.records.records, whole) and m.hausdorff.shape == (3, 2, 24, len(thr))
    by_hand = DM.measures_from_records(DM.DistanceMapVerifier(obs, thr).add(ens).records())
    for k in ("hausdorff", "med_model_to_obs", "med_obs_to_model", "zhu", "csi", "baddeley_1", "baddeley_2", "baddeley_inf"):
        assert np.array_equal(getattr(m, k), getattr(by_hand, k), equal_nan=True), k
    one = DM.DistanceMapVerifier(od[1], thr).add(ed[:, 1]).records().records                                      # (24, ny, nx): one day
    assert one.shape == (3, 1, 24, len(thr), 12) and np.array_equal(one[:, 0], whole[:, 1])
    with pytest.raises(ValueError):
        DM.DistanceMapVerifier(od, thr).add(ed[:, :, :-1])


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_the_held_ensemble(generator, monkeypatch):
    """one 48 x 48 day at ndomain 16, overlap 4, a dry tile and a NaN pixel in the observation; `chunk` is one unit's wet tiles on
    both sides, the batch condition _hourly.evaluate_field states, so that the hourly values the two sides see are the same"""
    S, thr = 6, (0.01, 0.05, 0.2)
    rng = np.random.default_rng(31)
    obs = (rng.gamma(0.8, 0.6, (24, 48, 48)) * (rng.random((24, 48, 48)) < 0.5)).astype(np.float32)
    obs[:, :16, :16] = 0.0
    obs[3, 20, 30] = np.nan
    od = dev(obs)
    daily = od.sum(dim=0)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, daily, 1, latent=z[:1])[1].n_active
    held, info = F.disaggregate(generator, daily, S, latent=z, chunk=unit_tiles)
    want = DM.distmap_hourly(held, od, thr)
    assert np.array_equal(want.records.records, yn.records_np(held.cpu().numpy(), obs, thr))
    assert want.records.records.shape == (S, 1, 24, 3, 12) and (want.records.records[..., 1] > 0).any()
    for scenario_chunk in (1, 4, S):
        got = DM.distmap_field(generator, od if scenario_chunk == 4 else obs, S, thr, latent=z, scenario_chunk=scenario_chunk, chunk=unit_tiles)
        assert np.array_equal(got.records.records, want.records.records), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.distance_scenarios_field(obs, 3, thr, scenario_chunk=2, cutoff_px=8)
    np.random.seed(5)
    b = P.distance_scenarios_field(obs, 3, thr, scenario_chunk=3, cutoff_px=8)
    assert a.records.records.shape == (3, 1, 24, 3, 12) and a.records.cutoff16 == 128
    assert np.array_equal(a.records.records[..., 2], b.records.records[..., 2])                                 # the observation's side
    # the daily sum is NaN at (20, 30), so every hour of every scenario is; the observation only in hour 3
    assert (a.flags[:, :, 3] & 1 == 0).all() and (a.flags[:, :, 4] & 1 == 1).all()
    assert set(DM.MEASURES) <= set(a.summary())


def test_refusals_before_any_launch_and_device_pointer_checks():
    with pytest.raises(ValueError, match="max_map_bytes"):
        DM.DistanceMapVerifier(torch.zeros((24, 64, 64), dtype=torch.float32, device="cuda"), THR2, max_map_bytes=2 * 2 * 24 * 64 * 64 - 1)
    with pytest.raises(ValueError, match="2048"):
        DM.distance_maps(torch.zeros((24, 1, 2049), dtype=torch.float32, device="cuda"), THR2)
    L = lib()
    ny, nx, T = 16, 20, 2
    x = torch.zeros((2, 24, ny, nx), dtype=torch.float32, device="cuda")
    o = torch.zeros((24, ny, nx), dtype=torch.float32, device="cuda")
    maps = torch.full((24 * T * ny * nx + 1,), 7, dtype=torch.int16, device="cuda")
    sizes = torch.full((24 * T + 1,), -7, dtype=torch.int64, device="cuda")
    rec = torch.full((2 * 24 * T * 12 + 1,), -7, dtype=torch.int64, device="cuda")
    one = L.rdgan_dm_workspace_bytes(ny, nx, 1)
    ws = torch.zeros(one // 8 * 4, dtype=torch.int64, device="cuda")
    thr = np.array([0.1, 1.0])
    p = lambda t, k=0: ctypes.c_void_p(t.data_ptr() + k)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    th = thr.ctypes.data_as(ctypes.c_void_p)

    def call_maps(src=p(o), out=p(maps), sz=p(sizes), w=p(ws), nbytes=4 * one, nyy=ny):
        return L.rdgan_dm_maps(src, 1, 24 * ny * nx, nyy, nx, th, T, out, sz, w, nbytes, st)

    def call_rec(m=p(x), s=2, stride=24 * ny * nx, C=100, out=p(rec), w=p(ws), nbytes=4 * one, om=p(maps)):
        return L.rdgan_dm_records(m, s, stride, p(o), om, 1, ny, nx, th, T, C, out, w, nbytes, st)

    for kw in (dict(src=p(o, 2)), dict(out=p(maps, 1)), dict(sz=p(sizes, 4)), dict(w=p(ws, 4)), dict(nbytes=one - 1), dict(nyy=2049)):
        assert call_maps(**kw) == -2, kw
    for kw in (dict(m=p(x, 2)), dict(s=0), dict(s=4097), dict(stride=24 * ny * nx - 1), dict(C=15), dict(C=65535), dict(out=p(rec, 4)), dict(w=p(ws, 4)),
               dict(nbytes=one - 1), dict(om=p(maps, 1))):
        assert call_rec(**kw) == -2, kw
    torch.cuda.synchronize()
    assert (maps == 7).all() and (sizes == -7).all() and (rec == -7).all()                # no output touched
    assert call_maps() == 0 and call_rec() == 0
    torch.cuda.synchronize()
    assert (maps[:-1] == -1).all() and maps[-1] == 7 and (sizes[:-1] == 0).all() and sizes[-1] == -7           # empty sets: 0xFFFF everywhere
    r = rec[:-1].view(2, 24, T, 12)
    assert rec[-1] == -7 and (r[..., 0] == ny * nx).all() and (r[..., 1:11] == 0).all() and (r[..., 11] == 6).all()
