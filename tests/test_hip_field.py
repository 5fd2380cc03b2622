"""-m gpu: whole-field disaggregation (csrc/rdgan_field.hip.h, pr_disagg_radar_gan_amd/field.py) against the fp64 restatement
(tests/field_np.py): the blend kernel alone on random buffers, the scan and condition kernels bit for bit, the whole path around a
seeded generator, mass conservation, chunking, the drop-in of raindisagg_gan_pretrained and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, models
from pr_disagg_radar_gan_amd import field as F
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from pr_disagg_radar_gan_amd import weights as W
from tests import field_np as fn
from tests.hip_util import dev, ptr, stream

pytestmark = pytest.mark.gpu

# the blend against the fp64 restatement: at most 9 non-negative fp32 terms (product and sum rounded: covered by the terms' count)
# and 3 more roundings (wy, wx stored as fp32, their product): 12 * 2^-24 = 7e-7
BLEND_RTOL = 2e-6
# the whole path: what tests/test_hip_api.py::test_predict_batches_and_critic_predict grants the forward across batch splits
E2E_RTOL, E2E_ATOL_OF_MAX = 2e-5, 1e-8
MASS_RTOL = 1e-5                # tests/test_hip_api.py::test_generate_scenarios_example_case, one tile; the blend is a convex combination

BLEND_SHAPES = [(8, 11, 19, 3), (16, 20, 30, 4), (16, 32, 48, 0), (64, 70, 64, 8)]


def _blend_case(nd, ny, nx, overlap, seed):
    """two units over two days, random (not softmax) fractions, slots in scrambled order with a few -1; a dry and a NaN pixel"""
    rng = np.random.default_rng(seed)
    plan = fn.Plan(ny, nx, nd, overlap)
    T = plan.n_tiles
    m = 2 * T + 1
    frac = rng.random((m, 24, nd, nd), dtype=np.float32)
    slots = rng.permutation(m)[:2 * T].reshape(2, T).astype(np.int32)
    if overlap:
        slots[0, rng.integers(T)] = -1
        slots[1, rng.integers(T)] = -1
    daily = rng.gamma(0.6, 8.0, (2, ny, nx)).astype(np.float32) + np.float32(0.01)
    daily[0, 1, 2] = 0.0
    daily[1, ny - 1, nx - 2] = np.nan
    daily[1, ny // 2, :] = 0.0
    return plan, frac, slots, daily


@pytest.mark.parametrize("nd,ny,nx,overlap", BLEND_SHAPES)
def test_blend_kernel_against_restatement(nd, ny, nx, overlap):
    ref_plan, frac, slots, daily = _blend_case(nd, ny, nx, overlap, seed=nd + ny + nx)
    plan = F.tile_plan(ny, nx, nd, overlap)
    assert plan.n_tiles == ref_plan.n_tiles
    fd, dd = dev(frac), dev(daily)
    out = F.blend_device(fd, slots, plan, dd)
    again = F.blend_device(fd, slots, plan, dd)
    assert out.shape == (2, 24, ny, nx) and torch.equal(out.view(torch.int32), again.view(torch.int32))       # bit for bit
    out = out.cpu().numpy()
    ref = fn.blend(frac, slots, ref_plan, daily)
    assert np.array_equal(np.isnan(out), np.isnan(ref)) and np.isnan(ref).sum() == 24
    ok = ~np.isnan(ref)
    err = np.abs(out[ok] - ref[ok]) / np.where(ref[ok] == 0, 1.0, np.abs(ref[ok]))
    print(f"nd {nd} field {ny} x {nx} overlap {overlap}: {plan.n_tiles} tiles, worst relative error {err.max():.2e} (limit {BLEND_RTOL})")
    np.testing.assert_allclose(out, ref, rtol=BLEND_RTOL, atol=0, equal_nan=True)
    assert np.all(out[ref == 0] == 0)
    if overlap == 0 and ny % nd == 0 and nx % nd == 0:               # every pixel has one cover: one fp32 product, correctly rounded
        assert np.array_equal(out, ref.astype(np.float32), equal_nan=True)
    # units of the second day first: unit u is day (first_unit + u) % n_days
    out1 = F.blend_device(fd, slots, plan, dd, first_unit=1).cpu().numpy()
    np.testing.assert_allclose(out1, fn.blend(frac, slots, ref_plan, daily, first_unit=1), rtol=BLEND_RTOL, atol=0, equal_nan=True)


@pytest.mark.parametrize("nd,ny,nx,overlap", [(8, 11, 19, 3), (16, 20, 30, 4)])
def test_blend_one_hot_probes(nd, ny, nx, overlap):
    """A single tile's single pixel set in the buffer: the output is non-zero exactly at the mapped (h, y, x) of the units that
    reference the slot -- pins oy / ox, the tile order and the slot indexing."""
    plan = F.tile_plan(ny, nx, nd, overlap)
    T, origins = plan.n_tiles, plan.origins()
    rng = np.random.default_rng(7)
    daily = dev(np.ones((1, ny, nx), np.float32))
    for t in range(T):
        h, i, j = int(rng.integers(24)), int(rng.integers(nd)), int(rng.integers(nd))
        frac = np.zeros((3, 24, nd, nd), np.float32)
        frac[1, h, i, j] = 1.0
        t2 = (t + 1) % T
        slots = np.stack([np.zeros(T, np.int32), np.full(T, 2, np.int32), np.zeros(T, np.int32)])
        slots[0, t] = 1                                  # unit 0 holds the probe at tile t, unit 1 at tile t2, unit 2 nowhere
        slots[1, t2] = 1
        out = F.blend_device(dev(frac), slots, plan, daily).cpu().numpy()
        want = np.zeros(out.shape, bool)
        want[0, h, origins[t, 0] + i, origins[t, 1] + j] = True
        want[1, h, origins[t2, 0] + i, origins[t2, 1] + j] = True
        assert np.array_equal(out != 0, want), (t, h, i, j)


def test_blend_offsets_past_2_31():
    """fraction buffer and output of more than 2^31 elements each (a few days of a 1000-member ensemble are that large): overlap 0,
    so every output value is ONE product and can be checked exactly, the whole array on the device."""
    nd, ny, nx, units = 16, 32, 32, 90000
    plan = F.tile_plan(ny, nx, nd, 0)
    m = units * 4
    assert m * 24 * nd * nd > 2 ** 31 and units * 24 * ny * nx > 2 ** 31
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    frac = torch.rand((m, 24, nd, nd), generator=g, device="cuda")
    daily = torch.rand((3, ny, nx), generator=g, device="cuda") + 0.5
    slots = (np.arange(units - 1, -1, -1, dtype=np.int64)[:, None] * 4 + np.array([2, 0, 3, 1])[None, :]).astype(np.int32)
    out = F.blend_device(frac, slots, plan, daily)
    order = torch.tensor([2, 0, 3, 1], device="cuda")                # the slot of tile t is 4 (units - 1 - u) + (2, 0, 3, 1)[t]
    rows = frac.view(units, 4, 24, nd, nd)
    for u0 in range(0, units, 15000):
        u1 = min(units, u0 + 15000)
        src = rows[units - u1:units - u0].flip(0)[:, order]          # [u - u0, tile] = the tile's row of frac
        tiles = src.view(u1 - u0, 2, 2, 24, nd, nd).permute(0, 3, 1, 4, 2, 5).reshape(u1 - u0, 24, ny, nx)
        days = daily[torch.arange(u0, u1, device="cuda") % 3][:, None]
        assert torch.equal(out[u0:u1], days * tiles), (u0, u1)


@pytest.fixture(scope="module")
def field_case():
    rng = np.random.default_rng(11)
    daily = fn.example_field(rng)
    return daily, fn.Plan(20, 30, 16, 4), F.tile_plan(20, 30, 16, 4)


def test_scan_and_condition_kernels_bit_for_bit(field_case):
    daily, ref_plan, plan = field_case
    dd = dev(daily)
    counts = F.scan_device(dd, plan).cpu().numpy()
    want = fn.scan(daily, ref_plan)
    assert counts.dtype == np.int32 and np.array_equal(counts, want)
    assert want[..., 1].sum() > 0 and 0 < (want[..., 0] > 0).sum() < want[..., 0].size          # NaNs met, some tiles dry, some not
    entries = np.flatnonzero(counts[..., 0].reshape(-1) > 0).astype(np.int32)
    assert np.array_equal(entries, fn.active_entries(daily, ref_plan))
    cond = F.cond_device(dd, plan, entries, W.NORM_SCALE).cpu().numpy()
    ref = fn.cond_batch(daily, ref_plan, entries, W.NORM_SCALE)
    assert cond.shape == ref.shape == (len(entries), 16, 16, 1) and np.array_equal(cond.view(np.int32), ref.view(np.int32))
    scrambled = entries[::-1].copy()                     # any list of entries, in any order, repeats allowed
    scrambled[0] = scrambled[-1]
    cond = F.cond_device(dd, plan, scrambled, 3.5).cpu().numpy()
    assert np.array_equal(cond.view(np.int32), fn.cond_batch(daily, ref_plan, scrambled, 3.5).view(np.int32))


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


@pytest.mark.parametrize("bad", [-0.5, np.inf, -np.inf])
def test_negative_or_infinite_daily_value_is_refused(generator, field_case, bad):
    daily = field_case[0].copy()
    daily[1, 19, 29] = bad
    with pytest.raises(ValueError):
        F.disaggregate(generator, daily, 1)


def test_all_dry_field(generator):
    daily = np.zeros((2, 20, 30), np.float32)
    daily[1, 3, 4] = np.nan
    out, info = F.disaggregate(generator, daily, 2)
    out = out.cpu().numpy()
    assert (info.n_tiles, info.n_active, info.n_nan_pixels) == (6, 0, 1) and out.shape == (2, 2, 24, 20, 30)
    assert np.array_equal(np.isnan(out), np.broadcast_to(np.isnan(daily)[None, :, None], out.shape)) and np.nansum(np.abs(out)) == 0


@pytest.fixture(scope="module")
def end_to_end(generator, field_case):
    """mode -> (latent, product output with the default chunk, restatement's output, restatement's n_active, info); S = 3, D = 2"""
    daily, ref_plan, plan = field_case
    rng = np.random.default_rng(31)
    res = {}
    for mode, zshape in (("shared", (3, 2, 100)), ("independent", (3, 2, plan.n_tiles, 100))):
        z = rng.normal(size=zshape).astype(np.float32)
        out, info = F.disaggregate(generator, daily, 3, overlap=4, latent_mode=mode, latent=z)
        ref, n_active = fn.disaggregate(generator.predict, daily, z, ref_plan, W.NORM_SCALE, mode)
        res[mode] = (z, out.cpu().numpy(), ref, n_active, info)
    return res


def _assert_close(got, want, what):
    atol = E2E_ATOL_OF_MAX * np.nanmax(np.abs(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) - atol
    rel = (err / np.where(want[ok] == 0, 1.0, np.abs(want[ok]))).max()
    print(f"{what}: worst error beyond atol, relative: {rel:.2e} (limit {E2E_RTOL})")
    np.testing.assert_allclose(got, want, rtol=E2E_RTOL, atol=atol, equal_nan=True)


@pytest.mark.parametrize("mode", ["shared", "independent"])
def test_end_to_end_against_restatement(end_to_end, field_case, mode):
    daily = field_case[0]
    z, out, ref, n_active, info = end_to_end[mode]
    assert out.shape == ref.shape == (3, 2, 24, 20, 30) and out.dtype == np.float32
    nan = np.broadcast_to(np.isnan(daily)[None, :, None], out.shape)
    dry = np.broadcast_to((daily == 0)[None, :, None], out.shape)
    assert np.array_equal(np.isnan(out), nan)            # NaN exactly at the NaN pixels
    assert np.all(out[dry] == 0) and np.all(out[~dry & ~nan] > 0)                  # zeros exactly at the dry ones
    assert (info.n_tiles, info.n_active, info.n_nan_pixels) == (6, n_active, int(np.isnan(daily).sum()))
    _assert_close(out, ref, f"end to end, {mode}")


@pytest.mark.parametrize("mode", ["shared", "independent"])
def test_mass_conservation(end_to_end, field_case, mode):
    daily = field_case[0]
    out = end_to_end[mode][1]
    total = np.nansum(out.astype(np.float64), axis=2)
    want = np.broadcast_to(np.where(np.isnan(daily), 0.0, daily.astype(np.float64))[None], total.shape)
    err = np.abs(total - want)[want > 0] / want[want > 0]
    print(f"mass, {mode}: worst relative error {err.max():.2e} (limit {MASS_RTOL})")
    np.testing.assert_allclose(total, want, rtol=MASS_RTOL, atol=0)


def test_chunking(generator, end_to_end, field_case):
    daily, _, plan = field_case
    z, whole = end_to_end["shared"][:2]
    counts = fn.scan(daily, field_case[1])
    unit_tiles = int((counts[..., 0] > 0).sum(1).max())
    for chunk in (unit_tiles, 2 * unit_tiles + 1, 1):    # one unit per group; groups of several units; a chunk below one unit's tiles
        out, info = F.disaggregate(generator, daily, 3, latent=z, chunk=chunk)
        _assert_close(out.cpu().numpy(), whole, f"chunk {chunk} against the default")
    mine = torch.empty((3, 2, 24, 20, 30), device="cuda")
    out, _ = F.disaggregate(generator, dev(daily), 3, latent=z, out=mine)          # a CUDA plane in, a caller's tensor out
    assert out is mine
    _assert_close(mine.cpu().numpy(), whole, "a CUDA plane in, a caller's tensor out")


def test_device_dataset_plane(generator):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    rng = np.random.default_rng(5)
    data = rng.gamma(0.3, 2.0, (2, 24, 20, 30)).astype(np.float32)
    ds = DeviceDataset(data, ndomain=16)
    z = rng.normal(size=(1, 2, 100)).astype(np.float32)
    a, _ = F.disaggregate(generator, ds, 1, latent=z)
    b, _ = F.disaggregate(generator, ds.daily_plane(), 1, latent=z)
    assert ds.daily_plane() is ds.daily and a.shape == (1, 2, 24, 20, 30)
    _assert_close(a.cpu().numpy(), b.cpu().numpy(), "the data set against its plane")
    np.testing.assert_allclose(a.sum(2).cpu().numpy()[0], ds.daily.cpu().numpy(), rtol=MASS_RTOL)


def test_drop_in_equals_generate_scenarios(generator, monkeypatch):
    monkeypatch.setattr(P, "gen", generator)
    cond = (np.random.default_rng(9).gamma(0.6, 8.0, (16, 16, 1)) + 0.01)
    for n in (4, 1):
        np.random.seed(5)
        want = P.generate_scenarios(cond, n)
        np.random.seed(5)
        got = P.generate_scenarios_field(cond[..., 0], n, overlap=0)
        assert got.dtype == np.float64 and got.shape == want.shape == ((n, 24, 16, 16) if n > 1 else (24, 16, 16))     # the squeeze
        _assert_close(got, want, f"generate_scenarios_field against generate_scenarios, n = {n}")
    np.random.seed(5)
    _assert_close(P.generate_scenarios_field(cond, 1, overlap=0), got, "cond's own (nd, nd, 1) layout")


def test_cabi_bad_arguments_return_minus_2():
    lib = _lib.load()
    nd, ny, nx, ov, D = 16, 20, 30, 4, 2
    plan = F.tile_plan(ny, nx, nd, ov)
    T = plan.n_tiles
    daily = dev(np.ones((D, ny, nx), np.float32))
    counts = torch.full((D, T, 3), -7, dtype=torch.int32, device="cuda")
    cond = torch.full((2, nd, nd, 1), -7.0, device="cuda")
    frac = dev(np.ones((2, 24, nd, nd), np.float32))
    out = torch.full((1, 24, ny, nx), -7.0, device="cuda")
    yi, yw, xi, xw = plan.device_tables(daily.device)
    entries = np.array([0, D * T - 1], np.int32)
    slots = np.array([[0, 1, -1, 0, 1, -1]], np.int32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)

    def scan(daily=ptr(daily), n_days=D, ny=ny, nx=nx, nd=nd, ov=ov, counts=ptr(counts)):
        return lib.rdgan_field_scan(daily, n_days, ny, nx, nd, ov, counts, stream())

    def cnd(daily=ptr(daily), n_days=D, ny=ny, nx=nx, nd=nd, ov=ov, entries=hp(entries), m=2, scale=127.4, cond=ptr(cond)):
        return lib.rdgan_field_cond(daily, n_days, ny, nx, nd, ov, entries, m, scale, cond, stream())

    def blend(frac=ptr(frac), m=2, slots=hp(slots), units=1, first=0, yi=ptr(yi), yw=ptr(yw), xi=ptr(xi), xw=ptr(xw), daily=ptr(daily),
              n_days=D, ny=ny, nx=nx, nd=nd, ov=ov, out=ptr(out)):
        return lib.rdgan_field_blend(frac, m, slots, units, first, yi, yw, xi, xw, daily, n_days, ny, nx, nd, ov, out, stream())

    geometry = [dict(nd=12), dict(nd=128), dict(nd=0), dict(ov=-1), dict(ov=nd // 2 + 1), dict(ny=nd - 1), dict(nx=nd - 1), dict(n_days=0)]
    for fn_, extra in ((scan, [dict(daily=null), dict(counts=null)]),
                       (cnd, [dict(daily=null), dict(entries=null), dict(cond=null), dict(m=0), dict(scale=0.0),
                              dict(entries=hp(np.array([0, D * T], np.int32))), dict(entries=hp(np.array([-1, 0], np.int32)))]),
                       (blend, [dict(frac=null), dict(slots=null), dict(yi=null), dict(yw=null), dict(xi=null), dict(xw=null),
                                dict(daily=null), dict(out=null), dict(m=0), dict(units=0), dict(first=-1),
                                dict(slots=hp(np.array([[0, 1, -1, 0, 2, -1]], np.int32))),            # a slot >= m
                                dict(slots=hp(np.array([[0, 1, -2, 0, 1, -1]], np.int32)))])):
        for kw in geometry + extra:
            assert fn_(**kw) == -2, (fn_.__name__, kw)
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((cond == -7).all()) and bool((out == -7).all())         # nothing was launched
    assert scan() == 0 and cnd() == 0 and blend() == 0
    torch.cuda.synchronize()
    assert bool((counts[..., 0] == nd * nd).all()) and bool((cond == float(np.float32(1.0 / 127.4))).all()) and not bool((out == -7).any())
