"""GPU: the cascade kernels (csrc/rdgan_cascade.hip.h) and pr_disagg_radar_gan_amd/cascade.py against the numpy restatement
tests/cascade_np.py.  Everything is defined in integers, so every comparison but the round trip's is an equality."""
import functools

import numpy as np
import pytest
import torch

from tests import cascade_np as cn

pytestmark = pytest.mark.gpu

EDGE_SETS = {1: (0.5,), 2: (0.1, 1.0), 7: (0.02, 0.05, 0.1, 0.25, 0.5, 1.0, 2.0)}
ISO, START, ENCL, END = range(4)


def _cs():
    from pr_disagg_radar_gan_amd import cascade
    return cascade


@functools.lru_cache(maxsize=None)
def rain(seed, n, ny, nx, floor=0.0):
    """(n, 24, ny, nx) rain-like hours, never written to: wet spells of one to three hours seeded at 13 % of the pixel-hours, about 70 %
    of the pixel-hours dry, gamma amounts (plus `floor` mm where wet)"""
    rng = np.random.default_rng(seed)
    start = rng.random((n, 24, ny, nx)) < 0.13
    wet = start.copy()
    wet[:, 1:] |= start[:, :-1] & (rng.random((n, 23, ny, nx)) < 0.7)
    wet[:, 2:] |= start[:, :-2] & (rng.random((n, 22, ny, nx)) < 0.4)
    x = ((rng.gamma(0.5, 2.0, (n, 24, ny, nx)) + floor) * wet).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def mirror_state(seed, n, ny, nx, n_edges):
    s = cn.accumulate(rain(seed, n, ny, nx), EDGE_SETS[n_edges])
    s.setflags(write=False)
    return s


def device_state(x, edges, **kw):
    return _cs().CascadeCalibrator(edges, **kw).add(x).state().cpu().numpy()


# 3 x 5: odd, the scalar load path, fewer pixels than a wave; 8 x 8: the 16-byte path; 70 x 70: 1225 groups of four pixels a day, several
# workgroups per day and per call, so the LDS flush is exercised across workgroups
@pytest.mark.parametrize("n_edges", [1, 2, 7])
@pytest.mark.parametrize("n,ny,nx", [(9, 3, 5), (12, 8, 8), (7, 70, 70)])
def test_state_matches_yardstick(n, ny, nx, n_edges):
    x, want = rain(n * 100 + ny, n, ny, nx), mirror_state(n * 100 + ny, n, ny, nx, n_edges)
    assert (x == 0).mean() > 0.6
    NV, off = n_edges + 1, cn.offsets(n_edges + 1)
    kinds = want[:off["weight"]].reshape(3, 4, NV, 3)
    assert np.all(kinds.sum(axis=(0, 2, 3)) > 0) and np.all(kinds.sum(axis=(0, 1, 2)) > 0)          # all four positions, all three types
    got = device_state(x, EDGE_SETS[n_edges])
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(device_state(torch.from_numpy(np.array(x)).cuda(), EDGE_SETS[n_edges]), want)


@pytest.mark.parametrize("n,ny,nx,pad", [(9, 3, 5, 3), (12, 8, 8, 4), (12, 8, 8, 1), (7, 70, 70, 8)])
def test_state_does_not_depend_on_the_grouping(n, ny, nx, pad):
    cs = _cs()
    x, want = rain(n * 100 + ny, n, ny, nx), mirror_state(n * 100 + ny, n, ny, nx, 2)
    one_by_one = cs.CascadeCalibrator()
    for d in range(n):
        one_by_one.add(x[d])
    assert np.array_equal(one_by_one.state().cpu().numpy(), want)
    split = cs.CascadeCalibrator().add(x[:2]).add(x[2:].reshape(n - 2, 1, 24, ny, nx))
    assert np.array_equal(split.state().cpu().numpy(), want)
    day = 24 * ny * nx
    wide = torch.full((n, day + pad), float("nan"), device="cuda")
    wide[:, :day] = torch.from_numpy(np.array(x)).cuda().reshape(n, day)
    view = wide[:, :day].view(n, 24, ny, nx)
    assert view.stride(0) == day + pad and not view.is_contiguous()
    assert np.array_equal(device_state(view, (0.1, 1.0)), want)
    off_by_one = torch.empty(n * day + 1, device="cuda")[1:]                              # a base that is not 16-byte aligned
    off_by_one.copy_(torch.from_numpy(np.array(x)).cuda().reshape(-1))
    assert np.array_equal(device_state(off_by_one.view(n, 24, ny, nx), (0.1, 1.0)), want)


def test_bad_and_dry_days():
    cs = _cs()
    x = np.array(rain(5, 10, 8, 8))
    x[0] = 0.0                                                                            # 64 dry pixel-days
    x[1, :, :2] = 0.0                                                                     # 16 more
    x[2, 3, 0, 0], x[2, 4, 0, 0] = np.nan, 1.0                                            # one pixel-day, two bad hours
    x[3, 0, 1, 1], x[4, 23, 7, 7], x[5, 12, 4, 3] = np.inf, -0.5, 2048.0
    x[6, 5, 2, 2] = np.float32(2047.999)                                                  # the largest admitted
    x[0, 7, 3, 3] = -np.inf                                                               # bad, not dry
    want = cn.accumulate(x)
    dry = int((np.where(np.isfinite(x), x, 1.0).sum(axis=1) == 0).sum())
    assert want[-3:].tolist() == [640, 5, dry] and dry >= 79
    got = device_state(x, (0.1, 1.0))
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):                                                       # the all-dry state is refused
        cs.calibrate(np.zeros((2, 24, 3, 5), np.float32))
    only_bad = np.zeros((1, 24, 2, 2), np.float32)
    only_bad[0, 0] = np.nan
    cal = cs.CascadeCalibrator().add(only_bad)
    assert cal.state().cpu().numpy()[-3:].tolist() == [4, 4, 0] and cal.state().sum().item() == 8
    with pytest.raises(ValueError):
        cal.result()
    assert cal.reset().add(np.array(rain(5, 10, 8, 8))).state().cpu().numpy()[-3].item() == 640


def test_model_thresholds_and_fallback():
    cs = _cs()
    x = np.array(rain(11, 12, 8, 8))
    x[:, 8:16] = 0.0                                                                      # the middle third dry: no enclosed 8 h box
    want = cn.accumulate(x)
    table, fallbacks = cn.build_model(want, 2)
    assert want[:36 * 3].reshape(3, 4, 3, 3)[0, ENCL].sum() == 0 and want[:36 * 3].reshape(3, 4, 3, 3)[1:, ENCL].sum() > 0
    assert all(fallbacks[("type", (0, ENCL, v))] == 1 and fallbacks[("weight", (0, ENCL, v))] == 1 for v in (1, 2))
    model = cs.calibrate(x)
    assert np.array_equal(model.state, want) and np.array_equal(model.table, table) and model.table.dtype == np.uint32
    assert (model.n_days, model.n_bad, model.n_dry) == tuple(want[-3:].tolist())
    p = model.probabilities()
    pooled = want[:36 * 3].reshape(3, 4, 3, 3)[0, :, 1].sum(axis=0)                       # the enclosed row of class 1: the positions pooled
    assert np.allclose(p["type"][0, ENCL, 1], pooled / pooled.sum(), atol=1e-7) and np.allclose(p["type"].sum(-1), 1, atol=1e-6)
    for n_edges, edges in EDGE_SETS.items():
        m = cs.calibrate(rain(1208, 12, 8, 8), edges)
        assert np.array_equal(m.table, cn.build_model(mirror_state(1208, 12, 8, 8, n_edges), n_edges)[0])


@functools.lru_cache(maxsize=None)
def models():
    """{edges: (CascadeModel, the mirror's table)} calibrated once on 12 days of 8 x 8, by the mirror"""
    cs = _cs()
    out = {}
    for edges in ((), (0.1, 1.0), EDGE_SETS[7]):
        state = cn.accumulate(rain(1208, 12, 8, 8), edges)
        out[edges] = (cs.CascadeModel(state, edges), cn.build_model(state, len(edges))[0])
    return out


@functools.lru_cache(maxsize=None)
def conditions(ny, nx):
    """(3, ny, nx) daily sums of rain-like days with the special values the definition names"""
    cond = np.array(rain(77 + ny, 3, ny, nx).sum(axis=1))
    flat = cond.reshape(3, -1)
    flat[0, :4] = 0.0, 1.0 / 1024, 2.0 / 1024, 3.0 / 1024                                   # V = 0, 1 (cannot split), 2, 3
    flat[1, :5] = np.nan, np.inf, -np.inf, -1.0, 16384.0                                  # masked, each kind
    flat[2, :3] = np.float32(16383.999), 1.4 / 1024, 1e-5                                 # V = 2^24 - 1; V = 1 after rounding; V = 0
    cond.setflags(write=False)
    return cond


@pytest.mark.parametrize("edges", [(), (0.1, 1.0), EDGE_SETS[7]])
@pytest.mark.parametrize("ny,nx", [(3, 5), (8, 8)])
def test_generation_matches_yardstick(ny, nx, edges):
    model, table = models()[edges]
    assert np.array_equal(model.table, table)
    cond = conditions(ny, nx)
    want, want_units = cn.generate(table, edges, cond, 2, seed=4)
    out, units = model.generate(cond, 2, seed=4, return_units=True)
    assert out.shape == units.shape == (3, 2, 24, ny, nx) and out.dtype == torch.float32 and units.dtype == torch.int32
    out, units = out.cpu().numpy(), units.cpu().numpy()
    assert np.array_equal(units, want_units) and np.array_equal(out, want, equal_nan=True)
    # the children of every node sum to its volume: the hours to V, whatever path the tree took
    V, masked = cn.quantise(cond, cn.MAX_COND)
    total = units.astype(np.int64).sum(axis=2)
    assert np.array_equal(np.where(masked[:, None], -24, V[:, None]) + 0 * total, total) and masked.sum() == 5
    assert np.isnan(out[np.broadcast_to(masked[:, None, None], out.shape)]).all() and np.isfinite(out[~np.broadcast_to(masked[:, None, None], out.shape)]).all()
    assert out[~np.isnan(out)].min() >= 0 and np.array_equal(out[~np.isnan(out)], units[units >= 0] * np.float32(2.0 ** -10))
    assert V.reshape(3, -1)[2, 0] == (1 << 24) - 1 and V.reshape(3, -1)[0, 1] == 1 and V.reshape(3, -1)[2, 1] == 1
    assert np.array_equal(model.generate(torch.from_numpy(np.array(cond)).cuda(), 2, seed=4).cpu().numpy(), want, equal_nan=True)


def test_a_pick_depends_on_seed_member_and_query_only():
    model, table = models()[(0.1, 1.0)]
    cond = conditions(8, 8)
    whole = model.generate(cond, 5, seed=9, return_units=True)[1].cpu().numpy()
    assert np.array_equal(whole, cn.generate(table, (0.1, 1.0), cond, 5, seed=9)[1])
    assert np.array_equal(whole[:, 2:], model.generate(cond, 3, seed=9, first_member=2, return_units=True)[1].cpu().numpy())
    assert np.array_equal(whole[1:], model.generate(cond[1:], 5, seed=9, first_query=1, return_units=True)[1].cpu().numpy())
    assert not np.array_equal(whole, model.generate(cond, 5, seed=10, return_units=True)[1].cpu().numpy())
    far = model.generate(cond[:1], 1, seed=2 ** 64 - 1, first_member=2 ** 62, first_query=2 ** 32 - 1, return_units=True)[1].cpu().numpy()
    assert np.array_equal(far, cn.generate(table, (0.1, 1.0), cond[:1], 1, seed=2 ** 64 - 1, first_member=2 ** 62, first_query=2 ** 32 - 1)[1])


@pytest.mark.parametrize("ny,nx", [(3, 5), (8, 8), (6, 12)])
@pytest.mark.parametrize("patch", [1, 2, 3, 16])
def test_patch_shares_the_draws_of_a_block(ny, nx, patch):
    model, table = models()[(0.1, 1.0)]
    cond = np.array(conditions(ny, nx))
    cond[0] = 7.25                                                                        # equal volumes: equal pixels within a block
    units = model.generate(cond, 2, seed=3, patch=patch, return_units=True)[1].cpu().numpy()
    assert np.array_equal(units, cn.generate(table, (0.1, 1.0), cond, 2, seed=3, patch=patch)[1])
    for y0 in range(0, ny, patch):
        for x0 in range(0, nx, patch):
            block = units[0, :, :, y0:y0 + patch, x0:x0 + patch]
            assert np.all(block == block[:, :, :1, :1])
    if patch >= max(ny, nx):
        assert np.all(units[0] == units[0, :, :, :1, :1])
    else:
        assert not np.all(units[0] == units[0, :, :, :1, :1])


def test_both_store_paths_agree():
    """nx a multiple of 4 into an output that is 16-byte aligned, and into views that are not: the 16-byte and the 4-byte stores"""
    model, table = models()[(0.1, 1.0)]
    cond = conditions(8, 8)
    want, want_units = cn.generate(table, (0.1, 1.0), cond, 2, seed=6)
    shape = (3, 2, 24, 8, 8)
    n = int(np.prod(shape))
    for shift in (0, 1, 2, 4):
        buf = torch.full((n + 4,), -7.0, device="cuda")
        out = buf[shift:shift + n].view(shape)
        assert out.data_ptr() % 16 == (4 * shift) % 16
        back = model.generate(cond, 2, seed=6, out=out)
        assert back.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want, equal_nan=True)
        assert np.all(buf[:shift].cpu().numpy() == -7.0) and np.all(buf[shift + n:].cpu().numpy() == -7.0)      # nothing beside the view
    odd = conditions(3, 5)                                                                # nx % 4 != 0
    assert np.array_equal(model.generate(odd, 2, seed=6).cpu().numpy(), cn.generate(table, (0.1, 1.0), odd, 2, seed=6)[0], equal_nan=True)


def test_round_trip_reproduces_the_type_frequencies():
    """The one statistical test, deterministic by the counter RNG: calibrate on data, generate 204 800 pixel-days from the data's own
    daily sums, calibrate on the output.  Every type frequency with at least 1 000 samples lies within 5 binomial standard deviations
    of the model's probability.  Seed and sizes were chosen so that tests/cascade_np.py alone passes this on the CPU (checked with
    round_trip_check below on the mirror's own output, which the device equals: 36 rows, the largest deviation 2.26 standard deviations)."""
    cs = _cs()
    x = rain(2024, 40, 16, 16, floor=0.05)
    model = cs.calibrate(x)
    assert np.array_equal(model.state, cn.accumulate(x))
    out = model.generate(np.array(x.sum(axis=1)), 20, seed=1)
    again = cs.calibrate(out.reshape(40 * 20, 24, 16, 16))
    assert again.n_days == 204800 and again.n_bad == 0
    rows, worst = round_trip_check(model.table, again.state, 2)
    assert rows >= 30 and worst <= 5.0, (rows, worst)


def round_trip_check(table, state, n_edges):
    """-> (rows with >= 1000 samples, the largest |f - p| / sqrt(p (1 - p) / n) over their types); a type of probability 0 or 1 must be
    met never or always"""
    NV = n_edges + 1
    p = cn.probabilities(table, n_edges)["type"].reshape(-1, 3)
    c = np.asarray(state[:36 * NV], dtype=np.float64).reshape(-1, 3)
    rows, worst = 0, 0.0
    for pr, cr in zip(p, c):
        n = cr.sum()
        if n < 1000:
            continue
        rows += 1
        for pk, ck in zip(pr, cr):
            sd = np.sqrt(pk * (1 - pk) / n)
            if sd == 0:
                worst = max(worst, 0.0 if ck / n == pk else np.inf)
            else:
                worst = max(worst, abs(ck / n - pk) / sd)
    return rows, worst


def test_wrappers_and_the_experiment():
    cs = _cs()
    from pr_disagg_radar_gan_amd import multivariate as mv
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    from pr_disagg_radar_gan_amd.ensemble import crps_ensemble_device
    model, table = models()[(0.1, 1.0)]
    rng = np.random.default_rng(21)
    reals = (rng.gamma(0.3, 2.0, (3, 24, 8, 8)) + 1e-3).astype(np.float32)
    rd = torch.from_numpy(reals).cuda()
    dsum = rd.sum(1)
    one = cs.generate_one_per_day(reals, model, seed=5, patch=2)
    assert one.shape == (3, 24, 8, 8) and torch.equal(one, model.generate(dsum, 1, seed=5, patch=2)[:, 0])
    assert np.array_equal(one.cpu().numpy(), cn.generate(table, (0.1, 1.0), dsum.cpu().numpy(), 1, seed=5, patch=2)[0][:, 0])
    assert torch.equal(cs.generate_one_per_day(rd, model, seed=5, patch=2), one)
    crps = cs.crps_for_days(reals, model, n_members=16, seed=5)
    ens = model.generate(dsum, 16, seed=5)
    by_hand = torch.stack([crps_ensemble_device(ens[i], rd[i]) for i in range(3)]).mean(dim=(2, 3)).cpu().numpy()
    assert crps.shape == (3, 24) and np.isfinite(crps).all() and np.array_equal(crps, by_hand)
    T.configure(ndomain=8)
    gen = T.create_generator(seed=2)
    clim = (rng.gamma(0.5, 4.0, (20, 24, 8, 8)) * (rng.random((20, 24, 8, 8)) < 0.4)).astype(np.float32)
    m, seed = 16, 5
    res = mv.multivariate_experiment(gen, reals, clim, n_members=m, seed=seed, cascade=model, cascade_patch=8)
    assert set(res.es) == set(res.vs) == {"gan", "random", "cascade"}
    for d in range(3):
        members = model.generate(rd[d:d + 1].sum(1), m, seed=seed, first_query=d, patch=8)[0]
        assert res.es["cascade"][d] == mv.energy_score(members, rd[d]).item() and res.vs["cascade"][d] == mv.variogram_score(members, rd[d]).item()
    assert all(np.isfinite(v).all() and v.shape == (3,) and v.dtype == np.float64 for t in (res.es, res.vs) for v in t.values())
    assert set(res.summary(N=100)["es"]) == {"gan", "random", "cascade", "gan-random", "gan-cascade"}
    without = mv.multivariate_experiment(gen, reals, clim, n_members=m, seed=seed)
    none = mv.multivariate_experiment(gen, reals, clim, n_members=m, seed=seed, cascade=None)
    assert set(without.es) == set(none.es) == {"gan", "random"}
    for t in ("es", "vs"):
        for k in ("gan", "random"):
            assert np.array_equal(getattr(without, t)[k], getattr(none, t)[k]) and np.array_equal(getattr(none, t)[k], getattr(res, t)[k])
