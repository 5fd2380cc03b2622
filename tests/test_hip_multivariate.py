"""-m gpu: the joint-field scores (csrc/rdgan_mvscore.hip.h, pr_disagg_radar_gan_amd/multivariate.py) against the numpy yardstick
(tests/mvscore_np.py): the energy score's two sums to a relative 1e-10, the variogram score's counts exactly and its sums of squares
to 1e-6 of the sum of o^2 + mean^2; the exact zero of equal members; ES of one position against the CRPS kernel; the bit-for-bit
promises (repeat, days split over calls, workspace size, shared against per-day form); the experiment against the scores called by
hand."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mvscore_np as mn

pytestmark = pytest.mark.gpu

ES_RTOL = 1e-10       # summation order only: d eps64 <= 1.1e5 * 1.1e-16 on a squared distance, half of that after the root; all terms >= 0
VS_RTOL = 1e-6        # one fp32 ulp (6e-8) on each v_k and on o, carried through 2 (|o| + mean) delta, against the sum of o^2 + mean^2


def _mv():
    from pr_disagg_radar_gan_amd import multivariate
    return multivariate


def rain(rng, shape, dry=0.6):
    """gamma-distributed amounts with about 60 % zeros, as small_case of tests/test_analog_host.py builds them"""
    return (rng.gamma(0.5, 4.0, shape) * (rng.random(shape) < 1.0 - dry)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(D, m, ny, nx):
    """(ens (D, m, 24, ny, nx), obs (D, 24, ny, nx)), shared by the tests and never written to: a few NaN observations in every day, and with D = 3 the last day fully masked"""
    rng = np.random.default_rng(100000 * D + 1000 * m + 10 * ny + nx)
    ens, obs = rain(rng, (D, m, 24, ny, nx)), rain(rng, (D, 24, ny, nx))
    for d in range(D):
        for _ in range(3):
            obs[d, rng.integers(24), rng.integers(ny), rng.integers(nx)] = np.nan
    if D == 3:
        obs[2] = np.nan
        obs[1] = rain(rng, (24, ny, nx))                                                   # and one day without a NaN
    return ens, obs


@functools.lru_cache(maxsize=None)
def energy_reference(D, m, ny, nx, shared):
    ens, obs = case(D, m, ny, nx)
    return np.array([mn.energy_terms(ens[0 if shared else d], obs[d]) for d in range(D)])


def raw_energy(ens, obs, shared, extra_words=0, fill=0):
    """the C entry with a workspace of the minimum size plus extra_words, filled with `fill`"""
    from pr_disagg_radar_gan_amd import _lib
    lib = _lib.load()
    D, (m, _, ny, nx) = obs.shape[0], ens.shape[-4:]
    nbytes = lib.rdgan_mv_energy_workspace_bytes(m, D, int(shared))
    assert nbytes > 0
    ws = torch.full((nbytes // 8 + extra_words,), fill, dtype=torch.int64, device="cuda")
    so, sp = torch.empty(D, dtype=torch.float64, device="cuda"), torch.empty(D, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.rdgan_mv_energy(p(ens), p(obs), m, D, ny, nx, int(shared), p(so), p(sp), p(ws), ws.numel() * 8,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return so, sp


def raw_variogram(ens, obs, shared, order, radius, max_lag, extra_words=0, fill=0):
    from pr_disagg_radar_gan_amd import _lib
    lib = _lib.load()
    D, (m, _, ny, nx) = obs.shape[0], ens.shape[-4:]
    nbytes = lib.rdgan_mv_variogram_workspace_bytes(D, ny, nx, radius, max_lag, int(shared))
    assert nbytes > 0
    ws = torch.full((nbytes // 8 + extra_words,), fill, dtype=torch.int64, device="cuda")
    side = 2 * radius + 1
    sq = torch.empty((D, max_lag + 1, side, side), dtype=torch.float64, device="cuda")
    cnt = torch.empty((D, max_lag + 1, side, side), dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.rdgan_mv_variogram(p(ens), p(obs), m, D, ny, nx, int(shared), float(order), radius, max_lag, p(sq), p(cnt), p(ws), ws.numel() * 8,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return sq, cnt


def same(a, b):
    """bit for bit, NaN included"""
    return all(np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True) for x, y in zip(a, b))


# m: below, at and across the 64-row tile (with the observation as row m: 65 rows at m = 64), a diagonal plus an off-diagonal tile;
# planes: d = 360 is no multiple of the chunk of 32, 16 x 16, and 70 x 67 (d = 112 560)
ES_CASES = [(3, m, 3, 5) for m in (1, 2, 63, 64, 65, 130)] + [(1, 2, 3, 5), (1, 65, 16, 16), (1, 5, 70, 67), (3, 5, 70, 67)]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("D,m,ny,nx", ES_CASES)
def test_energy_terms_match_yardstick(D, m, ny, nx, shared):
    mv = _mv()
    ens, obs = case(D, m, ny, nx)
    want = energy_reference(D, m, ny, nx, shared)
    e = torch.from_numpy(ens[0] if shared else ens).cuda()
    o = torch.from_numpy(obs).cuda()
    so, sp = mv.energy_terms(e, o)
    assert so.dtype == sp.dtype == torch.float64 and tuple(so.shape) == tuple(sp.shape) == (D,)
    got = np.stack([so.cpu().numpy(), sp.cpu().numpy()], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    print(f"D {D} m {m} plane {ny}x{nx} shared {shared}: worst relative error {np.nanmax(np.where(want == 0, 0, rel)):.2e} (limit {ES_RTOL:.0e})")
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if D == 3:
        assert np.isnan(got[2]).all() and not np.isnan(got[:2]).any()                      # the fully masked day, and only it
    keep = ~np.isnan(want)
    assert np.all(np.abs(got - want)[keep] <= ES_RTOL * np.abs(want)[keep])
    if m == 1:
        assert np.all(got[:2, 1] == 0.0) if D == 3 else got[0, 1] == 0.0
    # two calls agree; days scored one per call equal the same days in one call; the workspace size changes nothing
    assert same(mv.energy_terms(e, o), (so, sp))
    for d in range(D):
        one = mv.energy_terms(e if shared else e[d:d + 1], o[d:d + 1])
        assert same(one, (so[d:d + 1], sp[d:d + 1])), d
    assert same(raw_energy(e, o, shared), (so, sp)) and same(raw_energy(e, o, shared, extra_words=4099, fill=-1), (so, sp))
    # the scores from the sums, and numpy inputs
    for fair in (False, True):
        es = mv.energy_score(ens[0] if shared else ens, obs, fair=fair).cpu().numpy()
        spread = got[:, 1] / (m * (m - 1)) if fair and m > 1 else (got[:, 1] * 0 if fair else got[:, 1] / (m * m))
        assert np.allclose(es, got[:, 0] / m - spread, rtol=1e-14, atol=0, equal_nan=True)          # (torch divides by a reciprocal)


def test_equal_members_are_exactly_zero_apart():
    """analog ensembles repeat donors: a pair of equal members adds exactly 0 (the Gram form would add about 1e-8 |a|)"""
    mv = _mv()
    ens, obs = case(1, 65, 16, 16)
    base = ens[0, :60]
    dup = np.concatenate([base, base[:10]])                                               # 70 members over two tiles, 10 of them repeats
    e, o = torch.from_numpy(dup).cuda(), torch.from_numpy(obs[0]).cuda()
    _, sp = mv.energy_terms(e, o)
    # by hand: every pair of the 60 once, and the pairs of a repeat with the 59 members other than its original, and among the repeats
    _, p60 = mn.energy_terms(base, obs[0])
    _, p10 = mn.energy_terms(base[:10], obs[0])
    cross = sum(np.sqrt(np.sum((base[i].astype(np.float64) - base[j])[~np.isnan(obs[0])] ** 2)) for i in range(10) for j in range(60) if i != j)
    want = p60 + p10 + cross
    assert abs(sp.item() - want) <= ES_RTOL * want
    flat = torch.from_numpy(np.broadcast_to(base[7], (130, 24, 16, 16)).copy()).cuda()     # all equal: diagonal and off-diagonal tiles
    so, sp = mv.energy_terms(flat, o)
    assert sp.item() == 0.0 and so.item() > 0.0
    so, sp = mv.energy_terms(flat, torch.stack([o, o]))                                    # the shared form's member launch as well
    assert sp.tolist() == [0.0, 0.0]
    so, sp = mv.energy_terms(flat[:5], flat[0])                                            # equal to the observation
    assert so.item() == 0.0 and sp.item() == 0.0 and mv.energy_score(flat[:5], flat[0]).item() == 0.0


def test_energy_of_one_position_is_the_crps_kernel_s():
    """All but one pixel-hour masked: ES is the ensemble CRPS of that pixel.  The margin is that of the fp32 CRPS kernel's own test
    (tests/test_hip_ensemble.py: rtol 2e-5, atol 2e-6 against the definition).  On the CPU, the closed form evaluated in fp32 (sorted
    members, fp32 sums) differs from the fp64 one on this data, at every pixel-hour, by at most 2.7 % of that margin."""
    mv = _mv()
    from pr_disagg_radar_gan_amd.ensemble import crps_ensemble_device
    ens, obs = case(1, 130, 3, 5)
    e = torch.from_numpy(ens[0]).cuda()
    full = rain(np.random.default_rng(8), (24, 3, 5)) + np.float32(0.25)
    crps = crps_ensemble_device(e, torch.from_numpy(full).cuda()).cpu().numpy()
    for pos in ((0, 0, 0), (11, 1, 3), (23, 2, 4)):
        y = np.full((24, 3, 5), np.nan, np.float32)
        y[pos] = full[pos]
        es = mv.energy_score(e, torch.from_numpy(y).cuda()).item()
        want = mn.crps_ensemble(ens[0][(slice(None),) + pos], float(full[pos]))
        print(f"{pos}: ES {es!r}, fp64 CRPS {want!r}, CRPS kernel {crps[pos]!r}")
        assert abs(es - want) <= 1e-12 * max(1.0, abs(want))
        assert abs(es - crps[pos]) <= 2e-6 + 2e-5 * abs(want)


# (D, m, ny, nx, radius, max_lag): every (radius, max_lag) and plane of the list, m in {1, 7, 200}; 70 x 67: anchors and halos across
# the 16 x 16 tile borders; radius 4: 40 and 81 displacements in groups of 16; radius 0: lag 0 has no displacement at all
VS_CASES = [(3, 200, 3, 5, 4, 3), (1, 1, 3, 5, 0, 1), (1, 7, 16, 16, 2, 0), (3, 200, 16, 16, 2, 1), (1, 7, 16, 16, 4, 3), (1, 7, 70, 67, 2, 1),
            (1, 1, 70, 67, 4, 3), (3, 7, 70, 67, 0, 1)]


@pytest.mark.parametrize("order", [0.5, 1])
@pytest.mark.parametrize("D,m,ny,nx,radius,max_lag", VS_CASES)
def test_variogram_tables_match_yardstick(D, m, ny, nx, radius, max_lag, order):
    mv = _mv()
    ens, obs = case(D, m, ny, nx)
    e, o = torch.from_numpy(ens).cuda(), torch.from_numpy(obs).cuda()
    vs, sq, cnt = mv.variogram_score(e, o, p=order, radius=radius, max_lag=max_lag, return_tables=True)
    side = 2 * radius + 1
    assert tuple(sq.shape) == tuple(cnt.shape) == (D, max_lag + 1, side, side) and sq.dtype == torch.float64 and cnt.dtype == torch.int64
    w = mn.default_weights(radius, max_lag)
    for d in range(D):
        want_sq, want_cnt, norm = mn.variogram_tables(ens[d], obs[d], order, radius, max_lag, return_norm=True)
        got_sq, got_cnt = sq[d].cpu().numpy(), cnt[d].cpu().numpy()
        assert np.array_equal(got_cnt, want_cnt)
        if np.isnan(obs[d]).all():
            assert np.isnan(got_sq[w > 0]).all() and np.all(got_sq[w == 0] == 0) and np.all(got_cnt == 0) and np.isnan(vs[d].item())
            continue
        err = np.abs(got_sq - want_sq)
        print(f"day {d} m {m} plane {ny}x{nx} r {radius} L {max_lag} p {order}: worst |sq - yardstick| / sum(o^2 + mean^2) "
              f"{np.max(np.where(norm > 0, err / np.where(norm > 0, norm, 1), 0)):.2e} (limit {VS_RTOL:.0e})")
        assert np.all(err <= VS_RTOL * norm) and np.all(got_sq[w == 0] == 0)
        assert abs(vs[d].item() - np.sum(w * got_sq)) <= 1e-12 * np.sum(w * got_sq)
    # the shared form equals the per-day form fed the same ensemble D times, bit for bit
    rep = e[:1].expand(D, -1, -1, -1, -1).contiguous()
    per_day = mv.variogram_score(rep, o, p=order, radius=radius, max_lag=max_lag, return_tables=True)
    shared = mv.variogram_score(e[0], o, p=order, radius=radius, max_lag=max_lag, return_tables=True)
    assert same(per_day, shared)
    # two calls agree; days one per call; the workspace size changes nothing
    assert same(mv.variogram_score(e, o, p=order, radius=radius, max_lag=max_lag, return_tables=True), (vs, sq, cnt))
    for d in range(D):
        one = mv.variogram_score(e[d], o[d], p=order, radius=radius, max_lag=max_lag, return_tables=True)
        assert same(one, (vs[d:d + 1], sq[d:d + 1], cnt[d:d + 1])), d
        one = mv.variogram_score(e[0], o[d:d + 1], p=order, radius=radius, max_lag=max_lag, return_tables=True)
        assert same(one, tuple(t[d:d + 1] for t in shared)), d
    for sh, ee, ref in ((False, e, (sq, cnt)), (True, e[0].contiguous(), shared[1:])):
        assert same(raw_variogram(ee, o, sh, order, radius, max_lag), ref)
        assert same(raw_variogram(ee, o, sh, order, radius, max_lag, extra_words=4099, fill=-1), ref)


def test_variogram_weights_and_normalisation():
    mv = _mv()
    ens, obs = case(3, 200, 16, 16)
    e, o = torch.from_numpy(ens[0]).cuda(), torch.from_numpy(obs[:2]).cuda()
    vs, sq, cnt = mv.variogram_score(e, o, return_tables=True)
    w = np.random.default_rng(0).random((2, 5, 5))
    keep = mn.default_weights(2, 1) > 0
    got = mv.variogram_score(e, o, weights=w).cpu().numpy()
    want = (sq.cpu().numpy() * (w * keep)).sum(axis=(1, 2, 3))
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    norm = mv.variogram_score(e, o, normalised=True).cpu().numpy()
    assert np.allclose(norm, vs.cpu().numpy() / (cnt.cpu().numpy() * mn.default_weights(2, 1)).sum(axis=(1, 2, 3)), rtol=1e-12, atol=0)
    assert np.allclose(vs.cpu().numpy(), [mn.variogram_score(ens[0], obs[d]) for d in range(2)], rtol=1e-6, atol=0)


def test_cabi_refuses_bad_arguments_on_the_device():
    from pr_disagg_radar_gan_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    g, null, st = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    energy = lambda ens=g, obs=g, m=5, so=g, sp=g, ws=g: lib.rdgan_mv_energy(ens, obs, m, 1, 3, 5, 0, so, sp, ws, 1 << 19, st)
    vario = lambda ens=g, obs=g, m=5, p=0.5, r=1, L=1, sq=g, cnt=g, ws=g: lib.rdgan_mv_variogram(ens, obs, m, 1, 3, 5, 0, p, r, L, sq, cnt, ws, 1 << 19, st)
    assert energy() == 0 and vario() == 0 and vario(p=1.0) == 0
    for kw in (dict(ens=null), dict(obs=null), dict(so=null), dict(sp=null), dict(ws=null), dict(m=0), dict(m=8193)):
        assert energy(**kw) == -2, kw
    for kw in (dict(ens=null), dict(obs=null), dict(sq=null), dict(cnt=null), dict(ws=null), dict(m=0), dict(m=8193), dict(r=5), dict(L=4), dict(p=2.0),
               dict(p=0.75)):
        assert vario(**kw) == -2, kw
    assert lib.rdgan_mv_energy_workspace_bytes(0, 1, 0) == -2 and lib.rdgan_mv_energy_workspace_bytes(8193, 1, 0) == -2
    assert lib.rdgan_mv_variogram_workspace_bytes(1, 3, 5, 5, 1, 0) == -2 and lib.rdgan_mv_variogram_workspace_bytes(1, 3, 5, 1, 4, 0) == -2
    torch.cuda.synchronize()


def test_experiment_equals_the_scores_called_by_hand():
    mv = _mv()
    from pr_disagg_radar_gan_amd import ensemble, rainfarm, weights as W
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    from pr_disagg_radar_gan_amd.analog import AnalogLibrary
    T.configure(ndomain=8)
    gen = T.create_generator(seed=2)
    rng = np.random.default_rng(21)
    reals = (rng.gamma(0.3, 2.0, (3, 24, 8, 8)) + 1e-3).astype(np.float32)
    clim = rain(rng, (40, 24, 8, 8))
    library = AnalogLibrary(rain(rng, (12, 24, 8, 8), dry=0.4))
    m, seed, slopes = 16, 5, (2.2, 1.3)
    res = mv.multivariate_experiment(gen, reals, clim, slopes=slopes, library=library, n_members=m, seed=seed)
    assert set(res.es) == set(res.vs) == {"gan", "random", "rainfarm", "analog"}
    rd = torch.from_numpy(reals).cuda()
    by_hand = {"gan": [], "rainfarm": [], "analog": []}
    for d in range(3):
        dsum = torch.from_numpy(reals[d]).sum(0)
        frac = ensemble.generate_ensemble_device(gen, (dsum / W.NORM_SCALE).numpy()[..., None], m, seed=seed + d)
        by_hand["gan"].append(frac * (dsum / W.NORM_SCALE * W.NORM_SCALE).to(frac.device))
        by_hand["rainfarm"].append(rainfarm.downscale_device(rd[d].sum(0), *slopes, n_members=m, seed=seed, first_member=d * m))
        by_hand["analog"].append(library.generate(rd[d:d + 1].sum(1), m, k=10, seed=seed, weights="rank", first_query=d)[0])
    for name, members in by_hand.items():
        for d in range(3):
            assert res.es[name][d] == mv.energy_score(members[d], rd[d]).item(), (name, d)
            assert res.vs[name][d] == mv.variogram_score(members[d], rd[d]).item(), (name, d)
    assert np.array_equal(res.es["random"], mv.energy_score(clim, reals).cpu().numpy())
    assert np.array_equal(res.vs["random"], mv.variogram_score(clim, reals).cpu().numpy())
    assert np.allclose(res.es["random"], [mn.energy_score(clim, reals[d]) for d in range(3)], rtol=1e-10, atol=0)
    assert all(np.isfinite(v).all() and v.shape == (3,) and v.dtype == np.float64 for t in (res.es, res.vs) for v in t.values())
    s = res.summary(N=200)
    assert set(s) == {"es", "vs"}
    for name, table in (("es", res.es), ("vs", res.vs)):
        assert set(s[name]) == {"gan", "random", "rainfarm", "analog", "gan-random", "gan-rainfarm", "gan-analog"}
        assert abs(s[name]["gan"] - table["gan"].mean()) < 1e-12 * abs(table["gan"].mean())
        for b in ("random", "rainfarm", "analog"):
            entry = s[name][f"gan-{b}"]
            assert set(entry) == {"ttest_p", "bootstrap"} and 0 <= entry["ttest_p"] <= 1 and entry["bootstrap"].shape == (3,)
            assert abs(entry["bootstrap"][0] - (table["gan"] - table[b]).mean()) <= 1e-12 * abs((table["gan"] - table[b]).mean())
    few = mv.multivariate_experiment(gen, reals[:1], clim, n_members=m, seed=seed)                # neither slopes nor a library
    assert set(few.es) == {"gan", "random"} and few.es["gan"][0] == res.es["gan"][0] and few.vs["random"][0] == res.vs["random"][0]
