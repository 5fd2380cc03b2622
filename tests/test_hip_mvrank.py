"""-m gpu: the multivariate rank histograms (csrc/rdgan_mvrank.hip.h, pr_disagg_radar_gan_amd/multivariate_ranks.py) against the numpy
yardstick (tests/mvrank_np.py).  Every result is an integer and every assertion an equality: the sums behind the average-rank and
band-depth pre-ranks at every tile width and on both sides of each switch point, with bad, constant, duplicated and signed-zero
columns; the leave-one-out MST lengths against Prim in numpy and against the closed form of points on a line; the routes from an
ensemble to the observation's ranks."""
import functools

import numpy as np
import pytest
import torch

from tests import mvrank_np as mr

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 64, 65, 512, 513, 1024, 1025, 2049)                                         # N: both sides of the switch points of TP and of the sums' home
PLANES = ((1, 1), (3, 5), (17, 9))                                                         # 1, 15 and 153 positions: no multiple of 8
CASES = [(N, pl) for N in SIZES for pl in PLANES] + [(4096, (1, 1))]


def _mr():
    from pr_disagg_radar_gan_amd import multivariate_ranks
    return multivariate_ranks


def rain(rng, shape, dry=0.6):
    return (rng.gamma(0.5, 4.0, shape) * (rng.random(shape) < 1.0 - dry)).astype(np.float32)


def tile_positions(N):
    return 64 if N <= 512 else 32 if N <= 1024 else 16 if N <= 2048 else 8


@functools.lru_cache(maxsize=None)
def case(N, plane):
    """(ens (m, 24, ny, nx), obs (24, ny, nx)), shared and never written to.  Hour 5 is dry for everyone; hour 7 has a constant wet
    column and hour 2 one of zeros of both signs; hour 3 a -0.0 in a column that varies; the observation is NaN at the first and
    the last position of the first tile (hour 9), one member is NaN at the first position of the second tile (hour 10) and infinite
    at the last position of the plane (hour 11); members 1 and 3 are equal where there are that many."""
    ny, nx = plane
    m, P, tp = N - 1, ny * nx, tile_positions(N)
    rng = np.random.default_rng(1000 * N + P)
    ens, obs = rain(rng, (m, 24, ny, nx)), rain(rng, (24, ny, nx))
    if m >= 4:
        ens[3] = ens[1]
    e, o = ens.reshape(m, 24, P), obs.reshape(24, P)
    e[:, 5], o[5] = 0.0, 0.0
    e[:, 7, 0], o[7, 0] = 2.5, 2.5
    e[:, 2, 0], o[2, 0] = 0.0, 0.0
    e[::2, 2, 0] = -0.0
    e[0, 3, 0] = -0.0
    o[9, 0] = o[9, min(tp, P) - 1] = np.nan
    e[m // 2, 10, min(tp, P - 1)] = np.nan
    e[m - 1, 11, P - 1] = -np.inf
    return ens, obs


@functools.lru_cache(maxsize=None)
def reference(N, plane):
    return mr.prerank_sums_by_hour(*case(N, plane))


@pytest.mark.parametrize("N,plane", CASES)
def test_prerank_sums_equal_numpy(N, plane):
    MR = _mr()
    ens, obs = case(N, plane)
    want, want_valid = reference(N, plane)
    P = plane[0] * plane[1]
    assert want_valid[5] == P and want_valid[9] == max(P - 2, 0) and want_valid[10] == P - 1 and want_valid[11] == P - 1
    assert np.array_equal(want[5], np.tile([P * (N + 1), P * (N - 1) * (N - 2)], (N, 1)))  # the dry hour in closed form
    sums, n_valid = MR.prerank_sums(ens, obs, by_hour=True)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (1, 24, N, 2) and tuple(n_valid.shape) == (1, 24)
    assert np.array_equal(n_valid[0].cpu().numpy(), want_valid)
    assert np.array_equal(sums[0].cpu().numpy(), want)
    day, day_valid = MR.prerank_sums(ens, obs)
    assert np.array_equal(day[0].cpu().numpy(), want.sum(axis=0)) and int(day_valid[0]) == want_valid.sum()
    for runs in (1, 2, 1000):                                                              # the result does not depend on the runs
        s, v = MR.prerank_sums(ens, obs, by_hour=True, position_runs=runs)
        assert torch.equal(s, sums) and torch.equal(v, n_valid), runs


def test_shared_form_per_day_form_and_input_kinds():
    MR = _mr()
    rng = np.random.default_rng(77)
    ens = rain(rng, (64, 24, 3, 5))
    obs = rain(rng, (3, 24, 3, 5))
    obs[0, 4, 1, 1] = np.nan
    obs[2] = np.nan                                                                        # a day without a valid position
    want = [mr.prerank_sums(ens, obs[d]) for d in range(3)]
    shared, nv = MR.prerank_sums(ens, obs)
    assert tuple(shared.shape) == (3, 65, 2)
    for d in range(3):
        assert np.array_equal(shared[d].cpu().numpy(), want[d][0]) and int(nv[d]) == want[d][1]
    assert int(nv[2]) == 0 and int(shared[2].abs().sum()) == 0
    per_day, nv2 = MR.prerank_sums(np.broadcast_to(ens, (3,) + ens.shape), obs)
    assert torch.equal(per_day, shared) and torch.equal(nv2, nv)
    dev, nv3 = MR.prerank_sums(torch.from_numpy(ens).cuda(), torch.from_numpy(obs).cuda())   # CUDA tensors against numpy arrays
    assert torch.equal(dev, shared) and torch.equal(nv3, nv)
    other = rain(rng, (3, 64, 24, 3, 5))                                                   # a different ensemble every day
    got, _ = MR.prerank_sums(other, obs, by_hour=True)
    for d in range(2):
        assert np.array_equal(got[d].cpu().numpy(), mr.prerank_sums_by_hour(other[d], obs[d])[0])


def lattice_distances(rng, n, spread):
    """the L1 distances of n points with small integer coordinates: many zero and equal edges"""
    pts = rng.integers(0, spread, (n, 4))
    return np.abs(pts[:, None] - pts[None, :]).sum(-1).astype(np.int64)


@pytest.mark.parametrize("n", (1, 2, 3, 64, 65, 257, 300))
def test_mst_equals_numpy_prim(n):
    MR = _mr()
    rng = np.random.default_rng(n)
    for spread in ((2, 50) if n < 257 else (3,)):                                          # (the yardstick takes a second per matrix at 300)
        dist = lattice_distances(rng, n, spread)
        got = MR.mst_leave_one_out(torch.from_numpy(dist).cuda())
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), mr.mst_leave_one_out(dist)), spread
    if n >= 257:
        return
    big = lattice_distances(rng, n, 1 << 20) * ((1 << 18) - 1)                             # edges close to 2^40
    assert big.max() < 1 << 40
    assert np.array_equal(MR.mst_leave_one_out(torch.from_numpy(big).cuda()).cpu().numpy(), mr.mst_leave_one_out(big))
    if n >= 2:
        big[0, 1] = 1 << 40
        with pytest.raises(ValueError):
            MR.mst_leave_one_out(torch.from_numpy(big).cuda())


def test_mst_of_4096_points_on_a_line():
    """one valid position and distinct values: the tree without i is the range of the other values"""
    MR = _mr()
    rng = np.random.default_rng(4096)
    e = rng.permutation(65536)[:4096].astype(np.int64)                                     # distinct features, in 1 / 32 mm
    x = (e / 32.0).astype(np.float32)
    obs = np.full((24, 1, 1), np.nan, np.float32)
    obs[6] = x[0]
    ens = rain(rng, (4095, 24, 1, 1))
    ens[:, 6, 0, 0] = x[1:]
    got, n_valid = MR.mst_preranks(ens, obs)
    order = np.sort(e)
    lo = np.where(e == order[0], order[1], order[0])
    hi = np.where(e == order[-1], order[-2], order[-1])
    assert int(n_valid) == 1 and np.array_equal(got.cpu().numpy(), hi - lo)


@pytest.mark.parametrize("pool", (1, 4))
def test_mst_preranks_end_to_end(pool):
    MR = _mr()
    rng = np.random.default_rng(pool)
    ens, obs = rain(rng, (20, 24, 6, 7)), rain(rng, (24, 6, 7))
    obs[3, 5, 6] = np.nan                                                                  # a rim block of pool 4
    ens[4, 8, 0, 0] = 3000.0                                                               # bad for this route alone
    want, want_valid = mr.mst_preranks(ens, obs, pool)
    got, n_valid = MR.mst_preranks(ens, obs, pool)
    assert int(n_valid) == want_valid == 24 * (42 if pool == 1 else 4) - 2
    assert np.array_equal(got.cpu().numpy(), want)
    dev, _ = MR.mst_preranks(torch.from_numpy(ens).cuda(), torch.from_numpy(obs).cuda(), pool)
    mixed, _ = MR.mst_preranks(ens, torch.from_numpy(obs).cuda(), pool)
    assert torch.equal(dev, got) and torch.equal(mixed, got)


def test_ranks_of_the_observation_end_to_end():
    MR = _mr()
    rng = np.random.default_rng(9)
    ens, obs = rain(rng, (3, 9, 24, 4, 5)), rain(rng, (3, 24, 4, 5))
    obs[1] = np.nan                                                                        # an empty case
    obs[2, 0, 0, 0] = np.nan
    res = MR.multivariate_ranks(ens, obs, pool=2)
    assert res.kinds == MR.KINDS and res.n_members == 9
    for d in (0, 2):
        sums, nv = mr.prerank_sums(ens[d], obs[d])
        mst, nm = mr.mst_preranks(ens[d], obs[d], 2)
        for kind, rho, n in (("average", sums[:, 0], nv), ("band_depth", sums[:, 1], nv), ("mst", mst, nm)):
            b, e = mr.observation_ranks(rho)
            assert (res.below[kind][d], res.equal[kind][d], res.n_valid[kind][d]) == (b, e, n), (kind, d)
    for kind in MR.KINDS:
        assert res.n_valid[kind][1] == 0 and res.n_empty(kind) == 1 and res.histogram(kind).sum() == 2
    days = MR.ranks_for_days(lambda d: ens[d], obs, pool=2)
    hourly = MR.multivariate_ranks(ens, obs, kinds=("average", "band_depth"), by_hour=True)
    for kind in MR.KINDS:
        assert all(np.array_equal(getattr(days, f)[kind], getattr(res, f)[kind]) for f in ("below", "equal", "n_valid"))
    assert hourly.below["average"].shape == (3, 24) and hourly.n_empty("band_depth") == 24
    sums, nv = mr.prerank_sums_by_hour(ens[2], obs[2])
    b, e = mr.observation_ranks(sums[..., 1])
    assert np.array_equal(hourly.below["band_depth"][2], b) and np.array_equal(hourly.equal["band_depth"][2], e)
    assert np.array_equal(hourly.n_valid["average"][2], nv)
    assert set(MR.compare(res, hourly, n_bins=2)) == {"average", "band_depth"}


def test_rank_experiment_equals_the_ranks_called_by_hand():
    """the twin of test_hip_multivariate.test_experiment_equals_the_scores_called_by_hand, on its inputs: every method's members
    built by hand by the seed rules, ranked by multivariate_ranks, equal the experiment's -- and, scored by energy_score, equal
    multivariate_experiment's on the same arguments: the two experiments see the same members"""
    MR = _mr()
    from pr_disagg_radar_gan_amd import cascade, ensemble, multivariate as mv, rainfarm, weights as W
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    from pr_disagg_radar_gan_amd.analog import AnalogLibrary
    T.configure(ndomain=8)
    gen = T.create_generator(seed=2)
    rng = np.random.default_rng(21)
    reals = (rng.gamma(0.3, 2.0, (3, 24, 8, 8)) + 1e-3).astype(np.float32)
    clim = rain(rng, (40, 24, 8, 8))
    days = rain(rng, (12, 24, 8, 8), dry=0.4)
    library, model = AnalogLibrary(days), cascade.calibrate(days)
    m, seed, slopes = 16, 5, (2.2, 1.3)
    args = dict(slopes=slopes, library=library, n_members=m, seed=seed, cascade=model, cascade_patch=8)
    res = MR.multivariate_rank_experiment(gen, reals, clim, kinds=MR.KINDS, pool=2, **args)
    order = ["gan", "random", "rainfarm", "analog", "cascade"]
    assert list(res) == order
    rd = torch.from_numpy(reals).cuda()
    by_hand = {name: [] for name in order if name != "random"}
    for d in range(3):
        dsum = torch.from_numpy(reals[d]).sum(0)
        frac = ensemble.generate_ensemble_device(gen, (dsum / W.NORM_SCALE).numpy()[..., None], m, seed=seed + d)
        by_hand["gan"].append(frac * (dsum / W.NORM_SCALE * W.NORM_SCALE).to(frac.device))
        by_hand["rainfarm"].append(rainfarm.downscale_device(rd[d].sum(0), *slopes, n_members=m, seed=seed, first_member=d * m))
        by_hand["analog"].append(library.generate(rd[d:d + 1].sum(1), m, k=10, seed=seed, weights="rank", first_query=d)[0])
        by_hand["cascade"].append(model.generate(rd[d:d + 1].sum(1), m, seed=seed, first_query=d, patch=8)[0])

    def same(got, want, at=slice(None)):
        assert got.kinds == want.kinds and got.n_members == want.n_members
        for kind in want.kinds:
            for f in ("below", "equal", "n_valid"):
                assert np.array_equal(getattr(got, f)[kind][at], getattr(want, f)[kind]), (kind, f)

    for name, members in by_hand.items():
        assert res[name].n_members == m
        for d in range(3):
            same(res[name], MR.multivariate_ranks(members[d], rd[d], kinds=MR.KINDS, pool=2), slice(d, d + 1))
    same(res["random"], MR.multivariate_ranks(clim, reals, kinds=MR.KINDS, pool=2))
    assert res["random"].n_members == 40 and all(res[name].below[k].shape == (3,) for name in order for k in MR.KINDS)
    hourly = MR.multivariate_rank_experiment(gen, reals, clim, n_members=m, seed=seed, by_hour=True, kinds=("average", "band_depth"))
    assert list(hourly) == ["gan", "random"]
    for d in range(3):
        same(hourly["gan"], MR.multivariate_ranks(by_hand["gan"][d], rd[d], kinds=("average", "band_depth"), by_hour=True), slice(d, d + 1))
    same(hourly["random"], MR.multivariate_ranks(clim, reals, kinds=("average", "band_depth"), by_hour=True))
    assert hourly["gan"].below["average"].shape == (3, 24)
    scores = mv.multivariate_experiment(gen, reals, clim, **args)                          # the same members, scored
    assert list(scores.es) == list(scores.vs) == order
    for name, members in by_hand.items():
        for d in range(3):
            assert scores.es[name][d] == mv.energy_score(members[d], rd[d]).item(), (name, d)
    assert np.array_equal(scores.es["random"], mv.energy_score(clim, reals).cpu().numpy())
