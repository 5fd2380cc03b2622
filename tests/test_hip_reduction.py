"""-m gpu: scenario reduction (csrc/rdgan_reduce.hip.h, pr_disagg_radar_gan_amd/reduction.py) against the numpy restatement
(tests/reduction_np.py, itself checked on the CPU by tests/test_reduction_host.py).  Everything is an integer: every comparison is an
equality."""
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, models, reduction as RD, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import reduction_np as rn
from tests.hip_util import dev

pytestmark = pytest.mark.gpu


def host(t):
    """a tensor on the host as numpy; uint16 travels as its int16 bits"""
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def eq(t, a):
    a = np.asarray(a)
    return tuple(t.shape) == a.shape and np.array_equal(host(t).astype(np.int64), a.astype(np.int64))


def features_of(feat, bad):
    """a ScenarioFeatures holding the given features (S, Pf) uint16 and bad bits (Pf,), without an hourly array behind it"""
    S, pf = feat.shape
    f = RD.ScenarioFeatures()
    f.lib, f.device, f.n_members, f.n_positions = _lib.load(), torch.device("cuda", torch.cuda.current_device()), S, pf
    padded = np.zeros((S, RD.padded_positions(pf)), np.uint16)
    padded[:, :pf] = feat
    bits = np.zeros(RD.bad_words(pf) * 32, np.uint64)
    bits[:pf] = bad
    words = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    f._chunks = [torch.from_numpy(padded.view(np.int16)).cuda()]
    f.bad = torch.from_numpy(words.view(np.int32)).cuda()
    return f


@functools.lru_cache(maxsize=None)
def random_features(S, pf, seed, masked=0.0):
    """shared: copy before writing"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 65536, (S, pf)).astype(np.uint16), rng.random(pf) < masked


def check_distances(feat, bad, splits=(None,)):
    """the distances against the mirror, once per way of cutting the positions into ranges (None: the entry's own choice)"""
    want, want_valid = rn.distances_fast(feat, bad)
    held = features_of(feat, bad)
    for position_splits in splits:
        dist, n_valid = RD.member_distances(held, position_splits=position_splits)
        assert dist.dtype == torch.int64 and n_valid.dtype == torch.int64 and eq(dist, want) and int(n_valid) == want_valid, position_splits
        assert torch.equal(dist, dist.t()) and not dist.diagonal().any()                   # symmetry and the zero diagonal, directly
    return want, want_valid


def random_dist(rng, S, top, low=1):
    """a symmetric matrix with a zero diagonal and off-diagonal entries in low .. top - 1"""
    d = np.triu(rng.integers(low, top, (S, S)).astype(np.int64), 1)
    return d + d.T


def check_select(d, k):
    """select() against the mirror: picks, costs, assignment, counts and the prefixes"""
    S = len(d)
    r = RD.select(dev(d, torch.int64), k)
    chosen, cost = rn.select_fast(d, k)
    a, counts = rn.assign(d, chosen)
    assert (r.chosen.dtype, r.cost.dtype, r.assign.dtype, r.counts.dtype) == (np.int32, np.int64, np.int32, np.int32)
    assert np.array_equal(r.chosen, chosen) and np.array_equal(r.cost, cost) and np.array_equal(r.assign, a) and np.array_equal(r.counts, counts)
    assert r.counts.sum() == S and np.array_equal(r.dist_chosen, d[chosen]) and r.n_members == S
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
def edge_case_array():
    """(2, 3, 24, 5, 7): roundings on .5 with an even and an odd neighbour, the clamp, the four kinds of bad value"""
    rng = np.random.default_rng(3)
    x = (rng.gamma(0.6, 3.0, (2, 3, 24, 5, 7)) * (rng.random((2, 3, 24, 5, 7)) < 0.6)).astype(np.float32)
    x[0, 0, 0, 0, :6] = (0.015625, 0.046875, 0.078125, 0.109375, 2047.99, 2047.0)         # .5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, the clamp
    x[1, 0, 0, 1, :4] = (np.nan, -1.0, np.inf, 2048.0)
    x[0, 2, 23, 4, 6] = -np.inf
    x[1, 1, 23, 2, 3] = np.nan
    x[0, 1, 5, 2, 2] = np.nan                                                             # here every hour is seen
    return x


@pytest.mark.parametrize("pool", [1, 2, 4, 8])
def test_features_rounding_clamp_bad_values_and_pooling(pool):
    """a 5 x 7 plane: every pool has rim blocks, pool 8 a single block smaller than itself"""
    x = edge_case_array()
    feat, bad = rn.features(x, pool)
    pf = 3 * 24 * (-(-5 // pool)) * (-(-7 // pool))
    if pool == 1:
        assert feat[0, :6].tolist() == [0, 2, 2, 4, 65535, 65504] and bad.any(axis=0).sum() == 7 and bad[1, 7:11].all() and not feat[1, 7:11].any()
    for members in (dev(x), x):                                                           # a tensor, then numpy in
        f = RD.ScenarioFeatures(pool).add(members)
        assert f.features.dtype == torch.uint16 and tuple(f.features.shape) == (2, RD.padded_positions(pf)) and tuple(f.bad.shape) == (RD.bad_words(pf),)
        assert eq(f.features[:, :pf], feat) and not host(f.features[:, pf:]).any() and eq(f.bad_mask(), bad.any(axis=0))
        assert (f.n_members, f.member_shape, f.n_positions, f.n_valid) == (2, (3, 24, 5, 7), pf, pf - int(bad.any(axis=0).sum()))
    one = RD.ScenarioFeatures(pool).add(dev(x[:, 0]))                                      # members without a day axis
    f1, b1 = rn.features(x[:, 0], pool)
    assert eq(one.features[:, :pf // 3], f1) and eq(one.bad_mask(), b1.any(axis=0)) and one.member_shape == (24, 5, 7)


def test_features_strided_views_and_two_adds_equal_one():
    x = edge_case_array()
    for pool in (1, 2):
        feat, bad = rn.features(x, pool)
        whole = RD.ScenarioFeatures(pool).add(dev(x))
        two = RD.ScenarioFeatures(pool).add(dev(x[:1])).add(x[1:])
        assert np.array_equal(host(two.features), host(whole.features)) and torch.equal(two.bad, whole.bad) and two.n_members == 2
        # a member axis with a stride wider than a member: a view of a wider buffer, on the scalar route (the stride is odd)
        wide = torch.full((2, 3 * 24 * 35 + 13), float("nan"), device="cuda")
        wide[:, :3 * 24 * 35] = dev(x).reshape(2, -1)
        view = wide[:, :3 * 24 * 35].view(2, 3, 24, 5, 7)
        assert view.stride(0) == 3 * 24 * 35 + 13
        f = RD.ScenarioFeatures(pool).add(view)
        assert eq(f.features[:, :feat.shape[1]], feat) and eq(f.bad_mask(), bad.any(axis=0))
    # the 16-byte route: pool 1 and an aligned, wider stride
    y = np.random.default_rng(5).gamma(0.7, 2.0, (4, 24, 3, 5)).astype(np.float32)
    y[2, 23, 2, 4] = 2048.0
    wide = torch.zeros((4, 24 * 15 + 16), device="cuda")
    wide[:, :24 * 15] = dev(y).reshape(4, -1)
    view = wide[:, :24 * 15].view(4, 24, 3, 5)
    f = RD.ScenarioFeatures().add(view[:1]).add(view[1:])
    f2, b2 = rn.features(y)
    assert eq(f.features, f2) and eq(f.bad_mask(), b2.any(axis=0)) and b2.sum() == 1 and f.n_members == 4 and f.n_valid == 359


def test_a_bad_value_in_a_later_add_masks_earlier_members():
    rng = np.random.default_rng(9)
    x = rng.gamma(0.7, 2.0, (5, 24, 6, 6)).astype(np.float32)
    x[4, 3, 2, :] = np.nan                                                                # the last member, added last
    feat, bad = rn.features(x, 2)
    want, nv = rn.distances(feat, bad)
    unmasked, _ = rn.distances(feat[:4], bad[:4])
    assert nv == 24 * 9 - 3 and (unmasked > want[:4, :4]).any()                           # the mask changes the earlier members' distances
    f = RD.ScenarioFeatures(2).add(x[:2]).add(dev(x[2:4]))
    d4, n4 = RD.member_distances(f)
    assert eq(d4, unmasked) and int(n4) == 24 * 9
    d5, n5 = RD.member_distances(f.add(x[4:]))
    assert eq(d5, want) and int(n5) == nv == f.n_valid
    back = RD.ScenarioFeatures(2).add(x[::-1].copy())                                     # the bad member first: the same matrix, mirrored
    assert eq(RD.member_distances(back)[0], want[::-1, ::-1])


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5), (2, 127), (63, 129), (64, 1000), (65, 129), (130, 1000), (130, 5), (65, 127)])
def test_distances_shapes(shape):
    """S = 130: the triangle of 3 x 3 tiles, diagonal tiles staged once, every off-diagonal tile mirrored; Pf around the 128-position
    chunk; a tenth of the positions masked"""
    S, pf = shape
    feat, bad = random_features(S, pf, 11 + S + pf, 0.1)
    want, nv = check_distances(feat, bad)
    assert S == 1 or (want[0, 1] > 0 and nv < pf) or pf == 5


def test_distances_position_splits_give_the_same_matrix():
    feat, bad = random_features(130, 1000, 21, 0.05)
    check_distances(feat, bad, splits=(1, 2, 7, 1000, None))
    feat, bad = random_features(3, 4099, 22, 0.1)                                         # 33 chunks in one workgroup, and cut
    check_distances(feat, bad, splits=(1, 2, 7, 33, None))


@pytest.mark.parametrize("pf", [40000, 70000])
def test_distances_past_the_flush_and_past_32_bits(pf):
    """features 0 against 65535.  40 000 positions cross the flush of the 32-bit sums (every 256 chunks = 32 768 positions) in one
    workgroup; 70 000 x 65535 = 4 587 450 000 > 2^32 would wrap a 32-bit sum that is never flushed.  Closed forms."""
    feat = np.zeros((2, pf), np.uint16)
    feat[0] = 65535
    held = features_of(feat, np.zeros(pf, bool))
    for position_splits in (1, 2, None):
        dist, n_valid = RD.member_distances(held, position_splits=position_splits)
        assert dist.cpu().tolist() == [[0, pf * 65535], [pf * 65535, 0]] and int(n_valid) == pf, position_splits
    feat[1, ::2] = 65535
    dist, _ = RD.member_distances(features_of(feat, np.zeros(pf, bool)), position_splits=1)
    assert dist.cpu().tolist() == [[0, pf // 2 * 65535], [pf // 2 * 65535, 0]]


def test_distances_identical_members_and_a_full_mask():
    feat, _ = random_features(5, 300, 13)
    feat = feat.copy()
    feat[3] = feat[1]
    want, nv = check_distances(feat, np.zeros(300, bool))
    assert want[1, 3] == 0 and np.array_equal(want[1], want[3]) and nv == 300
    want, nv = check_distances(feat, np.ones(300, bool))
    assert nv == 0 and not want.any()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 65, 300])
def test_selection_random_matrices(S):
    d = random_dist(np.random.default_rng(S), S, 1 << 30)
    for k in sorted({1, min(7, S), S}):
        r = check_select(d, k)
        assert len(set(r.chosen.tolist())) == k
    assert r.cost[-1] == 0 and sorted(r.chosen.tolist()) == list(range(S))                # k = S of distinct members: nothing is left
    assert (np.diff(r.cost) <= 0).all()
    for k in sorted({1, min(7, S), S}):                                                   # forward selection is nested
        p, q = r.prefix(k), RD.select(dev(d, torch.int64), k)
        assert all(np.array_equal(getattr(p, n), getattr(q, n)) for n in ("chosen", "cost", "assign", "counts", "dist_chosen"))


def test_selection_with_many_ties():
    for S in (5, 70):
        d = random_dist(np.random.default_rng(S), S, 3, low=0)                            # values 0 .. 2: ties at every step
        check_select(d, S)


def test_selection_duplicates_selected_skip_and_count_zero():
    """an ensemble with exact duplicates and k above the number of distinct members: a selected member is never picked again, and a
    pick that duplicates a smaller-indexed pick serves nobody"""
    rng = np.random.default_rng(31)
    base = (rng.integers(0, 3000, (4, 24, 4, 5)) / 32.0).astype(np.float32)
    x = base[[0, 1, 1, 2, 3, 1, 0]]                                                       # members 1, 2, 5 and 0, 6 are the same
    r = RD.reduce_hourly(dev(x), 6)
    want = rn.reduce(x, 6)
    assert all(np.array_equal(getattr(r, n), want[n]) for n in ("chosen", "cost", "assign", "counts"))
    assert len(set(r.chosen.tolist())) == 6 and not r.cost[3:].any() and r.cost[2] > 0 and r.counts.sum() == 7
    picked = dict(zip(r.chosen.tolist(), r.counts.tolist()))
    assert picked[1] == 3 and picked[0] == 2 and all(picked.get(u, 0) == 0 for u in (2, 5, 6))
    assert r.assign[[1, 2, 5]].tolist() == [1, 1, 1] and r.assign[[0, 6]].tolist() == [0, 0] and r.weights.sum() == pytest.approx(1.0)


def test_selection_all_equal_distances_and_large_entries():
    S = 70
    d = 7 * (1 - np.eye(S, dtype=np.int64))
    r = check_select(d, S)
    assert r.chosen.tolist() == list(range(S)) and r.cost.tolist() == [7 * (S - 1 - t) for t in range(S)]    # every tie: the smaller index
    r = check_select(np.zeros((S, S), np.int64), 5)
    assert r.chosen.tolist() == [0, 1, 2, 3, 4] and not r.cost.any() and r.counts.tolist() == [S, 0, 0, 0, 0]
    top = (1 << 52) // S                                                                   # entries near 2^52 / S
    big = random_dist(np.random.default_rng(8), S, top, low=top - 1000)
    r = check_select(big, 9)
    assert int(r.cost[0]) > (S - 1) * (top - 1000) > 1 << 51 and (int(r.cost[0]) << 12 | int(r.chosen[0])) < 1 << 64


# ---------------------------------------------------------------------------------------------------------------------------------
def same(r, want):
    return all(np.array_equal(getattr(r, n), want[n]) for n in ("chosen", "cost", "assign", "counts")) and r.n_valid == want["n_valid"]


def test_reduce_hourly_equals_the_restatement():
    rng = np.random.default_rng(17)
    x = (rng.gamma(0.6, 3.0, (20, 2, 24, 9, 11)) * (rng.random((20, 2, 24, 9, 11)) < 0.5)).astype(np.float32)
    x[7, 1, 3, 8, 10] = np.nan
    for pool, k in ((1, 5), (4, 20)):
        want = rn.reduce(x, k, pool)
        r = RD.reduce_hourly(dev(x) if pool == 1 else x, k, pool=pool)
        assert same(r, want) and r.n_valid == RD.n_positions((2, 24, 9, 11), pool) - 1 and r.n_members == 20
        assert np.allclose(r.mean_distance_mm, want["cost"] / (32.0 * 20 * want["n_valid"]), rtol=1e-12) and r.latent is None and r.hourly is None
        assert np.allclose(r.weights, want["counts"] / 20.0)


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_reduce_field_equals_reduce_hourly_of_disaggregate(generator, monkeypatch):
    """2 wet days of a 20 x 24 plane at ndomain 16, overlap 4, 6 scenarios; `chunk` is one unit's tiles on both sides (every tile of
    every day is wet), the batching for which evaluate_field promises equal values"""
    S, D, k = 6, 2, 3
    rng = np.random.default_rng(41)
    daily = (0.1 + rng.gamma(0.8, 6.0, (D, 20, 24))).astype(np.float32)
    daily[1, 3, 5] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(42).normal(size=(S, D, 100)).astype(np.float32)
    info = F.disaggregate(generator, dd, 1, latent=z[:1])[1]
    assert info.n_active == D * info.n_tiles and info.n_nan_pixels == 1
    hourly, _ = F.disaggregate(generator, dd, S, latent=z, chunk=info.n_tiles)
    for pool in (1, 4):
        want = RD.reduce_hourly(hourly, k, pool=pool)
        mirror = rn.reduce(hourly.cpu().numpy(), k, pool)
        assert same(want, mirror) and want.n_valid == RD.n_positions((D, 24, 20, 24), pool) - 24
        stored = RD.ScenarioFeatures(pool).add(hourly).features
        for scenario_chunk in (1, 4, 6):
            got = RD.reduce_field(generator, dd if scenario_chunk == 4 else daily, S, k, pool=pool, return_hourly=True, scenario_chunk=scenario_chunk,
                                  latent=z, chunk=info.n_tiles)
            assert same(got, mirror) and np.array_equal(got.latent, z[got.chosen]) and tuple(got.hourly.shape) == (k, D, 24, 20, 24)
            # the returned members are the chosen ones: their features are the stored features, bit for bit
            again = RD.ScenarioFeatures(pool).add(got.hourly).features
            assert torch.equal(again.view(torch.int16), stored.view(torch.int16)[got.chosen.astype(np.int64)])
            assert torch.equal(got.hourly.nan_to_num(-1.0), hourly[got.chosen.astype(np.int64)].nan_to_num(-1.0))
            p = got.prefix(2)
            assert np.array_equal(p.latent, z[got.chosen[:2]]) and tuple(p.hourly.shape) == (2, D, 24, 20, 24)
    # one day without a day axis, the latent drawn from the numpy RNG as disaggregate draws it, through the drop-in wrapper
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.reduce_scenarios_field(daily[0], S, k, pool=2, scenario_chunk=S)
    np.random.seed(5)
    z5 = np.random.normal(size=(S, 1, 100)).astype(np.float32)
    hourly2, _ = F.disaggregate(generator, dd[0], S, latent=z5, norm_scale=P.norm_scale)
    b = RD.reduce_hourly(hourly2, k, pool=2)
    assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("chosen", "cost", "assign", "counts")) and a.n_valid == b.n_valid
    assert np.array_equal(a.latent, z5[a.chosen]) and a.hourly is None


def test_reduce_field_without_a_wet_tile(generator):
    state = np.random.get_state()[1].copy()
    r = RD.reduce_field(generator, np.zeros((20, 24), np.float32), 5, 3, return_hourly=True)
    assert r.chosen.tolist() == [0, 1, 2] and not r.cost.any() and r.counts.tolist() == [5, 0, 0] and r.latent is None
    assert np.array_equal(np.random.get_state()[1], state)                                # no latent was drawn
    assert tuple(r.hourly.shape) == (3, 24, 20, 24) and not r.hourly.any() and r.n_valid == 24 * 20 * 24


def test_c_entries_refuse_bad_arguments_and_touch_nothing():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x = dev(edge_case_array())
    feat = torch.full((2, 2520), -3, dtype=torch.int16, device="cuda")
    bad = torch.full((79,), -3, dtype=torch.int32, device="cuda")
    for kw in (dict(n=0), dict(stride=3 * 24 * 35 - 1), dict(pool=3), dict(fstride=2512), dict(D=0)):
        a = {**dict(n=2, stride=3 * 24 * 35, D=3, pool=1, fstride=2520), **kw}
        assert lib.rdgan_red_features(x.data_ptr(), a["n"], a["stride"], a["D"], 5, 7, a["pool"], feat.data_ptr(), a["fstride"], bad.data_ptr(), st) == -2, kw
    dist = torch.full((2, 2), -3, dtype=torch.int64, device="cuda")
    nv = torch.full((1,), -3, dtype=torch.int64, device="cuda")
    for S, fstride, pf, splits in ((0, 2520, 2520, 0), (2, 2512, 2520, 0), (2, 2520, 2520, -1), (2, 2520, 0, 0)):
        assert lib.rdgan_red_distances(feat.data_ptr(), bad.data_ptr(), S, fstride, pf, splits, dist.data_ptr(), nv.data_ptr(), st) == -2
    out = torch.full((8,), -3, dtype=torch.int32, device="cuda")
    cost = torch.full((2,), -3, dtype=torch.int64, device="cuda")
    ws = torch.full((8,), -3, dtype=torch.int64, device="cuda")
    for S, k, nbytes in ((2, 3, 64), (2, 0, 64), (2, 2, 39), (0, 1, 64)):
        assert lib.rdgan_red_select(dist.data_ptr(), S, k, out.data_ptr(), cost.data_ptr(), out[2:].data_ptr(), out[4:].data_ptr(), ws.data_ptr(),
                                    nbytes, st) == -2
    torch.cuda.synchronize()
    assert all((t == -3).all() for t in (feat, bad, dist, nv, out, cost, ws))
