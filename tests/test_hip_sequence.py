"""-m gpu: chaining scenarios across midnight (csrc/rdgan_sequence.hip.h, pr_disagg_radar_gan_amd/sequence.py) against the numpy
restatement (tests/sequence_np.py, itself checked on the CPU by tests/test_sequence_host.py).  Everything is an integer: every
comparison is an equality."""
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, models, sequence as SQ, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import sequence_np as sn
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


def edges_of(feat, bad, first_hour=0, last_hour=23):
    """a SeamEdges holding the given features (S, D, 2, P) uint16 and bad bits (D, 2, P), without an hourly array behind it"""
    S, D, _, P = feat.shape
    e = SQ.SeamEdges(first_hour, last_hour)
    e.lib, e.device, e.n_members, e.n_days, e.plane_shape = _lib.load(), torch.device("cuda", torch.cuda.current_device()), S, D, (1, P)
    f = np.zeros((S, D, 2, SQ.padded_plane(P)), np.uint16)
    f[..., :P] = feat
    bits = np.zeros((D, 2, SQ.bad_words(P) * 32), np.uint64)
    bits[..., :P] = bad
    words = (bits.reshape(D, 2, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    e._chunks = [torch.from_numpy(f.view(np.int16)).cuda()]
    e.bad = torch.from_numpy(words.view(np.int32)).cuda()
    return e


@functools.lru_cache(maxsize=None)
def random_features(S, D, P, seed, top=65536):
    """shared: copy before writing"""
    rng = np.random.default_rng(seed)
    feat = rng.integers(0, top, (S, D, 2, P)).astype(np.uint16)
    return feat, np.zeros((D, 2, P), bool)


def check_costs(feat_a, bad_a, shift=1, feat_b=None, bad_b=None, splits=(None,)):
    """the costs against the mirror, once per way of cutting the pixels into ranges (None: the entry's own choice)"""
    want, want_valid = sn.seam_costs(feat_a, bad_a, shift, feat_b, bad_b)
    other = None if feat_b is None else edges_of(feat_b, bad_b)
    for pixel_splits in splits:
        costs, n_valid = SQ.seam_costs(edges_of(feat_a, bad_a), shift, other, pixel_splits=pixel_splits)
        assert costs.dtype == torch.int64 and n_valid.dtype == torch.int64 and eq(costs, want) and eq(n_valid, want_valid), pixel_splits
    return want, want_valid


# ---------------------------------------------------------------------------------------------------------------------------------
def edge_case_array():
    """(2, 3, 24, 5, 7): roundings on .5 with an even and an odd neighbour, the clamp, the four kinds of bad value"""
    rng = np.random.default_rng(3)
    x = (rng.gamma(0.6, 3.0, (2, 3, 24, 5, 7)) * (rng.random((2, 3, 24, 5, 7)) < 0.6)).astype(np.float32)
    x[0, 0, 0, 0, :6] = (0.015625, 0.046875, 0.078125, 0.109375, 2047.99, 2047.0)         # .5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, the clamp
    x[1, 0, 0, 1, :4] = (np.nan, -1.0, np.inf, 2048.0)
    x[0, 2, 23, 4, 6] = -np.inf
    x[1, 1, 23, 2, 3] = np.nan
    x[0, 1, 5, 2, 2] = np.nan                                                             # not an edge hour: must not be seen
    return x


def test_edges_rounding_clamp_and_bad_values():
    x = edge_case_array()
    feat, bad = sn.edge_features(x)
    assert feat[0, 0, 0, :6].tolist() == [0, 2, 2, 4, 65535, 65504] and bad.sum() == 6 and bad[0, 0, 7:11].all() and not feat[1, 0, 0, 7:11].any()
    e = SQ.SeamEdges().add(dev(x))
    assert e.features.dtype == torch.uint16 and tuple(e.features.shape) == (2, 3, 2, 40) and tuple(e.bad.shape) == (3, 2, 2)
    assert eq(e.features[..., :35], feat) and not host(e.features[..., 35:]).any() and eq(e.bad_mask(), bad)
    assert (e.n_members, e.n_days, e.plane_shape) == (2, 3, (5, 7))
    for hours in ((11, 12), (23, 0), (5, 5)):
        e = SQ.SeamEdges(*hours).add(x)                                                   # numpy in
        feat, bad = sn.edge_features(x, *hours)
        assert eq(e.features[..., :35], feat) and eq(e.bad_mask(), bad), hours


def test_edges_strided_views_and_two_adds_equal_one():
    x = edge_case_array()
    feat, bad = sn.edge_features(x)
    whole = SQ.SeamEdges().add(dev(x))
    two = SQ.SeamEdges().add(dev(x[:1])).add(dev(x[1]))                                   # (5-d, then one member as 4-d)
    assert np.array_equal(host(two.features), host(whole.features)) and torch.equal(two.bad, whole.bad) and two.n_members == 2
    assert eq(two.features[..., :35], feat) and eq(two.bad_mask(), bad)
    # a leading axis with a stride wider than a day: days as a view of a wider buffer (one member), on the scalar route
    wide = torch.full((3, 24 * 35 + 13), float("nan"), device="cuda")
    wide[:, :24 * 35] = dev(x[1]).reshape(3, -1)
    view = wide[:, :24 * 35].view(3, 24, 5, 7)
    assert view.stride(0) == 24 * 35 + 13
    e = SQ.SeamEdges().add(view)
    f1, b1 = sn.edge_features(x[1:])
    assert eq(e.features[..., :35], f1) and eq(e.bad_mask(), b1)
    # the 16-byte route: a plane of 8 x 8 and an aligned, wider stride
    y = np.random.default_rng(5).gamma(0.7, 2.0, (4, 2, 24, 8, 8)).astype(np.float32)
    y[2, 1, 23, 7, 7] = 2048.0
    wide = torch.zeros((8, 24 * 64 + 16), device="cuda")
    wide[:, :24 * 64] = dev(y).reshape(8, -1)
    e = SQ.SeamEdges().add(wide[:, :24 * 64].view(8, 24, 8, 8)[:2]).add(wide[:, :24 * 64].view(8, 24, 8, 8)[2:].view(3, 2, 24, 8, 8))
    f2, b2 = sn.edge_features(y)
    assert eq(e.features, f2) and eq(e.bad_mask(), b2) and b2.sum() == 1 and e.n_members == 4


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (63, 63, 7), (64, 64, 1), (65, 65, 7), (5, 3, 4099)])
def test_costs_shapes(shape):
    Sa, Sb, P = shape
    fa, bad = random_features(Sa, 3, P, 11)
    if Sa == Sb:
        check_costs(fa, bad)
    else:
        fb, _ = random_features(Sb, 3, P, 12)
        check_costs(fa, bad, 1, fb, bad)


def test_costs_past_32_bits():
    """P = 70 000 with 65535 against 0: 4 587 450 000 > 2^32.  The chunk loop of k_seq_costs adds its 32-bit sums to 64-bit ones every
    256 chunks of 128 pixels; with pixel_splits=1 one workgroup walks all 547 chunks, 70 000 x 65535 wraps a 32-bit sum that is never
    flushed (or flushed after more than 512 chunks), and the answer is known in closed form.  With 2 ranges a workgroup walks 274
    chunks and meets one flush; left to the entry (547 ranges of one chunk) the total is formed by the 64-bit atomics alone."""
    P = 70000
    feat = np.zeros((2, 2, 2, P), np.uint16)
    feat[0, 0, 1] = 65535
    feat[1, 0, 1, ::2] = 65535
    e = edges_of(feat, np.zeros((2, 2, P), bool))
    for pixel_splits in (1, 2, None):
        costs, n_valid = SQ.seam_costs(e, pixel_splits=pixel_splits)
        assert costs.cpu().tolist() == [[[4587450000, 4587450000], [2293725000, 2293725000]]] and n_valid.cpu().tolist() == [P], pixel_splits


def test_costs_many_chunks_in_one_workgroup():
    """the chunk loop itself -- the barrier before LDS is overwritten, the prefetch of the next chunk, the panels reused: random
    features and masks on both sides over 33 chunks (P = 4099) walked by 1, 2, 5 and 33 workgroups, more ranges asked for than there
    are chunks, and two tiles of rows over 8 chunks in one workgroup each"""
    rng = np.random.default_rng(17)
    fa, fb = random_features(3, 3, 4099, 15)[0], random_features(5, 3, 4099, 16)[0]
    bad_a, bad_b = rng.random((3, 2, 4099)) < 0.1, rng.random((3, 2, 4099)) < 0.1
    want, nv = check_costs(fa, bad_a, 1, fb, bad_b, splits=(1, 2, 5, 33, 1000, None))
    assert 0 < nv.min() and nv.max() < 4099 and want.min() > 0
    check_costs(fa, bad_a, 0, splits=(1, 3))
    f65 = random_features(65, 2, 1000, 18)[0]
    check_costs(f65, rng.random((2, 2, 1000)) < 0.05, splits=(1, None))


def test_costs_masks_identical_members_other_and_shift():
    feat, _ = random_features(5, 4, 300, 13)
    feat = feat.copy()
    feat[3] = feat[1]                                                                     # identical members: exactly 0 apart at shift 0 below
    feat[:, :, 1] = np.where(np.arange(300) % 3 == 0, feat[:, :, 0], feat[:, :, 1])
    bad = np.zeros((4, 2, 300), bool)
    bad[0, 1, 5:40] = True                                                                # the row side of boundary 0
    bad[1, 0, 30:77] = True                                                               # its column side, overlapping
    bad[2, 1, :] = True                                                                   # boundary 2 whole
    want, nv = check_costs(feat, bad)
    assert nv.tolist() == [300 - 72, 300, 0] and not want[2].any() and want[0].min() > 0
    assert np.array_equal(want[:, 1], want[:, 3]) and np.array_equal(want[:, :, 1], want[:, :, 3])
    w0, nv0 = check_costs(feat, bad, shift=0)                                             # hour pairs within the day
    assert w0.shape == (4, 5, 5) and nv0.tolist() == [300 - 35, 300 - 47, 0, 300]
    same = feat.copy()
    same[:, :, 1] = same[:, :, 0]
    ws, _ = check_costs(same, bad, shift=0)
    assert not np.diagonal(ws, axis1=1, axis2=2).any() and ws[0, 1, 3] == 0 and ws[0, 0, 1] > 0
    obs, _ = random_features(1, 4, 300, 14)                                               # observed days: an ensemble of one member
    obs_bad = np.zeros((4, 2, 300), bool)
    obs_bad[2, 0, 299] = obs_bad[1, 1, 0] = True                                          # its column side at boundary 1, its row side there
    wo, nvo = check_costs(feat, bad, 1, obs, obs_bad)
    assert wo.shape == (3, 5, 1) and nvo.tolist() == [300 - 35, 299, 0]
    wo, nvo = check_costs(obs, obs_bad, 1, feat, bad)
    assert wo.shape == (3, 1, 5) and nvo.tolist() == [300 - 47, 299, 300]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 65])
def test_min_plus_against_the_mirror(S):
    rng = np.random.default_rng(S)
    C = rng.integers(0, 4, (5, S, S)).astype(np.int64)                                    # values 0 .. 3: ties everywhere
    acc, back = SQ.min_plus(dev(C, torch.int64))
    want_acc, want_back = sn.min_plus(C)
    assert acc.dtype == torch.int64 and back.dtype == torch.int32 and eq(acc, want_acc) and eq(back, want_back)
    path, total = SQ.best_path(dev(C, torch.int64))
    want_path, want_total = sn.best_path(C)
    assert path.tolist() == want_path.tolist() and total == want_total and isinstance(total, int)


def test_min_plus_ties_and_costs_near_2_40():
    C = np.array([[[5, 1, 1], [5, 1, 0], [4, 1, 1]], [[2, 2, 9], [2, 2, 9], [0, 1, 9]]], np.int64)
    _, back = SQ.min_plus(dev(C, torch.int64))
    assert back.cpu().tolist() == [[2, 0, 1], [2, 2, 2]]                                  # three equal in column 1: the smallest i
    path, total = SQ.best_path(dev(np.zeros((3, 70, 70), np.int64), torch.int64))
    assert path.tolist() == [0, 0, 0, 0] and total == 0                                   # the smaller end member, the smaller i
    big = np.full((8, 5, 5), (1 << 40) - 1, np.int64)
    big[:, 3, 3] -= 1
    big[:, 4, 4] -= 1
    path, total = SQ.best_path(dev(big, torch.int64))
    assert path.tolist() == [3] * 9 and total == 8 * ((1 << 40) - 2) and sn.best_path(big)[0].tolist() == [3] * 9


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 65, 130])
def test_matching_with_many_ties(S):
    C = np.random.default_rng(S).integers(0, 4, (3, S, S)).astype(np.int64)
    perm, rounds = SQ.greedy_matching(dev(C, torch.int64), return_rounds=True)
    assert perm.dtype == torch.int32 and eq(perm, sn.greedy_matching(C)) and 1 <= rounds <= S
    assert all(sorted(row) == list(range(S)) for row in perm.cpu().tolist())


def test_matching_constant_matrix_worst_case_rounds_and_idle_rounds():
    perm, rounds = SQ.greedy_matching(torch.full((2, 70, 70), 7, dtype=torch.int64, device="cuda"), return_rounds=True)
    assert perm.cpu().tolist() == [list(range(70))] * 2 and rounds == 70                  # a constant matrix: the identity, a pair a round
    S = 64
    ij = np.add.outer(np.arange(S), np.arange(S)).astype(np.int64)
    assert sn.greedy_rounds(ij)[1] == S                                                   # one pair a round
    shifted = np.where((np.arange(S)[None, :] - np.arange(S)[:, None]) % S == 1, 0, (1 << 40) - 1).astype(np.int64)
    assert sn.greedy_rounds(shifted)[1] == 1                                              # every row's minimum is its column's: one round
    C = dev(np.stack([ij, shifted]), torch.int64)                                         # the second is complete at once and idles
    perm, rounds = SQ.greedy_matching(C, return_rounds=True)
    assert perm.cpu().tolist() == [list(range(S)), [(i + 1) % S for i in range(S)]] and rounds == S
    # the entry itself: S - 1 rounds leave exactly one row free, one more completes it, further rounds change nothing
    lib = _lib.load()
    nbytes = lib.rdgan_seq_workspace_bytes(S, 2)
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda")
    out = torch.full((2, S), -7, dtype=torch.int32, device="cuda")
    free = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    call = lambda init, n: lib.rdgan_seq_match(C.data_ptr(), 2, S, init, n, out.data_ptr(), free.data_ptr(), ws.data_ptr(), nbytes,
                                               torch.cuda.current_stream().cuda_stream)
    assert call(1, S - 1) == 0 and free.cpu().tolist() == [1, 0] and out[0].cpu().tolist() == list(range(S - 1)) + [-1]
    assert call(0, 1) == 0 and free.cpu().tolist() == [0, 0] and torch.equal(out, perm)
    assert call(0, 5) == 0 and free.cpu().tolist() == [0, 0] and torch.equal(out, perm)
    assert call(1, 0) == 0 and free.cpu().tolist() == [S, S] and (out == -1).all()          # init alone


# ---------------------------------------------------------------------------------------------------------------------------------
def planted(S=8, D=4, ny=6, nx=6, seed=7):
    """distinct random fields; day d + 1's member pi_d(s) starts with exactly the field day d's member s ends with"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(1, 2000, (S, D, 24, ny, nx)) / 32.0).astype(np.float32)              # exact in 1/32 mm, all distinct fields
    pis = [rng.permutation(S) for _ in range(D - 1)]
    for d, pi in enumerate(pis):
        x[pi, d + 1, 0] = x[np.arange(S), d, 23]
    return x, np.stack(pis)


def test_planted_series_are_recovered():
    x, pis = planted()
    S, D = x.shape[:2]
    xd = dev(x)
    r = SQ.chain(xd)
    assert np.array_equal(r.perm, pis) and r.perm.dtype == np.int32 and np.array_equal(r.order, sn.series_order(pis))
    assert not r.matched.any() and r.path_total == 0 and not r.path_cost.any() and r.n_valid.tolist() == [36] * (D - 1)
    assert all(r.path[d + 1] == pis[d][r.path[d]] for d in range(D - 1)) and r.path[-1] == 0
    assert (r.random > 0).all() and (r.diagonal > 0).all()
    series = SQ.reorder(xd, r.order)
    assert torch.equal(series[:, :-1, 23], series[:, 1:, 0])                              # hour 23 is the next day's hour 0
    assert np.array_equal(series.cpu().numpy(), sn.reorder(x, r.order))
    assert all(sorted(row) == list(range(S)) for row in r.order.tolist())
    # the statistics against the mirror's costs, in mm/h per valid pixel
    feat, bad = sn.edge_features(x)
    C, nv = sn.seam_costs(feat, bad)
    assert np.allclose(r.random, C.mean(axis=(1, 2)) / (32 * nv), rtol=1e-12)
    assert np.allclose(r.diagonal, np.diagonal(C, axis1=1, axis2=2).mean(axis=1) / (32 * nv), rtol=1e-12)
    # reorder on another per-member, per-day tensor: here the members' own indices
    tags = torch.arange(S, device="cuda")[:, None].expand(S, D).contiguous()
    assert np.array_equal(SQ.reorder(tags, r.order).cpu().numpy().T, r.order)
    # observed days: the first series itself, so its seams cost 0; days 1 -> 2 declared not consecutive
    c = SQ.compare(r, series[0], consecutive=[True, False, True])
    assert c.observed[0] == 0 and np.isnan(c.observed[1]) and c.observed[2] == 0 and c.observed_within.shape == (D,)
    f11, b11 = sn.edge_features(series[0].cpu().numpy()[None], first_hour=12, last_hour=11)
    cw, nw = sn.seam_costs(f11, b11, shift=0)
    assert np.allclose(c.observed_within, cw[:, 0, 0] / (32 * nw), rtol=1e-12) and (c.observed_within > 0).all() and c.matched is r.matched


def test_fully_masked_boundary_gives_nan_statistics():
    x, _ = planted(S=3, D=3)
    x[1, 1, 23] = np.nan                                                                  # every pixel of boundary 1 is bad for one member
    r = SQ.chain(x)
    assert r.n_valid.tolist() == [36, 0] and np.isnan(r.random[1]) and np.isnan(r.matched[1]) and r.matched[0] == 0
    assert r.perm[1].tolist() == [0, 1, 2]                                                # all costs 0: the identity


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in ("order", "perm", "path", "n_valid", "random", "diagonal",
                                                                                       "matched", "path_cost")) and a.path_total == b.path_total


def test_chain_field_equals_chain_of_disaggregate(generator, monkeypatch):
    """3 wet days of a 20 x 24 plane at ndomain 16, overlap 4, 4 scenarios; `chunk` is one unit's tiles on both sides (every tile of
    every day is wet), the batching for which evaluate_field promises equal values"""
    S, D = 4, 3
    rng = np.random.default_rng(41)
    daily = (0.1 + rng.gamma(0.8, 6.0, (D, 20, 24))).astype(np.float32)
    daily[1, 3, 5] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(42).normal(size=(S, D, 100)).astype(np.float32)
    info = F.disaggregate(generator, dd, 1, latent=z[:1])[1]
    assert info.n_active == D * info.n_tiles and info.n_nan_pixels == 1
    hourly, _ = F.disaggregate(generator, dd, S, latent=z, chunk=info.n_tiles)
    want = SQ.chain(hourly)
    feat, bad = sn.edge_features(hourly.cpu().numpy())
    C, nv = sn.seam_costs(feat, bad)
    assert nv.tolist() == [20 * 24 - 1] * 2 and np.array_equal(want.perm, sn.greedy_matching(C)) and want.path.tolist() == sn.best_path(C)[0].tolist()
    for scenario_chunk in (1, 3, 4):
        got = SQ.chain_field(generator, dd if scenario_chunk == 3 else daily, S, scenario_chunk=scenario_chunk, latent=z, chunk=info.n_tiles)
        assert same(got, want), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.chain_scenarios_field(daily, S, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert same(a, SQ.chain(hourly2))


def test_c_entries_refuse_bad_arguments_and_touch_nothing():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x = dev(edge_case_array())
    feat = torch.full((2, 3, 2, 40), -3, dtype=torch.int16, device="cuda")
    bad = torch.full((3, 2, 2), -3, dtype=torch.int32, device="cuda")
    for kw in (dict(n=5), dict(stride=24 * 35 - 1), dict(h0=24), dict(h1=-1), dict(D=0)):
        a = {**dict(n=6, stride=24 * 35, D=3, h0=0, h1=23), **kw}
        assert lib.rdgan_seq_edges(x.data_ptr(), a["n"], a["stride"], 5, 7, a["D"], a["h0"], a["h1"], feat.data_ptr(), bad.data_ptr(), st) == -2, kw
    costs = torch.full((2, 2, 2), -3, dtype=torch.int64, device="cuda")
    nv = torch.full((2,), -3, dtype=torch.int64, device="cuda")
    for shift, splits in ((-1, 0), (3, 0), (1, -1)):
        assert lib.rdgan_seq_costs(feat.data_ptr(), bad.data_ptr(), 2, feat.data_ptr(), bad.data_ptr(), 2, 3, 35, shift, splits, costs.data_ptr(),
                                   nv.data_ptr(), st) == -2
    torch.cuda.synchronize()
    assert (feat == -3).all() and (bad == -3).all() and (costs == -3).all() and (nv == -3).all()
