"""CPU: the numpy restatement of scenario reduction (tests/reduction_np.py) against brute force and answers worked out by hand; the
argument checks of pr_disagg_radar_gan_amd/reduction.py and of the C entries; header against _lib.py and the kernel's constants."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _hourly, _lib, reduction as RD
from tests import reduction_np as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_dist(rng, S, top):
    """a symmetric matrix with a zero diagonal and entries below top"""
    a = rng.integers(0, top, (S, S)).astype(np.int64)
    d = np.triu(a, 1)
    return d + d.T


def total(dist, picks):
    return int(np.asarray(dist)[list(picks)].min(axis=0).sum())


def test_first_pick_is_the_argmin_of_the_row_sums():
    rng = np.random.default_rng(0)
    for n in range(50):
        S = int(rng.integers(1, 13))
        d = random_dist(rng, S, int(rng.integers(1, 6)))                                  # small values: ties
        chosen, cost = rn.select(d, 1)
        sums = d.sum(axis=1)
        assert chosen[0] == int(np.argmin(sums)) and cost[0] == sums.min(), n             # (argmin: the first of equals)


def test_every_step_is_the_exhaustive_minimum_and_prefixes_nest():
    rng = np.random.default_rng(1)
    for n in range(40):
        S = int(rng.integers(1, 13))
        d = random_dist(rng, S, int(rng.integers(1, 8)) if n % 2 else 1000)
        chosen, cost = rn.select(d, S)
        fast = rn.select_fast(d, S)
        assert np.array_equal(chosen, fast[0]) and np.array_equal(cost, fast[1])
        assert sorted(chosen.tolist()) == list(range(S)) and cost[-1] == 0                # every member once; all picked: nothing left
        for t in range(S):
            J = chosen[:t].tolist()
            best = min((total(d, J + [c]), c) for c in range(S) if c not in J)
            assert (int(cost[t]), int(chosen[t])) == best, (n, t)
            assert total(d, chosen[:t + 1]) == cost[t]
        for k in (1, (S + 1) // 2, S):                                                    # nesting: select(d, k) is a prefix of select(d, S)
            c, z = rn.select(d, k)
            assert np.array_equal(c, chosen[:k]) and np.array_equal(z, cost[:k])
            a, counts = rn.assign(d, c)
            assert counts.sum() == S and len(counts) == k and set(a.tolist()) <= set(c.tolist())
            assert all(d[a[j], j] == d[c, j].min() for j in range(S))


def test_forward_selection_against_all_subsets_of_two():
    """forward selection is greedy, not optimal: its two picks never beat the best pair, and its first pick is the best single"""
    rng = np.random.default_rng(2)
    d = random_dist(rng, 9, 50)
    chosen, cost = rn.select(d, 2)
    best_pair = min(total(d, p) for p in itertools.combinations(range(9), 2))
    assert cost[1] >= best_pair and cost[0] == min(total(d, (u,)) for u in range(9)) and cost[1] <= cost[0]


def test_duplicates_selected_skip_and_count_zero():
    d = random_dist(np.random.default_rng(3), 4, 100) + 1 - np.eye(4, dtype=np.int64)    # distinct members: off-diagonal > 0
    dup = d[np.ix_([0, 1, 1, 2, 3, 1], [0, 1, 1, 2, 3, 1])]                               # members 1, 2 and 5 are the same
    chosen, cost = rn.select(dup, 6)
    assert sorted(chosen.tolist()) == list(range(6))                                      # a selected member is never picked again
    assert cost[3] == 0 and not cost[3:].any()                                            # four distinct members: then nothing is left
    a, counts = rn.assign(dup, chosen)
    assert counts.sum() == 6
    first = min(t for t, u in enumerate(chosen) if u in (1, 2, 5))
    assert chosen[first] == 1 and counts[first] == 3                                      # ties go to the smaller index ...
    assert all(counts[t] == 0 for t, u in enumerate(chosen) if u in (2, 5))               # ... so its duplicates serve nobody
    assert a[2] == 1 and a[5] == 1 and a[1] == 1


def test_all_equal_distances_and_large_entries():
    S = 7
    d = 5 * (1 - np.eye(S, dtype=np.int64))
    chosen, cost = rn.select(d, S)
    assert chosen.tolist() == list(range(S)) and cost.tolist() == [5 * (S - 1 - t) for t in range(S)]
    a, counts = rn.assign(d, chosen[:3])
    assert a.tolist() == [0, 1, 2, 0, 0, 0, 0] and counts.tolist() == [5, 1, 1]
    big = ((1 << 52) // S - 1) * (1 - np.eye(S, dtype=np.int64))
    big[0, 1] = big[1, 0] = big[0, 1] - 1
    chosen, cost = rn.select(big, 2)
    # (the second pick is 2, not 1: member 1 is the one member 0 already serves a little better)
    assert chosen.tolist() == [0, 2] and cost[0] == (S - 1) * ((1 << 52) // S - 1) - 1 and (int(cost[0]) << 12 | 6) < 1 << 64
    assert np.array_equal(rn.select_fast(big, 2)[0], chosen) and np.array_equal(rn.select_fast(big, 2)[1], cost)


def test_pooled_feature_rounding_at_rim_blocks():
    x = np.zeros((1, 24, 5, 7), np.float32)
    x[0, 0] = np.arange(35, dtype=np.float32).reshape(5, 7) / 32                           # e = 0 .. 34, row-major
    feat, bad = rn.features(x, 1)
    assert feat.shape == (1, 24 * 35) and feat[0, :35].tolist() == list(range(35)) and not bad.any()
    f2, _ = rn.features(x, 2)                                                             # 3 x 4 blocks; the last row and column are rims
    assert f2.shape == (1, 24 * 12)
    e = np.arange(35).reshape(5, 7)
    assert f2[0, 0] == (0 + 1 + 7 + 8 + 2) // 4 and f2[0, 3] == (6 + 13 + 1) // 2          # a full block; the right rim: n = 2
    assert f2[0, 8] == (28 + 29 + 1) // 2 and f2[0, 11] == 34                              # the bottom rim: n = 2; the corner: n = 1
    f4, _ = rn.features(x, 4)                                                             # 2 x 2 blocks of 16, 12, 4 and 3 pixels
    assert f4[0, :4].tolist() == [(int(e[:4, :4].sum()) + 8) // 16, (int(e[:4, 4:].sum()) + 6) // 12, (28 + 29 + 30 + 31 + 2) // 4, (32 + 33 + 34 + 1) // 3]
    f8, _ = rn.features(x, 8)                                                             # one block of 35 pixels
    assert f8.shape == (1, 24) and f8[0, 0] == (595 + 17) // 35 == 17
    # the half rounds up in the pooled mean (n / 2 is added), the pixel value rounds to even
    y = np.zeros((1, 24, 2, 2), np.float32)
    y[0, 0] = [[1 / 32, 0], [1 / 32, 0]]                                                  # sum 2 over 4: (2 + 2) // 4 = 1
    y[0, 1] = [[1 / 32, 0], [0, 0]]                                                       # sum 1 over 4: (1 + 2) // 4 = 0
    y[0, 2] = [[0.015625, 0.046875], [0.078125, 2047.99]]                                 # 0, 2, 2 and the clamp 65535
    y[0, 3] = [[np.nan, 5], [5, 5]]
    fy, by = rn.features(y, 2)
    assert fy[0, :4].tolist() == [1, 0, (0 + 2 + 2 + 65535 + 2) // 4, 0] and by[0, :4].tolist() == [False, False, False, True]
    fy1, by1 = rn.features(y, 1)
    assert fy1[0, 8:12].tolist() == [0, 2, 2, 65535] and by1[0, 12:16].tolist() == [True, False, False, False]


def test_mask_is_order_free_and_distances_by_hand():
    feat = np.array([[1, 2, 3, 4], [10, 0, 0, 65535], [1, 2, 9, 0]], np.uint16)
    bad = np.zeros((3, 4), bool)
    bad[2, 3] = True                                                                      # the last member masks position 3 for all
    d, nv = rn.distances(feat, bad)
    assert nv == 3 and d.tolist() == [[0, 14, 6], [14, 0, 20], [6, 20, 0]]
    d2, nv2 = rn.distances(feat[::-1], bad[::-1])
    assert nv2 == 3 and np.array_equal(d2, d[::-1, ::-1])
    d3, _ = rn.distances_fast(feat, bad.any(axis=0))
    assert np.array_equal(d3, d) and np.array_equal(d, d.T) and not np.diagonal(d).any()
    d4, nv4 = rn.distances(feat, np.zeros(4, bool))
    assert nv4 == 4 and d4[0, 1] == 14 + 65531


class NoDevice(RD.ScenarioFeatures):
    """a ScenarioFeatures as far as the host checks go: S members of a pinned shape, nothing on a device"""

    def __init__(self, S=3, shape=(2, 24, 3, 4), **kw):
        super().__init__(**kw)
        self.n_members, self.member_shape, self.device = S, shape, torch.device("cpu")


def test_argument_errors():
    for pool in (0, 3, 16, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError):
            RD.ScenarioFeatures(pool=pool)
        with pytest.raises(ValueError):
            RD.reduce_hourly(np.zeros((2, 24, 3, 4), np.float32), 1, pool=pool)
    for most in (0, -1, 1.5, None):
        with pytest.raises(ValueError):
            RD.ScenarioFeatures(max_feature_bytes=most)
    f = RD.ScenarioFeatures(pool=4)
    assert (f.pool, f.n_members, f.max_feature_bytes) == (4, 0, 8 << 30)
    for bad in (np.zeros((24, 3, 4)), np.zeros((2, 2, 2, 24, 3, 4)), np.zeros((2, 23, 3, 4)), np.zeros((0, 24, 3, 4)), torch.zeros(2, 24, 3, 4),
                np.zeros((2, 24, 3, 4), dtype=complex), np.broadcast_to(np.float32(0), (4097, 24, 1, 1))):
        with pytest.raises(ValueError):                                                   # (among them: a torch tensor on the host)
            RD.ScenarioFeatures().add(bad)
    pinned = NoDevice()
    for bad in (np.zeros((2, 2, 24, 3, 5), np.float32), np.zeros((2, 3, 24, 3, 4), np.float32), np.zeros((2, 24, 3, 4), np.float32),
                np.broadcast_to(np.float32(0), (4094, 2, 24, 3, 4))):
        with pytest.raises(ValueError):                                                   # another plane, other days, no day axis, 3 + 4094 members
            pinned.add(bad)
    # the 2^52 bound: Pf 65535 S < 2^52.  4096 members of a (700, 24, 1024, 1024) day hold 1.76e10 positions each
    with pytest.raises(ValueError, match="2\\^52"):
        NoDevice(S=4095, shape=(700, 24, 1024, 1024)).add(np.broadcast_to(np.float32(0), (1, 700, 24, 1024, 1024)))
    RD.check_admission(1, (1 << 52) // 65535, 1 << 62)
    with pytest.raises(ValueError, match="2\\^52"):
        RD.check_admission(1, (1 << 52) // 65535 + 1, 1 << 62)
    with pytest.raises(ValueError, match="2\\^52"):
        RD.check_admission(4096, (1 << 40) // 65535 + 1, 1 << 62)
    # max_feature_bytes: 2 bytes per member and padded position; 24 * 3 * 4 = 288 positions
    with pytest.raises(ValueError, match="max_feature_bytes"):
        RD.ScenarioFeatures(max_feature_bytes=2 * 5 * 288 - 1).add(np.zeros((5, 24, 3, 4), np.float32))
    with pytest.raises(ValueError, match="max_feature_bytes"):
        NoDevice(S=3, shape=(24, 3, 4), max_feature_bytes=2 * 5 * 288 - 1).add(np.zeros((2, 24, 3, 4), np.float32))
    with pytest.raises(ValueError, match="max_feature_bytes"):
        RD.reduce_hourly(np.zeros((5, 24, 3, 4), np.float32), 2, max_feature_bytes=100)
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: no CPU fallback
        with pytest.raises(_lib.RdganError):
            RD.ScenarioFeatures().add(np.zeros((2, 24, 3, 4), np.float32))
        with pytest.raises(_lib.RdganError):
            RD.ScenarioFeatures(max_feature_bytes=2 * 5 * 288).add(np.zeros((5, 24, 3, 4), np.float32))
    for args in ((None,), (RD.ScenarioFeatures(),), (NoDevice(), 0), (NoDevice(), 1.5), (NoDevice(), True)):
        with pytest.raises(ValueError):
            RD.member_distances(*args)
    ok = torch.zeros((3, 3), dtype=torch.int64)
    for dist, k in ((ok, 1), (np.zeros((3, 3), np.int64), 1), (torch.zeros((3, 3)), 1), (torch.zeros((3, 4), dtype=torch.int64), 1),
                    (torch.zeros((1, 3, 3), dtype=torch.int64), 1), (torch.zeros((0, 0), dtype=torch.int64), 1),
                    (torch.zeros((1, 1), dtype=torch.int64).expand(4097, 4097), 1)):
        with pytest.raises(ValueError):                                                   # (the first: int64 and square, but on the host)
            RD.select(dist, k)
    for k in (0, 4, -1, 1.0, True, None):                                                 # k out of range: before the device
        with pytest.raises(ValueError, match="k must be"):
            RD.select(torch.zeros((3, 3), dtype=torch.int64, device="meta"), k)
        with pytest.raises(ValueError, match="k must be"):
            RD.reduce_hourly(np.zeros((3, 24, 3, 4), np.float32), k)

    class Gen:
        ndomain, n_cond_channels = 16, 1

    for kw in (dict(daily=np.zeros((8, 20))), dict(n_scenarios=0), dict(n_scenarios=4097), dict(scenario_chunk=0), dict(k=0), dict(k=4), dict(k=1.0),
               dict(pool=3), dict(latent_mode="none"), dict(max_feature_bytes=100), dict(latent=np.zeros((3, 2, 100)))):
        with pytest.raises(ValueError):
            RD.reduce_field(**{**dict(gen=Gen(), daily=np.zeros((20, 20)), n_scenarios=3, k=2), **kw})


def test_reduction_prefix_weights_and_curve():
    rng = np.random.default_rng(5)
    S = 9
    d = random_dist(rng, S, 1000)
    chosen, cost = rn.select(d, 5)
    a, counts = rn.assign(d, chosen)
    r = RD.Reduction(chosen, cost, a, counts, d[chosen], S, n_valid=10)
    assert np.allclose(r.weights, counts / S) and r.weights.sum() == pytest.approx(1.0)
    assert np.allclose(r.mean_distance_mm, cost / (32.0 * S * 10)) and np.isnan(RD.Reduction(chosen, cost, a, counts, d[chosen], S).mean_distance_mm).all()
    for k in (1, 3, 5):
        p = r.prefix(k)
        want_a, want_c = rn.assign(d, chosen[:k])
        assert np.array_equal(p.chosen, chosen[:k]) and np.array_equal(p.cost, cost[:k]) and np.array_equal(p.assign, want_a)
        assert np.array_equal(p.counts, want_c) and p.counts.sum() == S and p.assign.dtype == np.int32 and p.counts.dtype == np.int32
    for k in (0, 6, 1.0):
        with pytest.raises(ValueError):
            r.prefix(k)


def test_cabi_argument_checks():
    """the four C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    ws = lib.rdgan_red_workspace_bytes
    assert ws(1, 1) == 24 and ws(100, 20) == 800 + 160 + 104 and ws(4096, 4096) == 2 * 8 * 4096 + 4096 and ws(3, 2) == 24 + 16 + 8
    for a in ((0, 1), (4097, 1), (1, 0), (3, 4), (-1, -1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # 16-byte aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)

    def features(x=good, n=3, stride=2 * 24 * 15, D=2, ny=3, nx=5, pool=1, f=good, fstride=720, bad=good):
        return lib.rdgan_red_features(x, n, stride, D, ny, nx, pool, f, fstride, bad, st)

    for kw in (dict(x=null), dict(f=null), dict(bad=null), dict(x=by(2)), dict(f=by(8)), dict(bad=by(2)), dict(n=0), dict(n=4097), dict(D=0), dict(ny=0),
               dict(nx=0), dict(ny=4097, nx=4096, stride=2 * 24 * 4097 * 4096), dict(stride=2 * 24 * 15 - 1), dict(pool=0), dict(pool=3), dict(pool=16),
               dict(pool=-1), dict(fstride=712), dict(fstride=724), dict(pool=2, fstride=184), dict(n=4096, D=700, ny=1024, nx=1024, stride=700 * 24 << 20, fstride=700 * 24 << 20)):
        assert features(**kw) == -2, kw

    def distances(f=good, bad=good, S=3, fstride=720, pf=720, splits=0, d=good, nv=good):
        return lib.rdgan_red_distances(f, bad, S, fstride, pf, splits, d, nv, st)

    for kw in (dict(f=null), dict(bad=null), dict(d=null), dict(nv=null), dict(f=by(8)), dict(bad=by(2)), dict(d=by(4)), dict(nv=by(4)), dict(S=0), dict(S=4097),
               dict(pf=0), dict(pf=721), dict(fstride=716), dict(splits=-1), dict(S=1, pf=(1 << 52) // 65535 + 1, fstride=1 << 40),
               dict(S=4096, pf=(1 << 40) // 65535 + 1, fstride=1 << 30)):
        assert distances(**kw) == -2, kw

    def select(d=good, S=5, k=2, chosen=good, cost=good, assign=good, counts=good, w=good, nbytes=40 + 16 + 8):
        return lib.rdgan_red_select(d, S, k, chosen, cost, assign, counts, w, nbytes, st)

    for kw in (dict(d=null), dict(chosen=null), dict(cost=null), dict(assign=null), dict(counts=null), dict(w=null), dict(d=by(4)), dict(cost=by(4)),
               dict(w=by(4)), dict(chosen=by(2)), dict(assign=by(2)), dict(counts=by(2)), dict(S=0), dict(S=4097, nbytes=1 << 30), dict(k=0), dict(k=6, nbytes=1 << 20),
               dict(k=-1), dict(nbytes=63), dict(nbytes=0), dict(nbytes=-8)):
        assert select(**kw) == -2, kw


def test_header_and_lib_agree_on_the_reduction_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "int*": "c_void_p", "long long*": "c_void_p",
             "const long long*": "c_void_p", "unsigned short*": "c_void_p", "const unsigned short*": "c_void_p", "unsigned int*": "c_void_p",
             "const unsigned int*": "c_void_p"}
    names = ("rdgan_red_workspace_bytes", "rdgan_red_features", "rdgan_red_distances", "rdgan_red_select")
    assert tuple(sorted(n for n in _lib.SIGNATURES if n.startswith("rdgan_red_"))) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_red_\w+)\(", header, re.M)))) == tuple(sorted(names))
    lib = _lib.load()
    for name in names:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)


def test_python_constants_are_the_kernel_header_s():
    csrc = os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc")
    text = "".join(open(os.path.join(csrc, h)).read() for h in ("rdgan_reduce.hip.h", "rdgan_sequence.hip.h", "rdgan_hourly_host.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert value("RD_SEQ_MAXS") == RD.MAX_MEMBERS == _hourly.MAX_MEMBERS == rn.MAX_MEMBERS == 1 << (64 - RD.KEY_BITS)
    assert (RD.UNIT, RD.FEATMAX, RD.KEY_BITS, max(RD.POOLS)) == (value("RD_SEQ_UNIT"), value("RD_SEQ_FEATMAX"), value("RD_RED_KEYBITS"), value("RD_RED_MAXPOOL"))
    assert (rn.UNIT, rn.FEATMAX, rn.MAX_DEPTH) == (RD.UNIT, RD.FEATMAX, value("RD_DEPTH_MAX"))
    assert RD.MAX_PLANE == value("RD_HOURLY_MAXPLANE") and RD.MAX_ELEMS == value("RD_HOURLY_MAXELEMS")
    # a pooled sum of 64 clamped features and the rounding term fit 32 bits; a selection workgroup's m fits LDS
    assert max(RD.POOLS) ** 2 * RD.FEATMAX + 32 < 2 ** 32 and RD.MAX_MEMBERS * 8 <= 64 << 10
    assert [RD.padded_positions(p) for p in (1, 8, 9, 35)] == [8, 8, 16, 40] and [RD.bad_words(p) for p in (1, 32, 33, 70000)] == [1, 1, 2, 2188]
    assert RD.n_positions((24, 5, 7), 1) == 840 and RD.n_positions((2, 24, 5, 7), 2) == 2 * 24 * 12 and RD.n_positions((24, 5, 7), 8) == 24
