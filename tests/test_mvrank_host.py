"""CPU: the numpy yardstick of the multivariate rank histograms (tests/mvrank_np.py) against answers worked out by hand, against
its identities and against its own calibration on exchangeable and on under-dispersed draws; the argument checks of
pr_disagg_radar_gan_amd/multivariate_ranks.py and of the C entries; header against _lib.py and the kernel header's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, multivariate_ranks as MR, reduction as R
from tests import mvrank_np as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rdgan_mvr_mst", "rdgan_mvr_ranks", "rdgan_mvr_ranks_workspace_bytes")
CHI2_9_999 = 27.88                                                                         # the 99.9 % point of chi-square, 9 dof


def rain(rng, shape, dry=0.6):
    """gamma-distributed amounts with about 60 % zeros"""
    return (rng.gamma(0.5, 4.0, shape) * (rng.random(shape) < 1.0 - dry)).astype(np.float32)


def test_three_vectors_two_positions_with_a_tie():
    """N = 3: position 0 holds (obs, x1, x2) = (1, 1, 5), position 1 holds (2, 0, 1)"""
    obs, ens = np.array([1.0, 2.0], np.float32), np.array([[1.0, 0.0], [5.0, 1.0]], np.float32)
    sums, n_valid = mr.prerank_sums(ens, obs)
    # position 0: lt = (0, 0, 2), gt = (1, 1, 0); position 1: lt = (2, 0, 1), gt = (0, 2, 1); N + 1 = 4, (N - 1)(N - 2) = 2
    assert n_valid == 2
    assert sums[:, 0].tolist() == [(0 - 1 + 4) + (2 - 0 + 4), (0 - 1 + 4) + (0 - 2 + 4), (2 - 0 + 4) + (1 - 1 + 4)]   # 9, 5, 10
    # twice the mid-ranks: position 0 (1.5, 1.5, 3), position 1 (3, 1, 2)
    assert sums[:, 0].tolist() == [2 * 1.5 + 2 * 3, 2 * 1.5 + 2 * 1, 2 * 3 + 2 * 2]
    # depth: position 0: the tied pair each lie in the other's closed interval with x2: (2, 2, 0); position 1: the middle one only
    assert sums[:, 1].tolist() == [2 + 0, 2 + 0, 0 + 2]
    assert mr.observation_ranks(sums[:, 0]) == (1, 0) and mr.observation_ranks(sums[:, 1]) == (0, 2)
    # a NaN of a member leaves the position out for everyone
    ens2 = ens.copy()
    ens2[1, 1] = np.nan
    sums2, n2 = mr.prerank_sums(ens2, obs)
    assert n2 == 1 and sums2.tolist() == [[3, 2], [3, 2], [6, 0]]
    assert mr.prerank_sums(np.full((2, 2), np.inf, np.float32), obs) [1] == 0


def test_band_depth_of_the_median_and_of_an_extreme():
    z = np.arange(7, dtype=np.float32)                                                     # distinct values at one position, N = 7
    sums, _ = mr.prerank_sums(z[1:, None], z[:1])
    depth = sums[:, 1]
    assert depth[3] == 2 * 3 * 3 and depth[0] == 0 and depth[6] == 0                       # the median: 3 below x 3 above pairs, twice
    assert depth.tolist() == [2 * k * (6 - k) for k in range(7)]
    same = np.zeros((7, 1), np.float32)                                                    # all equal: every pair holds everyone
    sums, _ = mr.prerank_sums(same[1:], same[0])
    assert sums[:, 1].tolist() == [6 * 5] * 7 and sums[:, 0].tolist() == [8] * 7


def test_mst_of_four_collinear_points():
    x = np.array([0, 1, 3, 7], np.int64)
    dist = np.abs(x[:, None] - x[None, :])
    assert mr.prim(dist) == 7 and mr.prim_fast(dist) == 7
    # without an end point the tree is the range of the rest; without an inner point the range stays
    assert mr.mst_leave_one_out(dist).tolist() == [6, 7, 7, 3] and mr.mst_leave_one_out(dist, fast=False).tolist() == [6, 7, 7, 3]
    assert mr.mst_leave_one_out(dist[:2, :2]).tolist() == [0, 0] and mr.mst_leave_one_out(dist[:1, :1]).tolist() == [0]
    rng = np.random.default_rng(5)
    pts = rng.integers(0, 4, (9, 6))                                                       # many equal and zero edges
    d = np.abs(pts[:, None] - pts[None, :]).sum(-1)
    assert mr.mst_leave_one_out(d).tolist() == mr.mst_leave_one_out(d, fast=False).tolist()


def test_identities():
    rng = np.random.default_rng(11)
    ens, obs = rain(rng, (8, 24, 3, 5)), rain(rng, (24, 3, 5))
    obs[3, 1, 2] = np.nan
    ens[4, 0, 0, 0] = -np.inf
    sums, n_valid = mr.prerank_sums(ens, obs)
    N = 9
    assert n_valid == 24 * 15 - 2 and sums[:, 0].sum() == n_valid * N * (N + 1)
    neg, n2 = mr.prerank_sums(-ens, -obs)
    assert n2 == n_valid and np.array_equal(neg[:, 1], sums[:, 1])                         # depth: invariant under negation
    assert np.array_equal(neg[:, 0], 2 * (N + 1) * n_valid - sums[:, 0])
    by_hour, nv_hour = mr.prerank_sums_by_hour(ens, obs)
    assert np.array_equal(by_hour.sum(axis=0), sums) and nv_hour.sum() == n_valid
    ens[4, 0, 0, 0] = 0.0
    perm = rng.permutation(8)
    a, na = mr.mst_preranks(ens, obs, pool=2)
    b, nb = mr.mst_preranks(ens[perm], obs, pool=2)
    assert na == nb and a[0] == b[0] and np.array_equal(a[1:][perm], b[1:])
    s1, _ = mr.prerank_sums(ens, obs)
    s2, _ = mr.prerank_sums(ens[perm], obs)
    assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1:][perm], s2[1:])
    # the features are those of the reduction's yardstick
    from tests import reduction_np as rn
    z = np.concatenate([obs[None], ens])
    feat, bad = mr.features(z, 2)
    f2, b2 = rn.features(z, 2)
    assert np.array_equal(feat[:, ~bad], f2.astype(np.int64)[:, ~bad]) and np.array_equal(bad, b2.any(axis=0))


@pytest.fixture(scope="module")
def calibration():
    """600 cases of N = 10 at P = 24 4 4: exchangeable draws, and an ensemble whose spread about its own mean is halved"""
    rng = np.random.default_rng(2)
    out = {"flat": {k: [] for k in MR.KINDS}, "narrow": {k: [] for k in MR.KINDS}}
    for _ in range(600):
        z = rain(rng, (10, 24, 4, 4))
        mean = z[1:].mean(axis=0, dtype=np.float32)
        for name, ens in (("flat", z[1:]), ("narrow", mean + np.float32(0.5) * (z[1:] - mean))):
            sums, _ = mr.prerank_sums(ens, z[0])
            mst, _ = mr.mst_preranks(ens, z[0])
            for k, rho in (("average", sums[:, 0]), ("band_depth", sums[:, 1]), ("mst", mst)):
                out[name][k].append(mr.observation_ranks(rho))
    return {name: {k: tuple(np.array(c) for c in zip(*v)) for k, v in kinds.items()} for name, kinds in out.items()}


def test_reference_is_calibrated_on_exchangeable_draws(calibration):
    for kind in MR.KINDS:
        below, equal = calibration["flat"][kind]
        h = mr.histogram(below, equal, 9, seed=0)
        assert h.sum() == 600 and mr.chi_square(h) < CHI2_9_999, (kind, h)
        res = MR.MultivariateRanks((kind,), 9, {kind: below}, {kind: equal}, {kind: np.full(600, 384)})
        assert np.array_equal(res.histogram(kind, seed=0), h)                              # the module's host side: the same draw
        assert abs(res.reliability_index(kind) - np.abs(h / 600 - 0.1).sum()) < 1e-15


def test_half_spread_shows_in_band_depth_and_mst(calibration):
    below, equal = calibration["narrow"]["band_depth"]
    h = mr.histogram(below, equal, 9, seed=0)
    assert h[0] > 600 / 4, h                                                               # the observation is an outlier too often
    below, equal = calibration["narrow"]["mst"]
    h = mr.histogram(below, equal, 9, seed=0)
    assert h[0] > 600 / 4 and mr.chi_square(h) > CHI2_9_999, h                             # the tree is shortest without the observation


def test_result_object():
    below = {"average": np.array([0, 3, 1, 2]), "mst": np.array([1, 1, 0, 3])}
    equal = {"average": np.array([0, 0, 2, 0]), "mst": np.zeros(4, np.int64)}
    n_valid = {"average": np.array([5, 5, 5, 0]), "mst": np.array([5, 5, 5, 0])}
    res = MR.MultivariateRanks(("average", "mst"), 3, below, equal, n_valid)
    assert res.n_cases("mst") == 3 and res.n_empty("mst") == 1
    assert res.histogram("mst").tolist() == [1, 2, 0, 0] and res.histogram("mst", n_bins=2).tolist() == [3, 0]
    u = np.random.default_rng(7).integers(0, np.array([0, 0, 2]) + 1)
    assert res.ranks("average", seed=7).tolist() == (np.array([0, 3, 1]) + u).tolist()
    assert res.reliability_index("mst", n_bins=2) == 1.0
    s = res.summary(n_bins=2)
    assert s["mst"]["cases"] == 3 and s["mst"]["empty"] == 1 and s["mst"]["low"] == 1.0 and s["mst"]["high"] == 0.0
    c = MR.compare(res, MR.MultivariateRanks(("mst",), 7, {"mst": below["mst"]}, {"mst": equal["mst"]}, {"mst": n_valid["mst"]}), n_bins=2)
    assert list(c) == ["mst"] and c["mst"]["reliability_index_difference"] == 0.0
    for call in (lambda: res.histogram("band_depth"), lambda: res.histogram("mst", n_bins=3), lambda: res.histogram("mst", n_bins=0),
                 lambda: res.ranks("mst", seed=-1), lambda: MR.compare(res, None)):
        with pytest.raises(ValueError):
            call()
    empty = MR.MultivariateRanks(("mst",), 3, {"mst": np.zeros(1, np.int64)}, {"mst": np.zeros(1, np.int64)}, {"mst": np.zeros(1, np.int64)})
    assert empty.histogram("mst").sum() == 0 and np.isnan(empty.reliability_index("mst"))
    b, e = MR.observation_ranks(np.array([[3, 1, 3, 5], [0, 0, 0, 0]]))
    assert b.tolist() == [1, 0] and e.tolist() == [1, 3]
    assert MR.observation_ranks(torch.tensor([2, 1, 1]))[0] == 2


def test_argument_errors():
    ens, obs = np.zeros((3, 24, 2, 5), np.float32), np.zeros((24, 2, 5), np.float32)
    bad_pairs = ((np.zeros((3, 23, 2, 5)), obs), (np.zeros((24, 2, 5)), obs), (ens, np.zeros((24, 2, 4))), (ens, np.zeros((24, 5))),
                 (np.zeros((0, 24, 2, 5)), obs), (np.zeros((2, 3, 24, 2, 5)), obs), (np.zeros((2, 3, 24, 2, 5)), np.zeros((3, 24, 2, 5))),
                 (torch.zeros(3, 24, 2, 5), obs), (ens, torch.zeros(24, 2, 5)), (np.zeros((3, 24, 2, 5), dtype=complex), obs),
                 (np.broadcast_to(np.float32(0), (4096, 24, 1, 1)), np.zeros((24, 1, 1))))
    for e, o in bad_pairs:
        for fn in (MR.prerank_sums, MR.multivariate_ranks):
            with pytest.raises(ValueError):
                fn(e, o)
    for kw in (dict(by_hour=1), dict(position_runs=0), dict(position_runs=1.0), dict(position_runs=True)):
        with pytest.raises(ValueError):
            MR.prerank_sums(ens, obs, **kw)
    for kw in (dict(kinds=()), dict(kinds=("rank",)), dict(kinds=("mst", "mst")), dict(kinds=("average", "mst"), by_hour=True), dict(kinds="mst", by_hour=True),
               dict(pool=3), dict(by_hour="yes")):
        with pytest.raises(ValueError):
            MR.multivariate_ranks(ens, obs, **kw)
    assert MR.check_kinds("average", True) == ("average",) and MR.check_kinds(MR.KINDS) == MR.KINDS
    for args in ((ens, obs, 3), (ens[0], obs), (ens, obs[None]), (ens, np.zeros((24, 2, 4), np.float32)), (torch.zeros(3, 24, 2, 5), obs)):
        with pytest.raises(ValueError):
            MR.mst_preranks(*args)
    with pytest.raises(ValueError):
        MR.check_mst_admission(4097, 10)
    with pytest.raises(ValueError):
        MR.check_mst_admission(3, (1 << 40) // 65535 + 1)                                  # a distance could reach 2^40
    MR.check_mst_admission(4096, (1 << 40) // 65535)
    for d in (np.zeros((3, 3), np.int64), torch.zeros(3, 3), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
              torch.zeros(3, 3, dtype=torch.int64), torch.zeros(0, 0, dtype=torch.int64)):
        with pytest.raises(ValueError):
            MR.mst_leave_one_out(d)
    with pytest.raises(ValueError):
        MR.observation_ranks(np.zeros((4, 1)))
    if not torch.cuda.is_available():                                                      # valid arguments reach the device: no CPU fallback
        for fn in (MR.prerank_sums, MR.multivariate_ranks, MR.mst_preranks):
            with pytest.raises(_lib.RdganError):
                fn(ens, obs)
    reals = np.zeros((2, 24, 2, 5), np.float32)
    for args, kw in (((None, reals), {}), ((lambda d: ens, np.zeros((24, 2, 5))), {}), ((lambda d: ens, reals), dict(kinds=("crps",))),
                     ((lambda d: ens, reals), dict(by_hour=True)), ((lambda d: ens, reals), dict(pool=16)), ((lambda d: ens, torch.zeros(2, 24, 2, 5)), {})):
        with pytest.raises(ValueError):
            MR.ranks_for_days(*args, **kw)
    sq, clim = np.zeros((2, 24, 8, 8), np.float32), np.zeros((5, 24, 8, 8), np.float32)
    for args, kw in (((None, reals, clim), {}), ((None, sq, np.zeros((5, 24, 8, 4))), {}), ((None, sq, clim), dict(slopes=(1.0,))),
                     ((None, sq, clim), dict(library="days")), ((None, sq, clim), dict(n_members=0)), ((None, sq, clim), dict(n_members=4096)),
                     ((None, sq, clim), dict(seed=-1)), ((None, sq, clim), dict(kinds=("mst",), by_hour=True)), ((None, sq, clim), dict(pool=3)),
                     ((None, sq, clim), dict(query_groups=np.zeros(2, np.int32))), ((None, sq, clim), dict(cascade="model")), ((None, sq[0], clim), {}),
                     ((None, sq, np.broadcast_to(np.float32(0), (4096, 24, 8, 8))), {})):
        with pytest.raises(ValueError):
            MR.multivariate_rank_experiment(*args, **kw)


def test_cabi_argument_checks():
    """the C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    wsb = lib.rdgan_mvr_ranks_workspace_bytes
    assert wsb(1, 1, 0) == 8 and wsb(4095, 2 ** 20, 1) == 8
    for a in ((0, 1, 0), (4096, 1, 0), (1, 0, 0), (1, 2 ** 20 + 1, 0), (1, 1, 2), (1, 1, -1)):
        assert wsb(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)

    def ranks(ens=good, obs=good, m=5, D=2, ny=3, nx=5, shared=0, runs=0, sums=good, nv=good, ws=good, nbytes=8):
        return lib.rdgan_mvr_ranks(ens, obs, m, D, ny, nx, shared, runs, sums, nv, ws, nbytes, st)

    for kw in (dict(ens=null), dict(obs=null), dict(sums=null), dict(nv=null), dict(ws=null), dict(ens=by(2)), dict(obs=by(1)), dict(sums=by(4)), dict(nv=by(4)),
               dict(ws=by(4)), dict(m=0), dict(m=4096), dict(D=0), dict(D=2 ** 20 + 1), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4097), dict(shared=2),
               dict(shared=-1), dict(runs=-1), dict(nbytes=7), dict(nbytes=0), dict(nbytes=-8), dict(m=4095, ny=4096, nx=4096),
               dict(m=2048, D=2 ** 20, ny=64, nx=64)):
        assert ranks(**kw) == -2, kw

    def mst(dist=good, n=5, out=good):
        return lib.rdgan_mvr_mst(dist, n, out, st)

    for kw in (dict(dist=null), dict(out=null), dict(dist=by(4)), dict(out=by(4)), dict(n=0), dict(n=-1), dict(n=4097)):
        assert mst(**kw) == -2, kw


def test_header_and_lib_agree_on_the_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "long long*": "c_void_p", "const long long*": "c_void_p"}
    assert tuple(sorted(n for n in _lib.SIGNATURES if n.startswith("rdgan_mvr_"))) == NAMES
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_mvr_\w+)\(", header, re.M)))) == NAMES
    lib = _lib.load()
    for name in NAMES:
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
    text = "".join(open(os.path.join(csrc, h)).read() for h in ("rdgan_mvrank.hip.h", "rdgan_sequence.hip.h", "rdgan_hourly_host.h"))

    def value(name):
        expr = re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1)
        expr = re.sub(r"RD_\w+", lambda m: str(value(m.group(0))), expr)
        return eval(re.sub(r"(?<=\d)L+\b", "", expr).replace("/", "//"))

    assert (MR.MAX_VECTORS, MR.MAX_MEMBERS, MR.MAX_DAYS, MR.MAX_DIST, MR.NHOURS, MR.MAX_ELEMS, MR.MAX_PLANE) == tuple(
        value(n) for n in ("RD_MVR_MAXN", "RD_MVR_MAXM", "RD_MVR_MAXDAYS", "RD_MVR_MAXDIST", "RD_HOURS", "RD_HOURLY_MAXELEMS", "RD_HOURLY_MAXPLANE"))
    assert MR.MAX_VECTORS == R.MAX_MEMBERS and R.FEATMAX == value("RD_SEQ_FEATMAX")
    # the tile: 64 / 32 / 16 / 8 positions with switch points at N = 512, 1024, 2048; with the run's sums it stays inside 160 KB of LDS
    tile, tp_max, tp_min, acc_max = (value(n) for n in ("RD_MVR_TILE_BYTES", "RD_MVR_MAXTP", "RD_MVR_MINTP", "RD_MVR_ACC_MAXN"))
    assert (tile, tp_max, tp_min) == (128 * 1024, 64, 8) and tile // (4 * tp_max) == 512 and tile // (4 * tp_min) == MR.MAX_VECTORS
    assert tile + 16 * acc_max + 4096 <= 160 * 1024
    assert value("RD_MVR_MST_KEYS") == 16 and value("RD_MVR_THREADS") == 256
    import pr_disagg_radar_gan_amd
    assert pr_disagg_radar_gan_amd.multivariate_ranks is MR
