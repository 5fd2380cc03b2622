"""CPU: the numpy restatement of the space-time definitions (tests/spacetime_np.py) against plain Python loops, closed forms and
identities; the derived quantities and argument checks of pr_disagg_radar_gan_amd/spacetime.py; header against _lib.py and the
kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, spacetime as ST
from tests import spacetime_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("R", [1, 2])
def test_restatement_against_plain_loops(R):
    x = sn.rain_like((2, 24, 7, 9), 5 + R, wet=0.3)
    x[1, 4, 3, 4] = np.nan
    x[0, 9, 2, 2] = 0.5                                             # exactly at a threshold
    thr = (0.5, 2.0)
    o = sn.spacetime_np(x, thr, R, 2)
    same(o, sn.spacetime_loops(x, thr, R, 2))
    sn.check_identities(o)
    assert o["n_bad_pixels"] == 1 and o["n_days"] == 2 and o["shift_hist"].sum() > 0
    assert sn.flat_state(o).shape == (ST.state_count(2, R, 2),)


def test_all_dry_days():
    o = sn.spacetime_np(np.zeros((3, 24, 5, 6), np.float32), (0.0, 1.0), 2, 3)
    assert np.array_equal(o["no_shift"], np.array([[3 * 23, 3 * 22, 3 * 21]] * 2)) and o["shift_hist"].sum() == 0
    assert o["joint"].sum() == 0 and o["wet_first"].sum() == 0 and o["dist_best"].sum() == 0 and o["dist_zero"].sum() == 0
    sn.check_identities(o)


def test_all_wet_days():
    n, ny, nx, R, K = 2, 6, 7, 2, 2
    o = sn.spacetime_np(np.full((n, 24, ny, nx), 3.0, np.float32), (1.0,), R, K)
    assert o["no_shift"].sum() == 0 and o["dist_best"].sum() == 0 and o["dist_zero"].sum() == 0
    for k in range(1, K + 1):                                       # every dist is 0: the tie goes to "did not move"
        assert o["shift_hist"][0, k - 1, R, R] == n * (24 - k) == o["shift_hist"][0, k - 1].sum()
    for k in range(K + 1):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                assert o["pairs"][k, dy + R, dx + R] == n * (24 - k) * (ny - abs(dy)) * (nx - abs(dx))
    assert np.array_equal(o["joint"][0], o["pairs"]) and np.array_equal(o["wet_first"][0], o["pairs"])
    sn.check_identities(o)


@pytest.mark.parametrize("step", [(1, 0), (0, -1), (1, -1), (0, 0)])
def test_moving_blob(step):
    """an L of 5 pixels that moves by `step` per hour inside the core: every pair of hours k apart has shift k step, dist 0"""
    R, K, ny, nx = 2, 3, 32, 31
    start = (R + (0 if step[0] >= 0 else 23), R + (0 if step[1] >= 0 else 23))
    x = sn.moving_blob(2, ny, nx, start, step)
    o = sn.spacetime_np(x, (1.0,), R, K)
    for k in range(1, K + 1):
        dy, dx = k * step[0], k * step[1]
        if max(abs(dy), abs(dx)) <= R:
            assert o["shift_hist"][0, k - 1, dy + R, dx + R] == 2 * (24 - k) == o["shift_hist"][0, k - 1].sum()
            assert o["dist_best"][0, k - 1] == 0 and o["no_shift"][0, k - 1] == 0
            assert o["dist_zero"][0, k - 1] == (0 if step == (0, 0) else 2 * (24 - k) * 2 * len(set(sn.L_BLOB) - {(y + dy, c + dx) for y, c in sn.L_BLOB}))
        else:
            assert o["dist_best"][0, k - 1] > 0
    assert o["joint"][0, 1, step[0] + R, step[1] + R] == 2 * 23 * 5
    sn.check_identities(o)


@pytest.mark.parametrize("a,b,want", sn.TIES)
def test_three_level_tie_break(a, b, want):
    R = 2
    o = sn.spacetime_np(sn.tie_day(a, b), (0.5,), R, 1)
    same(o, sn.spacetime_loops(sn.tie_day(a, b), (0.5,), R, 1))
    assert o["shift_hist"][0, 0, want[0] + R, want[1] + R] == 1 == o["shift_hist"].sum() and o["no_shift"][0, 0] == 22
    assert o["dist_best"][0, 0] == 1 and o["dist_zero"][0, 0] == (1 if want == (0, 0) else 3)


def test_threshold_is_dry_and_uninformative_pairs():
    R = 1
    x = np.zeros((1, 24, 5, 5), np.float32)
    x[0, 0, 2, 2], x[0, 1, 2, 2] = 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))
    x[0, 2, 0, 0] = 5.0                                             # wet on the rim only: A of the pair (2, 3) has nothing in the core
    x[0, 3, 2, 2] = 5.0
    x[0, 4, 4, 4] = 5.0                                             # B of (3, 4) wet on the rim only: informative, B counts in the plane
    o = sn.spacetime_np(x, (1.0,), R, 1)
    assert o["wet_first"][0, 0, R, R] == 4                          # the value at the threshold is dry
    assert o["shift_hist"].sum() == 2 and o["no_shift"][0, 0] == 21  # (1, 2): A wet in the core, B on the rim; (3, 4) likewise
    assert o["shift_hist"][0, 0, R, R] == 2                         # B out of the core's reach: every dist ties, "did not move"
    sn.check_identities(o)


def hand_stats():
    """T = 1, R = 1, K = 1: 10 informative pairs -- 6 did not move, 3 moved by (0, 1), 1 by (-1, -1) -- and 2 without a shift"""
    T, R, K = 1, 1, 1
    o = sn.empty_state(T, R, K)
    o["n_days"] = 1
    o["shift_hist"][0, 0, 1, 1], o["shift_hist"][0, 0, 1, 2], o["shift_hist"][0, 0, 0, 0] = 6, 3, 1
    o["no_shift"][0, 0], o["dist_best"][0, 0], o["dist_zero"][0, 0] = 2, 5, 20
    o["pairs"][:] = 100
    o["wet_first"][:], o["wet_second"][:], o["joint"][:] = 20, 20, 4      # independent: phi = 0
    o["joint"][0, 0, 1, 1] = 20                                             # k = 0, d = 0: the same pixels, phi = 1
    o["wet_first"][0, 1, 0, 0] = 0                                          # never wet: no correlation
    return ST.stats_from_state(sn.flat_state(o), (0.5,), R, K), o


def test_derived_quantities_and_compare():
    s, o = hand_stats()
    assert s.n_days == 1 and s.radius == 1 and s.max_lag == 1 and np.array_equal(s.shift_hist, o["shift_hist"])
    phi = s.indicator_correlation()
    assert phi.shape == (1, 2, 3, 3) and phi[0, 0, 1, 1] == 1.0 and phi[0, 0, 0, 0] == 0.0 and np.isnan(phi[0, 1, 0, 0])
    assert s.shift_distribution().shape == (1, 1, 3, 3) and np.allclose(s.shift_distribution()[0, 0, 1], [0, 0.6, 0.3])
    assert np.allclose(s.mean_shift()[0, 0], [-0.1, 0.2]) and np.allclose(s.mean_speed(), (3 + np.sqrt(2)) / 10)
    assert np.allclose(s.stationary_fraction(), 0.6) and np.allclose(s.informative_fraction(), 10 / 12) and np.allclose(s.shift_gain(), 0.75)
    c = ST.compare(s, s)
    assert all(np.all(c[k] == 0) for k in ("tv_shift", "mean_speed", "stationary_fraction", "shift_gain"))
    assert np.all(c["max_abs_correlation"] == 0)
    o["shift_hist"][0, 0, 1, 1], o["shift_hist"][0, 0, 1, 2] = 3, 6
    o["joint"][0, 1, 2, 2] = 20
    other = ST.stats_from_state(sn.flat_state(o), (0.5,), 1, 1)
    c = ST.compare(s, other)
    assert c["tv_shift"][0, 0] == pytest.approx(0.3) and c["stationary_fraction"][0, 0] == pytest.approx(0.3)
    assert c["mean_speed"][0, 0] == pytest.approx(-0.3) and c["max_abs_correlation"].tolist() == [[0.0, 1.0]]
    empty = ST.stats_from_state(sn.flat_state(sn.empty_state(1, 1, 1)), (0.5,), 1, 1)
    for q in (empty.mean_speed(), empty.stationary_fraction(), empty.informative_fraction(), empty.shift_gain(), empty.mean_shift(),
              empty.shift_distribution(), empty.indicator_correlation(), ST.compare(empty, empty)["max_abs_correlation"]):
        assert np.all(np.isnan(q))
    for other in (ST.stats_from_state(sn.flat_state(sn.empty_state(1, 1, 1)), (0.7,), 1, 1),
                  ST.stats_from_state(sn.flat_state(sn.empty_state(1, 2, 1)), (0.5,), 2, 1),
                  ST.stats_from_state(sn.flat_state(sn.empty_state(1, 1, 2)), (0.5,), 1, 2), None):
        with pytest.raises(ValueError):
            ST.compare(s, other)
    with pytest.raises(ValueError):
        ST.split_state(np.zeros(5), 1, 1, 1)


def test_state_layout_round_trip():
    T, R, K = 2, 1, 2
    D, PT = 9, ST.per_threshold(R, K)
    assert PT == (3 * 3 + 2) * 9 + 6 and ST.state_count(T, R, K) == 27 + 2 * PT + 2
    d = ST.split_state(np.arange(ST.state_count(T, R, K)), T, R, K)
    assert d["pairs"][1, 0, 0] == 9 and d["pairs"][2, 2, 2] == 26
    assert d["wet_first"][0, 0, 0, 0] == 27 and d["wet_second"][0, 0, 0, 0] == 54 and d["joint"][0, 2, 2, 2] == 107
    assert d["shift_hist"][0, 0, 0, 0] == 108 and d["shift_hist"][0, 1, 0, 1] == 118 and d["no_shift"][0].tolist() == [126, 127]
    assert d["dist_best"][0].tolist() == [128, 129] and d["dist_zero"][0].tolist() == [130, 131] and d["wet_first"][1, 0, 0, 0] == 27 + PT
    assert d["n_days"] == 27 + 2 * PT and d["n_bad_pixels"] == 28 + 2 * PT
    o = sn.spacetime_np(sn.rain_like((1, 24, 5, 6), 3, wet=0.3), (0.5, 2.0), R, K)
    back = ST.split_state(sn.flat_state(o), T, R, K)
    same({k: np.asarray(v) for k, v in o.items()}, {k: np.asarray(v) for k, v in back.items()})


def test_argument_errors():
    for thr in ((), tuple(range(9)), (1.0, 0.5), (-1.0,), (np.nan,), (1.0, 1.0), "x"):
        with pytest.raises(ValueError):
            ST.SpaceTimeStructure(thr)
    for radius in (0, 9, 4.0, True, "4"):
        with pytest.raises(ValueError):
            ST.SpaceTimeStructure((0.1,), radius=radius)
    for lag in (0, 7, 1.0, True):
        with pytest.raises(ValueError):
            ST.SpaceTimeStructure((0.1,), max_lag=lag)
    for ppp in (0, 23, 65521, 48.0, True):
        with pytest.raises(ValueError):
            ST.SpaceTimeStructure((0.1,), planes_per_pass=ppp)
    st = ST.SpaceTimeStructure((0.1,), radius=2)
    for bad in (np.zeros((24, 5)), np.zeros((23, 5, 5)), np.zeros((2, 25, 5, 5)), np.zeros((0, 24, 5, 5)), np.zeros((24, 5, 5), dtype=complex),
                torch.zeros(24, 5, 5), np.zeros((24, 4, 9), np.float32), np.zeros((24, 9, 4), np.float32)):
        with pytest.raises(ValueError):
            st.add(bad)
    with pytest.raises(ValueError):
        st.state()
    st.plane_shape = (5, 6)                                         # as after a first add
    with pytest.raises(ValueError):
        st.add(np.zeros((24, 5, 7), np.float32))
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            ST.spacetime_structure(np.zeros((24, 5, 5), np.float32), (0.1,), radius=2)

    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    good = dict(gen=NoGenerator(), daily=np.zeros((20, 30), np.float32), n_scenarios=3, thresholds=(0.1,))
    for kw in (dict(thresholds=()), dict(radius=0), dict(radius=9), dict(max_lag=7), dict(planes_per_pass=0), dict(n_scenarios=0),
               dict(scenario_chunk=0), dict(overlap=9), dict(latent_mode="each"), dict(daily=np.zeros((2, 2, 20, 30), np.float32)),
               dict(daily=torch.zeros(20, 30)), dict(chunk=0), dict(norm_scale=0.0), dict(daily=np.zeros((16, 30), np.float32), radius=8)):
        with pytest.raises(ValueError):
            ST.spacetime_structure_field(**{**good, **kw})


def test_tile_shape_mirrors_the_kernel_header():
    for ny, nx, R in ((3, 3, 1), (256, 256, 4), (256, 256, 8), (300, 129, 4), (9, 600, 4), (600, 17, 1), (4096, 4096, 8)):
        bh, cw = ST.tile_shape(ny, nx, R)
        assert 1 <= bh <= ny and 1 <= cw <= 8
        assert 2 * bh * cw + 2 * (bh + 2 * R) * (cw + 2) <= ST.LDS_WORDS
    assert ST.tile_shape(256, 256, 4) == (128, 4) and ST.tile_shape(600, 17, 1)[0] < 600 and ST.tile_shape(9, 600, 4) == (9, 8)


def test_cabi_argument_checks():
    """the three C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    sc, ws = lib.rdgan_spacetime_state_count, lib.rdgan_spacetime_workspace_bytes
    for T, R, K in ((1, 1, 1), (4, 4, 1), (8, 8, 6), (2, 3, 5)):
        assert sc(T, R, K) == ST.state_count(T, R, K)
    for a in ((0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 7)):
        assert sc(*a) == -2, a
    assert ws(5, 7, 2, 24) == 24 * 3 * 5 * 8 and ws(9, 65, 1, 48) == 48 * 2 * 9 * 2 * 8 and ws(4096, 4096, 8, 24) == 24 * 9 * 2 ** 24 // 8
    for a in ((0, 7, 1, 24), (5, 0, 1, 24), (5, 7, 0, 24), (5, 7, 9, 24), (5, 7, 1, 0), (5, 7, 1, 65521), (4097, 4096, 1, 24), (-1, -1, 1, 24)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                 # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])
    day = 24 * 3 * 5 * 8

    def acc(x=good_p, n=1, stride=24 * 35, ny=5, nx=7, th=hp(thr), T=2, R=2, K=1, counts=good_p, ws=good_p, nbytes=day):
        return lib.rdgan_spacetime_accumulate(x, n, stride, ny, nx, th, T, R, K, counts, ws, nbytes, ctypes.c_void_p(0))

    unsorted, negative, nan = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0])), hp(np.array([np.nan, 1.0]))
    for kw in (dict(x=null), dict(counts=null), dict(ws=null), dict(th=null), dict(x=odd_p), dict(counts=four_p), dict(ws=four_p),
               dict(n=0), dict(ny=0), dict(nx=0), dict(ny=4), dict(R=3), dict(nx=4, stride=24 * 20), dict(ny=4097, nx=4096), dict(n=2 ** 40),
               dict(stride=24 * 35 - 1), dict(T=0), dict(T=9), dict(th=unsorted), dict(th=negative), dict(th=nan), dict(R=0), dict(R=9),
               dict(K=0), dict(K=7), dict(nbytes=day - 1), dict(nbytes=0), dict(nbytes=-5)):
        assert acc(**kw) == -2, kw


def test_header_and_lib_agree_on_the_spacetime_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "long long*": "c_void_p"}
    for name in ("rdgan_spacetime_state_count", "rdgan_spacetime_workspace_bytes", "rdgan_spacetime_accumulate"):
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)


def test_python_constants_are_the_kernel_header_s():
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_spacetime.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (ST.MAX_RADIUS, ST.MAX_LAG, ST.MAX_PLANE, ST.MAX_PASS, ST.MAX_TILE_WORDS, ST.LDS_WORDS, ST.NHOURS) == tuple(
        value(m) for m in ("RD_ST_MAXR", "RD_ST_MAXK", "RD_HOURLY_MAXPLANE", "RD_ST_MAXPASS", "RD_ST_MAXCW", "RD_ST_LDS_WORDS", "RD_HOURS"))
    assert value("RD_ST_HPB") * value("RD_ST_GROUPS") == 24 and ST.MAX_PASS % 24 == 0
