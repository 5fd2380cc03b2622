"""CPU: the bins, the derived quantities and the argument checks of pr_disagg_radar_gan_amd/scaling.py against the numpy restatement
(tests/scaling_np.py) and answers worked out by hand; the C entries' refusals; header against _lib.py and the kernel's constants."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, scaling as SC
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import scaling_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MAX = 24 * 2048 * 1024 * 4096                                              # every pixel-hour of a 64 x 64 day at the largest good value, 2048 - 2^-13


def test_bins_at_every_edge():
    edges = SC.bin_edges()
    assert edges.shape == (SC.N_BINS + 1,) and edges[0] == 0 and np.all(np.diff(edges) > 0) and edges[-1] == 1 << 38 and R_MAX < edges[-1]
    for i in range(SC.N_BINS):                                               # the bins partition [0, 2^38), which holds [0, 24 * 2^33)
        lo, hi = int(edges[i]), int(edges[i + 1])
        assert sn.bin_of(lo) == i and sn.bin_of(hi - 1) == i and (i == 0 or sn.bin_of(lo - 1) == i - 1), i
        assert SC.bin_of([lo, hi - 1]).tolist() == [i, i], i
        if i >= 8:
            assert hi * 8 <= lo * 9 and lo == (8 + (i - 8) % 8) << ((i - 8) // 8)            # edge ratio at most 9/8
    # the largest R, 24 * 4096 * 2^21 = 1.5 * 2^37 (the largest good value times 1024 rounds up to 2^21), has e = 37 and the bits 100
    # below the leading one: bin 284; the last
    # bin of that octave, 287, ends the table at 2^38
    assert SC.bin_of([0, 1, 7, 8, 9, 15, 16, 17, 18, 1 << 37, R_MAX, (1 << 38) - 1]).tolist() == [0, 1, 7, 8, 9, 15, 16, 16, 17, 280, 284, 287]
    assert sn.bin_of(R_MAX) == 284 and sn.bin_of(1 << 37) == 280 and sn.bin_of((1 << 38) - 1) == 287 and R_MAX == 24 * 2 ** 33 < 1 << 38
    rng = np.random.default_rng(0)
    R = np.concatenate([rng.integers(0, 1 << k, 200) for k in (4, 12, 26, 38)])
    assert SC.bin_of(R).tolist() == [sn.bin_of(v) for v in R] == sn.bins_of(R).tolist()
    assert SC.bin_of(R.reshape(4, 200)).shape == (4, 200)
    for bad in (-1, 1 << 38):
        with pytest.raises(ValueError):
            SC.bin_of([0, bad])
    v = SC.bin_values()
    assert v[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, np.sqrt(72.0)] and np.all(v[8:] ** 2 * 8 <= edges[8:-1].astype(float) ** 2 * 9 * (1 + 1e-15))


@functools.lru_cache(maxsize=None)
def small_field():
    """(3, 24, 20, 19): rain-like, mostly zeros, one bad pixel-hour; the state the restatement gives at A = 4"""
    rng = np.random.default_rng(3)
    wet = rng.random((3, 24, 20, 19)) < 0.25
    x = (rng.gamma(0.5, 6.0, wet.shape) * wet).astype(np.float32)
    x[1, 5, 7, 7] = np.nan
    return x, sn.scaling_np(x, 4)


def test_restatement_by_hand():
    # one wet pixel-hour of 3 mm at hour 7, pixel (2, 3) of a 5 x 6 plane: one wet box-window per level pair
    x = np.zeros((24, 5, 6), np.float32)
    x[7, 2, 3] = 3.0
    o = sn.scaling_np(x, 2)
    assert o["n_boxes"].tolist() == [[30 * 24 // T for T in sn.DURATIONS], [6 * 24 // T for T in sn.DURATIONS], [24 // T for T in sn.DURATIONS]]
    assert np.all(o["n_wet"] == 1) and np.all(o["sum1"] == 3072) and np.all(o["max_R"] == 3072) and not o["n_void"].any()
    assert np.all(o["hist"][:, :, sn.bin_of(3072)] == 1) and np.array_equal(o["hist"][:, :, 0], o["n_boxes"] - 1)
    assert np.all(np.array(sn.sum2(o)) == 3072 ** 2) and o["n_bad"] == 0 and o["n_days_total"] == 1
    # the rim: pixel (4, 5) lies in no box of side 2 or 4, a bad value there voids only its own pixel's windows
    x[3, 4, 5] = np.nan
    o = sn.scaling_np(x, 2)
    assert o["n_void"].tolist() == [[1] * 5, [0] * 5, [0] * 5] and o["n_bad"] == 1
    # a bad pixel-hour voids exactly the windows that hold its hour
    x[9, 0, 0] = -1.0
    o = sn.scaling_np(x, 2)
    assert o["n_void"].tolist() == [[2] * 5, [1] * 5, [1] * 5] and o["n_bad"] == 2
    # the one box of side 4 holds both pixels: its day is void, its 8-hour window 0 .. 7 holds the wet hour and not the bad one
    assert o["n_wet"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 0]]
    s = SC.stats_from_state(sn.flat_state(o), 2)
    assert np.array_equal(s.n_void, o["n_void"]) and s.n_bad == 2 and s.n_days_total == 1


def test_moments_exact_and_within_the_bin_bound():
    x, o = small_field()
    s = SC.stats_from_state(sn.flat_state(o), 4)
    assert s.space_levels == 4 and s.widths() == (1, 2, 4, 8, 16) and s.n_bad == 1 and s.n_days_total == 3
    assert [[int(v) for v in row] for row in s.sum2()] == sn.sum2(o)
    for q in (0, 1, 2):
        np.testing.assert_allclose(s.moment(q), sn.exact_moment(x, 4, q), rtol=1e-12)
    assert np.array_equal(s.moment(0), s.wet_fraction()) and np.array_equal(s.moment(1), s.mean_intensity())
    np.testing.assert_allclose(s.max_intensity(), o["max_R"] / (np.outer(4.0 ** np.arange(5), sn.DURATIONS) * 1024))
    for q in (0.5, 1.5, 3, 4):
        ratio = s.moment(q) / sn.exact_moment(x, 4, q)
        bound = (9 / 8) ** (q / 2)
        assert np.all(ratio <= bound * (1 + 1e-12)) and np.all(ratio >= (1 - 1e-12) / bound), (q, ratio.min(), ratio.max())
    # the quantiles: the bin of the exact quantile's box sum
    p = (0.0, 0.5, 0.9, 0.99, 1.0)
    got = s.quantiles(p)
    assert got.shape == (5, 5, 5)
    for a in range(5):
        for b in range(5):
            R, void = sn.box_sums(x, a, b)
            v = np.sort(R[~void])
            for k, pk in enumerate(p):
                exact = v[max(int(np.ceil(pk * v.size)), 1) - 1]
                assert got[k, a, b] == SC.bin_values()[sn.bin_of(exact)] / (4.0 ** a * sn.DURATIONS[b] * 1024), (a, b, pk)
    for bad in ((-0.1,), (1.5,), "x", 0.5):
        with pytest.raises(ValueError):
            s.quantiles(bad)
    for bad in (-1, np.inf, np.nan):
        with pytest.raises(ValueError):
            s.moment(bad)


def planted(A=4, slope_wet=1, slope2=-1):
    """a state whose moments are exact power laws of the box side s = 2^a at every time level and constant over the durations:
    M_0 = (s / 2^A)^slope_wet, M_1 = 2 mm/h, M_2 = 16 s^slope2 mm^2/h^2; powers of two, so that every word is an integer"""
    o = sn.empty_state(A)
    for a in range(A + 1):
        for b in range(5):
            n = 4 ** (A - a) * 1024
            o["n_boxes"][a, b] = n
            o["n_wet"][a, b] = n >> (slope_wet * (A - a))
            o["sum1"][a, b] = n * 4 ** a * sn.DURATIONS[b] * 1024 * 2         # mean intensity 2 mm/h at every scale
            # M_2 = 16 * 2^(slope2 a) mm^2/h^2: sum2 = M_2 n (4^a T 1024)^2, all of it in the low word
            o["sum2_ll"][a, b] = (16 << (4 if slope2 < 0 else 0)) * n * (4 ** a * sn.DURATIONS[b] * 1024) ** 2 >> (4 - slope2 * a if slope2 < 0 else -slope2 * a)
    return o


def test_exponents_return_planted_slopes():
    s = SC.stats_from_state(sn.flat_state(planted()), 4)
    fit = s.exponents((0, 1, 2), "space")
    assert fit.slopes.shape == (3, 5) and fit.scales == (1, 2, 4, 8, 16) and fit.levels == (0, 1, 2, 3, 4) and fit.qs == (0.0, 1.0, 2.0)
    np.testing.assert_allclose(fit.slopes, [[1.0] * 5, [0.0] * 5, [-1.0] * 5], atol=1e-12)
    np.testing.assert_allclose(fit.intercepts, [[-4 * np.log(2)] * 5, [np.log(2)] * 5, [np.log(16)] * 5], atol=1e-12)
    assert np.all(fit.residuals < 1e-12)
    dim, res = s.box_dimension("space")
    np.testing.assert_allclose(dim, 1.0, atol=1e-12)
    sub = s.exponents((2,), "space", levels=(1, 3))
    np.testing.assert_allclose(sub.slopes, -1.0, atol=1e-12)
    assert sub.scales == (2, 8) and np.all(np.isnan(sub.residuals))          # two points: nothing left over
    # a level off the line shows in the residuals
    o = planted()
    o["sum2_ll"][2] *= 2
    off = SC.stats_from_state(sn.flat_state(o), 4).exponents((2,), "space")
    assert np.all(off.residuals > 0.1)
    t = s.exponents((1, 2), "time")
    assert t.slopes.shape == (2, 5) and t.scales == (1, 2, 4, 8, 24)
    np.testing.assert_allclose(t.slopes, 0.0, atol=1e-12)
    for kw in (dict(axis="x"), dict(levels=(0,) * 2), dict(levels=(0, 5)), dict(levels=(0, 1.5)), dict(levels=3), dict(qs=()), dict(qs=(-1,)), dict(qs="x")):
        with pytest.raises(ValueError):
            s.exponents(**{"qs": (1,), **kw})
    assert np.all(np.isnan(s.exponents((1,), levels=(2,)).slopes))


def test_constant_and_dry_fields():
    c = SC.stats_from_state(sn.flat_state(sn.scaling_np(np.full((2, 24, 16, 16), 0.5, np.float32), 4)), 4)
    for axis, d in (("space", 2.0), ("time", 1.0)):
        dim, res = c.box_dimension(axis)
        np.testing.assert_allclose(dim, d, atol=1e-12)
        np.testing.assert_allclose(res, 0.0, atol=1e-12)
        np.testing.assert_allclose(c.exponents((1, 2), axis).slopes, 0.0, atol=1e-12)           # a constant field does not scale
    np.testing.assert_allclose(c.mean_intensity(), 0.5)
    np.testing.assert_allclose(c.moment(2), 0.25)
    assert np.all(c.wet_fraction() == 1) and np.all(c.quantiles((0.1, 0.9)) == c.quantiles((0.5,)))
    d = SC.stats_from_state(sn.flat_state(sn.scaling_np(np.zeros((24, 8, 8), np.float32), 3)), 3)
    assert np.all(d.wet_fraction() == 0) and np.all(d.mean_intensity() == 0) and np.all(d.quantiles((0.5, 1.0)) == 0)
    for axis in ("space", "time"):
        assert np.all(np.isnan(d.exponents((0, 1, 2, 3), axis).slopes)) and np.all(np.isnan(d.box_dimension(axis)[0]))
    none = SC.stats_from_state(np.zeros(SC.state_count(2), np.int64), 2)
    for v in (none.wet_fraction(), none.mean_intensity(), none.max_intensity(), none.moment(2), none.moment(3), none.quantiles((0.5,)),
              none.exponents((1,), "time").slopes):
        assert np.all(np.isnan(v))


def test_compare():
    x, o = small_field()
    s = SC.stats_from_state(sn.flat_state(o), 4)
    c = SC.compare(s, s)
    assert c["qs"] == SC.DEFAULT_ORDERS and c["space_levels"] == 4
    for k, shape in (("wet_fraction", (5, 5)), ("log_moment", (3, 5, 5)), ("exponents_space", (3, 5)), ("exponents_time", (3, 5)), ("tv_hist", (5, 5))):
        assert c[k].shape == shape and np.all(c[k] == 0), k
    o2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o.items()}
    moved = int(o2["hist"][0, 0, 0]) // 2                                    # half of the dry pixel-hours become wet, bin 1
    o2["hist"][0, 0, 0] -= moved
    o2["hist"][0, 0, 1] += moved
    o2["n_wet"][0, 0] += moved
    c = SC.compare(s, SC.stats_from_state(sn.flat_state(o2), 4))
    assert np.isclose(c["tv_hist"][0, 0], moved / o["n_boxes"][0, 0], rtol=1e-12) and np.isclose(c["wet_fraction"][0, 0], -moved / o["n_boxes"][0, 0], rtol=1e-12)
    assert not c["tv_hist"][1:].any() and not c["tv_hist"][0, 1:].any()
    for other in (SC.stats_from_state(np.zeros(SC.state_count(3), np.int64), 3), None, o):
        with pytest.raises(ValueError):
            SC.compare(s, other)                                             # states whose levels differ are refused


def test_state_layout_round_trip():
    A = 2
    flat = np.arange(SC.state_count(A))
    assert SC.state_count(A) == 3 * 5 * 296 + 2 and SC.RECORD == 296 == sn.RECORD and SC.WORDS == sn.ORDER and SC.DURATIONS == sn.DURATIONS
    d = SC.split_state(flat, A)
    assert [int(d[k][0, 0]) for k in SC.WORDS] == list(range(8)) and d["hist"][0, 0].tolist() == list(range(8, 296))
    assert d["n_boxes"][1, 2] == (1 * 5 + 2) * 296 and d["hist"][2, 4, 287] == 15 * 296 - 1 and (d["n_days_total"], d["n_bad"]) == (15 * 296, 15 * 296 + 1)
    assert np.array_equal(sn.flat_state(d), flat)                            # the yardstick's order is the module's
    with pytest.raises(ValueError):
        SC.split_state(np.zeros(5), 0)
    # a smaller A is a prefix
    assert np.array_equal(SC.split_state(flat[:SC.state_count(1) - 2].tolist() + [0, 0], 1)["hist"], d["hist"][:2])


class NoGenerator:
    ndomain, n_cond_channels = 16, 1


def test_argument_errors(monkeypatch):
    for bad in (-1, 7, 2.0, True, "x"):
        with pytest.raises(ValueError):
            SC.ScalingStructure(bad)
    assert SC.ScalingStructure().space_levels is None and SC.ScalingStructure(6).space_levels == 6
    assert [SC.largest_space_levels(*s) for s in ((1, 1), (3, 9), (16, 16), (70, 67), (33, 130), (64, 64), (4096, 128))] == [0, 1, 4, 6, 5, 6, 6]
    sc = SC.ScalingStructure(3)
    too_large = np.broadcast_to(np.float32(0), (24, 4097, 4096))
    for bad in (np.zeros((24, 5)), np.zeros((23, 8, 8)), np.zeros((2, 25, 8, 8)), np.zeros((0, 24, 8, 8)), np.zeros((24, 8, 8), dtype=complex),
                torch.zeros(24, 8, 8), too_large, np.zeros((24, 7, 9), np.float32)):         # the last: boxes of 8 above the plane
        with pytest.raises(ValueError):
            sc.add(bad)
    with pytest.raises(ValueError):
        SC.ScalingStructure().add(too_large)
    with pytest.raises(ValueError):
        sc.state()
    with pytest.raises(ValueError):
        SC.scaling_structure(np.zeros((24, 4, 5), np.float32), 3)
    sc.plane_shape = (8, 8)                                                  # as after a first add
    with pytest.raises(ValueError):
        sc.add(np.zeros((24, 8, 9), np.float32))
    assert sc.reset() is sc and sc.plane_shape is None and sc.space_levels == 3
    if not torch.cuda.is_available():                                        # valid arguments reach the device: there is no CPU fallback
        for A in (None, 2):
            with pytest.raises(_lib.RdganError):
                SC.scaling_structure(np.zeros((24, 4, 5), np.float32), A)
        auto = SC.ScalingStructure()
        with pytest.raises(_lib.RdganError):
            auto.add(np.zeros((24, 64, 64), np.float32))
        with pytest.raises(_lib.RdganError):                                 # nothing was pinned by the call that failed
            auto.add(np.zeros((24, 4, 4), np.float32))

    good = dict(daily=np.zeros((20, 30), np.float32), n_scenarios=3)
    bad_field = (dict(space_levels=5), dict(space_levels=-1), dict(n_scenarios=0), dict(scenario_chunk=0), dict(overlap=9), dict(latent_mode="each"),
                 dict(daily=np.zeros((2, 2, 20, 30), np.float32)))
    for kw in bad_field + (dict(daily=torch.zeros(20, 30)), dict(chunk=0), dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            SC.scaling_structure_field(**{**good, "gen": NoGenerator(), **kw})
    monkeypatch.setattr(P, "gen", NoGenerator())
    for kw in bad_field:
        with pytest.raises(ValueError):
            P.scaling_scenarios_field(**{**good, **kw})


def test_cabi_argument_checks():
    """the three C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    count = lib.rdgan_scaling_state_count
    assert [count(a) for a in (0, 2, 6, -1, 7)] == [5 * 296 + 2, SC.state_count(2), 35 * 296 + 2, -2, -2]
    ws = lib.rdgan_scaling_workspace_bytes
    assert ws(5, 7, 2) == ws(1, 1, 0) == ws(64, 64, 6) == ws(4096, 4096, 6) == SC.WORKSPACE == 8
    for a in ((0, 7, 0), (5, 0, 0), (5, 7, 3), (5, 7, -1), (64, 64, 7), (4097, 4096, 0), (2 ** 25, 1, 0), (-1, -1, 0), (63, 64, 6)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                          # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)

    def acc(x=good_p, n=1, stride=24 * 35, ny=5, nx=7, A=2, counts=good_p, ws=good_p, nbytes=8):
        return lib.rdgan_scaling_accumulate(x, n, stride, ny, nx, A, counts, ws, nbytes, ctypes.c_void_p(0))

    for kw in (dict(x=null), dict(counts=null), dict(ws=null), dict(x=odd_p), dict(counts=four_p), dict(ws=four_p), dict(n=0), dict(n=-1), dict(ny=0),
               dict(nx=0), dict(ny=-5), dict(ny=4097, nx=4096, A=0), dict(ny=4096, nx=4096, A=0, stride=24 * 2 ** 24, n=2 ** 16 + 1), dict(n=2 ** 40),
               dict(stride=24 * 35 - 1), dict(A=-1), dict(A=3), dict(A=7), dict(A=7, ny=128, nx=128, stride=24 * 128 * 128), dict(nbytes=7), dict(nbytes=0),
               dict(nbytes=-5)):
        assert acc(**kw) == -2, kw


def test_header_lib_and_constants_agree():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "long long*": "c_void_p"}
    names = ("rdgan_scaling_state_count", "rdgan_scaling_workspace_bytes", "rdgan_scaling_accumulate")
    assert tuple(sorted(n for n in _lib.SIGNATURES if "scaling" in n)) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_scaling_\w+)\(", header, re.M)))) == tuple(sorted(names))
    for name in names:
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
    assert "const float* hourly, long n, long day_stride" in header[header.index("int rdgan_scaling_accumulate"):]
    # the record the header lists is the one split_state uses
    block = header[header.index("Scaling of hourly fields"):]
    listed = [(int(off), name) for off, name in re.findall(r"^ \*\s+(\d+)\s+(\w+?)(?:\[288\])?:", block, re.M)[:9]]
    assert listed == list(enumerate(SC.WORDS)) + [(SC.N_FIXED, "hist")]
    assert "(A + 1) * 5 * 296 + 2" in block and f"{SC.RECORD}" == "296"
    # the Python constants are the kernel header's
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_scaling.hip.h")).read()
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1))
    assert (SC.MAX_SPACE_LEVELS, SC.N_TIME, SC.N_BINS, SC.SPLIT, SC.N_FIXED, SC.WORKSPACE) == tuple(
        value(m) for m in ("RD_SC_MAXA", "RD_SC_NT", "RD_SC_BINS", "RD_SC_SPLIT", "RD_SC_HIST", "RD_SC_WORKSPACE"))
    assert tuple(range(8)) == tuple(value("RD_SC_" + w.upper().replace("N_", "N")) for w in SC.WORDS)
    assert (SC._NBOXES, SC._NVOID, SC._NWET, SC._SUM1, SC._SUM2_HH, SC._SUM2_HL, SC._SUM2_LL, SC._MAX_R) == tuple(range(8))
