"""CPU: the two numpy restatements of the areal-extremes definitions (tests/areal_np.py) against each other and against answers
worked out by hand; the derived quantities and argument checks of pr_disagg_radar_gan_amd/areal.py; header against _lib.py and the
kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, areal as AR
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import areal_np as an

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
only = an.only_nonzero


def test_the_two_restatements_agree_on_random_small_arrays():
    rng = np.random.default_rng(1)
    for (ny, nx), widths in (((1, 1), (1,)), ((3, 4), (1, 2, 3)), ((5, 4), (2, 4)), ((6, 7), (1, 3, 6))):
        x = (rng.gamma(0.5, 4.0, (3, 24, ny, nx)) * (rng.random((3, 24, ny, nx)) < 0.5)).astype(np.float32)
        x[0, 3, ny // 2, nx // 2] = np.nan
        x[1, 20, 0, 0] = -1.0
        x[1, 7, ny - 1, nx - 1] = np.inf
        x[2, 0] = (rng.integers(0, 4096, (ny, nx)) + 0.5) / 1024                           # quantisation ties
        x[2, 5, 0, 0] = 2048.0
        windows, levels = (1, 2, 5, 24), (0.0, 0.5, 3.0, 40.0)
        a, da = an.areal_np(x, windows, widths, levels, maxima=an.day_maxima_brute)
        b, db = an.areal_np(x, windows, widths, levels, maxima=an.day_maxima)
        assert np.array_equal(da, db) and np.array_equal(an.flat_state(a), an.flat_state(b))
        an.check_identities(a)
        assert a["n_bad"] == 4 and a["n_days_total"] == 3


def test_restatement_against_answers_by_hand():
    # one wet pixel-hour of 3 mm: every window finds it, a box of width w holds it alone, ARF = 1 / w^2
    x = np.zeros((24, 5, 6), np.float32)
    x[7, 2, 3] = 3.0
    o, d = an.areal_np(x, (1, 3, 24), (1, 2, 5), (1.0, 3.0, 3.5))
    assert np.all(d == 3 * 1024) and only(o["n_days"]) == {(k, w): 1 for k in range(3) for w in range(3)}
    # the smallest start hour whose window holds hour 7: 7, 5, 0
    assert only(o["start_hour"]) == {(0, w, 7): 1 for w in range(3)} | {(1, w, 5): 1 for w in range(3)} | {(2, w, 0): 1 for w in range(3)}
    # 20 / w^2: 20, 5, 0
    assert only(o["arf_hist"]) == {(k, 0, 20): 1 for k in range(3)} | {(k, 1, 5): 1 for k in range(3)} | {(k, 2, 0): 1 for k in range(3)}
    # the areal MEAN is 3, 0.75, 0.12 mm: two levels, none, none
    assert only(o["level_count"]) == {(k, 0, 2): 1 for k in range(3)} | {(k, 1, 0): 1 for k in range(3)} | {(k, 2, 0): 1 for k in range(3)}
    # a constant field: every key ties, so every start hour is 0, and ARF is 1
    c, d = an.areal_np(np.full((2, 24, 4, 4), 0.25, np.float32), (1, 6), (1, 4), ())
    assert d.tolist() == [[[256, 16 * 256], [6 * 256, 96 * 256]]] * 2
    assert only(c["start_hour"]) == {(k, w, 0): 2 for k in range(2) for w in range(2)} and only(c["arf_hist"]) == {(k, w, 20): 2 for k in range(2) for w in range(2)}
    assert np.array_equal(c["sum_A"], c["sum_A1"] * np.array([1, 16])) and np.array_equal(c["max_A"] * 2, c["sum_A_all"])
    # a dry day is counted and dry; an all-NaN day is void; a NaN in every 2 x 2 box leaves width 1 alone
    x = np.zeros((3, 24, 3, 3), np.float32)
    x[1] = np.nan
    x[2, :, 1, 1] = np.nan
    x[2, 4, 0, 0] = 1.0
    o, d = an.areal_np(x, (1, 24), (1, 2), (0.5,))
    assert d.tolist() == [[[0, 0], [0, 0]], [[-1, -1], [-1, -1]], [[1024, -1], [1024, -1]]]
    assert o["n_days"].tolist() == [[2, 1]] * 2 and o["n_void"].tolist() == [[1, 2]] * 2 and o["n_dry"].tolist() == [[1, 1]] * 2
    assert o["n_bad"] == 24 * 9 + 24 and o["n_days_total"] == 3
    an.check_identities(o)
    # ties to even: 0.5 / 1024 -> 0, 1.5 / 1024 -> 2, 2.5 / 1024 -> 2
    assert an.quantise(np.array([0.5, 1.5, 2.5], np.float32) / 1024)[0].tolist() == [0, 2, 2]
    assert an.quantise(np.array([np.nan, -np.inf, -1e-9, 2048.0, 2047.9990234375, -0.0], np.float32))[1].tolist() == [True, True, True, True, False, False]
    assert an.level_q((0.0, 0.00048828125, 49152.0)) == [0, 0, 49152 * 1024]


def hand_state():
    """K = 1 window, W = 2 widths (1, 4), L = 2 levels (1, 4 mm), three counted days and one void day for width 4"""
    o = an.empty_state(1, 2, 2)
    o["n_days_total"], o["n_bad"] = 4, 7
    o["n_days"][0], o["n_void"][0], o["n_dry"][0] = (4, 3), (0, 1), (1, 1)
    o["level_count"][0, 0], o["level_count"][0, 1] = (1, 1, 2), (2, 1, 0)
    o["start_hour"][0, 0, [0, 5]], o["start_hour"][0, 1, [0, 6]] = (1, 3), (1, 2)
    o["arf_hist"][0, 0, 20], o["arf_hist"][0, 1, [5, 10]] = 3, (1, 1)
    o["sum_A"][0], o["sum_A1"][0], o["sum_A_all"][0], o["max_A"][0] = (12 * 1024, 48 * 1024), (12 * 1024, 8 * 1024), (12 * 1024, 48 * 1024), (6 * 1024, 32 * 1024)
    return o


def test_derived_quantities_on_a_hand_made_state():
    s = AR.stats_from_state(an.flat_state(hand_state()), (3,), (1, 4), (1.0, 4.0))
    assert s.windows == (3,) and s.widths == (1, 4) and s.levels == (1.0, 4.0) and s.n_days_total == 4 and s.n_bad == 7
    assert np.allclose(s.mean_depth(), [[3.0, 1.0]]) and np.allclose(s.max_depth(), [[6.0, 2.0]])
    assert np.allclose(s.exceedance(), [[[0.75, 0.5], [1 / 3, 0.0]]])
    assert np.all(np.diff(s.exceedance(), axis=2) <= 0)                                   # monotone in the level
    assert np.allclose(s.arf(), [[1.0, 48 / (16 * 8)]])
    assert only(s.start_hour_distribution() * 12) == {(0, 0, 0): 3, (0, 0, 5): 9, (0, 1, 0): 4, (0, 1, 6): 8}
    assert only(s.arf_distribution() * 2) == {(0, 0, 20): 2, (0, 1, 5): 1, (0, 1, 10): 1}
    # a constant field has ARF 1
    c = an.areal_np(np.full((2, 24, 4, 4), 0.25, np.float32), (1, 6), (1, 4), (0.2, 0.3, 1.0, 2.0))[0]
    cs = AR.stats_from_state(an.flat_state(c), (1, 6), (1, 4), (0.2, 0.3, 1.0, 2.0))
    assert np.all(cs.arf() == 1.0) and np.all(cs.arf_distribution()[:, :, 20] == 1.0)
    assert np.allclose(cs.mean_depth(), [[0.25, 0.25], [1.5, 1.5]]) and np.allclose(cs.max_depth(), cs.mean_depth())
    assert cs.exceedance().tolist() == [[[1, 0, 0, 0]] * 2, [[1, 1, 1, 0]] * 2]
    # an empty state: NaN wherever the denominator is 0
    none = AR.stats_from_state(np.zeros(AR.state_count(1, 2, 2), np.int64), (3,), (1, 4), (1.0, 4.0))
    for q in (none.mean_depth(), none.max_depth(), none.exceedance(), none.start_hour_distribution(), none.arf(), none.arf_distribution()):
        assert np.all(np.isnan(q))
    assert none.exceedance().shape == (1, 2, 2) and none.arf_distribution().shape == (1, 2, 21)
    no_levels = AR.stats_from_state(np.zeros(AR.state_count(1, 2, 0), np.int64), (3,), (1, 4), ())
    assert no_levels.exceedance().shape == (1, 2, 0)


def test_compare():
    s = AR.stats_from_state(an.flat_state(hand_state()), (3,), (1, 4), (1.0, 4.0))
    c = AR.compare(s, s)
    for k in ("mean_depth", "exceedance", "arf", "tv_start_hour", "tv_arf"):
        assert np.all(c[k] == 0), k
    assert c["mean_depth"].shape == (1, 2) and c["exceedance"].shape == (1, 2, 2) and c["tv_arf"].shape == (1, 2)
    o2 = hand_state()
    o2["start_hour"][0, 0, [0, 5]] = (3, 1)
    o2["sum_A_all"][0, 0] = 16 * 1024
    c = AR.compare(s, AR.stats_from_state(an.flat_state(o2), (3,), (1, 4), (1.0, 4.0)))
    assert c["tv_start_hour"].tolist() == [[0.5, 0.0]] and c["mean_depth"].tolist() == [[-1.0, 0.0]]
    flat = an.flat_state(hand_state())
    for other in (AR.stats_from_state(flat, (4,), (1, 4), (1.0, 4.0)), AR.stats_from_state(flat, (3,), (1, 5), (1.0, 4.0)),
                  AR.stats_from_state(flat, (3,), (1, 4), (1.0, 5.0)), None):
        with pytest.raises(ValueError):
            AR.compare(s, other)


def test_state_layout_round_trip():
    K, W, L = 2, 3, 2
    rec = L + 53
    flat = np.arange(AR.state_count(K, W, L))
    assert AR.state_count(K, W, L) == K * W * rec + 2
    d = AR.split_state(flat, K, W, L)
    assert d["level_count"][0, 1].tolist() == [rec, rec + 1, rec + 2] and d["start_hour"][0, 0, 0] == L + 1 and d["arf_hist"][0, 0, 20] == L + 45
    assert [int(d[k][0, 0]) for k in ("sum_A", "sum_A1", "sum_A_all", "max_A", "n_days", "n_void", "n_dry")] == list(range(L + 46, L + 53))
    assert d["n_dry"][1, 2] == K * W * rec - 1 and d["n_days_total"] == K * W * rec and d["n_bad"] == K * W * rec + 1
    assert np.array_equal(an.flat_state(d), flat)                                         # the yardstick's order is the module's
    assert {k: v.shape[2:] for k, v in d.items() if k not in ("n_days_total", "n_bad")} == \
        {k: v.shape[2:] for k, v in an.empty_state(K, W, L).items() if k not in ("n_days_total", "n_bad")}
    with pytest.raises(ValueError):
        AR.split_state(np.zeros(5), 1, 1, 0)


class NoGenerator:
    ndomain, n_cond_channels = 16, 1


def test_argument_errors(monkeypatch):
    ok = dict(windows=(1, 3), widths=(1, 2), levels=(1.0,))
    bad_lists = (dict(windows=()), dict(windows=(3, 1)), dict(windows=(1, 1)), dict(windows=(0, 1)), dict(windows=(25,)), dict(windows=tuple(range(1, 10))),
                 dict(windows=(1.0,)), dict(windows=(True,)), dict(windows=3), dict(widths=()), dict(widths=(2, 1)), dict(widths=(2, 2)), dict(widths=(0,)),
                 dict(widths=(65,)), dict(widths=tuple(range(1, 10))), dict(widths=(2.0,)), dict(widths="x"), dict(levels=(2.0, 1.0)), dict(levels=(1.0, 1.0)),
                 dict(levels=(-0.5,)), dict(levels=(np.nan,)), dict(levels=(np.inf,)), dict(levels=(2048.0 * 24 + 1,)), dict(levels=tuple(range(17))),
                 dict(levels="x"), dict(levels=3.0))
    for kw in bad_lists:
        with pytest.raises(ValueError):
            AR.ArealExtremes(**{**ok, **kw})
    for days in (0, 65536, 2.5, True):
        with pytest.raises(ValueError):
            AR.ArealExtremes(**ok, workspace_days=days)
    assert AR.check_windows(range(1, 9)).tolist() == list(range(1, 9)) and AR.check_widths((64,)).tolist() == [64] and AR.check_levels(()).size == 0
    assert AR.check_levels((0, 49152)).tolist() == [0.0, 49152.0] and AR.ArealExtremes((24,), (64,)).levels.size == 0
    ae = AR.ArealExtremes(**ok)
    too_large = np.broadcast_to(np.float32(0), (24, 4097, 4096))
    for bad in (np.zeros((24, 5)), np.zeros((23, 4, 5)), np.zeros((2, 25, 4, 5)), np.zeros((0, 24, 4, 5)), np.zeros((24, 4, 5), dtype=complex),
                torch.zeros(24, 4, 5), too_large, np.zeros((24, 1, 5), np.float32)):        # the last: width 2 above the plane
        with pytest.raises(ValueError):
            ae.add(bad)
    with pytest.raises(ValueError):
        ae.add(np.zeros((24, 4, 5), np.float32), depths_out=torch.zeros(1, 2, 2, dtype=torch.int64))           # on the host
    with pytest.raises(ValueError):
        ae.state()
    with pytest.raises(ValueError):
        AR.areal_extremes(np.zeros((24, 4, 5), np.float32), (1,), (5,))
    with pytest.raises(ValueError):
        AR.areal_extremes(torch.zeros(24, 4, 5), (1,), (1,), return_depths=True)
    ae.plane_shape = (4, 5)                                                               # as after a first add
    with pytest.raises(ValueError):
        ae.add(np.zeros((24, 4, 6), np.float32))
    assert ae.reset() is ae and ae.plane_shape is None
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            AR.areal_extremes(np.zeros((24, 4, 5), np.float32), **ok)
        with pytest.raises(_lib.RdganError):
            AR.areal_extremes(np.zeros((24, 4, 5), np.float32), **ok, return_depths=True)

    good = dict(daily=np.zeros((20, 30), np.float32), n_scenarios=3, **ok)
    bad_field = bad_lists + (dict(widths=(1, 21)), dict(n_scenarios=0), dict(scenario_chunk=0), dict(overlap=9), dict(latent_mode="each"),
                             dict(daily=np.zeros((2, 2, 20, 30), np.float32)))
    for kw in bad_field + (dict(daily=torch.zeros(20, 30)), dict(workspace_days=0), dict(chunk=0), dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            AR.areal_extremes_field(**{**good, "gen": NoGenerator(), **kw})
    monkeypatch.setattr(P, "gen", NoGenerator())
    for kw in bad_field:
        with pytest.raises(ValueError):
            P.areal_extremes_field(**{**good, **kw})


def test_cabi_argument_checks():
    """the three C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    count = lib.rdgan_areal_state_count
    assert [count(*a) for a in ((1, 1, 0), (8, 8, 16), (2, 3, 2), (0, 1, 0), (9, 1, 0), (1, 0, 0), (1, 9, 0), (1, 1, -1), (1, 1, 17))] == \
        [55, 64 * 69 + 2, AR.state_count(2, 3, 2), -2, -2, -2, -2, -2, -2]
    ws = lib.rdgan_areal_workspace_bytes
    one = 576 + 24 * 35 * 5
    assert ws(5, 7, 1) == one and ws(5, 7, 3) == 3 * one and ws(1, 1, 1) == 576 + 120 and ws(1, 3, 2) == 2 * (576 + 360)
    assert ws(4096, 4096, 65535) == 65535 * (576 + 120 * 2 ** 24)
    for a in ((0, 7, 1), (5, 0, 1), (5, 7, 0), (5, 7, 65536), (4097, 4096, 1), (2 ** 25, 1, 1), (-1, -1, 1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                                       # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    ip = lambda *v: np.array(v, np.int32).ctypes.data_as(ctypes.c_void_p)
    dp = lambda *v: np.array(v, np.float64).ctypes.data_as(ctypes.c_void_p)

    def acc(x=good_p, n=1, stride=24 * 35, ny=5, nx=7, k=ip(1, 3), K=2, w=ip(1, 5), W=2, lv=dp(1.0, 2.0), L=2, counts=good_p, depths=null, ws=good_p,
            nbytes=one):
        return lib.rdgan_areal_accumulate(x, n, stride, ny, nx, k, K, w, W, lv, L, counts, depths, ws, nbytes, ctypes.c_void_p(0))

    for kw in (dict(x=null), dict(counts=null), dict(ws=null), dict(k=null), dict(w=null), dict(lv=null), dict(x=odd_p), dict(counts=four_p), dict(ws=four_p),
               dict(depths=four_p), dict(n=0), dict(ny=0), dict(nx=0), dict(ny=-5), dict(ny=4097, nx=4096), dict(n=2 ** 40), dict(stride=24 * 35 - 1),
               dict(K=0), dict(K=9), dict(k=ip(3, 1)), dict(k=ip(1, 1)), dict(k=ip(0, 1)), dict(k=ip(1, 25)), dict(W=0), dict(W=9), dict(w=ip(5, 1)),
               dict(w=ip(0, 5)), dict(w=ip(1, 6)), dict(w=ip(1, 65), ny=70, nx=70, stride=24 * 4900, nbytes=576 + 120 * 4900), dict(L=-1), dict(L=17),
               dict(lv=dp(2.0, 1.0)), dict(lv=dp(1.0, 1.0)), dict(lv=dp(-1.0, 1.0)), dict(lv=dp(np.nan, 1.0)), dict(lv=dp(1.0, np.inf)),
               dict(lv=dp(1.0, 49153.0)), dict(nbytes=one - 1), dict(nbytes=0), dict(nbytes=-5)):
        assert acc(**kw) == -2, kw


def test_header_and_lib_agree_on_the_areal_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "const int*": "c_void_p", "long long*": "c_void_p"}
    names = ("rdgan_areal_state_count", "rdgan_areal_workspace_bytes", "rdgan_areal_accumulate")
    assert tuple(sorted(n for n in _lib.SIGNATURES if "areal" in n)) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_areal_\w+)\(", header, re.M)))) == tuple(sorted(names))
    for name in names:
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
    # the record the header lists is the one of the constants, L = 0
    block = header[header.index("Areal extremes of hourly fields"):]
    listed = dict((name, int(off or 0)) for off, name in re.findall(r"^ \*\s+(?:L \+ (\d+)|0)\s+(\w+)", block, re.M)[:10])
    offsets = (0, AR._START, AR._ARF, AR._SUM_A, AR._SUM_A1, AR._SUM_ALL, AR._MAX_A, AR._NDAYS, AR._NVOID, AR._NDRY)
    assert listed == {name: (off + 1 if name != "level_count" else 0) for name, off in zip(an.ORDER, offsets)}
    assert f"K * W * (L + {AR.N_FIXED + 1}) + 2" in header


def test_python_constants_are_the_kernel_header_s():
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_areal.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (AR.MAX_WINDOWS, AR.MAX_WIDTHS, AR.MAX_WIDTH, AR.MAX_LEVELS, AR.N_ARF, AR.N_FIXED, AR.MAX_PLANE, AR.MAX_PASS, AR.NHOURS) == tuple(
        value(m) for m in ("RD_AR_MAXK", "RD_AR_MAXW", "RD_AR_MAXWIDTH", "RD_AR_MAXL", "RD_AR_NARF", "RD_AR_FIXED", "RD_HOURLY_MAXPLANE", "RD_AR_MAXPASS", "RD_HOURS"))
    offsets = (AR._START, AR._ARF, AR._SUM_A, AR._SUM_A1, AR._SUM_ALL, AR._MAX_A, AR._NDAYS, AR._NVOID, AR._NDRY)
    assert offsets == tuple(value(m) for m in ("RD_AR_START", "RD_AR_ARF", "RD_AR_SUM_A", "RD_AR_SUM_A1", "RD_AR_SUM_ALL", "RD_AR_MAX_A", "RD_AR_NDAYS",
                                               "RD_AR_NVOID", "RD_AR_NDRY"))
    assert tuple(np.cumsum((0, 24, AR.N_ARF, 1, 1, 1, 1, 1, 1, 1))) == offsets + (AR.N_FIXED,)
    assert value("RD_AR_SLOTS") == AR.MAX_WIDTHS + 1 and AR.UNIT == 1024
