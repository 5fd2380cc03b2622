"""CPU: the numpy restatement of the storm definitions (tests/storms_np.py) against answers worked out by hand and identities; the
derived quantities and argument checks of pr_disagg_radar_gan_amd/storms.py; header against _lib.py and the kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, storms as SM
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import storms_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


only = sn.only_nonzero


def test_one_pixel_wet_for_five_hours():
    for (y, x), c in (((2, 3), 0), ((0, 3), 1), ((4, 6), 1), ((2, 0), 1)):                # class by the plane's rim
        a = np.zeros((1, 24, 5, 7), np.float32)
        a[0, 3:8, y, x] = 2.0
        for conn in (4, 8):
            for reach in (0, 1, 4):
                o, lab = sn.storms_np(a, (0.5, 2.0), conn, reach, want_labels=0)
                assert only(o["storms"]) == {(0, c): 1} and only(o["duration_hist"]) == {(0, c, 4): 1} and only(o["start_hour"]) == {(0, c, 3): 1}
                assert only(o["size_hist"]) == {(0, c, 2): 1} and only(o["size_sum"]) == {(0, c): 5} and only(o["size_sq_sum"]) == {(0, c): 25}
                assert only(o["size_by_duration"]) == {(0, c, 4): 5} and only(o["volume_by_duration"]) == {(0, c, 4): 5 * 2 * 65536}
                assert only(o["storms_per_day"]) == {(0, 1): 1, (1, 0): 1} and only(o["longest_duration"]) == {(0, 5): 1, (1, 0): 1}
                assert only(o["wet_pixels"]) == {(0, h): 1 for h in range(3, 8)} and o["n_days"] == 1 and o["n_bad_pixels"] == 0
                assert set(np.unique(lab).tolist()) == {-1, 3 * 35 + y * 7 + x} and (lab >= 0).sum() == 5
                sn.check_identities(o)


def test_days_never_link():
    a = np.zeros((2, 24, 5, 7), np.float32)
    a[0, 23, 2, 3], a[1, 0, 2, 3] = 1.0, 1.0
    o, lab = sn.storms_np(a, (0.5,), 8, 4, want_labels=0)
    assert only(o["storms"]) == {(0, 2): 2} and only(o["duration_hist"]) == {(0, 2, 0): 2} and only(o["start_hour"]) == {(0, 2, 0): 1, (0, 2, 23): 1}
    assert only(o["storms_per_day"]) == {(0, 1): 2} and only(o["longest_duration"]) == {(0, 1): 2} and o["n_days"] == 2
    assert lab[0, 23, 2, 3] == 23 * 35 + 17 and lab[1, 0, 2, 3] == 17
    sn.check_identities(o)


def test_stepping_pixel():
    a = sn.stepping_pixel(5, 30)[None]
    for conn in (4, 8):
        o = sn.storms_np(a, (0.5,), conn, 1)
        assert only(o["storms"]) == {(0, 3): 1} and only(o["duration_hist"]) == {(0, 3, 23): 1} and only(o["size_sum"]) == {(0, 3): 24}
        assert only(o["longest_duration"]) == {(0, 24): 1}
        o = sn.storms_np(a, (0.5,), conn, 0)
        # hour 0 at column 0: the rim and the day; hour 23 at column 23: the day alone
        assert only(o["storms"]) == {(0, 0): 22, (0, 2): 1, (0, 3): 1} and only(o["duration_hist"].sum(axis=1)) == {(0, 0): 24}
        assert only(o["start_hour"].sum(axis=1)) == {(0, h): 1 for h in range(24)} and only(o["storms_per_day"]) == {(0, 24): 1}
        assert only(o["longest_duration"]) == {(0, 1): 1}
        sn.check_identities(o)
    two = sn.stepping_pixel(9, 60, row=1)
    two[np.arange(24), 7, 2 * np.arange(24)] = 1                                          # and one that steps two columns per hour
    assert sn.storms_np(two, (0.5,), 8, 1)["storms"].sum() == 1 + 24 and sn.storms_np(two, (0.5,), 8, 2)["storms"].sum() == 2


def test_inverting_checkerboard():
    for ny, nx in ((4, 6), (5, 7)):
        a = sn.inverting_checkerboard(ny, nx)
        n = int(a.sum())
        o = sn.storms_np(a, (0.5,), 4, 0)
        assert o["storms"].sum() == n == o["size_hist"][0, :, 0].sum() and only(o["duration_hist"].sum(axis=1)) == {(0, 0): n}
        assert only(o["storms_per_day"]) == {(0, 64): 1}
        sn.check_identities(o)
        o, lab = sn.storms_np(a, (0.5,), 4, 1, want_labels=0)
        assert only(o["storms"]) == {(0, 3): 1} and only(o["size_sum"]) == {(0, 3): n} and only(o["duration_hist"]) == {(0, 3, 23): 1}
        assert set(np.unique(lab).tolist()) == {-1, 0}
        assert sn.storms_np(a, (0.5,), 8, 0)["storms"].sum() == 24                        # a cell per hour, none overlaps the next


def test_bad_values_and_volume():
    a = np.zeros((1, 24, 7, 11), np.float32)
    a[0, 5:8, 3, 2:9] = 2.0                                                               # an interior bar of 7, three hours
    assert only(sn.storms_np(a, (0.5,), 8, 0)["storms"]) == {(0, 0): 1}
    for badv in (np.nan, np.inf, -np.inf):
        a[0, 6, 3, 5] = badv                                                              # cuts the bar of hour 6; hours 5 and 7 hold it together
        o, lab = sn.storms_np(a, (0.5,), 8, 0, want_labels=0)
        assert o["n_bad_pixels"] == 1 and only(o["storms"]) == {(0, 1): 1} and only(o["size_sum"]) == {(0, 1): 20} and lab[0, 6, 3, 5] == -1
        assert only(o["volume_by_duration"]) == {(0, 1, 2): 20 * 2 * 65536}
    a[0, 5, 3, 2:9], a[0, 7, 3, 2:9] = 0.0, 0.0                                           # alone it falls into two
    assert only(sn.storms_np(a, (0.5,), 8, 4)["storms"]) == {(0, 1): 2}
    a[0, 6, 3, 5], a[0, 9, 1, 1] = 2.0, np.nan                                            # a bad pixel in another hour is no neighbour
    assert only(sn.storms_np(a, (0.5,), 8, 4)["storms"]) == {(0, 0): 1}
    assert sn.quantum(np.array([3e9, 2.0 ** -17, 3 * 2.0 ** -17, 1.0], np.float32)).tolist() == [2 ** 36, 0, 2, 65536]


@pytest.mark.parametrize("p_wet", [0.02, 0.1, 0.3])
def test_identities_on_random_fields(p_wet):
    rng = np.random.default_rng(int(p_wet * 100))
    x = (rng.gamma(0.6, 3.0, (2, 24, 9, 13)) * (rng.random((2, 24, 9, 13)) < p_wet)).astype(np.float32)
    x[0, 2, 4, 6], x[1, 5, 0, 0] = np.nan, np.inf
    count = {}
    for conn in (4, 8):
        for reach in (0, 1, 4):
            o, lab = sn.storms_np(x, (0.0, 0.5, 4.0), conn, reach, want_labels=1)
            sn.check_identities(o)
            assert o["n_bad_pixels"] == 2 and o["n_days"] == 2 and np.array_equal(lab, sn.labels_np(x, 0.5, conn, reach))
            assert sn.flat_state(o).shape == (3 * SM.N_COUNTS + 2,)
            # a label is the smallest index of its storm, and a storm's hours are contiguous
            for d in range(2):
                for name in np.unique(lab[d][lab[d] >= 0]):
                    hours = np.unique(np.argwhere(lab[d] == name)[:, 0])
                    assert lab[d].ravel()[name] == name and np.flatnonzero(lab[d].ravel() == name)[0] == name
                    assert np.array_equal(hours, np.arange(hours[0], hours[-1] + 1))
            count[conn, reach] = int(o["storms"][1].sum())
    assert count[8, 4] <= count[8, 1] <= count[8, 0] <= count[4, 0] and count[8, 1] <= count[4, 1]


def hand_state():
    """threshold 0, day 0: storm A (class 0, start 5, 1 hour, 1 voxel, 2 mm), B (class 0, start 10, 3 hours, 6 voxels of 1 mm) and
    C (class 2, start 0, 2 hours, 4 voxels of 3 mm); day 1 dry.  Threshold 1: nothing wet."""
    o = sn.empty_state(2)
    o["n_days"], o["n_bad_pixels"] = 2, 3
    o["wet_pixels"][0, [5, 10, 11, 12, 0, 1]] = 1, 2, 2, 2, 2, 2
    o["storms"][0] = 2, 0, 1, 0
    o["duration_hist"][0, 0, [0, 2]], o["duration_hist"][0, 2, 1] = 1, 1
    o["start_hour"][0, 0, [5, 10]], o["start_hour"][0, 2, 0] = 1, 1
    o["size_hist"][0, 0, [0, 2]], o["size_hist"][0, 2, 2] = 1, 1
    o["size_sum"][0], o["size_sq_sum"][0] = (7, 0, 4, 0), (37, 0, 16, 0)
    o["size_by_duration"][0, 0, [0, 2]], o["size_by_duration"][0, 2, 1] = (1, 6), 4
    o["volume_by_duration"][0, 0, [0, 2]], o["volume_by_duration"][0, 2, 1] = (2 * 65536, 6 * 65536), 12 * 65536
    o["storms_per_day"][0, [0, 3]], o["longest_duration"][0, [0, 3]] = 1, 1
    o["storms_per_day"][1, 0], o["longest_duration"][1, 0] = 2, 2
    return o


def test_derived_quantities_and_compare():
    o = hand_state()
    sn.check_identities(o)
    s = SM.stats_from_state(sn.flat_state(o), (0.5, 3.0), 8, 1, 48)
    assert (s.n_days, s.n_bad_pixels, s.n_pixels, s.connectivity, s.reach) == (2, 3, 48, 8, 1)
    third = 1 / 3
    assert np.allclose(s.duration_distribution()[0, :4], [third, third, third, 0]) and np.allclose(s.duration_distribution(True)[0, :3], [0.5, 0, 0.5])
    assert np.allclose(s.mean_duration()[0], 2.0) and np.allclose(s.mean_duration(True)[0], 2.0)
    assert np.allclose(s.start_hour_distribution()[0, [0, 5, 10]], third) and np.allclose(s.start_hour_distribution()[0].sum(), 1.0)
    assert np.allclose(s.size_distribution()[0, :3], [third, 0, 2 * third]) and np.allclose(s.mean_size()[0], 11 / 3)
    assert np.allclose(s.mean_size(True)[0], 3.5)
    assert np.allclose(s.size_weighted_mean_duration()[0], 27 / 11)
    assert np.allclose(s.volume_share_by_duration()[0, :4], [0.1, 0.6, 0.3, 0])
    mi = s.mean_intensity_by_duration()
    assert mi[0, :3].tolist() == [2.0, 3.0, 1.0] and np.isnan(mi[0, 3]) and np.isnan(s.mean_intensity_by_duration(True)[0, 1])
    assert np.allclose(s.mean_storms_per_day(), [1.5, 0.0])
    assert only(s.storms_per_day_distribution() * 2) == {(0, 0): 1, (0, 3): 1, (1, 0): 2}
    assert only(s.longest_duration_distribution() * 2) == {(0, 0): 1, (0, 3): 1, (1, 0): 2}
    assert np.allclose(s.one_hour_fraction()[0], 1 / 11)
    # threshold 1 has no storm: NaN wherever the denominator is 0
    for v in (s.duration_distribution(), s.mean_duration(), s.start_hour_distribution(), s.size_distribution(), s.mean_size(),
              s.size_weighted_mean_duration(), s.volume_share_by_duration(), s.mean_intensity_by_duration(), s.one_hour_fraction()):
        assert np.all(np.isnan(v[1]))
    assert s.storms_per_day_distribution()[1, 0] == 1.0 and s.longest_duration_distribution()[1, 0] == 1.0
    none = SM.stats_from_state(np.zeros(SM.N_COUNTS + 2, np.int64), (0.5,), 4, 0, 48)
    assert np.all(np.isnan(none.mean_storms_per_day())) and np.all(np.isnan(none.storms_per_day_distribution()))

    c = SM.compare(s, s)
    assert c["thresholds"] == (0.5, 3.0)
    for k in ("tv_duration", "tv_duration_complete", "tv_start_hour", "tv_size", "tv_longest_duration", "mean_duration", "mean_storms_per_day",
              "one_hour_fraction", "volume_share_by_duration"):
        assert np.all(c[k][0] == 0), k
    o2 = hand_state()                                                                     # storm A lasts two hours instead of one
    o2["duration_hist"][0, 0, :2] = 0, 1
    o2["size_by_duration"][0, 0, :2] = 0, 1
    o2["volume_by_duration"][0, 0, :2] = 0, 2 * 65536
    o2["longest_duration"][0, [3, 4]] = 0, 1
    c = SM.compare(s, SM.stats_from_state(sn.flat_state(o2), (0.5, 3.0), 8, 1, 48))
    assert c["tv_duration"][0] == pytest.approx(third) and c["tv_duration_complete"][0] == pytest.approx(0.5) and c["tv_start_hour"][0] == 0
    assert c["tv_longest_duration"][0] == pytest.approx(0.5) and c["mean_duration"][0] == pytest.approx(-third)
    assert c["one_hour_fraction"][0] == pytest.approx(1 / 11) and c["mean_storms_per_day"][0] == 0
    assert np.allclose(c["volume_share_by_duration"][0, :3], [0.1, -0.1, 0])
    flat = sn.flat_state(o)
    for other in (SM.stats_from_state(flat[SM.N_COUNTS:], (3.0,), 8, 1, 48), SM.stats_from_state(flat, (0.5, 3.0), 4, 1, 48),
                  SM.stats_from_state(flat, (0.5, 3.0), 8, 0, 48), None):
        with pytest.raises(ValueError):
            SM.compare(s, other)
    with pytest.raises(ValueError):
        SM.split_state(np.zeros(5), 1)


def test_state_layout_round_trip():
    flat = np.arange(2 * SM.N_COUNTS + 2)
    d = SM.split_state(flat, 2)
    assert d["wet_pixels"][1, 0] == 622 and d["storms"][0, 3] == 27 and d["duration_hist"][0, 1, 0] == 52 and d["start_hour"][0, 0, 23] == 147
    assert d["size_hist"][0, 1, 0] == 248 and d["size_sum"][0, 0] == 332 and d["size_sq_sum"][0, 3] == 339 and d["size_by_duration"][0, 0, 0] == 340
    assert d["volume_by_duration"][0, 3, 23] == 531 and d["storms_per_day"][0, 64] == 596 and d["longest_duration"][0, 24] == 621
    assert d["n_days"] == 1244 and d["n_bad_pixels"] == 1245
    assert np.array_equal(sn.flat_state(d), flat)                                         # the yardstick's order is the module's
    assert {k: v.shape[1:] for k, v in d.items() if k[:2] != "n_"} == {k: v.shape[1:] for k, v in sn.empty_state(2).items() if k[:2] != "n_"}


class NoGenerator:
    ndomain, n_cond_channels = 16, 1


def test_argument_errors(monkeypatch):
    for thr in ((), tuple(range(9)), (1.0, 0.5), (-1.0,), (np.nan,), (1.0, 1.0), "x"):
        with pytest.raises(ValueError):
            SM.StormStructure(thr)
    for conn in (0, 6, 8.0, True, "8"):
        with pytest.raises(ValueError):
            SM.StormStructure((0.1,), connectivity=conn)
    for reach in (-1, 5, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            SM.StormStructure((0.1,), reach=reach)
        with pytest.raises(ValueError):
            SM.check_reach(reach)
    for dpp in (0, 2731, 2.5, True):
        with pytest.raises(ValueError):
            SM.StormStructure((0.1,), days_per_pass=dpp)
    assert [SM.check_reach(r) for r in range(5)] == list(range(5)) and SM.check_days_per_pass(None) is None and SM.check_days_per_pass(2730) == 2730
    ss = SM.StormStructure((0.1,))
    too_large = np.broadcast_to(np.float32(0), (24, 4096, 2048))                          # a plane the cells take, a day beyond 2^27 voxels
    for bad in (np.zeros((24, 5)), np.zeros((23, 4, 5)), np.zeros((2, 25, 4, 5)), np.zeros((0, 24, 4, 5)), np.zeros((24, 4, 5), dtype=complex),
                torch.zeros(24, 4, 5), too_large):
        with pytest.raises(ValueError):
            ss.add(bad)
    with pytest.raises(ValueError):
        ss.add(np.zeros((24, 4, 5), np.float32), label_threshold=1)
    with pytest.raises(ValueError):
        ss.add(np.zeros((24, 4, 5), np.float32), labels_out=torch.zeros(24, 4, 5, dtype=torch.int32))           # on the host
    with pytest.raises(ValueError):
        ss.state()
    for kw in (dict(hourly=torch.zeros(24, 4, 5)), dict(hourly=too_large), dict(connectivity=5), dict(reach=5), dict(threshold=-1.0),
               dict(hourly=np.zeros((24, 5)))):
        with pytest.raises(ValueError):
            SM.label_storms(**{**dict(hourly=np.zeros((24, 4, 5), np.float32), threshold=0.1), **kw})
    ss.plane_shape = (4, 5)                                                               # as after a first add
    with pytest.raises(ValueError):
        ss.add(np.zeros((24, 4, 6), np.float32))
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            SM.storm_structure(np.zeros((24, 4, 5), np.float32), (0.1,))
        with pytest.raises(_lib.RdganError):
            SM.label_storms(np.zeros((24, 4, 5), np.float32), 0.1)

    good = dict(daily=np.zeros((20, 30), np.float32), n_scenarios=3, thresholds=(0.1,))
    bad_field = (dict(thresholds=()), dict(connectivity=5), dict(reach=5), dict(reach=-1), dict(n_scenarios=0), dict(scenario_chunk=0), dict(overlap=9),
                 dict(latent_mode="each"), dict(daily=np.zeros((2, 2, 20, 30), np.float32)))
    for kw in bad_field + (dict(daily=torch.zeros(20, 30)), dict(days_per_pass=0), dict(chunk=0), dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            SM.storm_structure_field(**{**good, "gen": NoGenerator(), **kw})
    monkeypatch.setattr(P, "gen", NoGenerator())
    for kw in bad_field:
        with pytest.raises(ValueError):
            P.storm_structure_field(**{**good, **kw})


def test_cabi_argument_checks():
    """the three C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    assert [lib.rdgan_storms_state_count(T) for T in (0, 1, 8, 9, -1)] == [-2, 624, 8 * 622 + 2, -2, -2]
    ws = lib.rdgan_storms_workspace_bytes
    one = 24 * 35 * 24 + 8 + 24 * 8
    assert ws(5, 7, 1) == one and ws(5, 7, 3) == 3 * one and ws(2048, 2048, 2730) == 2730 * (24 * 2 ** 22 * 24 + 8 + 24 * 8)
    for a in ((0, 7, 1), (5, 0, 1), (5, 7, 0), (5, 7, 2731), (4096, 2048, 1), (2 ** 25, 1, 1), (-1, -1, 1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                                       # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])

    def acc(x=good_p, n=1, stride=24 * 35, ny=5, nx=7, th=hp(thr), T=2, conn=8, reach=1, counts=good_p, labels=null, lt=0, ws=good_p, nbytes=one):
        return lib.rdgan_storms_accumulate(x, n, stride, ny, nx, th, T, conn, reach, counts, labels, lt, ws, nbytes, ctypes.c_void_p(0))

    unsorted, negative, nan = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0])), hp(np.array([np.nan, 1.0]))
    for kw in (dict(x=null), dict(counts=null), dict(ws=null), dict(th=null), dict(x=odd_p), dict(counts=four_p), dict(ws=four_p), dict(labels=odd_p),
               dict(n=0), dict(ny=0), dict(nx=0), dict(ny=4096, nx=2048), dict(n=2 ** 40), dict(stride=24 * 35 - 1), dict(T=0), dict(T=9),
               dict(th=unsorted), dict(th=negative), dict(th=nan), dict(conn=0), dict(conn=6), dict(reach=-1), dict(reach=5),
               dict(labels=good_p, lt=2), dict(labels=good_p, lt=-1), dict(nbytes=one - 1), dict(nbytes=0), dict(nbytes=-5)):
        assert acc(**kw) == -2, kw


def test_header_and_lib_agree_on_the_storm_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "long long*": "c_void_p", "int*": "c_void_p"}
    for name in ("rdgan_storms_state_count", "rdgan_storms_workspace_bytes", "rdgan_storms_accumulate"):
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
    # the flat order the header lists is the one of the constants
    listed = dict((name, int(off)) for off, name in re.findall(r"^ \*\s+(\d+)  (\w+)\[", header[header.index("Storms of hourly fields"):], re.M)[:11])
    assert listed == dict(zip(sn.ORDER, (SM._WET, SM._STORMS, SM._DUR, SM._START, SM._HIST, SM._SSUM, SM._SSQ, SM._SBD, SM._VBD, SM._SPD, SM._LONGEST)))
    assert f"T * {SM.N_COUNTS} + 2" in header


def test_python_constants_are_the_kernel_header_s():
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_storms.hip.h")).read()
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (SM.N_COUNTS, SM.N_CLASSES, SM.N_BINS, SM.N_SPD, SM.N_LONGEST, SM.MAX_DAY, SM.MAX_PASS, SM.MAX_REACH) == tuple(
        value(m) for m in ("RD_SM_NC", "RD_SM_NCLASS", "RD_SM_NBINS", "RD_SM_NSPD", "RD_SM_NLONG", "RD_SM_MAXDAY", "RD_SM_MAXPASS", "RD_SM_MAXREACH"))
    offsets = (SM._WET, SM._STORMS, SM._DUR, SM._START, SM._HIST, SM._SSUM, SM._SSQ, SM._SBD, SM._VBD, SM._SPD, SM._LONGEST)
    assert offsets == tuple(value(m) for m in ("RD_SM_WET", "RD_SM_STORMS", "RD_SM_DUR", "RD_SM_START", "RD_SM_HIST", "RD_SM_SSUM", "RD_SM_SSQ",
                                               "RD_SM_SBD", "RD_SM_VBD", "RD_SM_SPD", "RD_SM_LONGEST"))
    # every array has the length the next offset leaves it
    sizes = (24, 4, 4 * 24, 4 * 24, 4 * SM.N_BINS, 4, 4, 4 * 24, 4 * 24, SM.N_SPD, SM.N_LONGEST)
    assert tuple(np.cumsum((0,) + sizes)) == offsets + (SM.N_COUNTS,)
    assert SM.MAX_PASS == 65535 // 24 and value("RD_SM_VOXEL_BYTES") == 24 and (SM.NHOURS, SM.MAX_PLANE) == (24, 1 << 24)
    assert SM.N_BINS == int(np.log2(SM.MAX_DAY)) + 1
