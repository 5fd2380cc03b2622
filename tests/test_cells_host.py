"""CPU: the numpy restatement of the cell definitions (tests/cells_np.py) against closed forms and identities; the derived
quantities and argument checks of pr_disagg_radar_gan_amd/cells.py; header against _lib.py and the kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, cells as CL
from tests import cells_np as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def day(plane, hour=0):
    """a (1, 24, ny, nx) day, dry but for `plane` at `hour`"""
    x = np.zeros((1, 24) + plane.shape, np.float32)
    x[0, hour] = plane
    return x


def test_all_dry_and_all_wet():
    o = cn.cells_np(np.zeros((2, 24, 5, 7), np.float32), (0.0, 1.0))
    assert o["n_planes"] == 48 and np.all(o["dry_planes"] == 48) and np.all(o["cells_per_plane"][:, 0] == 48) and o["cells"].sum() == 0
    cn.check_identities(o)
    for conn in (4, 8):
        o, lab = cn.cells_np(np.full((1, 24, 5, 7), 2.0, np.float32), (1.0,), conn, want_labels=0)
        assert np.all(lab == 0) and np.all(o["cells"][0, 1] == 1) and o["cells"][0, 0].sum() == 0            # the rim cuts it off
        assert o["area_hist"][0, 1, 5] == 24 and o["area_sum"][0, 1] == 24 * 35 and o["area_sq_sum"][0, 1] == 24 * 35 * 35
        assert o["volume_by_area"][0, 1, 5] == 24 * 35 * 2 * 65536 and o["largest_area"][0, 5] == 24 and o["cells_per_plane"][0, 1] == 24
        cn.check_identities(o)


@pytest.mark.parametrize("ny,nx", [(5, 7), (6, 8), (9, 9)])
def test_checkerboard(ny, nx):
    x = day(cn.checkerboard(ny, nx), 3)
    o4, o8 = cn.cells_np(x, (0.5,), 4), cn.cells_np(x, (0.5,), 8)
    n = (ny * nx + 1) // 2
    assert o4["cells"][0, :, 3].sum() == n and o4["area_hist"][0, :, 0].sum() == n and o4["cells_per_plane"][0, min(n, 64)] == 1
    assert o8["cells"][0, :, 3].sum() == 1 and o8["area_sum"][0].sum() == n and o8["largest_area"][0, int(np.log2(n))] == 1
    assert o4["dry_planes"][0] == o8["dry_planes"][0] == 23
    cn.check_identities(o4), cn.check_identities(o8)


def test_corners_threshold_and_labels():
    p = np.zeros((6, 9), np.float32)
    p[0, 0], p[0, 8], p[5, 0], p[5, 8] = 3.0, 3.0, 3.0, 3.0
    p[2, 4] = 1.0                                                   # exactly at the threshold: dry
    p[3, 4] = np.nextafter(np.float32(1.0), np.float32(2.0))
    o, lab = cn.cells_np(day(p, 5), (1.0,), 8, want_labels=0)
    assert o["cells"][0, 1, 5] == 4 and o["cells"][0, 0, 5] == 1 and o["area_hist"][0].sum() == 5 and o["wet_pixels"][0, 5] == 5
    assert sorted(lab[0, 5][lab[0, 5] >= 0].tolist()) == [0, 8, 31, 45, 53] and lab[0, 5, 2, 4] == -1
    assert o["volume_by_area"][0, 1, 0] == 4 * 3 * 65536
    assert o["volume_by_area"][0, 0, 0] == int(np.rint(float(p[3, 4]) * 65536))
    cn.check_identities(o)


def test_nan_splits_a_cell_and_marks_it():
    p = np.zeros((7, 11), np.float32)
    p[3, 2:9] = 2.0                                                 # an interior bar of 7
    x = day(p, 0)
    o = cn.cells_np(x, (0.5,), 8)
    assert o["cells"][0, 0, 0] == 1 and o["cells"][0, 1, 0] == 0 and o["area_hist"][0, 0, 2] == 1
    for badv in (np.nan, np.inf, -np.inf):
        x[0, 0, 3, 5] = badv
        o, lab = cn.cells_np(x, (0.5,), 8, want_labels=0)
        assert o["n_bad_pixels"] == 1 and o["cells"][0, 1, 0] == 2 and o["cells"][0, 0, 0] == 0 and o["area_hist"][0, 1, 1] == 2
        assert lab[0, 0, 3, 5] == -1 and lab[0, 0, 3, 4] == 35 and lab[0, 0, 3, 6] == 39
    x[0, 0, 3, 5] = 2.0
    x[0, 0, 5, 9] = np.nan                                          # two away from the bar's end at (3, 8): not a neighbour
    assert cn.cells_np(x, (0.5,), 8)["cells"][0, 0, 0] == 1
    x[0, 0, 4, 9] = np.nan                                          # diagonal to (3, 8)
    assert cn.cells_np(x, (0.5,), 4)["cells"][0, 1, 0] == 1
    # the volume saturates at 2^20 per pixel and rounds half to even
    assert cn.quantum(np.array([3e9, 2.0 ** -17, 3 * 2.0 ** -17, 1.0], np.float32)).tolist() == [2 ** 36, 0, 2, 65536]


def test_stripes_against_a_run_length_count():
    rng = np.random.default_rng(4)
    col = rng.random(40) < 0.5
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], col.astype(int), [0]]))))[::2]
    p = np.zeros((40, 6), np.float32)
    p[col] = 1.0                                                    # whole rows: every run of wet rows is one cell of 6 L pixels
    for conn in (4, 8):
        o = cn.cells_np(day(p, 7), (0.5,), conn)
        assert o["cells"][0, :, 7].sum() == len(runs) and o["area_sum"][0].sum() == 6 * runs.sum() and o["area_sq_sum"][0].sum() == 36 * (runs ** 2).sum()
        assert o["largest_area"][0, int(np.log2(6 * runs.max()))] == 1
        cn.check_identities(o)


@pytest.mark.parametrize("p_wet", [0.05, 0.41, 0.59, 0.9])
def test_identities_on_random_fields(p_wet):
    rng = np.random.default_rng(int(p_wet * 100))
    x = (rng.gamma(0.6, 3.0, (2, 24, 9, 13)) * (rng.random((2, 24, 9, 13)) < p_wet)).astype(np.float32)
    x[0, 2, 4, 6], x[1, 5, 0, 0] = np.nan, np.inf
    for conn in (4, 8):
        o, lab = cn.cells_np(x, (0.0, 0.5, 4.0), conn, want_labels=1)
        cn.check_identities(o)
        assert o["n_bad_pixels"] == 2 and np.array_equal(lab, cn.labels_np(x, 0.5, conn))
        assert cn.flat_state(o).shape == (3 * CL.N_COUNTS + 2,)
    assert cn.cells_np(x, (0.5,), 8)["cells"].sum() <= cn.cells_np(x, (0.5,), 4)["cells"].sum()


def test_patterns():
    for ny, nx in ((13, 17), (130, 70)):
        for conn in (4, 8):
            for fig in (cn.spiral(ny, nx), cn.serpentine(ny, nx)):
                lab = cn.label_plane(fig > 0, conn)
                assert set(np.unique(lab).tolist()) == {-1, 0} and (lab == 0).sum() == (fig > 0).sum() > ny * nx // 3


def _stats(x, thr, conn=8):
    o = cn.cells_np(x, thr, conn)
    return CL.stats_from_state(cn.flat_state(o), thr, conn, x.shape[-1] * x.shape[-2])


def test_derived_quantities_and_compare():
    # hour 0: a single pixel of 2 mm and an interior 2 x 2 block of 1 mm; hour 1: a rim pixel of 4 mm; the other 22 hours dry
    x = np.zeros((1, 24, 6, 8), np.float32)
    x[0, 0, 1, 1], x[0, 0, 3:5, 4:6], x[0, 1, 0, 3] = 2.0, 1.0, 4.0
    s = _stats(x, (0.5, 3.0))
    assert s.n_planes == 24 and s.n_pixels == 48 and s.cell_count_by_hour()[0, :3].tolist() == [2, 1, 0]
    assert s.cell_count_by_hour(interior_only=True)[0, :2].tolist() == [2, 0]
    assert np.allclose(s.mean_cells_per_plane(), [3 / 24, 1 / 24])
    assert np.allclose(s.cells_per_plane_distribution()[0, :3], [22 / 24, 1 / 24, 1 / 24])
    assert np.allclose(s.area_distribution()[0, :3], [2 / 3, 0, 1 / 3]) and np.allclose(s.area_distribution(True)[0, [0, 2]], 0.5)
    assert np.allclose(s.mean_area(), [2.0, 1.0]) and np.allclose(s.area_weighted_mean_area(), [(1 + 16 + 1) / 6, 1.0])
    assert np.allclose(s.speckle_fraction(), [2 / 6, 1.0])
    mi = s.mean_intensity_by_area()
    assert mi[0, 0] == 3.0 and mi[0, 2] == 1.0 and np.isnan(mi[0, 1]) and mi[1, 0] == 4.0
    assert np.allclose(s.largest_cell_distribution()[0, [0, 2, 25]], [1 / 24, 1 / 24, 22 / 24])
    assert np.allclose(s.wet_fraction_by_hour()[0, :3], [5 / 48, 1 / 48, 0])
    c = CL.compare(s, s)
    assert all(np.all(c[k] == 0) for k in ("tv_area", "tv_cells_per_plane", "tv_largest_cell", "speckle_fraction", "wet_fraction_by_hour"))
    y = x.copy()
    y[0, 2, 2, 2] = 1.0
    c = CL.compare(s, _stats(y, (0.5, 3.0)))
    assert c["tv_cells_per_plane"][0] == pytest.approx(1 / 24) and c["tv_area"][0] == pytest.approx(abs(2 / 3 - 3 / 4)) and c["mean_area"][0] == pytest.approx(2 - 7 / 4)
    empty = _stats(np.zeros((1, 24, 3, 3), np.float32), (0.5,))
    assert np.all(np.isnan(empty.mean_area())) and np.all(np.isnan(empty.speckle_fraction())) and empty.largest_cell_distribution()[0, 25] == 1.0
    for other in (_stats(x, (0.5,)), _stats(x, (0.5, 3.0), 4), None):
        with pytest.raises(ValueError):
            CL.compare(s, other)
    with pytest.raises(ValueError):
        CL.split_state(np.zeros(5), 1)


def test_state_layout_round_trip():
    d = CL.split_state(np.arange(2 * CL.N_COUNTS + 2), 2)
    assert d["wet_pixels"][1, 0] == 317 and d["cells"][0, 1, 0] == 48 and d["area_hist"][0, 1, 0] == 97 and d["area_sum"][0, 1] == 123
    assert d["area_sq_sum"][0, 0] == 124 and d["volume_by_area"][0, 0, 1] == 127 and d["cells_per_plane"][0, 64] == 240
    assert d["largest_area"][0, 0] == 241 and d["dry_planes"][0] == 266 and d["area_by_area"][0, 1, 24] == 316
    assert d["n_planes"] == 634 and d["n_bad_pixels"] == 635


def test_argument_errors():
    for thr in ((), tuple(range(9)), (1.0, 0.5), (-1.0,), (np.nan,), (1.0, 1.0), "x"):
        with pytest.raises(ValueError):
            CL.CellStructure(thr)
    for conn in (0, 6, 8.0, True, "8"):
        with pytest.raises(ValueError):
            CL.CellStructure((0.1,), connectivity=conn)
    for ppp in (0, 65536, 2.5, True):
        with pytest.raises(ValueError):
            CL.CellStructure((0.1,), planes_per_pass=ppp)
    cs = CL.CellStructure((0.1,))
    for bad in (np.zeros((24, 5)), np.zeros((23, 4, 5)), np.zeros((2, 25, 4, 5)), np.zeros((0, 24, 4, 5)), np.zeros((24, 4, 5), dtype=complex),
                torch.zeros(24, 4, 5)):
        with pytest.raises(ValueError):
            cs.add(bad)
    with pytest.raises(ValueError):
        cs.add(np.zeros((24, 4, 5), np.float32), label_threshold=1)
    with pytest.raises(ValueError):
        cs.add(np.zeros((24, 4, 5), np.float32), labels_out=torch.zeros(24, 4, 5, dtype=torch.int32))           # on the host
    with pytest.raises(ValueError):
        cs.state()
    with pytest.raises(ValueError):
        CL.label_cells(torch.zeros(24, 4, 5), 0.1)
    cs.plane_shape = (4, 5)                                         # as after a first add
    with pytest.raises(ValueError):
        cs.add(np.zeros((24, 4, 6), np.float32))
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            CL.cell_structure(np.zeros((24, 4, 5), np.float32), (0.1,))
        with pytest.raises(_lib.RdganError):
            CL.label_cells(np.zeros((24, 4, 5), np.float32), 0.1)

    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    good = dict(gen=NoGenerator(), daily=np.zeros((20, 30), np.float32), n_scenarios=3, thresholds=(0.1,))
    for kw in (dict(thresholds=()), dict(connectivity=5), dict(planes_per_pass=0), dict(n_scenarios=0), dict(scenario_chunk=0), dict(overlap=9),
               dict(latent_mode="each"), dict(daily=np.zeros((2, 2, 20, 30), np.float32)), dict(daily=torch.zeros(20, 30)), dict(chunk=0),
               dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            CL.cell_structure_field(**{**good, **kw})


def test_cabi_argument_checks():
    """the two C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    ws = lib.rdgan_cells_workspace_bytes
    assert ws(5, 7, 1) == 35 * 16 + 8 and ws(5, 7, 3) == 3 * ws(5, 7, 1) and ws(4096, 4096, 2) == 2 * (16 * 2 ** 24 + 8)
    for a in ((0, 7, 1), (5, 0, 1), (5, 7, 0), (5, 7, 65536), (4097, 4096, 1), (2 ** 25, 1, 1), (-1, -1, 1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                 # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])

    def acc(x=good_p, n=1, stride=24 * 35, ny=5, nx=7, th=hp(thr), T=2, conn=8, counts=good_p, labels=null, lt=0, ws=good_p, nbytes=35 * 16 + 8):
        return lib.rdgan_cells_accumulate(x, n, stride, ny, nx, th, T, conn, counts, labels, lt, ws, nbytes, ctypes.c_void_p(0))

    unsorted, negative, nan = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0])), hp(np.array([np.nan, 1.0]))
    for kw in (dict(x=null), dict(counts=null), dict(ws=null), dict(th=null), dict(x=odd_p), dict(counts=four_p), dict(ws=four_p), dict(labels=odd_p),
               dict(n=0), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4096), dict(n=2 ** 40), dict(stride=24 * 35 - 1), dict(T=0), dict(T=9),
               dict(th=unsorted), dict(th=negative), dict(th=nan), dict(conn=0), dict(conn=6), dict(labels=good_p, lt=2), dict(labels=good_p, lt=-1),
               dict(nbytes=35 * 16 + 7), dict(nbytes=0), dict(nbytes=-5)):
        assert acc(**kw) == -2, kw


def test_header_and_lib_agree_on_the_cells_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "long long*": "c_void_p", "int*": "c_void_p"}
    for name in ("rdgan_cells_workspace_bytes", "rdgan_cells_accumulate"):
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)


def test_python_constants_are_the_kernel_header_s():
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_cells.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (CL.N_COUNTS, CL.N_BINS, CL.N_KPP, CL.MAX_PLANE, CL.MAX_PASS, CL.NHOURS) == tuple(
        value(m) for m in ("RD_CL_NC", "RD_CL_NBINS", "RD_CL_NKP", "RD_HOURLY_MAXPLANE", "RD_CL_MAXPASS", "RD_HOURS"))
    assert (CL._WET, CL._CELLS, CL._HIST, CL._ASUM, CL._ASQ, CL._VBA, CL._KPP, CL._LARGEST, CL._DRY, CL._ABA) == tuple(
        value(m) for m in ("RD_CL_WET", "RD_CL_CELLS", "RD_CL_HIST", "RD_CL_ASUM", "RD_CL_ASQ", "RD_CL_VBA", "RD_CL_KPP", "RD_CL_LARGEST", "RD_CL_DRY",
                           "RD_CL_ABA"))
    assert value("RD_CL_TILE") == 64 and 16 * value("RD_CL_THREADS") == value("RD_CL_TILE") ** 2
