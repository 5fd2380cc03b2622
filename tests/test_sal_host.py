"""CPU: sal_from_records, summary and compare of pr_disagg_radar_gan_amd/sal.py on hand-built numpy records against the yardstick's
formulas (tests/sal_np.py); the yardstick itself on closed forms; argument errors raised before any device call; the two C entries'
argument checks and the workspace size against the kernel header's formula."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, sal as SL
from tests import sal_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = (0.1, 1.0)


def records(x, thr=THR, conn=8):
    r = sn.records_np(x, thr, conn)
    return SL.PlaneRecords(r["plane"], r["objects"], r["vr"], x.shape[-2], x.shape[-1], tuple(float(np.float32(t)) for t in thr), conn)


def test_yardstick_on_closed_forms():
    p = np.zeros((9, 12), np.float32)
    p[2:4, 3:6] = 2.0                                                # 6 pixels of 2 mm: q = 2048 each
    p[7, 10] = 0.5                                                  # wet at 0.1 only
    p[0, 0], p[8, 11], p[5, 5] = np.nan, -3.0, 5000.0               # bad; clamped to 0; clamped to 2048 - 1/1024
    (n_bad, M0, Mx, My), objs, vrs = sn.plane_record(p, THR, 8)
    top = 2048 * 1024 - 1
    assert n_bad == 1 and M0 == 6 * 2048 + 512 + top and Mx == 2048 * 2 * (3 + 4 + 5) + 512 * 10 + top * 5
    assert My == 2048 * 3 * (2 + 3) + 512 * 7 + top * 5
    assert objs == [(3, 8, M0), (2, 7, M0 - 512)]
    V1 = (6 * 2048 * 6.0 + top * 1.0) / (M0 - 512)
    assert vrs[1][0] == pytest.approx(V1, rel=1e-15)
    cx, cy = Mx / M0, My / M0
    r1 = (6 * 2048 * math.hypot(4 - cx, 2.5 - cy) + top * math.hypot(5 - cx, 5 - cy)) / (M0 - 512)
    assert vrs[1][1] == pytest.approx(r1, rel=1e-14)
    assert sn.mass(np.array([0.0, 2.0 ** -11, 3 * 2.0 ** -11, 1.0, 2047.9995, 3e9, -1.0], np.float32)).tolist() == [0, 0, 2, 1024, top, top, 0]
    # an object without mass (below 1/2048 mm) counts as an object and weighs nothing
    z = np.zeros((3, 3), np.float32)
    z[1, 1] = 2.0 ** -13
    assert sn.plane_record(z, (0.0,), 4) == ((0, 0, 0, 0), [(1, 1, 0)], [(0.0, 0.0)])


def test_sal_from_records_against_the_yardstick_and_nan_rules():
    rng = np.random.default_rng(3)
    obs = (rng.gamma(0.7, 2.0, (2, 24, 9, 13)) * (rng.random((2, 24, 9, 13)) < 0.3)).astype(np.float32)
    ens = (rng.gamma(0.7, 2.5, (3, 2, 24, 9, 13)) * (rng.random((3, 2, 24, 9, 13)) < 0.3)).astype(np.float32)
    obs[0, 0], ens[:, 0, 1], obs[0, 2], ens[:, 0, 2] = 0.0, 0.0, 0.0, 0.0        # dry obs: A = 2; dry model: A = -2; both dry
    obs[1, 3, 2, 2] = np.nan                                         # a mask mismatch
    ens[1, 1, 4] = np.nan                                            # a model plane without a valid pixel
    obs[1, 5], ens[:, 1, 5] = 0.5, 0.5                               # wet at 0.1 only, one object each, the same
    m, o = records(ens), records(obs)
    got = SL.sal_from_records(m, o)
    assert got.S.shape == (3, 2, 24, 2) and got.mask_mismatch.dtype == bool
    for s in range(3):
        for d in range(2):
            for h in range(24):
                for t in range(2):
                    rec = lambda r, i: tuple(int(v) for v in r.plane[i]) + (int(r.objects[i + (t, 0)]),) + tuple(float(v) for v in r.vr[i + (t,)])
                    want = sn.sal_pair(rec(m, (s, d, h)), rec(o, (d, h)), 9, 13)
                    have = tuple(getattr(got, c)[s, d, h, t] for c in ("S", "A", "L1", "L2", "L", "mask_mismatch"))
                    for w, g in zip(want, have):
                        assert (math.isnan(w) and math.isnan(g)) or w == g or abs(w - g) <= 4 * 2.0 ** -52 * abs(w), (s, d, h, t, want, have)
    assert np.all(got.A[:, 0, 0] == 2.0) and np.all(np.isnan(got.S[:, 0, 0])) and np.all(np.isnan(got.L1[:, 0, 0])) and np.all(np.isnan(got.L2[:, 0, 0]))
    assert np.all(got.A[:, 0, 1] == -2.0) and np.all(np.isnan(got.L[:, 0, 1]))
    for c in SL.COMPONENTS:
        assert np.all(np.isnan(getattr(got, c)[:, 0, 2])), c       # dry against dry
    assert np.all(got.mask_mismatch[:, 1, 3]) and not got.mask_mismatch[:, 0].any() and got.mask_mismatch[1, 1, 4].all()
    assert np.all(np.isnan(got.A[1, 1, 4])) and np.all(np.isnan(got.L1[1, 1, 4]))
    assert np.all(got.S[:, 1, 5, 0] == 0) and np.all(got.A[:, 1, 5] == 0) and np.all(got.L[:, 1, 5, 0] == 0) and np.all(np.isnan(got.S[:, 1, 5, 1]))
    # identical records: every defined component is exactly 0
    same = SL.sal_from_records(o, o)
    for c in SL.COMPONENTS:
        a = getattr(same, c)
        assert np.all((a == 0) | np.isnan(a)), c


def test_summary_and_compare_on_a_fixed_array():
    S = np.full((4, 24, 2), np.nan)
    S[:, :, 0] = np.array([-1.0, 0.0, 1.0, 2.0])[:, None]
    S[0, :, 1] = 0.5                                                 # threshold 1: one member defined
    z = np.zeros((4, 24, 2))
    a = SL.SAL((0.1, 1.0), 8, 5, 7, S=S, A=z, L1=z, L2=z + 0.25, L=z + 0.25, mask_mismatch=z.astype(bool))
    s = a.summary()
    assert s["S"]["median"].tolist() == [0.5, 0.5] and s["S"]["q25"].tolist() == [-0.25, 0.5] and s["S"]["q75"].tolist() == [1.25, 0.5]
    assert s["S"]["mean_abs"].tolist() == [1.0, 0.5] and s["S"]["undefined"].tolist() == [0.0, 0.75] and s["S"]["by_hour"].shape == (24, 2)
    assert np.all(s["S"]["by_hour"] == 0.5) and s["L"]["median"].tolist() == [0.25, 0.25] and s["mask_mismatch"] == 0.0
    empty = SL.SAL((0.1,), 8, 5, 7, *(np.full((2, 24, 1), np.nan),) * 5, mask_mismatch=np.zeros((2, 24, 1), bool)).summary()
    assert np.isnan(empty["A"]["median"][0]) and empty["A"]["undefined"][0] == 1.0 and np.all(np.isnan(empty["A"]["by_hour"]))
    c = SL.compare(a, a)
    assert all(np.all((c[k][f] == 0) | np.isnan(c[k][f])) for k in SL.COMPONENTS for f in c[k])
    b = SL.SAL((0.1, 1.0), 8, 5, 7, S=S + 1.0, A=z, L1=z, L2=z, L=z, mask_mismatch=z.astype(bool))
    c = SL.compare(a, b.summary())
    assert c["S"]["median"].tolist() == [-1.0, -1.0] and c["L"]["mean_abs"].tolist() == [0.25, 0.25]
    with pytest.raises(ValueError):
        SL.compare(a, SL.SAL((0.1,), 8, 5, 7, *(np.zeros((1, 24, 1)),) * 5, mask_mismatch=np.zeros((1, 24, 1), bool)))
    with pytest.raises(ValueError):
        SL.compare(a, None)


def test_mismatched_records_are_refused():
    x = np.zeros((1, 24, 5, 7), np.float32)
    a = records(x)
    for other in (records(np.zeros((1, 24, 7, 5), np.float32)), records(x, (0.1, 2.0)), records(x, THR, 4),
                  None):
        with pytest.raises(ValueError):
            SL.sal_from_records(a, other)
    with pytest.raises(ValueError):
        SL.sal_from_records(records(np.zeros((2, 24, 5, 7), np.float32)), records(np.zeros((3, 24, 5, 7), np.float32)))


def test_argument_errors_before_any_device_call():
    good = np.zeros((24, 4, 5), np.float32)
    for thr in ((), tuple(range(9)), (1.0, 0.5), (-1.0,), (np.nan,), "x"):
        with pytest.raises(ValueError):
            SL.plane_records(good, thr)
        with pytest.raises(ValueError):
            SL.sal_hourly(good[None], good, thr)
    for kw in (dict(connectivity=6), dict(connectivity=True), dict(planes_per_pass=0), dict(planes_per_pass=65536)):
        with pytest.raises(ValueError):
            SL.plane_records(good, (0.1,), **kw)
        with pytest.raises(ValueError):
            SL.sal_hourly(good[None], good, (0.1,), **kw)
    overflow = np.broadcast_to(np.float32(0), (24, 64, 1 << 18))     # 2^21 * 2^18 * 2^24 = 2^63
    for bad in (torch.zeros(24, 4, 5), np.zeros((23, 4, 5)), np.zeros((24, 5)), np.zeros((0, 24, 4, 5)), np.zeros((24, 4, 5), dtype=complex), overflow):
        with pytest.raises(ValueError):
            SL.plane_records(bad, (0.1,))
    SL.check_plane(63, 1 << 18)
    with pytest.raises(ValueError):
        SL.check_plane(1 << 12, 1 << 13)                             # 2^25 pixels
    for ens, obs in ((good, good), (np.zeros((2, 24, 4, 6), np.float32), good), (torch.zeros(1, 24, 4, 5), good), (good[None], torch.zeros(24, 4, 5)),
                     (np.broadcast_to(np.float32(0), (4097, 24, 4, 5)), good), (np.broadcast_to(np.float32(0), (1, 24, 64, 1 << 18)), overflow)):
        with pytest.raises(ValueError):
            SL.sal_hourly(ens, obs, (0.1,))
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            SL.plane_records(good, (0.1,))
        with pytest.raises(_lib.RdganError):
            SL.sal_hourly(good[None], good, (0.1,))

    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    ok = dict(gen=NoGenerator(), observed=np.zeros((24, 20, 30), np.float32), n_scenarios=3, thresholds=(0.1,))
    for kw in (dict(thresholds=()), dict(connectivity=5), dict(planes_per_pass=0), dict(n_scenarios=0), dict(n_scenarios=4097), dict(scenario_chunk=0),
               dict(overlap=9), dict(latent_mode="each"), dict(observed=np.zeros((2, 2, 24, 20, 30), np.float32)), dict(observed=torch.zeros(24, 20, 30)),
               dict(observed=np.zeros((20, 30), np.float32)), dict(daily=np.zeros((20, 31), np.float32)), dict(chunk=0), dict(norm_scale=0.0),
               dict(observed=np.broadcast_to(np.float32(0), (24, 64, 1 << 18)))):
        with pytest.raises(ValueError):
            SL.sal_field(**{**ok, **kw})
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RdganError):
            SL.sal_field(**ok)


def test_cabi_argument_checks_and_workspace_bytes():
    """the two C entries refuse a bad argument before they touch the device: callable without one.  The size is
    rd_sal_ws_bytes(plane, P) = rd_cl_ws_bytes(plane, P) + P (32 plane + 40 ceil(plane / 4096) + 192), restated here from the header"""
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_sal.hip.h")).read()
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("LL", ""))
    assert (value("RD_SAL_CHUNK"), value("RD_SAL_MAXMOMENT")) == (SL.CHUNK, SL.MAX_MOMENT) and value("RD_SAL_NPART") == 5 and value("RD_SAL_SINK") == 24
    assert "rd_cl_ws_bytes(plane, P) + P * (plane * 32 + rd_sal_chunks(plane) * RD_SAL_NPART * 8 + RD_SAL_SINK * 8)" in text
    lib = _lib.load()
    ws = lib.rdgan_sal_workspace_bytes
    want = lambda ny, nx, P: P * (ny * nx * 16 + 8) + P * (ny * nx * 32 + -(-ny * nx // 4096) * 40 + 192)
    for ny, nx, P in ((5, 7, 1), (70, 130, 5), (4096, 4096, 2)):
        assert ws(ny, nx, P) == want(ny, nx, P), (ny, nx, P)
        assert ws(ny, nx, P) == P * ws(ny, nx, 1)
    for a in ((0, 7, 1), (5, 0, 1), (5, 7, 0), (5, 7, 65536), (4097, 4096, 1), (2 ** 25, 1, 1), (-1, -1, 1), (64, 1 << 18, 1), (1 << 18, 64, 1)):
        assert ws(*a) == -2, a
    assert ws(63, 1 << 18, 1) > 0
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                 # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])
    one = want(5, 7, 1)

    def rec(x=good_p, n=1, stride=24 * 35, ny=5, nx=7, th=hp(thr), T=2, conn=8, plane=good_p, obj=good_p, vr=good_p, ws=good_p, nbytes=one):
        return lib.rdgan_sal_records(x, n, stride, ny, nx, th, T, conn, plane, obj, vr, ws, nbytes, ctypes.c_void_p(0))

    unsorted, negative, nan = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0])), hp(np.array([np.nan, 1.0]))
    for kw in (dict(x=null), dict(plane=null), dict(obj=null), dict(vr=null), dict(ws=null), dict(th=null), dict(x=odd_p), dict(plane=four_p),
               dict(obj=four_p), dict(vr=four_p), dict(ws=four_p), dict(n=0), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4096), dict(n=2 ** 40),
               dict(stride=24 * 35 - 1), dict(T=0), dict(T=9), dict(th=unsorted), dict(th=negative), dict(th=nan), dict(conn=0), dict(conn=6),
               dict(nbytes=one - 1), dict(nbytes=0), dict(nbytes=-5),
               dict(ny=64, nx=1 << 18, stride=24 << 24, nbytes=1 << 40), dict(ny=1 << 18, nx=64, stride=24 << 24, nbytes=1 << 40)):
        assert rec(**kw) == -2, kw


def test_header_and_lib_agree_on_the_sal_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "long long*": "c_void_p", "double*": "c_void_p"}
    for name in ("rdgan_sal_workspace_bytes", "rdgan_sal_records"):
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
