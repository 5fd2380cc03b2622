"""CPU: the yardstick of the distance-map verification (tests/distmap_np.py) and measures_from_records of
pr_disagg_radar_gan_amd/distmap.py on closed forms; the separable transform against the brute force; floor(sqrt(double(v))) against
the integer root for every 256 d2 a 2048 x 2048 plane can produce; the host arithmetic against exact fractions; NaN rules; argument
errors raised before any device call; the C entries' argument checks and the workspace size against the kernel header's formula."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, distmap as DM
from tests import distmap_np as yn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52


def day(plane):
    """(24, ny, nx): the plane in every hour"""
    return np.broadcast_to(np.asarray(plane, np.float32), (24,) + np.shape(plane)).copy()


def measures_of(members, obs, thr, C=None, lam=0.5):
    ny, nx = obs.shape[-2:]
    rec = yn.records_np(members, obs, thr, C)
    pr = DM.PairRecords(rec, tuple(thr), yn.default_cutoff16(ny, nx) if C is None else C, ny, nx)
    return DM.measures_from_records(pr, lam)


def close(got, want, ulps=4):
    """a float against a Fraction or a float (None: NaN)"""
    if want is None:
        return math.isnan(got)
    return abs(Fraction(got) - Fraction(want)) <= ulps * ULP * abs(Fraction(want))


def test_separable_transform_equals_the_brute_force():
    rng = np.random.default_rng(0)
    for ny, nx, p in ((1, 1, 1.0), (1, 9, 0.3), (9, 1, 0.3), (7, 13, 0.1), (20, 33, 0.02), (33, 20, 0.5), (40, 40, 0.003), (65, 67, 0.01)):
        m = rng.random((ny, nx)) < p
        m[rng.integers(ny), rng.integers(nx)] = True
        assert np.array_equal(yn.d2_brute(m), yn.d2_separable(m)), (ny, nx)
    assert yn.d2_brute(np.zeros((4, 5), bool)) is None and yn.d2_separable(np.zeros((4, 5), bool)) is None
    # one set pixel: d2 is the squared distance to it; D its quantised root
    m = np.zeros((6, 9), bool)
    m[2, 3] = True
    yy, xx = np.indices(m.shape)
    assert np.array_equal(yn.d2_np(m), (yy - 2) ** 2 + (xx - 3) ** 2)
    assert yn.quantise(yn.d2_np(m))[5, 8] == math.isqrt(256 * 34) == 93 and yn.quantise(yn.d2_np(m))[2, 3] == 0
    maps, sizes = yn.maps_np(day(np.where(m, 2.0, 0.0)), (0.5, 3.0))
    assert maps.dtype == np.uint16 and maps.shape == (24, 2, 6, 9) and sizes.tolist() == [[1, 0]] * 24
    assert (maps[:, 1] == 0xFFFF).all() and maps[0, 0, 5, 8] == 93


def test_the_fp64_root_is_the_integer_root_for_every_distance_a_plane_can_hold():
    """D = floor(sqrt((double)(256 d2))) in the kernel: equal to isqrt for every dy^2 + dx^2 with dy, dx <= 2047"""
    sq = np.arange(2048, dtype=np.int64) ** 2
    top = 0
    for dy in range(0, 2048, 64):                                    # 64 rows of the table at a time
        v = 256 * (sq[dy:dy + 64, None] + sq[None, :])
        r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
        assert np.all(r * r <= v) and np.all((r + 1) * (r + 1) > v)       # r is the integer root, by its definition
        top = max(top, int(r.max()))
    assert top == math.isqrt(256 * 2 * 2047 ** 2) == 46318 and top < 0xFFFF and 256 * 2 * 2047 ** 2 < 2 ** 31
    for v in (0, 1, 255, 256, 46318 ** 2 - 1, 46318 ** 2, 2 ** 31 - 1):
        assert int(math.floor(math.sqrt(float(v)))) == math.isqrt(v)
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_distmap.hip.h")).read()
    assert "__dsqrt_rn((double)(best << 8))" in text and "2^-17" in text  # the kernel takes this root, and says why it may


def test_closed_forms():
    thr = (0.5,)
    rng = np.random.default_rng(1)
    f = np.where(rng.random((12, 15)) < 0.3, 2.0, 0.0).astype(np.float32)
    f[0, 0] = 2.0
    # identical fields: every distance 0
    m = measures_of(day(f)[None], day(f), thr)
    for a in (m.hausdorff, m.med_model_to_obs, m.med_obs_to_model, m.baddeley(1), m.baddeley(2), m.baddeley(np.inf), m.zhu):
        assert np.all(a == 0)
    assert np.all(m.csi == 1) and np.all(m.flags == 0) and m.hausdorff.shape == (1, 1, 24, 1)
    # one wet pixel each, k pixels apart: Hausdorff, both MED and Delta_inf are floor(16 k) / 16.  For Delta_inf this holds where
    # 16 k is whole: |d(x, A) - d(x, B)| <= k gives |D(x, A) - D(x, B)| <= 16 k then.  Otherwise the two floors of a pixel behind
    # one of the sets can differ by floor(16 k) + 1 (the last pair: 129 against floor(16 sqrt(65)) = 128), and by no more
    for (ay, ax), (by, bx) in (((2, 3), (2, 8)), ((1, 1), (4, 5)), ((0, 0), (11, 14)), ((7, 2), (3, 9))):
        a, b = np.zeros((12, 15), np.float32), np.zeros((12, 15), np.float32)
        a[ay, ax], b[by, bx] = 1.0, 1.0
        m = measures_of(day(a)[None], day(b), thr)
        k2 = (ay - by) ** 2 + (ax - bx) ** 2
        want = math.isqrt(256 * k2) / 16
        assert want == math.floor(16 * math.hypot(ay - by, ax - bx)) / 16
        for got in (m.hausdorff, m.med_model_to_obs, m.med_obs_to_model):
            assert np.all(got == want), ((ay, ax), (by, bx))
        whole = math.isqrt(256 * k2) ** 2 == 256 * k2
        assert np.all(m.baddeley(np.inf) == want) if whole else np.all((m.baddeley(np.inf) == want) | (m.baddeley(np.inf) == want + 1 / 16))
        assert np.all(m.csi == 0) and np.all(m.zhu == 0.5 * math.sqrt(2 / 180) + 0.5 * want)
    # an empty member set: MED, Hausdorff and Zhu are NaN, Delta is finite and what the cutoff implies
    b = np.zeros((12, 15), np.float32)
    b[3, 4] = 1.0
    DB = yn.quantise(yn.d2_np(b > 0.5))
    for C in (None, 40, 16 * 4):
        c = yn.default_cutoff16(12, 15) if C is None else C
        m = measures_of(day(np.zeros((12, 15)))[None], day(b), thr, C)
        assert np.all(np.isnan(m.hausdorff)) and np.all(np.isnan(m.med_model_to_obs)) and np.all(np.isnan(m.med_obs_to_model)) and np.all(np.isnan(m.zhu))
        assert np.all(m.flags == 2) and np.all(m.csi == 0)
        d = c - np.minimum(DB, c)
        assert close(m.baddeley(1)[0, 0, 0, 0], Fraction(int(d.sum()), 16 * 180)) and m.baddeley(np.inf)[0, 0, 0, 0] == d.max() / 16
        assert close(m.baddeley(2)[0, 0, 0, 0], math.sqrt(Fraction(int((d * d).sum()), 256 * 180)), 8)
    assert yn.default_cutoff16(12, 15) == math.ceil(16 * math.hypot(11, 14)) == DM.cutoff16(None, 12, 15)
    # both empty: Delta is 0, csi 0 / 0
    m = measures_of(day(np.zeros((12, 15)))[None], day(np.zeros((12, 15))), thr)
    assert np.all(m.flags == 6) and np.all(m.baddeley(1) == 0) and np.all(m.baddeley(np.inf) == 0) and np.all(np.isnan(m.csi)) and np.all(np.isnan(m.hausdorff))


def test_bad_pixels_valid_counts_and_flags():
    thr = (0.5, 1.5)
    a, b = np.zeros((6, 8), np.float32), np.zeros((6, 8), np.float32)
    a[1, 1], a[4, 6], b[1, 2], b[4, 6] = 2.0, 1.0, 2.0, np.nan          # the member's (4, 6) lies on a bad observed pixel
    a[0, 7] = np.inf
    rec = yn.records_np(day(a)[None], day(b), thr)[0, 0, 0]
    assert rec[0, 0] == 46 and rec[0, 1:4].tolist() == [1, 1, 0] and rec[0, 11] == 1
    assert rec[0, 4] == 16 and rec[0, 5] == 16 and rec[0, 6] == 16 and rec[0, 7] == 16          # distances run across the bad pixels
    assert rec[1, 1:4].tolist() == [1, 1, 0] and rec[1, 11] == 1
    # n_valid = 0: every measure NaN
    m = measures_of(day(np.full((3, 3), np.nan))[None], day(np.ones((3, 3))), (0.5,))
    assert np.all(m.records.records[..., 0] == 0) and np.all(np.isnan(m.baddeley(1))) and np.all(np.isnan(m.baddeley(2))) and np.all(np.isnan(m.baddeley(np.inf)))
    assert np.all(np.isnan(m.hausdorff)) and np.all(m.flags == 3)


def test_measures_against_exact_fractions():
    rng = np.random.default_rng(3)
    thr = (0.1, 1.0)
    obs = (rng.random((2, 24, 9, 11)) * 3 * (rng.random((2, 24, 9, 11)) < 0.3)).astype(np.float32)
    ens = (rng.random((2, 2, 24, 9, 11)) * 3 * (rng.random((2, 2, 24, 9, 11)) < 0.3)).astype(np.float32)
    ens[0, 0, 0, 2, 2], obs[1, 3, 0, 0], ens[1, 1, 5] = np.nan, np.inf, 0.0
    lam = 0.25
    m = measures_of(ens, obs, thr, 70, lam)
    r = m.records.records
    assert r.shape == (2, 2, 24, 2, 12)
    for idx in np.ndindex(r.shape[:-1]):
        n, nA, nB, nAB, s4, s5, m6, m7, s8, s9, m10, fl = (int(v) for v in r[idx])
        both = not fl & 6
        med = Fraction(s4, 16 * nB) if both and nB else None
        assert close(m.med_model_to_obs[idx], med) and close(m.med_obs_to_model[idx], Fraction(s5, 16 * nA) if both and nA else None)
        assert close(m.hausdorff[idx], Fraction(max(m6, m7), 16) if both and nA and nB else None, 0)
        assert close(m.baddeley(1)[idx], Fraction(s8, 16 * n)) and close(m.baddeley(np.inf)[idx], Fraction(m10, 16), 0)
        assert close(m.baddeley(2)[idx], math.sqrt(Fraction(s9, 256 * n)), 4)
        assert close(m.csi[idx], Fraction(nAB, nA + nB - nAB) if nA + nB - nAB else None)
        if med is None:
            assert math.isnan(m.zhu[idx])
        else:
            assert abs(m.zhu[idx] - (lam * math.sqrt(Fraction(nA + nB - 2 * nAB, n)) + (1 - lam) * float(med))) <= 8 * ULP * max(1.0, m.zhu[idx])
    s = m.summary()
    assert s["thresholds"] == thr and s["cutoff_px"] == 70 / 16 and set(DM.MEASURES) <= set(s)
    for name in DM.MEASURES:
        assert all(s[name][k].shape == (24, 2) for k in ("median", "q25", "q75", "undefined"))
    assert s["hausdorff"]["undefined"][5, 0] == 0.25 and np.allclose(s["csi"]["median"][0], np.nanmedian(m.csi[:, :, 0].reshape(-1, 2), axis=0))
    d = DM.compare(m, m)
    assert all(np.all((d[name]["undefined"] == 0)) for name in DM.MEASURES)
    with pytest.raises(ValueError):
        DM.compare(m, measures_of(ens, obs, thr, 71))
    with pytest.raises(ValueError):
        DM.compare(m, 3)


def test_argument_errors_before_any_device_call():
    good = np.zeros((24, 16, 20), np.float32)
    for thr in ((), tuple(range(9)), (1.0, 0.5), (-1.0,), (np.nan,), "x"):
        with pytest.raises(ValueError):
            DM.DistanceMapVerifier(good, thr)
        with pytest.raises(ValueError):
            DM.distance_maps(good, thr)
        with pytest.raises(ValueError):
            DM.distmap_hourly(good[None], good, thr)
    wide, tall = np.broadcast_to(np.float32(0), (24, 2, 2049)), np.broadcast_to(np.float32(0), (24, 2049, 2))
    for bad in (torch.zeros(24, 16, 20), np.zeros((23, 16, 20)), np.zeros((24, 20)), np.zeros((24, 16, 20), dtype=complex), wide, tall):
        with pytest.raises(ValueError):
            DM.DistanceMapVerifier(bad, (0.1,))
        with pytest.raises(ValueError):
            DM.distance_maps(bad, (0.1,))
    for kw in (dict(planes_per_pass=0), dict(planes_per_pass=(1 << 20) + 1), dict(planes_per_pass=1.5), dict(cutoff_px=0.9), dict(cutoff_px=4096),
               dict(cutoff_px=np.nan), dict(cutoff_px="3"), dict(cutoff_px=True), dict(max_map_bytes=2 * 24 * 16 * 20 - 1), dict(max_map_bytes=0),
               dict(max_map_bytes=1.5)):
        with pytest.raises(ValueError):
            DM.DistanceMapVerifier(good, (0.1,), **kw)
        with pytest.raises(ValueError):
            DM.distmap_hourly(good[None], good, (0.1,), **kw)
    with pytest.raises(ValueError, match="max_map_bytes"):
        DM.DistanceMapVerifier(np.broadcast_to(np.float32(0), (100, 24, 512, 512)), (0.1, 1.0))       # 2.5 GB of maps
    for kw in (dict(planes_per_pass=0), dict(planes_per_pass=True)):
        with pytest.raises(ValueError):
            DM.distance_maps(good, (0.1,), **kw)
    assert DM.cutoff16(1, 5, 5) == 16 and DM.cutoff16(4095.875, 5, 5) == 65534 and DM.cutoff16(2.53, 5, 5) == 40 and DM.cutoff16(None, 1, 1) == 16
    assert DM.cutoff16(None, 2048, 2048) == 46319 and DM.cutoff16(None, 4, 5) == 80
    for ens in (good, np.zeros((2, 24, 16, 21), np.float32), torch.zeros(1, 24, 16, 20), np.broadcast_to(np.float32(0), (4097, 24, 16, 20))):
        with pytest.raises(ValueError):
            DM.distmap_hourly(ens, good, (0.1,))
    for lam in (-0.1, 1.1, "x", np.nan):
        with pytest.raises(ValueError):
            DM.distmap_hourly(good[None], good, (0.1,), zhu_lambda=lam)
        with pytest.raises(ValueError):
            DM.measures_from_records(DM.PairRecords(np.zeros((1, 12), np.int64), (0.1,), 16, 4, 4), lam)
    for rec in (np.zeros((1, 11), np.int64), np.zeros((1, 12), np.float64)):
        with pytest.raises(ValueError):
            DM.measures_from_records(DM.PairRecords(rec, (0.1,), 16, 4, 4))
    with pytest.raises(ValueError):
        DM.measures_from_records(np.zeros((1, 12), np.int64))
    # add's own checks, on a verifier built without a device
    v = object.__new__(DM.DistanceMapVerifier)
    v.shape, v._parts = (24, 16, 20), []
    for members in (torch.zeros(2, 24, 16, 20), np.zeros((2, 24, 16, 21), np.float32), np.broadcast_to(np.float32(0), (4097, 24, 16, 20)), good):
        with pytest.raises(ValueError):
            v.add(members)
    with pytest.raises(ValueError):
        v.records()
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            DM.DistanceMapVerifier(good, (0.1,))
        with pytest.raises(_lib.RdganError):
            DM.distance_maps(good, (0.1,))
        with pytest.raises(_lib.RdganError):
            DM.distmap_hourly(good[None], good, (0.1,))

    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    ok = dict(gen=NoGenerator(), observed=np.zeros((24, 20, 30), np.float32), n_scenarios=3, thresholds=(0.1,))
    for kw in (dict(thresholds=()), dict(cutoff_px=0.5), dict(planes_per_pass=0), dict(max_map_bytes=100), dict(zhu_lambda=2), dict(n_scenarios=0),
               dict(n_scenarios=4097), dict(scenario_chunk=0), dict(overlap=9), dict(latent_mode="each"),
               dict(observed=np.zeros((2, 2, 24, 20, 30), np.float32)), dict(observed=torch.zeros(24, 20, 30)), dict(observed=np.zeros((20, 30), np.float32)),
               dict(observed=np.broadcast_to(np.float32(0), (24, 2049, 30))), dict(daily=np.zeros((20, 31), np.float32)), dict(chunk=0),
               dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            DM.distmap_field(**{**ok, **kw})
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RdganError):
            DM.distmap_field(**ok)


def test_cabi_argument_checks_and_workspace_bytes():
    """the C entries refuse a bad argument before they touch the device: callable without one.  The size restates the header: per
    plane 1 + 8 masks of ny ceil(nx / 64) words and 8 set sizes"""
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_distmap.hip.h")).read()
    assert "return (1 + RD_THR_MAX) * ny * ((nx + 63) / 64) * 8 + RD_THR_MAX * 8;" in text and "#define RD_DM_MAXSIDE 2048" in text
    lib = _lib.load()
    ws = lib.rdgan_dm_workspace_bytes
    want = lambda ny, nx, planes: planes * (9 * ny * -(-nx // 64) * 8 + 64)
    for a in ((64, 64, 1), (8, 8, 7), (65, 67, 3), (1, 200, 2), (200, 1, 2), (2048, 2048, 5), (1100, 40, 1 << 20)):
        assert ws(*a) == want(*a), a
    for a in ((0, 64, 1), (64, 0, 1), (2049, 64, 1), (64, 2049, 1), (64, 64, 0), (64, 64, (1 << 20) + 1), (-1, -1, 1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                 # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    two_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])
    unsorted, negative, nan = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0])), hp(np.array([np.nan, 1.0]))
    ny, nx = 16, 20
    day_elems, one = 24 * ny * nx, want(16, 20, 1)

    def maps(x=good_p, n=2, stride=day_elems, ny=ny, nx=nx, th=hp(thr), T=2, out=good_p, sizes=good_p, ws=good_p, nbytes=one):
        return lib.rdgan_dm_maps(x, n, stride, ny, nx, th, T, out, sizes, ws, nbytes, ctypes.c_void_p(0))

    for kw in (dict(x=null), dict(out=null), dict(sizes=null), dict(ws=null), dict(th=null), dict(x=two_p), dict(out=odd_p), dict(sizes=four_p),
               dict(ws=four_p), dict(n=0), dict(ny=0), dict(nx=0), dict(ny=2049, stride=24 * 2049 * nx), dict(nx=2049, stride=24 * ny * 2049),
               dict(n=1 << 40, stride=day_elems), dict(stride=day_elems - 1), dict(T=0), dict(T=9), dict(th=unsorted), dict(th=negative), dict(th=nan),
               dict(nbytes=one - 1), dict(nbytes=0), dict(nbytes=-5)):
        assert maps(**kw) == -2, kw
    P = 2 * day_elems

    def rec(m=good_p, s=2, stride=P, obs=good_p, om=good_p, n_days=2, ny=ny, nx=nx, th=hp(thr), T=2, C=100, out=good_p, ws=good_p, nbytes=one):
        return lib.rdgan_dm_records(m, s, stride, obs, om, n_days, ny, nx, th, T, C, out, ws, nbytes, ctypes.c_void_p(0))

    for kw in (dict(m=null), dict(obs=null), dict(om=null), dict(out=null), dict(ws=null), dict(th=null), dict(m=two_p), dict(obs=two_p), dict(om=odd_p),
               dict(out=four_p), dict(ws=four_p), dict(s=0), dict(s=4097), dict(n_days=0), dict(ny=0), dict(nx=0),
               dict(ny=2049, stride=2 * 24 * 2049 * nx), dict(nx=2049, stride=2 * 24 * ny * 2049), dict(n_days=1 << 40, stride=1 << 50),
               dict(s=4096, n_days=1 << 17, stride=day_elems << 17), dict(stride=P - 1), dict(T=0), dict(T=9), dict(th=unsorted), dict(th=negative),
               dict(th=nan), dict(C=15), dict(C=65535), dict(C=-1), dict(nbytes=one - 1), dict(nbytes=0), dict(nbytes=-5)):
        assert rec(**kw) == -2, kw


def test_header_and_lib_agree_on_the_distmap_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "long long*": "c_void_p", "unsigned short*": "c_void_p", "const unsigned short*": "c_void_p"}
    names = ("rdgan_dm_workspace_bytes", "rdgan_dm_maps", "rdgan_dm_records")
    assert tuple(sorted(n for n in _lib.SIGNATURES if n.startswith("rdgan_dm_"))) == tuple(sorted(names))
    for name in names:
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
    entries = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_eval_entries.h")).read()
    for name in names:
        assert f'extern "C" {"long" if name.endswith("bytes") else "int"} {name}(' in entries
