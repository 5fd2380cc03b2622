"""CPU: the numpy yardstick of the joint-field scores (tests/mvscore_np.py) against answers worked out by hand and against the
closed-form ensemble CRPS; the argument checks of pr_disagg_radar_gan_amd/multivariate.py and of the C entries; header against
_lib.py and the kernel header's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, multivariate as MV
from tests import mvscore_np as mn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rdgan_mv_energy", "rdgan_mv_energy_workspace_bytes", "rdgan_mv_variogram", "rdgan_mv_variogram_workspace_bytes")


def rain(rng, shape, dry=0.6):
    """gamma-distributed amounts with about 60 % zeros, as small_case of tests/test_analog_host.py builds them"""
    return (rng.gamma(0.5, 4.0, shape) * (rng.random(shape) < 1.0 - dry)).astype(np.float32)


def test_energy_by_hand():
    x = np.zeros((1, 24, 1, 2), np.float32)
    y = np.zeros((24, 1, 2), np.float32)
    x[0, 3, 0, 0], x[0, 7, 0, 1] = 3.0, 4.0                                              # |x - y| = 5
    assert mn.energy_terms(x, y) == (5.0, 0.0)
    assert mn.energy_score(x, y) == 5.0 and mn.energy_score(x, y, fair=True) == 5.0       # m = 1: the spread term is 0
    # two members at distance 3 and 4 from y and 5 apart
    x = np.zeros((2, 24, 1, 2), np.float32)
    x[0, 0, 0, 0], x[1, 0, 0, 1] = 3.0, 4.0
    assert mn.energy_terms(x, y) == (7.0, 5.0)
    assert mn.energy_score(x, y) == 3.5 - 5.0 / 4 and mn.energy_score(x, y, fair=True) == 3.5 - 5.0 / 2
    # an ensemble equal to the observation
    y = rain(np.random.default_rng(0), (24, 3, 4))
    x = np.broadcast_to(y, (5, 24, 3, 4))
    assert mn.energy_terms(x, y) == (0.0, 0.0) and mn.energy_score(x, y) == 0.0
    sq, count = mn.variogram_tables(x, y, 0.5, 2, 1)
    assert np.all(sq == 0.0) and count.sum() > 0
    # NaN positions are left out; none left: NaN
    y2 = y.copy()
    y2[2, 1, 1] = np.nan
    x2 = rain(np.random.default_rng(1), (3, 24, 3, 4))
    x3 = x2.copy()
    x3[:, 2, 1, 1] += 100.0
    assert mn.energy_terms(x2, y2) == mn.energy_terms(x3, y2)
    assert np.isnan(mn.energy_score(x2, np.full_like(y, np.nan)))


def test_variogram_by_hand():
    """a 1 x 2 plane, radius 1, one lag: lag 0 has the single displacement (0, 0, 1) with 24 pairs; lag 1 has (1, 0, -1), (1, 0, 0),
    (1, 0, 1) with 23, 46 and 23 pairs"""
    y = np.zeros((24, 1, 2), np.float32)
    y[:, 0, 1] = 4.0                                                                       # o = 2 across the plane (p = 0.5), 0 in time
    x = np.zeros((2, 24, 1, 2), np.float32)
    x[0, :, 0, 1], x[1, :, 0, 1] = 1.0, 9.0                                               # v = 1 and 3: mean 2
    sq, count = mn.variogram_tables(x, y, 0.5, 1, 1)
    want_count = np.zeros((2, 3, 3), np.int64)
    want_count[0, 1, 2], want_count[1, 1, 0], want_count[1, 1, 1], want_count[1, 1, 2] = 24, 23, 46, 23
    assert np.array_equal(count, want_count) and np.all(sq == 0.0)
    x[1, :, 0, 1] = 25.0                                                                   # v = 1 and 5: mean 3, (2 - 3)^2 per pair
    sq, count = mn.variogram_tables(x, y, 0.5, 1, 1)
    want = np.zeros((2, 3, 3))
    want[0, 1, 2], want[1, 1, 0], want[1, 1, 2] = 24.0, 23.0, 23.0
    assert np.array_equal(sq, want) and np.array_equal(count, want_count)
    vs = 24.0 + 46.0 / np.sqrt(2.0)                                                        # weights 1, 1 / sqrt(2) twice (and 1 on a zero)
    assert abs(mn.variogram_score(x, y, 0.5, 1, 1) - vs) < 1e-13
    assert abs(mn.variogram_score(x, y, 0.5, 1, 1, normalised=True) - vs / (24 + 46 + 46 / np.sqrt(2.0))) < 1e-15
    sq1, _ = mn.variogram_tables(x, y, 1, 1, 1)                                            # p = 1: o = 4, v = 1 and 25: mean 13
    assert sq1[0, 1, 2] == 24 * 81.0
    y[5, 0, 0] = np.nan                                                                    # hour 5's pair, and four pairs in time
    sq, count = mn.variogram_tables(x, y, 0.5, 1, 1)
    assert count[0, 1, 2] == 23 and count[1, 1, 1] == 44 and count[1, 1, 0] == 22 and count[1, 1, 2] == 22


def test_energy_of_one_position_is_the_crps():
    """with all but one pixel-hour masked the vector is a scalar and ES is the ensemble CRPS in closed form"""
    rng = np.random.default_rng(3)
    x = rain(rng, (40, 24, 3, 5))
    for pos, fair in (((7, 1, 2), False), ((0, 0, 0), False), ((23, 2, 4), True)):
        y = np.full((24, 3, 5), np.nan, np.float32)
        y[pos] = rng.gamma(0.5, 4.0)
        xs = x[(slice(None),) + pos].astype(np.float64)
        if fair:
            want = np.abs(xs - y[pos]).mean() - np.abs(xs[:, None] - xs[None, :]).sum() / (2.0 * 40 * 39)
        else:
            want = mn.crps_ensemble(xs, float(y[pos]))
        assert abs(mn.energy_score(x, y, fair=fair) - want) <= 1e-13 * max(1.0, abs(want))


def test_half_space_enumeration():
    for r in range(0, 5):
        for L in range(0, 4):
            d = mn.displacements(r, L)
            assert len(d) == ((2 * r + 1) ** 2 - 1) // 2 + L * (2 * r + 1) ** 2
            assert d == MV.displacements(r, L) and len(set(d)) == len(d)
            assert not any((-l, -di, -dj) in d for l, di, dj in d)                        # each unordered pair once
            w = MV.default_weights(r, L)
            assert np.array_equal(w, mn.default_weights(r, L)) and (w > 0).sum() == len(d)
    assert MV.default_weights(1, 1)[1, 0, 0] == 1 / np.sqrt(3.0) and MV.default_weights(1, 0)[0, 1, 1] == 0.0


def test_argument_errors():
    ens, obs = np.zeros((3, 24, 2, 5), np.float32), np.zeros((24, 2, 5), np.float32)
    bad_pairs = ((np.zeros((3, 23, 2, 5)), obs), (np.zeros((24, 2, 5)), obs), (ens, np.zeros((24, 2, 4))), (ens, np.zeros((24, 5))),
                 (np.zeros((0, 24, 2, 5)), obs), (np.zeros((2, 3, 24, 2, 5)), obs), (np.zeros((2, 3, 24, 2, 5)), np.zeros((3, 24, 2, 5))),
                 (torch.zeros(3, 24, 2, 5), obs), (ens, torch.zeros(24, 2, 5)), (np.zeros((3, 24, 2, 5), dtype=complex), obs),
                 (np.broadcast_to(np.float32(0), (8193, 24, 1, 1)), np.zeros((24, 1, 1))), (np.zeros((1, 3, 1, 24, 2, 5)), obs))
    for e, o in bad_pairs:
        for fn in (MV.energy_score, MV.energy_terms, MV.variogram_score):
            with pytest.raises(ValueError):
                fn(e, o)
    with pytest.raises(ValueError):
        MV.energy_score(ens, obs, fair=1)
    for kw in (dict(p=2), dict(p=0.25), dict(p="0.5"), dict(p=True), dict(radius=5), dict(radius=-1), dict(radius=1.0), dict(max_lag=4), dict(max_lag=-1),
               dict(max_lag=True), dict(weights=np.zeros((2, 5, 4))), dict(weights=np.full((2, 5, 5), np.nan)), dict(weights="unit")):
        with pytest.raises(ValueError):
            MV.variogram_score(ens, obs, **kw)
    if not torch.cuda.is_available():                                                      # valid arguments reach the device: no CPU fallback
        for fn in (MV.energy_score, MV.energy_terms, MV.variogram_score):
            with pytest.raises(_lib.RdganError):
                fn(ens, obs)
    reals = np.zeros((2, 24, 2, 5), np.float32)
    for args, kw in (((None, reals), {}), ((lambda d: ens, np.zeros((24, 2, 5))), {}), ((lambda d: ens, reals), dict(p=3)),
                     ((lambda d: ens, reals), dict(radius=9)), ((lambda d: ens, reals), dict(fair="yes")), ((lambda d: ens, torch.zeros(2, 24, 2, 5)), {})):
        with pytest.raises(ValueError):
            MV.scores_for_days(*args, **kw)
    sq, clim = np.zeros((2, 24, 8, 8), np.float32), np.zeros((5, 24, 8, 8), np.float32)
    for args, kw in (((None, reals, clim), {}), ((None, sq, np.zeros((5, 24, 8, 4))), {}), ((None, sq, clim), dict(slopes=(1.0,))),
                     ((None, sq, clim), dict(library="days")), ((None, sq, clim), dict(n_members=0)), ((None, sq, clim), dict(n_members=8193)),
                     ((None, sq, clim), dict(seed=-1)), ((None, sq, clim), dict(p=2)), ((None, sq, clim), dict(max_lag=4)),
                     ((None, sq, clim), dict(query_groups=np.zeros(2, np.int32))), ((None, sq[0], clim), {})):
        with pytest.raises(ValueError):
            MV.multivariate_experiment(*args, **kw)
    assert MV.check_order(1) == 1.0 and MV.check_order(np.float32(0.5)) == 0.5
    w = MV.check_weights(np.ones((2, 3, 3)), 1, 1)
    assert w[0, 1, 1] == 0 and w[0, 0, 2] == 0 and w[0, 1, 2] == 1 and w[1].min() == 1     # outside the half-space: ignored
    assert MV.energy_from_terms(7.0, 5.0, 2) == 3.5 - 1.25 and MV.energy_from_terms(7.0, 5.0, 2, fair=True) == 1.0
    assert MV.energy_from_terms(5.0, 0.0, 1, fair=True) == 5.0


def test_cabi_argument_checks():
    """the C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    ews, vws = lib.rdgan_mv_energy_workspace_bytes, lib.rdgan_mv_variogram_workspace_bytes
    assert ews(1, 1, 0) == 8 * (1 + 1 * 2) and ews(64, 3, 0) == 8 * (3 + 3 * 3 * 2) and ews(130, 3, 1) == 8 * (3 + 4 * 6 + 3 * 64)
    for a in ((0, 1, 0), (8193, 1, 0), (1, 0, 0), (1, 2 ** 20 + 1, 0), (1, 1, 2), (1, 1, -1), (8192, 2 ** 20, 0)):
        assert ews(*a) == -2, a
    units = 24 * 1 + 23 * 2                                                                # radius 2, lag 1, one tile: 12 and 25 displacements
    assert vws(3, 16, 16, 2, 1, 0) == 8 * (3 + 3 * units * 32) and vws(3, 16, 16, 2, 1, 1) == 8 * (3 + 3 * units * 32 + units * 16 * 256)
    assert vws(1, 17, 16, 4, 3, 0) == 8 * (1 + (24 * 3 + (23 + 22 + 21) * 6) * 2 * 32)
    for a in ((0, 4, 4, 1, 1, 0), (1, 0, 4, 1, 1, 0), (1, 4, 0, 1, 1, 0), (1, 4, 4, 5, 1, 0), (1, 4, 4, -1, 1, 0), (1, 4, 4, 1, 4, 0), (1, 4, 4, 1, -1, 0),
              (1, 4, 4, 1, 1, 2), (1, 4097, 4097, 1, 1, 0), (2 ** 20 + 1, 4, 4, 1, 1, 0)):
        assert vws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)

    def energy(ens=good, obs=good, m=5, D=2, ny=3, nx=5, shared=0, so=good, sp=good, ws=good, nbytes=1 << 20):
        return lib.rdgan_mv_energy(ens, obs, m, D, ny, nx, shared, so, sp, ws, nbytes, st)

    for kw in (dict(ens=null), dict(obs=null), dict(so=null), dict(sp=null), dict(ws=null), dict(ens=by(2)), dict(obs=by(1)), dict(so=by(4)), dict(sp=by(4)),
               dict(ws=by(4)), dict(m=0), dict(m=8193), dict(D=0), dict(D=2 ** 20 + 1), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4097), dict(shared=2),
               dict(shared=-1), dict(nbytes=8 * (2 + 2 * 2) - 1), dict(nbytes=0), dict(nbytes=-8), dict(shared=1, nbytes=8 * (2 + 3 + 64) - 1)):
        assert energy(**kw) == -2, kw

    def variogram(ens=good, obs=good, m=5, D=2, ny=3, nx=5, shared=0, p=0.5, r=1, L=1, sq=good, cnt=good, ws=good, nbytes=1 << 24):
        return lib.rdgan_mv_variogram(ens, obs, m, D, ny, nx, shared, p, r, L, sq, cnt, ws, nbytes, st)

    for kw in (dict(ens=null), dict(obs=null), dict(sq=null), dict(cnt=null), dict(ws=null), dict(ens=by(2)), dict(obs=by(2)), dict(sq=by(4)), dict(cnt=by(4)),
               dict(ws=by(4)), dict(m=0), dict(m=8193), dict(D=0), dict(ny=0), dict(nx=0), dict(shared=2), dict(p=2.0), dict(p=0.0), dict(p=0.25),
               dict(p=float("nan")), dict(r=5), dict(r=-1), dict(L=4), dict(L=-1), dict(nbytes=8 * (2 + 2 * (24 + 23) * 32) - 1), dict(nbytes=0)):
        assert variogram(**kw) == -2, kw


def test_header_and_lib_agree_on_the_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "double": "c_double", "void*": "c_void_p", "const float*": "c_void_p", "double*": "c_void_p",
             "long long*": "c_void_p"}
    assert tuple(sorted(n for n in _lib.SIGNATURES if n.startswith("rdgan_mv_"))) == NAMES
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_mv_\w+)\(", header, re.M)))) == NAMES
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
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_mvscore.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (MV.MAX_MEMBERS, MV.MAX_PLANE, MV.MAX_DAYS, MV.MAX_RADIUS, MV.MAX_LAG, MV.NHOURS) == tuple(
        value(n) for n in ("RD_MV_MAXM", "RD_HOURLY_MAXPLANE", "RD_MV_MAXDAYS", "RD_MV_MAXR", "RD_MV_MAXLAG", "RD_HOURS"))
    # the panels of the widest energy kernel (three, two buffers) fit the 64 KB a workgroup gets without asking; rows stay 16-byte aligned
    assert 2 * 3 * value("RD_MV_TILE") * value("RD_MV_LDK") * 4 <= 64 * 1024 and value("RD_MV_LDK") % 4 == 0 and value("RD_MV_LDK") >= value("RD_MV_CHUNK")
    assert value("RD_MV_TILE") * value("RD_MV_CHUNK") == value("RD_MV_STAGE") * value("RD_MV_THREADS")
    assert (value("RD_MV_VT") + 2 * value("RD_MV_MAXR")) ** 2 <= 3 * value("RD_MV_THREADS") and value("RD_MV_VT") ** 2 == value("RD_MV_THREADS")
    import pr_disagg_radar_gan_amd
    assert pr_disagg_radar_gan_amd.multivariate is MV
