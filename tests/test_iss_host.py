"""CPU: the yardstick of the intensity-scale verification (tests/iss_np.py) and IntensityScale of
pr_disagg_radar_gan_amd/intensity_scale.py on closed forms; the components' sum and the Q identity against the explicit wavelet
fields in exact fractions; the host arithmetic within 4 ulp of the fractions; NaN rules; argument errors raised before any device
call; the two C entries' argument checks and the workspace size against the kernel header's formula."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, intensity_scale as IS
from tests import iss_np as yn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52


def result_of(members, obs, thr, L):
    counts, tiles = yn.state_np(members, obs, thr, L)
    return IS.IntensityScale(tuple(float(np.float32(t)) for t in thr), L, obs.shape[-2], obs.shape[-1], counts, tiles)


def day(plane):
    """(24, ny, nx): the plane in every hour"""
    return np.broadcast_to(np.asarray(plane, np.float32), (24,) + np.shape(plane)).copy()


def close(got, want, ulps=4):
    """a float against a Fraction (None: NaN)"""
    if want is None:
        return math.isnan(got)
    return abs(Fraction(got) - want) <= ulps * ULP * abs(want)


def test_closed_forms():
    rng = np.random.default_rng(0)
    L = 3
    o = (rng.random((16, 16)) < 0.3).astype(np.float32)
    # a perfect forecast: every MSE 0, every ISS 1
    r = result_of(day(o)[None], day(o), (0.5,), L)
    assert np.all(r.mse() == 0) and np.all(r.skill() == 1) and np.all(r.skill(bias_corrected=True) == 1) and np.all(r.skill(by_hour=True) == 1)
    assert r.tiles.tolist() == [[4, 0]] * 24 and r.scales_px == (1, 2, 4, 8)
    # one wrong pixel in a tile: QZ_l = 1 at every level
    x = o.copy()
    x[3, 5] = 1 - x[3, 5]
    counts, tiles = yn.state_np(day(x)[None], day(o), (0.5,), L)
    qz = counts[0, 0, :, 0] - 2 * counts[0, 0, :, 2] + counts[0, 0, :, 1]
    assert qz.tolist() == [1] * (L + 1)
    # a checkerboard against an empty observation: MSE_0 = 1/4, no other mother component, father 1/4, total 1/2
    yy, xx = np.indices((16, 16))
    board = ((yy + xx) % 2).astype(np.float32)
    r = result_of(day(board)[None], day(np.zeros((16, 16))), (0.5,), L)
    assert r.mse()[0].tolist() == [0.25, 0.0, 0.0, 0.25] and r.mse().sum() == 0.5
    assert np.all(np.isnan(r.skill()))                                # e = 0
    z = yn.tiles_of(board, L).reshape(-1, 8, 8).astype(np.int64)
    assert yn.components_np(z) == [Fraction(1, 4), 0, 0, Fraction(1, 4)]
    assert r.contingency()[0].tolist() == [0, 24 * 128, 0, 24 * 128]
    enx, eno, rel = r.energy()
    assert enx[0].tolist() == [0.25, 0.0, 0.0, 0.25] and np.all(eno == 0) and rel[0, 0] == 1.0 and math.isnan(rel[0, 1])


@pytest.mark.parametrize("L,shape", [(2, (9, 14)), (3, (17, 8)), (4, (16, 35))])
def test_components_sum_and_identity_in_fractions(L, shape):
    rng = np.random.default_rng(L)
    obs = (rng.gamma(0.6, 2.0, (24,) + shape) * (rng.random((24,) + shape) < 0.4)).astype(np.float32)
    ens = (rng.gamma(0.6, 2.0, (3, 24) + shape) * (rng.random((3, 24) + shape) < 0.4)).astype(np.float32)
    ens[1, 2, 1, 1], obs[5, 4, 4] = np.nan, np.inf
    thr = (0.1, 1.0)
    counts, tiles = yn.state_np(ens, obs, thr, L)
    void = ~np.isfinite(yn.tiles_of(ens, L)).all(axis=(-2, -1)) | ~np.isfinite(yn.tiles_of(obs, L)).all(axis=(-2, -1))[None]
    assert void.any() and int(void.sum()) == int(tiles[:, 1].sum())
    r = IS.IntensityScale(thr, L, shape[0], shape[1], counts, tiles)
    for t, u in enumerate(thr):
        z = (yn.events(yn.tiles_of(ens, L), u).astype(np.int64) - yn.events(yn.tiles_of(obs, L), u).astype(np.int64)[None])[~void]
        q, n_valid = counts[t].sum(axis=0), int(tiles[:, 0].sum())
        assert n_valid == z.shape[0]
        want = yn.components_np(z)                                   # the explicit wavelet fields
        got = yn.mse_from_state(q, n_valid, L)                       # the Q identity
        assert got == want
        qz0 = int(q[0][0] - 2 * q[0][2] + q[0][1])
        assert sum(got) == Fraction(qz0, n_valid * 4 ** L) == Fraction(int(np.abs(z).sum()), z.size)
        assert all(close(g, w) for g, w in zip(r.mse()[t], want))
        for k in (0, 1):                                             # the energies: the same decomposition of either event field
            e = (yn.events(yn.tiles_of(ens, L), u) if k == 0 else np.broadcast_to(yn.events(yn.tiles_of(obs, L), u)[None], void.shape + z.shape[1:]))[~void]
            assert yn.energy_from_state(q, n_valid, L, k) == yn.components_np(e.astype(np.int64))


def test_host_arithmetic_within_4_ulp_of_the_fractions():
    rng = np.random.default_rng(7)
    L, T = 5, 3
    side = 1 << L
    # hand-built states of single tiles with very different sizes of count, up to 2^61 in a counter
    counts = np.zeros((T, 24, L + 1, 3), np.int64)
    tiles = np.zeros((24, 2), np.int64)
    for h in range(24):
        reps = int(rng.integers(1 << (40 * h // 23), 1 << (40 * h // 23 + 1)))       # the same tile-pair counted `reps` < 2^41 times
        tiles[h] = (reps, h)
        for t in range(T):
            x, o = rng.random((side, side)) < 0.2 * (t + 1), rng.random((side, side)) < 0.25
            for l in range(L + 1):
                sx, so = yn.block_sums(x, l), yn.block_sums(o, l)
                counts[t, h, l] = [reps * int((sx * sx).sum()), reps * int((so * so).sum()), reps * int((sx * so).sum())]
    assert counts.max() > 1 << 55
    r = IS.IntensityScale((0.1, 0.5, 1.0), L, 40, 40, counts, tiles)
    for t in range(T):
        for h in list(range(24)) + [None]:
            q = counts[t].astype(object).sum(axis=0) if h is None else counts[t, h]
            nv = int(tiles[:, 0].astype(object).sum()) if h is None else int(tiles[h, 0])
            pick = (lambda a: a[t]) if h is None else (lambda a: a[t, h])
            by = h is not None
            assert all(close(g, w) for g, w in zip(pick(r.mse(by)), yn.mse_from_state(q, nv, L)))
            for bc in (False, True):
                assert all(close(g, w) for g, w in zip(pick(r.skill(by, bias_corrected=bc)), yn.skill_from_state(q, nv, L, bc))), (t, h, bc)
            enx, eno, rel = r.energy(by)
            fx, fo = yn.energy_from_state(q, nv, L, 0), yn.energy_from_state(q, nv, L, 1)
            assert all(close(g, w) for g, w in zip(pick(enx), fx)) and all(close(g, w) for g, w in zip(pick(eno), fo))
            assert all(close(g, (a - b) / (a + b) if a + b else None) for g, a, b in zip(pick(rel), fx, fo))
    c = r.contingency()
    assert c.dtype == np.int64 and np.all(c.sum(axis=1) == int(tiles[:, 0].sum()) * 4 ** L)
    s = r.summary()
    assert s["skill"].shape == (T, L + 1) and s["skill_by_hour"].shape == (T, 24, L + 1) and s["void_tiles"] == sum(range(24))
    d = IS.compare(r, r)
    assert np.all(d["skill"] == 0) and np.all(d["energy_model"] == 0)
    with pytest.raises(ValueError):
        IS.compare(r, IS.IntensityScale((0.1,), L, 40, 40, counts[:1], tiles))
    with pytest.raises(ValueError):
        IS.compare(r, None)


def test_nan_rules_and_bias_corrected():
    L = 2
    z, one = np.zeros((8, 8), np.float32), np.ones((8, 8), np.float32)
    rng = np.random.default_rng(2)
    x = (rng.random((8, 8)) < 0.5).astype(np.float32)
    # e = 0 and e = 1: no skill; the MSE stays defined
    for o in (z, one):
        r = result_of(day(x)[None], day(o), (0.5,), L)
        assert np.all(np.isnan(r.skill())) and np.all(np.isfinite(r.mse()))
    assert np.all(np.isnan(result_of(day(x)[None], day(z), (0.5,), L).skill(bias_corrected=True)))       # B = x / 0
    # no valid tile: everything NaN, the contingency 0
    bad = np.full((8, 8), np.nan, np.float32)
    r = result_of(day(x)[None], day(bad), (0.5,), L)
    assert r.tiles[:, 0].sum() == 0 and r.tiles[:, 1].sum() == 24 * 4
    assert np.all(np.isnan(r.mse())) and np.all(np.isnan(r.skill())) and all(np.all(np.isnan(e)) for e in r.energy()) and np.all(r.contingency() == 0)
    # 0 / 0 energy: both sides empty
    r = result_of(day(z)[None], day(z), (0.5,), L)
    enx, eno, rel = r.energy()
    assert np.all(enx == 0) and np.all(eno == 0) and np.all(np.isnan(rel))
    # B = 1: the bias-corrected reference is the plain one
    o = np.roll(x, 3, axis=1)                                        # as many events, elsewhere
    r = result_of(day(x)[None], day(o), (0.5,), L)
    assert r.counts[0, 0, 0, 0] == r.counts[0, 0, 0, 1] and np.array_equal(r.skill(), r.skill(bias_corrected=True))
    assert np.all(np.isfinite(r.skill()))
    # B != 1: Casati (2010) in fractions
    o2 = o.copy()
    o2[:2] = 0
    r = result_of(day(x)[None], day(o2), (0.5,), L)
    q, nv = r.counts[0].sum(axis=0), int(r.tiles[:, 0].sum())
    assert all(close(g, w) for g, w in zip(r.skill(bias_corrected=True)[0], yn.skill_from_state(q, nv, L, True)))
    assert not np.array_equal(r.skill(), r.skill(bias_corrected=True))


def test_argument_errors_before_any_device_call():
    good = np.zeros((24, 16, 20), np.float32)
    for levels in (0, 11, 5, True, 2.0):                             # 2^5 > 16
        with pytest.raises(ValueError):
            IS.IntensityScaleVerifier(good, (0.1,), levels)
        with pytest.raises(ValueError):
            IS.intensity_scale_hourly(good[None], good, (0.1,), levels)
    assert IS.check_levels(None, 16, 20) == 4 and IS.check_levels(None, 5000, 3000) == 10 and IS.check_levels(3, 8, 8) == 3
    with pytest.raises(ValueError):
        IS.check_levels(None, 1, 7)
    for thr in ((), tuple(range(9)), (1.0, 0.5), (-1.0,), (np.nan,), "x"):
        with pytest.raises(ValueError):
            IS.IntensityScaleVerifier(good, thr)
        with pytest.raises(ValueError):
            IS.intensity_scale_hourly(good[None], good, thr)
    for bad in (torch.zeros(24, 16, 20), np.zeros((23, 16, 20)), np.zeros((24, 20)), np.zeros((24, 16, 20), dtype=complex),
                np.broadcast_to(np.float32(0), (24, 1 << 12, 1 << 13))):
        with pytest.raises(ValueError):
            IS.IntensityScaleVerifier(bad, (0.1,))
    for kw in (dict(pairs_per_pass=0), dict(pairs_per_pass=(1 << 30) + 1), dict(pairs_per_pass=1.5)):
        with pytest.raises(ValueError):
            IS.IntensityScaleVerifier(good, (0.1,), **kw)
    for ens in (good, np.zeros((2, 24, 16, 21), np.float32), torch.zeros(1, 24, 16, 20), np.broadcast_to(np.float32(0), (4097, 24, 16, 20))):
        with pytest.raises(ValueError):
            IS.intensity_scale_hourly(ens, good, (0.1,))
    # add's own checks, on a verifier built without a device
    v = object.__new__(IS.IntensityScaleVerifier)
    v.shape, v.levels, v.n_members, v._pairs_of_a_member = (24, 16, 20), 4, 0, 24 * 16 * 16
    for members in (torch.zeros(2, 24, 16, 20), np.zeros((2, 24, 16, 21), np.float32), np.broadcast_to(np.float32(0), (4097, 24, 16, 20)), good):
        with pytest.raises(ValueError):
            v.add(members)
    # the 2^62 refusal: 24 * 1024^2 pixel-pairs a member at L = 10 are 24 * 2^40 a member: 2^62 is passed by the 174763rd
    v.shape, v.levels, v._pairs_of_a_member = (24, 1024, 1024), 10, 24 << 20
    small = np.broadcast_to(np.float32(0), (1, 24, 1024, 1024))
    v.n_members = (1 << 62) // (24 << 40)
    assert v.n_members == 174762
    with pytest.raises(ValueError, match="2\\^62"):
        v.add(small)
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            IS.IntensityScaleVerifier(good, (0.1,))
        with pytest.raises(_lib.RdganError):
            IS.intensity_scale_hourly(good[None], good, (0.1,))

    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    ok = dict(gen=NoGenerator(), observed=np.zeros((24, 20, 30), np.float32), n_scenarios=3, thresholds=(0.1,))
    for kw in (dict(thresholds=()), dict(levels=0), dict(levels=5), dict(n_scenarios=0), dict(n_scenarios=4097), dict(scenario_chunk=0),
               dict(overlap=9), dict(latent_mode="each"), dict(observed=np.zeros((2, 2, 24, 20, 30), np.float32)), dict(observed=torch.zeros(24, 20, 30)),
               dict(observed=np.zeros((20, 30), np.float32)), dict(daily=np.zeros((20, 31), np.float32)), dict(chunk=0), dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            IS.intensity_scale_field(**{**ok, **kw})
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RdganError):
            IS.intensity_scale_field(**ok)


def test_cabi_argument_checks_and_workspace_bytes():
    """the two C entries refuse a bad argument before they touch the device: callable without one.  The size restates the header:
    8 bytes a pair up to L = 6, ceil(cy / 64) ceil(cx / 64) (8 x 4 x 20 x 4 + 8) above"""
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_iss.hip.h")).read()
    assert "(long)g.nby * g.nbx * (RD_ISS_MAXT * 4 * RD_ISS_REC * 4 + 8)" in text and "#define RD_ISS_REC 20" in text
    lib = _lib.load()
    ws = lib.rdgan_iss_workspace_bytes

    def want(ny, nx, L, pairs):
        if L <= 6:
            return 8 * pairs
        _, _, cy, cx = yn.crop(ny, nx, L)
        return pairs * -(-cy // 64) * -(-cx // 64) * (8 * 4 * 20 * 4 + 8)

    for a in ((64, 64, 6, 1), (8, 8, 3, 7), (131, 140, 7, 3), (300, 270, 8, 2), (4096, 4096, 10, 5), (2048, 1500, 10, 1 << 30)):
        assert ws(*a) == want(*a), a
    for a in ((0, 64, 1, 1), (64, 0, 1, 1), (64, 64, 0, 1), (64, 64, 11, 1), (64, 64, 7, 1), (127, 300, 7, 1), (300, 127, 7, 1), (64, 64, 6, 0),
              (64, 64, 6, (1 << 30) + 1), (4097, 4096, 6, 1), (-1, -1, 1, 1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                 # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])
    P = 24 * 16 * 20

    def acc(m=good_p, s=2, stride=P, obs=good_p, n_days=1, ny=16, nx=20, th=hp(thr), T=2, L=4, counts=good_p, tiles=good_p, ws=good_p, nbytes=8):
        return lib.rdgan_iss_accumulate(m, s, stride, obs, n_days, ny, nx, th, T, L, counts, tiles, ws, nbytes, ctypes.c_void_p(0))

    unsorted, negative, nan = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0])), hp(np.array([np.nan, 1.0]))
    for kw in (dict(m=null), dict(obs=null), dict(counts=null), dict(tiles=null), dict(ws=null), dict(th=null), dict(m=odd_p), dict(obs=odd_p),
               dict(counts=four_p), dict(tiles=four_p), dict(ws=four_p), dict(s=0), dict(s=4097), dict(n_days=0), dict(ny=0), dict(nx=0),
               dict(ny=4097, nx=4096, stride=24 * 4097 * 4096), dict(n_days=1 << 40, stride=1 << 50), dict(s=4096, n_days=1 << 17, stride=P << 17),
               dict(stride=P - 1), dict(T=0), dict(T=9), dict(th=unsorted), dict(th=negative), dict(th=nan), dict(L=0), dict(L=11), dict(L=5),
               dict(ny=128, nx=127, stride=24 * 128 * 127, L=7), dict(nbytes=7), dict(nbytes=0), dict(nbytes=-5),
               dict(ny=128, nx=128, stride=24 * 128 * 128, L=7, nbytes=want(128, 128, 7, 1) - 1)):
        assert acc(**kw) == -2, kw


def test_header_and_lib_agree_on_the_iss_entries():
    import re
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "long long*": "c_void_p"}
    for name in ("rdgan_iss_workspace_bytes", "rdgan_iss_accumulate"):
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
