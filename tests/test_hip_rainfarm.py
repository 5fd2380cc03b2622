"""-m gpu: the RainFARM kernels (rdgan_rainfarm.hip.h) against the reference's own values (tests/golden/rainfarm_reference.npz)
and the fp64 restatement (tests/rainfarm_np.py): slope statistics and fits, generation from given uniforms and from the counter RNG,
and the evaluation entry points."""
import os

import numpy as np
import pytest
import torch

from oracle import rng as orng
from tests import rainfarm_np as rn

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rainfarm_reference.npz")
STREAM_RAINFARM = 6                 # RD_STREAM_RAINFARM of csrc/rdgan_rng.h
# fp64 DFT and log on the device against numpy's fp64 FFT, relative error of the fitted slopes; about 3x the largest observed on
# the MI355X: 2.7e-15 / 2.0e-15 (alpha / beta, nd 8 fixture), 1.1e-16 / 3.3e-16 (nd 16 fixture), at most 4.4e-16 / 4.4e-15 (nd 24-64)
SLOPE_RTOL = 1.5e-14
# fp32 generation against the reference's fp64 day (stored as fp32), relative error on the wet pixels; about 3x the largest observed:
# 0.7-1.6e-6 on the fixture's days (fp64, fp32 and drop-in uniforms), 0.8e-6 (nd 8) rising to 2.3e-6 (nd 64) against the restatement
GEN_RTOL = 7e-6


def _ref():
    return np.load(FIXTURE)


def _rf():
    from pr_disagg_radar_gan_amd import rainfarm
    return rainfarm


def smooth_days(rng, nd, n, alpha=2.4, beta=1.5):
    """a calibration-like batch: days from the restatement's generator on smooth daily sums, with dry pixels and dry hours"""
    yy, xx = np.mgrid[0:nd, 0:nd] / nd
    sums = []
    for _ in range(n):
        c = rng.random(2)
        f = 30.0 * np.exp(-((yy - c[0]) ** 2 + (xx - c[1]) ** 2) / (0.2 + 0.3 * rng.random()) ** 2)
        f[f < 3.0] = 0.0
        sums.append(f)
    days = rn.generate(np.array(sums), rn.amplitudes(alpha, beta, nd), rng.random((n, 24, nd, nd)))
    days[0, 3] = 0.0
    days[-1, 10:12] = 0.0
    return days.astype(np.float32)


def _check_stats(st, x):
    sc, ss, tc, ts = rn.class_statistics(x)
    assert np.array_equal(st.spatial_counts, sc) and np.array_equal(st.temporal_counts, tc)      # dropped points exactly
    pres = sc > 0
    np.testing.assert_allclose(st.spatial_sums[pres], ss[pres], rtol=1e-10)
    np.testing.assert_allclose(st.temporal_sums[tc > 0], ts[tc > 0], rtol=1e-10)
    assert np.all(st.spatial_sums[~pres] == 0) and st.temporal_counts[0] == 0 and st.spatial_counts[0, 0] == 0


@pytest.mark.parametrize("nd", [8, 16])
def test_slopes_match_reference_fixture(nd):
    ref = _ref()
    x = ref[f"calib_nd{nd}"]
    st = _rf().slope_statistics(x)
    _check_stats(st, x)
    ea = abs(st.alpha / float(ref[f"calib_alpha_nd{nd}"]) - 1)
    eb = abs(st.beta / float(ref[f"calib_beta_nd{nd}"]) - 1)
    print(f"nd {nd}: alpha {st.alpha:.12f} rel err {ea:.2e}, beta {st.beta:.12f} rel err {eb:.2e} (limit {SLOPE_RTOL})")
    assert ea < SLOPE_RTOL and eb < SLOPE_RTOL
    a2, b2 = _rf().estimate_slopes(torch.from_numpy(x).cuda())
    assert a2 == st.alpha and b2 == st.beta                          # bit-identical on a repeat, from a device tensor
    assert _rf().estimate_alpha(x) == st.alpha and _rf().estimate_beta(x) == st.beta


@pytest.mark.parametrize("nd", [24, 32, 48, 64])
def test_slopes_match_restatement(nd):
    x = smooth_days(np.random.default_rng(nd), nd, 5)
    st = _rf().slope_statistics(x)
    _check_stats(st, x)
    a, b = rn.slopes(x)
    ea, eb = abs(st.alpha / a - 1), abs(st.beta / b - 1)
    print(f"nd {nd}: alpha rel err {ea:.2e}, beta rel err {eb:.2e}")
    assert ea < SLOPE_RTOL and eb < SLOPE_RTOL


def _gen_cases(ref):
    for i in range(int(ref["n_gen"])):
        nd, alpha, beta, seed = ref[f"gen{i}_params"]
        yield i, int(nd), float(alpha), float(beta), int(seed)


def _rel_err(got, want):
    wet = want != 0
    assert np.array_equal(got == 0, ~wet)
    return float(np.abs(got[wet] / want[wet] - 1).max())


def test_downscale_matches_reference_days():
    rf = _rf()
    ref = _ref()
    for i, nd, alpha, beta, seed in _gen_cases(ref):
        precip, want = ref[f"gen{i}_precip"], ref[f"gen{i}_day"]
        u = np.random.RandomState(seed).rand(1, 24, nd, nd)
        e64 = _rel_err(rf.downscale_device(precip, alpha, beta, uniforms=u).cpu().numpy()[0], want)
        e32 = _rel_err(rf.downscale_device(precip, alpha, beta, uniforms=u.astype(np.float32)).cpu().numpy()[0], want)
        np.random.seed(seed)
        drop = rf.downscale_spatiotemporal(precip, alpha, beta, 24)          # R's signature and R's own draws
        assert drop.shape == (24, nd, nd) and drop.dtype == np.float32
        e_drop = _rel_err(drop, want)
        print(f"case {i} (nd {nd}, beta {beta}): rel err fp64 uniforms {e64:.2e}, fp32 uniforms {e32:.2e}, drop-in {e_drop:.2e}")
        assert max(e64, e32, e_drop) < GEN_RTOL


def _check_output(out, precip):
    """finite, >= 0, exact 0 under a dry daily sum, hourly values summing to the daily sum"""
    out = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
    precip = np.broadcast_to(precip, (out.shape[0],) + tuple(precip.shape[-2:]))
    assert np.all(np.isfinite(out)) and np.all(out >= 0)
    assert np.all(out[np.broadcast_to(precip[:, None] == 0, out.shape)] == 0)
    np.testing.assert_allclose(out.astype(np.float64).sum(1), precip, rtol=1e-5, atol=0)


@pytest.mark.parametrize("nd", [8, 16, 24, 32, 48, 64])
def test_generation_matches_restatement(nd):
    rf = _rf()
    rng = np.random.default_rng(100 + nd)
    n = 3
    precip = rng.gamma(0.6, 12.0, (n, nd, nd))
    precip[rng.random(precip.shape) < 0.3] = 0.0
    precip = precip.astype(np.float32)
    u = rng.random((n, 24, nd, nd))
    alpha, beta = 1.9, 1.3
    out = rf.downscale_device(precip, alpha, beta, uniforms=u).cpu().numpy()
    _check_output(out, precip)
    want = rn.generate(precip, rn.amplitudes(alpha, beta, nd), u)
    err = _rel_err(out, want)
    print(f"nd {nd}: generation rel err vs fp64 {err:.2e}")
    assert err < GEN_RTOL


def mirror_uniforms(seed, members, nd):
    """numpy mirror of the counter-RNG phases (csrc/rdgan_rng.h rd_member_key), on oracle/rng.py's mix32 and make_key"""
    base = np.uint32(orng.make_key(seed, STREAM_RAINFARM))
    idx = np.arange(24 * nd * nd, dtype=np.uint32)
    hidx = orng.mix32(idx)
    out = []
    for m in members:
        lo, hi = np.uint32(m & 0xFFFFFFFF), np.uint32(m >> 32)
        key = orng.mix32(base ^ orng.mix32(lo ^ orng.mix32(hi ^ np.uint32(0x9E3779B9))))
        bits = orng.mix32(hidx ^ key)
        out.append((bits >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))
    return np.array(out).reshape(len(members), 24, nd, nd)


def test_counter_rng_matches_mirror_and_chunking():
    rf = _rf()
    nd, seed = 16, 987654321
    rng = np.random.default_rng(5)
    precip = (rng.gamma(0.6, 12.0, (nd, nd)) * (rng.random((nd, nd)) > 0.2)).astype(np.float32)
    far = 2 ** 32 // (24 * nd * nd) + 7                   # a flat element counter of this member would pass 2^32
    for first in (0, far, 2 ** 32 + 3):
        a = rf.downscale_device(precip, 1.7, 1.2, n_members=6, seed=seed, first_member=first)
        u = mirror_uniforms(seed, range(first, first + 6), nd)
        b = rf.downscale_device(precip, 1.7, 1.2, uniforms=u)
        assert torch.equal(a, b), first
        _check_output(a, precip)
        again = rf.downscale_device(precip, 1.7, 1.2, n_members=6, seed=seed, first_member=first)
        assert torch.equal(a, again)
        parts = torch.cat([rf.downscale_device(precip, 1.7, 1.2, n_members=2, seed=seed, first_member=first),
                           rf.downscale_device(precip, 1.7, 1.2, n_members=4, seed=seed, first_member=first + 2)])
        assert torch.equal(a, parts)
    other = rf.downscale_device(precip, 1.7, 1.2, n_members=6, seed=seed + 1)
    assert not torch.equal(other, rf.downscale_device(precip, 1.7, 1.2, n_members=6, seed=seed))


def test_broadcast_precip_equals_repeated():
    rf = _rf()
    nd = 24
    rng = np.random.default_rng(9)
    precip = (rng.gamma(0.6, 12.0, (nd, nd)) * (rng.random((nd, nd)) > 0.2)).astype(np.float32)
    a = rf.downscale_device(precip, 2.0, 0.9, n_members=5, seed=3)
    b = rf.downscale_device(np.repeat(precip[None], 5, 0), 2.0, 0.9, seed=3)
    assert torch.equal(a, b)


def test_crps_for_day_matches_numpy():
    rf = _rf()
    nd, n = 16, 48
    ref = _ref()
    real = ref["calib_nd16"][4]                                      # one day, mm/h
    got = rf.crps_for_day(real, 2.2, 1.3, n_members=n, seed=11)
    ens = rf.downscale_device(real.sum(0), 2.2, 1.3, n_members=n, seed=11).cpu().numpy()
    want = rn.crps_ensemble(real, ens).mean(axis=(1, 2))
    assert got.shape == (24,)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
    np.random.seed(4)
    g1 = rf.crps_for_day(real, 2.2, 1.3, n_members=8)                   # the global numpy RNG, R's order
    np.random.seed(4)
    u = np.random.rand(8, 24, nd, nd)
    e2 = rf.downscale_device(real.sum(0), 2.2, 1.3, uniforms=u).cpu().numpy()
    np.testing.assert_allclose(g1, rn.crps_ensemble(real, e2).mean(axis=(1, 2)), rtol=1e-5, atol=1e-7)


def test_generate_one_per_day_feeds_lsd_evaluation():
    rf = _rf()
    from pr_disagg_radar_gan_amd import spectral
    real = smooth_days(np.random.default_rng(21), 16, 6)
    gen = rf.generate_one_per_day(real, 2.3, 1.4, seed=8)
    assert isinstance(gen, torch.Tensor) and gen.is_cuda and tuple(gen.shape) == real.shape
    _check_output(gen, real.sum(1))
    res = spectral.lsd_evaluation(real, gen)
    n = 24 * len(real)
    assert res["gen_real"].total == n * (n - 1) and res["gen"].count > 0 and np.isfinite(res["gen_real"].mean)
    np.random.seed(2)
    g_np = rf.generate_one_per_day(torch.from_numpy(real).cuda(), 2.3, 1.4)
    np.random.seed(2)
    u = np.random.rand(len(real), 24, 16, 16)
    assert torch.equal(g_np, rf.downscale_device(torch.from_numpy(real).cuda().sum(1), 2.3, 1.4, uniforms=u))


def test_calibrate_on_device_dataset():
    rf = _rf()
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    nd = 16
    rng = np.random.default_rng(31)
    days = smooth_days(rng, 40, 3, alpha=2.0, beta=1.2)               # (3, 24, 40, 40) radar-like days
    idx = np.array([(d, y, x) for d in range(3) for y in (0, 8, 20, 24) for x in (0, 12, 24)], dtype=np.int32)
    ds = DeviceDataset(days, idx, ndomain=nd)
    np.random.seed(77)
    got = rf.calibrate(ds, n_calib=30, n_repeat=2)
    np.random.seed(77)
    for a, b in got:
        ixs = np.random.randint(len(idx), size=30)
        sel = idx[ixs]
        batch = np.array([days[d, :, y:y + nd, x:x + nd] for d, y, x in sel])
        wa, wb = rn.slopes(batch)
        assert abs(a / wa - 1) < SLOPE_RTOL and abs(b / wb - 1) < SLOPE_RTOL
    assert len(got) == 2 and got[0] != got[1]
