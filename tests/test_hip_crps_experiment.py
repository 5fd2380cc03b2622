"""-m gpu: the CRPS experiment's kernels (rdgan_crps.hip.h) against the fp64 mirrors (tests/crps_np.py), the existing ensemble CRPS
kernel, scipy's t-test and the reference's own bootstrap numbers (tests/golden/crps_stats_reference.npz), and the experiment's entry
points against the per-day functions they batch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import crps_np as cn

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crps_stats_reference.npz")
RTOL, ATOL = 2e-5, 2e-6             # the tolerance of test_crps_kernel_matches_definition (tests/test_hip_ensemble.py) for this quantity
P_RTOL = 2.2e-11                    # tests/test_crps_experiment_host.py: 10 x the worst observed error of the host's p-value
EPS = 2.0 ** -52


def _ce():
    from pr_disagg_radar_gan_amd import crps_experiment
    return crps_experiment


def _fields(rng, shape, dry):
    x = (rng.standard_exponential(shape, dtype=np.float32) * np.float32(1.5)) ** 2
    x[rng.random(shape, dtype=np.float32) < dry] = 0.0
    return x


@pytest.mark.parametrize("nd", [8, 16])
@pytest.mark.parametrize("n", [1, 2, 7, 300, 5000, 8192])
def test_kernel_matches_mirror(n, nd):
    ce = _ce()
    rng = np.random.default_rng(1000 * nd + n)
    dry = 0.3 + 0.3 * ((n % 7) / 6.0)                                # 30-60 % zeros
    ens = _fields(rng, (n, 24, nd, nd), dry)
    obs = _fields(rng, (257, 24, nd, nd), 0.4)
    obs[1] = ens.max(0)                                              # equal to the maximum
    obs[2] = ens.max(0) + 2.0                                        # above every member
    obs[5] = ens[n // 2]                                             # equal to a member
    want = cn.crps_fixed(ens, obs)
    want_h = cn.hourly_mean(want)
    e, o = torch.from_numpy(ens).cuda(), torch.from_numpy(obs).cuda()
    for D in (1, 3, 257):
        hourly, crps = ce.crps_fixed_ensemble_device(e, o[:D], per_position=True)
        assert tuple(hourly.shape) == (D, 24) and tuple(crps.shape) == (D, 24, nd, nd)
        got, got_h = crps.cpu().numpy(), hourly.cpu().numpy()
        err = np.abs(got - want[:D]) / (ATOL + RTOL * np.abs(want[:D]))
        err_h = np.abs(got_h - want_h[:D]) / (ATOL + RTOL * np.abs(want_h[:D]))
        print(f"n {n} nd {nd} D {D}: worst error / tolerance {err.max():.3f} (per position), {err_h.max():.3f} (hourly)")
        np.testing.assert_allclose(got, want[:D], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got_h, want_h[:D], rtol=RTOL, atol=ATOL)
        alone = ce.crps_fixed_ensemble_device(e, o[:D])                  # the hourly output alone
        assert torch.equal(alone, hourly)
        again_h, again = ce.crps_fixed_ensemble_device(e, o[:D], per_position=True)
        assert torch.equal(again, crps) and torch.equal(again_h, hourly)


def test_large_domain_and_outputs_alone():
    ce = _ce()
    from pr_disagg_radar_gan_amd import _lib
    rng = np.random.default_rng(64)
    n, D, nd = 7, 3, 64
    ens = _fields(rng, (n, 24, nd, nd), 0.5)
    obs = _fields(rng, (D, 24, nd, nd), 0.4)
    want = cn.crps_fixed(ens, obs)
    e, o = torch.from_numpy(ens).cuda(), torch.from_numpy(obs).cuda()
    hourly, crps = ce.crps_fixed_ensemble_device(e, o, per_position=True)
    np.testing.assert_allclose(crps.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(hourly.cpu().numpy(), cn.hourly_mean(want), rtol=RTOL, atol=ATOL)
    assert torch.equal(ce.crps_fixed_ensemble_device(ens, obs), hourly)              # numpy inputs, hourly alone
    # the per-position output alone, through the C ABI
    lib = _lib.load()
    only = torch.full_like(crps, -1.0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.rdgan_crps_fixed_ensemble(ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(only.data_ptr()),
                                       None, n, D, nd, st)
    assert rc == 0 and torch.equal(only, crps)


def test_nan_observation():
    ce = _ce()
    rng = np.random.default_rng(5)
    ens = _fields(rng, (300, 24, 16, 16), 0.4)
    obs = _fields(rng, (3, 24, 16, 16), 0.4)
    clean_h, clean = ce.crps_fixed_ensemble_device(ens, obs, per_position=True)
    obs[1, 7, 3, 11] = np.nan
    hourly, crps = ce.crps_fixed_ensemble_device(ens, obs, per_position=True)
    crps, hourly = crps.cpu().numpy(), hourly.cpu().numpy()
    assert np.isnan(crps[1, 7, 3, 11]) and np.isnan(crps).sum() == 1
    assert np.isnan(hourly[1, 7]) and np.isnan(hourly).sum() == 1
    keep = ~np.isnan(crps)
    assert np.array_equal(crps[keep], clean.cpu().numpy()[keep])
    assert np.array_equal(hourly[~np.isnan(hourly)], clean_h.cpu().numpy()[~np.isnan(hourly)])


def test_agrees_with_the_per_day_kernel():
    ce = _ce()
    from pr_disagg_radar_gan_amd.ensemble import crps_ensemble_device
    rng = np.random.default_rng(6)
    ens = torch.from_numpy(_fields(rng, (1000, 24, 16, 16), 0.45)).cuda()
    obs = torch.from_numpy(_fields(rng, (5, 24, 16, 16), 0.4)).cuda()
    _, crps = ce.crps_fixed_ensemble_device(ens, obs, per_position=True)
    for d in range(5):
        old = crps_ensemble_device(ens, obs[d])
        # both kernels are within (2e-5, 2e-6) of the definition: the sum of the two tolerances
        np.testing.assert_allclose(crps[d].cpu().numpy(), old.cpu().numpy(), rtol=4e-5, atol=4e-6)


def _any_order_bound(v):
    """|sum(v) / n - fp64 sum in another order / n| <= n 2^-52 mean|v|: every partial sum of either order is at most sum|v| and
    takes part in fewer than n roundings of 2^-53 relative each, so each side is within (n / 2) 2^-52 sum|v| / n of the exact mean"""
    v = np.asarray(v, dtype=np.float64)
    return len(v) * EPS * np.abs(v).mean()


@pytest.mark.parametrize("n", [1, 2, 50, 1023, 2400, 240000])
def test_moments_match_mirror(n):
    ce = _ce()
    rng = np.random.default_rng(n)
    x = rng.gamma(0.5, 0.2, n) - rng.gamma(0.5, 0.23, n) + 0.3
    cnt, mean, var = ce.moments_device(x)
    _, m, v = cn.moments(x)
    assert cnt == n and abs(mean - m) <= _any_order_bound(x)
    if n == 1:
        assert math.isnan(var)
    else:
        # the any-order bound on the sum of the squares (scaled to ddof = 1), plus what it does not cover: the roundings of the
        # squares themselves and of the division on either side, at most 4 x 2^-52 of the variance
        assert abs(var - v) <= _any_order_bound((x - m) ** 2) * n / (n - 1) + 4 * EPS * v
    again = ce.moments_device(torch.from_numpy(x).cuda())                               # bit-identical on a repeat
    assert np.array_equal(np.array(again), np.array((cnt, mean, var)), equal_nan=True)


def test_bootstrap_means_match_mirror():
    ce = _ce()
    rng = np.random.default_rng(11)
    for n, N, seed in ((2400, 40, 0), (50, 64, 12345678901234), (1500, 8, 3)):
        x = rng.gamma(0.5, 0.2, n) - 0.08
        got = ce.bootstrap_means_device(x, N, seed=seed)
        want = cn.bootstrap_means(x, seed, 0, N)
        assert np.abs(got.cpu().numpy() - want).max() <= _any_order_bound(x)
        assert torch.equal(got, ce.bootstrap_means_device(x, N, seed=seed))             # bit-identical on a repeat
        k = N // 3
        parts = torch.cat([ce.bootstrap_means_device(x, k, seed=seed), ce.bootstrap_means_device(x, N - k, seed=seed, first_resample=k)])
        assert torch.equal(got, parts)                                                   # first_resample continues the run
        assert not torch.equal(got, ce.bootstrap_means_device(x, N, seed=seed + 1))
    far = 2 ** 32 + 5                                                                    # the resample number is 64-bit
    got = ce.bootstrap_means_device(x, 3, seed=3, first_resample=far).cpu().numpy()
    assert np.abs(got - cn.bootstrap_means(x, 3, far, 3)).max() <= _any_order_bound(x)


def test_bootstrap_indices_bit_for_bit():
    """x_j = 64^j, n = 8: a resample's sum is exact in fp64 and its base-64 digits are how often each index was drawn; and a one-hot
    x at n = 37: n times the mean counts one index."""
    ce = _ce()
    n, N, seed = 8, 50, 99
    x = 64.0 ** np.arange(n)
    sums = np.rint(ce.bootstrap_means_device(x, N, seed=seed).cpu().numpy() * n).astype(np.int64)
    for r in range(N):
        digits = [(int(sums[r]) >> (6 * j)) & 63 for j in range(n)]
        assert digits == np.bincount(cn.bootstrap_indices(seed, r, n), minlength=n).tolist(), r
    n, N = 37, 20
    counts = np.array([np.bincount(cn.bootstrap_indices(seed, r, n), minlength=n) for r in range(N)])
    for j in range(n):
        x = np.zeros(n)
        x[j] = 1.0
        got = np.rint(ce.bootstrap_means_device(x, N, seed=seed).cpu().numpy() * n).astype(np.int64)
        assert np.array_equal(got, counts[:, j]), j


def test_ttest_against_scipy():
    """t = m sqrt(n) / sqrt(v) from the device's mean m and variance v.  scipy's own m and v and the device's each lie within the
    any-order bounds B_m, B_v of the exact values, so the two t differ by at most 2 (|dt/dm| B_m + |dt/dv| B_v) =
    2 (sqrt(n / v) B_m + |t| B_v / (2 v)), plus a few roundings of t itself (4 x 2^-52 |t|)."""
    ce = _ce()
    ref = np.load(FIXTURE)
    for i in range(int(ref["n_vectors"])):
        x = ref[f"x{i}"]
        t_ref, p_ref = ref[f"tp{i}"]
        t, p = ce.ttest_1samp(x)
        n, m, v = cn.moments(x)
        b_m, b_v = _any_order_bound(x), _any_order_bound((x - m) ** 2) * n / (n - 1)
        bound = 2 * (math.sqrt(n / v) * b_m + abs(t_ref) * b_v / (2 * v)) + 4 * EPS * abs(t_ref)
        print(f"x{i}: t {t!r} (scipy {t_ref!r}, |diff| {abs(t - t_ref):.2e}, bound {bound:.2e}), p {p!r} (scipy {p_ref!r})")
        assert abs(t - t_ref) <= bound
        if p_ref == 0 or p_ref == 1:
            assert p == p_ref
        else:
            assert abs(p / p_ref - 1) < P_RTOL
    t, p = ce.ttest_1samp(ref["x1"], popmean=0.01)
    assert abs(t - (ref["x1"].mean() - 0.01) / math.sqrt(ref["x1"].var(ddof=1) / 50)) < 1e-12 and 0 < p < 1


def test_bootstrap_against_the_reference_numbers():
    """Different RNGs, so the bound is statistical: two independent estimates of the p-quantile of N bootstrap means differ with
    standard deviation sqrt(2) sqrt(p (1 - p) / N) / phi(z_p) sigma_m, sigma_m = std(x) / sqrt(n); at p = 0.01, N = 10 000
    (phi(z_p) = 0.02665) five of those are 0.264 sigma_m."""
    ce = _ce()
    ref = np.load(FIXTURE)
    x = ref["x0"]
    assert len(x) == 2400 and int(ref["boot_N"]) == 10000 and int(ref["boot_perc"]) == 1
    got = ce.bootstrapped_difference_onesample(x, perc=1, N=10000, seed=0)
    want = ref["boot0"]
    sigma_m = x.std(ddof=1) / math.sqrt(len(x))
    print(f"bootstrap {got!r} reference {want!r}: lower / upper differ by {abs(got[1] - want[1]) / sigma_m:.3f} / "
          f"{abs(got[2] - want[2]) / sigma_m:.3f} sigma_m (limit 0.264)")
    assert got.shape == (3,) and abs(got[0] - want[0]) < 1e-12
    assert abs(got[1] - want[1]) <= 0.264 * sigma_m and abs(got[2] - want[2]) <= 0.264 * sigma_m
    assert got[1] < got[0] < got[2]
    assert np.array_equal(got, ce.bootstrapped_difference_onesample(torch.from_numpy(x).cuda(), 1, 10000, seed=0))


def _real_days(rng, D, nd=16):
    return (rng.gamma(0.3, 2.0, (D, 24, nd, nd)) + 1e-3).astype(np.float32)


def test_days_equal_the_per_day_functions():
    ce = _ce()
    from pr_disagg_radar_gan_amd import ensemble, rainfarm
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    from pr_disagg_radar_gan_amd.ensemble import crps_ensemble_device
    T.configure(ndomain=16)
    gen = T.create_generator(seed=2)
    reals = _real_days(np.random.default_rng(0), 3)
    n, seed = 96, 11
    got = ce.crps_for_days(gen, reals, n_fake_per_real=n, seed=seed)
    assert got.shape == (3, 24) and got.dtype == np.float32
    for d in range(3):
        assert np.array_equal(got[d], ensemble.crps_for_day(gen, reals[d], n_fake_per_real=n, seed=seed + d)), d
    assert np.array_equal(got, ce.crps_for_days(gen, torch.from_numpy(reals).cuda(), n_fake_per_real=n, seed=seed))
    rf = ce.rainfarm_crps_for_days(reals, 2.2, 1.3, n_members=n, seed=seed)
    assert rf.shape == (3, 24)
    assert np.array_equal(rf[0], rainfarm.crps_for_day(reals[0], 2.2, 1.3, n_members=n, seed=seed))
    for d in range(3):
        real = torch.from_numpy(reals[d]).cuda()
        ens = rainfarm.downscale_device(real.sum(0), 2.2, 1.3, n_members=n, seed=seed, first_member=d * n)
        assert np.array_equal(rf[d], crps_ensemble_device(ens, real).mean(dim=(1, 2)).cpu().numpy()), d
    np.random.seed(4)
    a = ce.rainfarm_crps_for_days(reals[:1], 2.2, 1.3, n_members=8)                     # the global numpy RNG, R's order
    np.random.seed(4)
    assert np.array_equal(a[0], rainfarm.crps_for_day(reals[0], 2.2, 1.3, n_members=8))


def test_experiment_end_to_end():
    ce = _ce()
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    T.configure(ndomain=16)
    gen = T.create_generator(seed=2)
    rng = np.random.default_rng(1)
    reals = _real_days(rng, 4)
    data = _real_days(rng, 3, nd=40)                                 # (3, 24, 40, 40) radar-like days
    idx = np.array([(d, y, x) for d in range(3) for y in (0, 8, 20, 24) for x in (0, 12, 24)], dtype=np.int32)
    np.random.seed(77)
    clim = ce.climatology_sample(DeviceDataset(data, idx, ndomain=16), n=300)
    np.random.seed(77)
    sel = idx[np.random.randint(len(idx), size=300)]
    assert np.array_equal(clim.cpu().numpy(), np.array([data[d, :, y:y + 16, x:x + 16] for d, y, x in sel]))
    res = ce.crps_experiment(gen, reals, clim, n_fake_per_real=64, seed=5)
    assert res.rainfarm is None and res.gan.shape == res.random.shape == (4, 24)
    want = cn.hourly_mean(cn.crps_fixed(clim.cpu().numpy(), reals))
    np.testing.assert_allclose(res.random, want, rtol=RTOL, atol=ATOL)
    assert np.array_equal(res.gan, ce.crps_for_days(gen, reals, n_fake_per_real=64, seed=5))
    s = res.summary(N=500)
    assert set(s) == {"gan", "random", "rainfarm", "ttest_p", "bootstrap"} and s["rainfarm"] is None
    assert abs(s["gan"] - res.gan.astype(np.float64).mean()) < 1e-12
    np.testing.assert_allclose(s["random"], want.mean(), rtol=RTOL, atol=ATOL)
    diff = (res.gan.astype(np.float64) - res.random.astype(np.float64)).ravel()
    assert 0 <= s["ttest_p"] <= 1 and s["bootstrap"].shape == (3,) and abs(s["bootstrap"][0] - diff.mean()) < 1e-12
    assert s["bootstrap"][1] <= s["bootstrap"][0] <= s["bootstrap"][2]
    res2 = ce.crps_experiment(gen, reals, clim, slopes=(2.2, 1.3), n_fake_per_real=64, seed=5)
    assert res2.rainfarm.shape == (4, 24) and np.all(np.isfinite(res2.rainfarm)) and np.array_equal(res2.random, res.random)
    assert np.isfinite(res2.summary(N=100)["rainfarm"])
