"""The CRPS experiment on the host: the sorted-prefix mirror (tests/crps_np.py) against the O(n^2) definition, the p-value of the
t-test against scipy's values (tests/golden/crps_stats_reference.npz, made by tests/golden/make_crps_stats_fixture.py), the mirror's
bootstrap indices, argument checks before any device call, and no CPU fallback of the device API."""
import os

import numpy as np
import pytest

from oracle import data_np as od
from pr_disagg_radar_gan_amd import crps_experiment as ce
from tests import crps_np as cn

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crps_stats_reference.npz")
# two-sided p-value of the host's incomplete beta function against scipy, relative error; 10 x the worst observed over the fixture's
# grid (12 values of t x 6 of df) and its four (t, p) pairs: 2.2e-12, at df = 239 999 (at most 2.2e-14 for df <= 2 399)
P_RTOL = 2.2e-11


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300])
def test_mirror_equals_definition(n):
    rng = np.random.default_rng(n)
    ens = rng.gamma(0.4, 2.0, (n, 4, 5)).astype(np.float32)
    ens[rng.random(ens.shape) < 0.6] = 0.0                           # dry members, ties
    obs = rng.gamma(0.4, 2.0, (9, 4, 5)).astype(np.float32)
    obs[0] = 0.0                                                     # equal to the dry members (or below every member)
    obs[1] = -1.0                                                    # below every member
    obs[2] = ens.max(0) + 3.0                                        # above every member
    obs[3] = ens.max(0)                                              # equal to the maximum
    obs[4] = ens[n // 2]                                             # equal to a member
    got = cn.crps_fixed(ens, obs)
    for d in range(len(obs)):
        np.testing.assert_allclose(got[d], od.crps_ensemble(obs[d], ens), rtol=0, atol=1e-12)
    obs[5, 1, 2] = np.nan
    got = cn.crps_fixed(ens, obs)
    assert np.isnan(got[5, 1, 2]) and np.isnan(got).sum() == 1


def test_p_value_against_scipy(ref):
    worst = 0.0
    for t, df, sf in zip(ref["grid_t"], ref["grid_df"], ref["grid_sf"]):
        want = min(1.0, 2.0 * sf)
        got = ce.t_two_sided_p(t, df)
        assert got == ce.t_two_sided_p(-t, df)
        if t == 0:
            assert got == 1.0
            continue
        worst = max(worst, abs(got / want - 1))
    for i in range(int(ref["n_vectors"])):
        t, p = ref[f"tp{i}"]
        got = ce.t_two_sided_p(t, len(ref[f"x{i}"]) - 1)
        if p == 0 or p == 1:
            assert got == p                                          # the underflowed p and the t = 0 case: exact
        else:
            worst = max(worst, abs(got / p - 1))
    print(f"worst relative error of the p-value: {worst:.2e} (limit {P_RTOL})")
    assert worst < P_RTOL
    assert ce.t_two_sided_p(1e200, 10) == 0.0 and ce.t_two_sided_p(float("inf"), 10) == 0.0
    assert np.isnan(ce.t_two_sided_p(float("nan"), 10))


def test_bootstrap_index_mirror():
    for n in (1, 2, 50, 2400):
        idx = cn.bootstrap_indices(3, 0, n)
        assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < n
    a, b = cn.bootstrap_indices(3, 5, 2400), cn.bootstrap_indices(3, 6, 2400)
    assert not np.array_equal(a, b) and np.array_equal(a, cn.bootstrap_indices(3, 5, 2400))
    assert not np.array_equal(a, cn.bootstrap_indices(4, 5, 2400))
    assert not np.array_equal(a, cn.bootstrap_indices(3, 5 + 2 ** 32, 2400))          # the resample number is 64-bit
    cnt = np.bincount(np.concatenate([cn.bootstrap_indices(1, r, 100) for r in range(400)]), minlength=100)
    assert abs(cnt - 400).max() < 5 * np.sqrt(400)                   # uniform: 400 +- 20 per value
    x = np.random.default_rng(0).normal(size=300)
    n, m, v = cn.moments(x)
    assert n == 300 and abs(m - x.mean()) < 1e-15 and abs(v / x.var(ddof=1) - 1) < 1e-14


def test_argument_checks_precede_the_device(monkeypatch):
    def no_device():
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(ce, "require_gpu", no_device)
    ens, obs = np.zeros((4, 24, 8, 8), np.float32), np.zeros((2, 24, 8, 8), np.float32)
    for bad_ens, bad_obs in ((ens[:, :23], obs), (ens, obs[0]), (ens, np.zeros((2, 24, 16, 16), np.float32)),
                             (np.zeros((4, 24, 8, 6), np.float32), obs), (np.zeros((8193, 24, 1, 1), np.float32), np.zeros((1, 24, 1, 1))),
                             (np.zeros((0, 24, 8, 8), np.float32), obs)):
        with pytest.raises(ValueError):
            ce.crps_fixed_ensemble_device(bad_ens, bad_obs)
    x = np.arange(10.0)
    for perc in (0, 50, -1, 75):
        with pytest.raises(ValueError):
            ce.bootstrapped_difference_onesample(x, perc=perc)
    with pytest.raises(ValueError):
        ce.bootstrapped_difference_onesample(x, N=0)
    with pytest.raises(ValueError):
        ce.bootstrapped_difference_onesample(x.reshape(2, 5))
    with pytest.raises(ValueError):
        ce.bootstrap_means_device(x, 4, first_resample=-1)
    with pytest.raises(ValueError):
        ce.ttest_1samp(np.zeros((0,)))
    with pytest.raises(ValueError):
        ce.crps_for_days(None, obs[0])
    with pytest.raises(ValueError):
        ce.crps_for_days(None, obs, n_fake_per_real=0)
    with pytest.raises(ValueError):
        ce.rainfarm_crps_for_days(np.zeros((2, 24, 12, 12), np.float32), 2.0, 1.0)     # ndomain outside the RainFARM kernels
    with pytest.raises(ValueError):
        ce.crps_experiment(None, obs, np.zeros((4, 24, 16, 16), np.float32))
    with pytest.raises(ValueError):
        ce.crps_experiment(None, obs, ens, slopes=(1.0,))

    class _DS:
        indices = None
        ndomain = 16
    with pytest.raises(ValueError):
        ce.climatology_sample(_DS(), n=9000)
    with pytest.raises(ValueError):
        ce.climatology_sample(_DS(), n=10)                           # no valid-tile indices


def test_c_abi_rejects_bad_arguments():
    """-2 before any HIP call, so checkable without a device"""
    import ctypes
    from pr_disagg_radar_gan_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.rdgan_crps_fixed_ensemble(p, p, p, p, 0, 1, 16, None) == -2
    assert lib.rdgan_crps_fixed_ensemble(p, p, p, p, 8193, 1, 16, None) == -2
    assert lib.rdgan_crps_fixed_ensemble(p, p, None, None, 10, 1, 16, None) == -2
    assert lib.rdgan_crps_fixed_ensemble(p, p, p, p, 10, 0, 16, None) == -2
    assert lib.rdgan_crps_fixed_ensemble(p, p, p, p, 10, 2 ** 31 // (24 * 256) + 1, 16, None) == -2     # D npos >= 2^31
    assert lib.rdgan_bootstrap_means(p, 0, 1, 0, 4, p, None) == -2
    assert lib.rdgan_bootstrap_means(p, 2 ** 32, 1, 0, 4, p, None) == -2
    assert lib.rdgan_bootstrap_means(p, 10, 1, -1, 4, p, None) == -2
    assert lib.rdgan_bootstrap_means(p, 10, 1, 0, 0, p, None) == -2
    assert lib.rdgan_moments_f64(p, 0, p, None) == -2
    assert lib.rdgan_moments_f64(None, 5, p, None) == -2


def test_no_cpu_fallback():
    import torch
    from pr_disagg_radar_gan_amd import _lib
    import pr_disagg_radar_gan_amd as pkg
    assert hasattr(pkg, "crps_experiment")                           # imported with the package, with or without a device
    if torch.cuda.is_available():
        return                                                       # the device tests cover the calls
    with pytest.raises(_lib.RdganError):
        ce.crps_fixed_ensemble_device(np.zeros((4, 24, 8, 8), np.float32), np.zeros((2, 24, 8, 8), np.float32))
    with pytest.raises(_lib.RdganError):
        ce.ttest_1samp(np.arange(5.0))
    with pytest.raises(_lib.RdganError):
        ce.bootstrapped_difference_onesample(np.arange(5.0))
