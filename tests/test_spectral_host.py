"""Log-spectral distance on the host: the fp64 restatement (tests/lsd_np.py) against the fixture produced by the reference's own
functions (tests/golden/make_lsd_fixture.py), closed forms, the bin count per ndomain, and no CPU fallback of the device API."""
import os

import numpy as np
import pytest

from tests import lsd_np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsd_reference.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


@pytest.mark.parametrize("nd", [8, 16, 64])
def test_restatement_reproduces_reference_spectra(ref, nd):
    spec = lsd_np.radial_spectra(ref[f"fields_nd{nd}"])
    want = ref[f"spectra_nd{nd}"]
    assert spec.shape == want.shape == (len(ref[f"fields_nd{nd}"]), lsd_np.K_TABLE[nd])
    np.testing.assert_allclose(spec, want, rtol=1e-10, atol=0)
    assert np.array_equal(want[-4], np.zeros(want.shape[1])) and np.array_equal(want[-3], np.zeros(want.shape[1]))


@pytest.mark.parametrize("nd", [8, 16, 64])
def test_restatement_reproduces_reference_matrices(ref, nd):
    want = ref[f"lsd_nd{nd}"]
    got = lsd_np.lsd_matrix(ref[f"spectra_nd{nd}"], ref[f"spectra_nd{nd}"])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.isnan(want).sum() == 2 and np.isinf(want).any()          # dry/constant pairs: NaN; one dry side: +inf
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-10, atol=0)
    assert np.all(np.diag(want) == 0)


@pytest.mark.parametrize("nd", sorted(lsd_np.K_TABLE))
def test_bins_per_ndomain(nd):
    assert lsd_np.n_bins(nd) == lsd_np.K_TABLE[nd]
    b = lsd_np.bin_map(nd)
    assert all((b == k).any() for k in range(0, lsd_np.K_TABLE[nd] + 2))      # every bin populated
    c = (2 * np.arange(nd) - (nd - 1)) / 2.0
    r = np.hypot(c[:, None], c[None, :])
    assert np.array_equal(b, np.floor(r).astype(int))                          # exact integers = floor of the fp64 radius here
    from pr_disagg_radar_gan_amd import _lib
    assert _lib.load().rdgan_spectra_bins(nd) == lsd_np.K_TABLE[nd]             # host code of the C ABI, no device needed


def test_closed_forms():
    rng = np.random.default_rng(7)
    for nd in (8, 16, 24, 64):
        one = np.zeros((nd, nd)); one[3, nd - 2] = 2.0
        np.testing.assert_allclose(lsd_np.radial_spectrum(one), 4.0, rtol=1e-12)           # single pixel: flat |F|^2 = v^2
        assert np.array_equal(lsd_np.radial_spectrum(np.full((nd, nd), 0.75)), np.zeros(lsd_np.K_TABLE[nd]))
        p = rng.gamma(0.5, 1.0, (5, lsd_np.K_TABLE[nd])) + 1e-3
        K = p.shape[1]
        np.testing.assert_allclose(np.diag(lsd_np.lsd_matrix(p, p, exclude_diagonal=False)), 0.0, atol=0)
        for c in (0.25, 3.0, 1e3):
            d = lsd_np.lsd_matrix(p, c * p, exclude_diagonal=False)
            np.testing.assert_allclose(np.diag(d), abs(10 * np.log10(c)) / np.sqrt(K), rtol=1e-12)


def test_hist_rule_edges():
    d = np.array([np.nan, np.inf, -0.0, 0.0, 0.999, 1.0, 9.999, 10.0, 11.0], dtype=np.float32)
    bins, under, over, nan, inf = lsd_np.hist_rule(d, 10, 0.0, 10.0)
    assert (under, over, nan, inf) == (0, 2, 1, 1)
    assert bins[0] == 3 and bins[1] == 1 and bins[9] == 1 and bins.sum() == 5


def test_device_api_has_no_cpu_fallback():
    import torch
    from pr_disagg_radar_gan_amd import _lib, ensemble, spectral
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    src = open(spectral.__file__).read()
    assert "oracle" not in src.replace("RdganError", "")
    if not torch.cuda.is_available():                  # with a GPU the device paths are tested in test_hip_spectral.py
        with pytest.raises(_lib.RdganError):
            spectral.radial_spectra_device(torch.zeros(2, 16, 16))
        with pytest.raises(_lib.RdganError):
            spectral.log_spectral_distance_device(np.zeros((3, 9), np.float32))
        with pytest.raises(_lib.RdganError):
            spectral.lsd_evaluation(np.zeros((1, 24, 16, 16), np.float32), np.zeros((1, 24, 16, 16), np.float32))
        T.configure(ndomain=16)
        with pytest.raises(_lib.RdganError):
            ensemble.generate_one_per_condition(T.create_generator(seed=0), np.zeros((2, 24, 16, 16), np.float32))
