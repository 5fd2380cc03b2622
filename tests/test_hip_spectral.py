"""-m gpu: radial spectra and pairwise log-spectral distance kernels (rdgan_spectral.hip.h) against the reference's own values
(tests/golden/lsd_reference.npz) and the fp64 restatement (tests/lsd_np.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import rdgan_np as onp
from tests import lsd_np

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsd_reference.npz")
# fp32 DFT against the reference's fp64 FFT, in dB on the bins with power; about 3x the largest error observed on the MI355X
SPEC_TOL_DB = 3e-5                  # observed: 4.4e-6 (nd 8), 6.1e-6 (16), 4.8e-6 (24), 5.5e-6 (32), 6.2e-6 (48), 1.1e-5 (64)
LSD_RTOL = 2e-5                    # fp32 difference form against fp64 on the same fp32 log-spectra


def _spectra(fields, log=True):
    from pr_disagg_radar_gan_amd.spectral import radial_spectra_device
    return radial_spectra_device(torch.from_numpy(np.ascontiguousarray(fields, dtype=np.float32)).cuda(), log=log).cpu().numpy()


def _check_spectra(got_db, fields):
    want_db = lsd_np.to_db(lsd_np.radial_spectra(fields))
    assert got_db.shape == want_db.shape
    assert np.array_equal(np.isneginf(got_db), np.isneginf(want_db)) and np.all(np.isfinite(got_db) | np.isneginf(got_db))
    fin = np.isfinite(want_db)
    return float(np.abs(got_db[fin] - want_db[fin]).max())


@pytest.mark.parametrize("nd", [8, 16, 64])
def test_spectra_match_reference_fixture(nd):
    ref = np.load(FIXTURE)
    f = ref[f"fields_nd{nd}"]
    got = _spectra(f)
    want = lsd_np.to_db(ref[f"spectra_nd{nd}"])
    assert np.array_equal(np.isneginf(got), np.isneginf(want))                  # dry and constant fields: every kept bin empty
    assert np.isneginf(got[-4]).all() and np.isneginf(got[-3]).all()
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max())
    print(f"nd {nd}: spectra max |error| vs the reference {err:.3e} dB (limit {SPEC_TOL_DB})")
    assert err < SPEC_TOL_DB
    lin = _spectra(f, log=False)
    np.testing.assert_allclose(lin, ref[f"spectra_nd{nd}"], rtol=SPEC_TOL_DB / 4.3, atol=0)


@pytest.mark.parametrize("nd", [24, 32, 48])
def test_spectra_match_restatement(nd):
    rng = np.random.default_rng(nd)
    f = rng.gamma(0.5, 1.5, (37, nd, nd))
    f[rng.random(f.shape) < 0.4] = 0.0
    f[0] = 0.0
    f[1] = 3.0
    f = f.astype(np.float32)
    err = _check_spectra(_spectra(f), f)
    print(f"nd {nd}: spectra max |error| vs fp64 {err:.3e} dB")
    assert err < SPEC_TOL_DB


def _lsd(a, b=None, **kw):
    from pr_disagg_radar_gan_amd.spectral import log_spectral_distance_device
    dev = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return log_spectral_distance_device(dev(a), None if b is None else dev(b), **kw)


def _random_db(rng, n, k, n_dry=0):
    s = 10 * np.log10(rng.gamma(0.8, 3.0, (n, k)) + 1e-4)
    s[rng.choice(n, size=n_dry, replace=False)] = -np.inf                    # dry fields: no power in any bin
    return s.astype(np.float32)


@pytest.mark.parametrize("nd", [8, 16, 64])
def test_matrix_matches_reference_matrices(nd):
    ref = np.load(FIXTURE)
    s = lsd_np.to_db(ref[f"spectra_nd{nd}"]).astype(np.float32)
    want = ref[f"lsd_nd{nd}"]
    got = _lsd(s, matrix=True).matrix.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-4, atol=1e-6)      # fp32 log-spectra in, as the device path has
    assert np.all(np.diag(got) == 0)


@pytest.mark.parametrize("n,m", [(1, 1), (7, 7), (129, 129), (1000, 1000), (7, 129), (129, 1000), (1000, 130)])
@pytest.mark.parametrize("excl", [True, False])
def test_matrix_matches_fp64(n, m, excl):
    rng = np.random.default_rng(n * 7919 + m)
    k = 9 if n != 1000 else 43
    a = _random_db(rng, n, k, n_dry=min(2, n - 1))
    b = _random_db(rng, m, k, n_dry=min(1, m - 1))
    got = _lsd(a, b, exclude_diagonal=excl, matrix=True).matrix.cpu().numpy()
    want = lsd_np.lsd_matrix_db(a, b, exclude_diagonal=excl)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=LSD_RTOL, atol=1e-6)
    if n == m:                                  # A is B against a copy of A
        same = _lsd(a, exclude_diagonal=excl, matrix=True)
        copy = _lsd(a, a.copy(), exclude_diagonal=excl, matrix=True)
        assert torch.equal(torch.nan_to_num(same.matrix, nan=-1.0), torch.nan_to_num(copy.matrix, nan=-1.0))
        assert np.array_equal(same.hist, copy.hist)
        assert np.array_equal([same.mean, same.std, same.min, same.max], [copy.mean, copy.std, copy.min, copy.max], equal_nan=True)


@pytest.mark.parametrize("n,m,bins,lo,hi", [(1000, 1000, 512, 0.0, 3.0), (777, 130, 64, 0.5, 2.0), (129, 1, 7, 0.0, 100.0)])
def test_histogram_exact_against_rule(n, m, bins, lo, hi):
    rng = np.random.default_rng(n + m)
    a = _random_db(rng, n, 15, n_dry=3)
    b = None if n == 1000 else _random_db(rng, m, 15, n_dry=min(1, m - 1))
    r = _lsd(a, b, bins=bins, range=(lo, hi), matrix=True)
    mm = n if b is None else m
    keep = np.ones((n, mm), dtype=bool)
    keep[np.arange(min(n, mm)), np.arange(min(n, mm))] = False   # the excluded diagonal (A is B or not) is not counted
    d = r.matrix.cpu().numpy()[keep]
    hb, under, over, nan, inf = lsd_np.hist_rule(d, bins, lo, hi)
    assert np.array_equal(r.hist, hb)
    assert (r.under, r.over, r.nan, r.inf) == (under, over, nan, inf)
    assert r.total == d.size == n * mm - min(n, mm)
    fin = d[np.isfinite(d)].astype(np.float64)
    assert r.count == fin.size
    np.testing.assert_allclose([r.mean, r.std], [fin.mean(), fin.std()], rtol=1e-6)
    assert (r.min, r.max) == (fin.min(), fin.max())
    again = _lsd(a, b, bins=bins, range=(lo, hi))
    assert np.array_equal(again.hist, r.hist) and (again.mean, again.std, again.min, again.max, again.total) == \
        (r.mean, r.std, r.min, r.max, r.total)                   # bit-identical repeated calls


def _rule_torch(d, bins, lo, hi):
    """hist_rule on the device for the large cases (the same fp32 operations)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    scale = float(np.float32(bins) / (hi32 - lo32))
    fin = d[torch.isfinite(d)]
    mid = fin[(fin >= float(lo32)) & (fin < float(hi32))]
    b = torch.clamp(torch.floor((mid - float(lo32)) * scale).to(torch.int64), max=bins - 1)
    return torch.bincount(b, minlength=bins).cpu().numpy()


def test_scale_24000_fields_equals_row_blocks():
    rng = np.random.default_rng(24000)
    n, bins, rng_ = 24000, 512, (0.0, 4.0)
    a = _random_db(rng, n, 9, n_dry=5)
    full = _lsd(a, bins=bins, range=rng_, exclude_diagonal=False)
    assert full.total == n * n
    acc = np.zeros(bins, np.int64)
    at = torch.from_numpy(a).cuda()
    for r0 in range(0, n, 4000):
        blk = _lsd(at[r0:r0 + 4000], at, bins=bins, range=rng_, exclude_diagonal=False, matrix=True).matrix
        acc += _rule_torch(blk, bins, *rng_)
        del blk
    assert np.array_equal(full.hist, acc)
    excl = _lsd(a, bins=bins, range=rng_)
    assert excl.total == n * n - n
    assert excl.nan == full.nan - 5 and excl.hist[0] == full.hist[0] - (n - 5)   # the diagonal: 0 dB, or NaN for a dry field


def test_total_beyond_32_bits():
    rng = np.random.default_rng(70000)
    n = 70000
    a = _random_db(rng, n, 9)
    r = _lsd(a, bins=256, range=(0.0, 4.0))
    assert n * n - n > 2 ** 32
    assert r.total == n * n - n and r.count + r.nan + r.inf == r.total and r.count == r.hist.sum() + r.under + r.over


def test_end_to_end_nd16():
    from pr_disagg_radar_gan_amd import ensemble, spectral
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    T.configure(ndomain=16)
    gen = T.create_generator(seed=3)
    rng = np.random.default_rng(50)
    n = 50
    real = rng.gamma(0.4, 1.5, (n, 24, 16, 16))
    real[rng.random(real.shape) < 0.5] = 0.0
    real[:, 5] = 0.0                                         # a dry hour every day
    real = real.astype(np.float32)
    z = rng.standard_normal((n, 100)).astype(np.float32)
    precip, am = ensemble.generate_one_per_condition(gen, real, latent=z, chunk=16)
    assert tuple(precip.shape) == (n, 24, 16, 16)
    params = [w.astype(np.float64) for w in gen.get_weights()]
    cond = real.sum(1) / np.float32(127.4)
    frac = onp.generator_forward(params, z.astype(np.float64), cond[..., None].astype(np.float64)).reshape(n, 24, 16, 16)
    np.testing.assert_allclose(precip.cpu().numpy(), frac * cond[:, None] * 127.4, rtol=3e-4,
                               atol=2e-6 * float(real.sum(1).max()))             # the fractions' tolerance, in mm/h
    np.testing.assert_allclose(am["gen"], precip.cpu().numpy().mean(axis=(2, 3)), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(am["real"], real.mean(axis=(2, 3)), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(am["fraction_gen"], frac.mean(axis=(2, 3)), rtol=3e-4, atol=1e-7)

    res = spectral.lsd_evaluation(real, precip, bins=200, range=(0.0, 5.0))
    g_host = precip.cpu().numpy().reshape(-1, 16, 16)
    s_real = lsd_np.to_db(lsd_np.radial_spectra(real.reshape(-1, 16, 16)))
    s_gen = lsd_np.to_db(lsd_np.radial_spectra(g_host))
    for key, (sa, sb) in {"real": (s_real, s_real), "gen": (s_gen, s_gen), "gen_real": (s_gen, s_real)}.items():
        d = lsd_np.lsd_matrix_db(sa, sb)
        d = d[~np.eye(len(sa), dtype=bool)]
        r = res[key]
        assert r.total == d.size == (24 * n) * (24 * n - 1), key
        assert (r.nan, r.inf) == (int(np.isnan(d).sum()), int(np.isinf(d).sum())), key
        fin = d[np.isfinite(d)]
        np.testing.assert_allclose([r.mean, r.std, r.min, r.max], [fin.mean(), fin.std(), fin.min(), fin.max()], rtol=1e-4,
                                   err_msg=key)
        ref_hist = np.histogram(fin, bins=200, range=(0.0, 5.0))[0]
        assert np.abs(r.hist - ref_hist).sum() <= 1e-3 * fin.size, key            # fp32 vs fp64 moves only edge cases
