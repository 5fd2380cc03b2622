"""Host side of the ensemble products (pr_disagg_radar_gan_amd/field_products.py): the numpy restatement (tests/products_np.py) against
a brute-force fp64 loop, against np.quantile and on its tie and NaN rules, and the argument errors of every Python entry, which are
raised before the device is touched.  No GPU needed."""
import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, field_products as FP
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import products_np as pn


def test_package_exports_the_module():
    import pr_disagg_radar_gan_amd
    assert pr_disagg_radar_gan_amd.field_products is FP


@pytest.mark.parametrize("windows", [(1,), (24,), (1, 2, 3, 6, 12, 24), (2, 3, 5, 7, 11, 13, 17, 23)])
def test_restatement_against_brute_force_on_integers(windows):
    """integer-valued fields: every fp32 window sum is exact, so the fp32 restatement and the fp64 loops must agree exactly"""
    rng = np.random.default_rng(sum(windows))
    x = rng.integers(0, 50, (3, 24, 4, 7)).astype(np.float32)
    x[0, :, 1, 2] = 0.0
    peaks, hour = pn.hourly_peaks(x, windows)
    ref, ref_hour, _ = pn.hourly_peaks_f64(x, windows)
    assert peaks.dtype == np.float32 and hour.dtype == np.uint8 and peaks.shape == (3, len(windows), 4, 7) and hour.shape == (3, 4, 7)
    assert np.array_equal(peaks.astype(np.float64), ref) and np.array_equal(hour, ref_hour)
    assert np.all(peaks[0, :, 1, 2] == 0) and hour[0, 1, 2] == 0
    if windows[-1] == 24:
        assert np.array_equal(peaks[:, -1].astype(np.float64), x.astype(np.float64).sum(1))
    assert np.all(np.diff(peaks, axis=1) >= 0)                   # non-negative hours: a longer window holds at least as much


def test_fp32_sums_are_sequential():
    """1 + 2^-24 + 2^-24 in fp32 from the left is 1 (each add rounds to even), pairwise it would be 1 + 2^-23"""
    x = np.zeros((1, 24, 1, 1), np.float32)
    x[0, 5:8, 0, 0] = (1.0, 2.0 ** -24, 2.0 ** -24)
    peaks, hour = pn.hourly_peaks(x, (3,))
    assert peaks[0, 0, 0, 0] == np.float32(1.0) and hour[0, 0, 0] == 3          # hours 3..5 already reach 1: the first wins


def test_first_index_wins_ties():
    x = np.zeros((1, 24, 1, 3), np.float32)
    x[0, [4, 9, 20], 0, 0] = 2.0                                 # three equal maxima
    x[0, 6:12, 0, 1] = 1.5                                       # a plateau
    x[0, 23, 0, 2] = 1.0
    peaks, hour = pn.hourly_peaks(x, (1, 3))
    assert hour[0, 0].tolist() == [4, 6, 23] and peaks[0, 0, 0].tolist() == [2.0, 1.5, 1.0]
    assert peaks[0, 1, 0].tolist() == [2.0, 4.5, 1.0]
    _, hour3 = pn.hourly_peaks(x, (3,))                          # the hour belongs to windows[0]
    assert hour3[0, 0].tolist() == [2, 6, 21]


def test_nan_rules():
    rng = np.random.default_rng(3)
    x = rng.random((2, 24, 2, 3)).astype(np.float32)
    x[1, 17, 1, 2] = np.nan
    peaks, hour = pn.hourly_peaks(x, (1, 6, 24))
    bad = np.zeros((2, 2, 3), bool)
    bad[1, 1, 2] = True
    assert np.array_equal(np.isnan(peaks), np.broadcast_to(bad[:, None], peaks.shape)) and np.array_equal(hour == 255, bad)
    m = rng.random((5, 4)).astype(np.float32)
    m[3, 1] = np.nan
    q, mean, ex, n_nan = pn.member_stats(m, (0.0, 0.5), (0.5,))
    col = np.array([False, True, False, False])
    assert n_nan == 1 and np.array_equal(np.isnan(q), np.broadcast_to(col, q.shape))
    assert np.array_equal(np.isnan(mean), col) and np.array_equal(np.isnan(ex), np.broadcast_to(col, ex.shape))


@pytest.mark.parametrize("S", [1, 2, 7, 100])
def test_member_stats_against_numpy(S):
    rng = np.random.default_rng(S)
    x = (rng.gamma(0.5, 6.0, (S, 33)) * (rng.random((S, 33)) > 0.6)).astype(np.float32)
    probs, thr = (0.0, 0.1, 0.5, 0.99, 1.0), (0.0, 1.0, 10.0)
    q, mean, ex, n_nan = pn.member_stats(x, probs, thr)
    assert n_nan == 0 and q.dtype == mean.dtype == ex.dtype == np.float32
    for j in range(33):
        col = x[:, j].astype(np.float64)
        assert np.array_equal(q[:, j], np.quantile(col, probs).astype(np.float32))
        assert mean[j] == np.float32(col.sum() / S)
        assert ex[:, j].tolist() == [np.float32(np.float64((col > t).sum()) / S) for t in thr]
    assert np.array_equal(q[0], x.min(0)) and np.array_equal(q[-1], x.max(0)) and np.all(np.diff(q, axis=0) >= 0)


class _Gen:
    ndomain, n_cond_channels = 16, 1


BAD_WINDOWS = [(3, 1), (1, 1, 3), (0, 1), (1, 25), tuple(range(1, 10)), (), (1.5, 3)]


def test_value_errors_before_any_device_call(monkeypatch):
    def no_gpu():
        raise AssertionError("an argument error must be raised before the device is touched")
    monkeypatch.setattr(F, "require_gpu", no_gpu)
    monkeypatch.setattr(FP, "require_gpu", no_gpu)
    monkeypatch.setattr(P, "gen", _Gen())
    ok = np.ones((20, 30), np.float32)
    plan = F.tile_plan(20, 30, 16, 4)
    T = plan.n_tiles
    frac, slots, daily = torch.zeros(2, 24, 16, 16), np.zeros((1, T), np.int32), torch.zeros(1, 20, 30)
    for w in BAD_WINDOWS:                               # unsorted, repeated, 0, 25, K = 9, none, not whole hours
        with pytest.raises(ValueError):
            FP.peaks_device(torch.zeros(2, 24, 5, 6), w)
        with pytest.raises(ValueError):
            FP.blend_peaks_device(frac, slots, plan, daily, w)
        with pytest.raises(ValueError):
            FP.disaggregate_peaks(_Gen(), ok, 2, windows=w)
        with pytest.raises(ValueError):
            FP.ensemble_products(_Gen(), ok, 2, windows=w)
        with pytest.raises(ValueError):
            P.scenario_products_field(ok, 2, windows=w)
    for shape in ((24, 5), (2, 23, 5, 6), (0, 24, 5, 6)):
        with pytest.raises(ValueError):
            FP.peaks_device(torch.zeros(shape))
    x = torch.zeros(5, 8)
    for probs in ((-0.1,), (0.5, 1.0000001), (float("nan"),), (), tuple(np.linspace(0, 1, 17))):              # outside [0, 1], Q = 0, 17
        with pytest.raises(ValueError):
            FP.member_stats_device(x, probs)
        with pytest.raises(ValueError):
            FP.ensemble_products(_Gen(), ok, 2, probs=probs)
        with pytest.raises(ValueError):
            P.scenario_products_field(ok, 2, probs=probs)
    for thr in (tuple(range(17)), (1.0, float("nan")), (float("inf"),)):                                        # T = 17, not finite
        with pytest.raises(ValueError):
            FP.member_stats_device(x, (0.5,), thr)
        with pytest.raises(ValueError):
            FP.ensemble_products(_Gen(), ok, 2, thresholds=thr)
        with pytest.raises(ValueError):
            P.scenario_products_field(ok, 2, thresholds=thr)
    with pytest.raises(ValueError):
        FP.ensemble_products(_Gen(), ok, 2, thresholds=np.ones((4, 2)))                # five windows, four rows
    for bad in (torch.zeros(0, 8), torch.zeros(4097, 2), torch.zeros(5, 0)):           # S = 0, S = 4097, no position
        with pytest.raises(ValueError):
            FP.member_stats_device(bad, (0.5,))
    with pytest.raises(ValueError):
        FP.member_stats_device(torch.zeros(16).as_strided((3, 8), (4, 1)), (0.5,))     # member stride 4 < P = 8
    with pytest.raises(ValueError):
        FP.member_stats_device(torch.zeros(3, 8, 2)[:, :, 0], (0.5,))                  # positions not contiguous
    with pytest.raises(ValueError):
        FP.ensemble_products(_Gen(), ok, 4097)
    # what field.disaggregate refuses, disaggregate_peaks refuses
    for kw in (dict(overlap=9), dict(latent_mode="per-pixel"), dict(latent=np.zeros((2, 100), np.float32)), dict(chunk=0)):
        with pytest.raises(ValueError):
            FP.disaggregate_peaks(_Gen(), ok, 2, **kw)
    with pytest.raises(ValueError):
        FP.disaggregate_peaks(_Gen(), np.ones((15, 30), np.float32), 2)
    with pytest.raises(ValueError):
        FP.blend_peaks_device(frac, np.zeros((1, T + 1), np.int32), plan, daily)
    with pytest.raises(ValueError):
        FP.blend_peaks_device(frac, np.full((1, T), 2, np.int32), plan, daily)


def test_no_gpu_means_rdgan_error(monkeypatch):
    if not torch.cuda.is_available():
        plan = F.tile_plan(20, 30, 16, 4)
        with pytest.raises(_lib.RdganError):
            FP.peaks_device(torch.zeros(2, 24, 5, 6))
        with pytest.raises(_lib.RdganError):
            FP.blend_peaks_device(torch.zeros(2, 24, 16, 16), np.zeros((1, 6), np.int32), plan, torch.zeros(1, 20, 30))
        with pytest.raises(_lib.RdganError):
            FP.member_stats_device(torch.zeros(5, 8), (0.5,))
        with pytest.raises(_lib.RdganError):
            FP.disaggregate_peaks(_Gen(), np.ones((20, 30), np.float32), 2)
        monkeypatch.setattr(P, "gen", _Gen())
        with pytest.raises(_lib.RdganError):
            P.scenario_products_field(np.ones((20, 30)), 2)
