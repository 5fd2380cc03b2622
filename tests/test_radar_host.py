"""CPU tests of the radar ingest's host side (data_pipeline: radar_lut, dates -> day of year, argument checks, the two file
formats) and of the numpy restatement the GPU tests compare with (tests/radar_np.py)."""
import datetime
import pickle

import numpy as np
import pytest

from oracle import data_np as od
from pr_disagg_radar_gan_amd import data_pipeline as dp
from tests import radar_np as rn


def test_radar_lut_is_the_reference_formula_in_float32():
    lut = dp.radar_lut()
    assert lut.dtype == np.float32 and lut.shape == (256,)
    assert np.isfinite(lut[:255]).all() and (lut[:255] >= np.finfo(np.float32).tiny).all()     # normal numbers: no flush-to-zero question
    assert np.isnan(lut[255])
    ref = rn.lut_f64()
    # fp32 power chain against fp64: the exponent dbz/10 * ln 10 / 1.5 reaches |7.2 ln 10|, so a few ulp (6e-8 each) of its
    # rounding are amplified to ~1e-6 relative; observed 1.1e-6
    err = np.max(np.abs(lut[:255] - ref) / ref)
    print("radar_lut relative error against fp64:", err)
    assert err < 1e-5
    np.testing.assert_allclose(lut[0], 2.4367e-5, rtol=1e-4)
    np.testing.assert_allclose(lut[150], 0.24367, rtol=1e-4)
    assert np.all(np.diff(lut[:255]) > 0)
    other = dp.radar_lut(missing=0, minutes=15)
    assert np.isnan(other[0]) and np.isfinite(other[255])
    np.testing.assert_allclose(other[1:255], 3 * lut[1:255], rtol=1e-6)


def test_restatement_equals_numpy_reshape_sum_bit_for_bit():
    lut = dp.radar_lut()
    for shape in ((3, 37, 45, 12), (3, 37, 45, 4)):
        c, h, d, n_missing = rn.case(*shape)
        n, ny, nx, fph = shape
        alt = lut[c].reshape(n, 24, fph, ny, nx).sum(axis=2)
        assert np.array_equal(h, alt, equal_nan=True)
        assert np.array_equal(d, h.sum(axis=1), equal_nan=True)
        assert n_missing == 83              # 2 single frames + the last element + 4 x 10 pixels x 2 hours
    c, h, d, _ = rn.case(3, 37, 45, 12)
    assert 5 < np.nanmax(h) < 20 and 20 < np.nanmax(d) < 60          # mm per hour / per day of the rain block
    day, y0, y1, x0, x1 = rn.PATCH
    assert np.isnan(h[day, 5:7, y0:y1, x0:x1]).all() and not np.isnan(h[day, 7, y0:y1, x0:x1]).any()
    assert np.isnan(h[0, 0, 3, 5]) and np.isnan(h[0, 0, 4, 6]) and np.isnan(h[2, 23, -1, -1])


@pytest.mark.parametrize("nd,stride,count", [(16, 16, 4), (16, 5, 32), (16, 1, 666), (8, 3, 88)])
def test_recipe_has_valid_boxes_but_none_over_missing_or_dry_data(nd, stride, count):
    _, h, _, _ = rn.case(3, 37, 45, 12)
    ref = od.valid_indices(h, nd, stride, 5, 20)
    assert len(ref) == count
    day, y0, y1, x0, x1 = rn.PATCH
    assert not any(t == 1 for t, _, _ in ref)                                                    # the dry day
    assert not any(t == day and i < y1 and i + nd > y0 and j < x1 and j + nd > x0 for t, i, j in ref)


def test_dates_to_day_of_year():
    dates = [datetime.date(2015, 1, 1), datetime.date(2015, 3, 1), datetime.date(2016, 3, 1), datetime.date(2016, 12, 31),
             datetime.date(2015, 12, 31)]
    assert dp.day_of_year(dates).tolist() == [1, 60, 61, 366, 365]
    d64 = np.arange("2011-12-30", "2012-01-03", dtype="datetime64[D]")
    assert dp.day_of_year(d64).tolist() == [364, 365, 1, 2]
    assert dp.day_of_year(d64).dtype == np.int64
    with pytest.raises(ValueError):
        dp.day_of_year(np.zeros((2, 2), "datetime64[D]"))


def test_bad_codes_raise_value_error_before_any_device_call():
    ok = np.zeros((2, 288, 5, 6), np.uint8)
    for fn in (dp.hourly_from_radar_codes, dp.DeviceDataset.from_radar_codes):
        with pytest.raises(ValueError):
            fn(ok.astype(np.float32))                                   # wrong dtype
        with pytest.raises(ValueError):
            fn(ok.astype(np.int8))
        with pytest.raises(ValueError):
            fn(ok[:, :287])                                             # not 24 * fph frames per day
        with pytest.raises(ValueError):
            fn(ok.reshape(-1, 5, 6)[:500])                              # not a whole number of days
        with pytest.raises(ValueError):
            fn(ok[0, 0])                                                # wrong number of dimensions
        with pytest.raises(ValueError):
            fn(ok, frames_per_hour=5)                                   # frame count the kernel does not take
        with pytest.raises(ValueError):
            fn(ok, frames_per_hour=6)                                   # 288 frames are not 24 * 6
        with pytest.raises(ValueError):
            fn(ok[:0])
        with pytest.raises(ValueError):
            fn([[1, 2]])                                                # not an array
    with pytest.raises(ValueError):
        dp.DeviceDataset.from_radar_codes(ok, dates=[datetime.date(2015, 1, 1)])       # one date for two days


def test_file_formats_round_trip(tmp_path):
    import torch
    _, h, _, _ = rn.case(3, 37, 45, 12)
    path = dp.write_npy(tmp_path / "20150101-20150103_tres1", torch.from_numpy(h.copy()), chunk_days=2)
    assert path.endswith("_tres1.npy")
    back = np.load(path, mmap_mode="r")                                # gan_train_cwgangp_pixelnorm.py:117
    assert back.dtype == np.float32 and back.shape == h.shape and np.array_equal(back, h, equal_nan=True)
    idx = od.valid_indices(h, 16, 5, 5, 20)
    pkl = dp.DeviceDataset.save_valid_indices(tmp_path / "valid.pkl", np.array(idx))
    with open(pkl, "rb") as f:
        got = pickle.load(f)
    assert got == idx and all(type(t) is tuple and all(type(v) is int for v in t) for t in got)
    assert np.array(got).shape == (len(idx), 3)                        # what T does with it (:120)
