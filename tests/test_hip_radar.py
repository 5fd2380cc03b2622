"""-m gpu: the radar ingest (csrc/rdgan_radar.hip.h) is BIT-IDENTICAL to its numpy restatement
(tests/radar_np.py) on all three vector paths, for any alignment, chunking and past 2^31 bytes; the valid-tile scan on the daily plane
gives the reference loop's and the existing kernel's answer; the data set built from codes feeds the gather unchanged."""
import ctypes
import datetime

import numpy as np
import pytest
import torch

from oracle import data_np as od
from tests import radar_np as rn
from tests.hip_util import lib, ptr, stream

pytestmark = pytest.mark.gpu


def _same(t, ref):
    return np.array_equal(t.cpu().numpy(), ref, equal_nan=True)


# planes: 37 x 45 = 1665 is odd (byte path); 38 x 46 = 1748 = 4 mod 16 (4 codes per lane); 40 x 48 = 1920 (16 codes per lane:
# 3 days x 120 groups = 360 lanes, two blocks, the second partial); 4 frames per hour on the byte path
@pytest.mark.parametrize("ny,nx,fph", [(37, 45, 12), (38, 46, 12), (40, 48, 12), (37, 45, 4)])
def test_hourly_daily_missing_are_bit_identical(ny, nx, fph):
    from pr_disagg_radar_gan_amd.data_pipeline import hourly_from_radar_codes
    c, h, d, n_missing = rn.case(3, ny, nx, fph)
    hourly, daily, got_missing = hourly_from_radar_codes(torch.from_numpy(c.copy()).cuda(), frames_per_hour=fph)
    assert hourly.shape == (3, 24, ny, nx) and daily.shape == (3, ny, nx) and hourly.dtype == torch.float32
    assert _same(hourly, h)
    assert _same(daily, d)
    assert got_missing == n_missing == 83
    # the flat (frames, ny, nx) form of the same codes
    h2, d2, m2 = hourly_from_radar_codes(torch.from_numpy(c.reshape(-1, ny, nx).copy()).cuda(), frames_per_hour=fph)
    assert _same(h2, h) and _same(d2, d) and m2 == n_missing


def test_misaligned_device_view_gives_the_same_result():
    from pr_disagg_radar_gan_amd.data_pipeline import hourly_from_radar_codes
    c, h, d, n_missing = rn.case(3, 40, 48, 12)
    for shift in (1, 4):                      # bytes; 4: dword-aligned only
        buf = torch.zeros(c.size + 16, dtype=torch.uint8, device="cuda")
        view = buf[shift:shift + c.size].view(c.shape)
        view.copy_(torch.from_numpy(c.copy()))
        assert view.data_ptr() % 16 == shift and view.is_contiguous()
        hourly, daily, got_missing = hourly_from_radar_codes(view)
        assert _same(hourly, h) and _same(daily, d) and got_missing == n_missing


@pytest.mark.parametrize("chunk_days", [1, 2, None])
def test_chunked_streaming_from_a_host_memmap(tmp_path, chunk_days):
    from pr_disagg_radar_gan_amd.data_pipeline import hourly_from_radar_codes
    c, h, d, n_missing = rn.case(3, 40, 48, 12)
    path = tmp_path / "codes.u8"
    c.tofile(path)
    mm = np.memmap(path, dtype=np.uint8, mode="r", shape=c.shape)
    single = hourly_from_radar_codes(torch.from_numpy(c.copy()).cuda())
    hourly, daily, got_missing = hourly_from_radar_codes(mm, chunk_days=chunk_days)       # 2: the last range is one day short
    assert torch.equal(hourly.view(torch.int32), single[0].view(torch.int32))
    assert torch.equal(daily.view(torch.int32), single[1].view(torch.int32))
    assert got_missing == single[2] == n_missing
    assert _same(hourly, h) and _same(daily, d)


def test_indexing_past_two_to_the_31():
    """40 x 48 pixels, just enough days that the codes pass 2^31 bytes: the first and the last day against the restatement"""
    from pr_disagg_radar_gan_amd.data_pipeline import hourly_from_radar_codes, radar_lut
    ny, nx, fpd = 40, 48, 288
    day_bytes = fpd * ny * nx
    n_days = 2 ** 31 // day_bytes + 2
    assert (n_days - 1) * day_bytes > 2 ** 31                  # the whole last day lies past the 32-bit range
    g = torch.Generator(device="cuda").manual_seed(0)
    codes = torch.empty((n_days, fpd, ny, nx), dtype=torch.uint8, device="cuda")
    step = 256
    for d0 in range(0, n_days, step):                          # (codes 0..255 uniformly: 255, missing, included)
        part = codes[d0:d0 + step]
        part.copy_(torch.randint(0, 256, part.shape, generator=g, device="cuda", dtype=torch.uint8))
    hourly, daily, n_missing = hourly_from_radar_codes(codes)
    lut = radar_lut()
    for day in (0, n_days - 1):
        c = codes[day:day + 1].cpu().numpy()
        h = rn.hourly(c, lut, 12)
        assert _same(hourly[day:day + 1], h)
        assert _same(daily[day:day + 1], rn.daily(h))
        assert np.isnan(h).any() and not np.isnan(h).all()
    assert n_missing == int(torch.isnan(hourly).sum().item())


@pytest.fixture(scope="module")
def scan_case():
    c, h, _, _ = rn.case(3, 37, 45, 12)
    return c, h


@pytest.mark.parametrize("nd,stride,count", [(16, 16, 4), (16, 5, 32), (16, 1, 666), (8, 3, 88)])
def test_valid_tile_scan_on_the_daily_plane(scan_case, nd, stride, count):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    c, h = scan_case
    ref = od.valid_indices(h, nd, stride, 5, 20)
    assert len(ref) == count > 0
    ds = DeviceDataset.from_radar_codes(c, ndomain=nd)
    assert ds.daily is not None and ds.n_missing == 83
    got = ds.valid_indices(stride, 5, 20)
    assert got == ref                                          # the reference loop, in its order
    old = DeviceDataset(h.copy(), ndomain=nd)
    assert old.daily is None
    assert old.valid_indices(stride, 5, 20) == ref             # the existing kernel (24 floats per pixel)
    plane = old.ensure_daily()
    assert torch.equal(plane.view(torch.int32), ds.daily.view(torch.int32)) and old.daily is plane
    assert old.valid_indices(stride, 5, 20) == ref             # ... and the new one on the plane built from the floats
    day, y0, y1, x0, x1 = rn.PATCH
    assert not any(t == 1 or (t == day and i < y1 and i + nd > y0 and j < x1 and j + nd > x0) for t, i, j in got)


def test_from_codes_to_gathered_batches():
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    c, h, d, _ = rn.case(3, 37, 45, 12)
    dates = [datetime.date(2016, 12, 30), datetime.date(2016, 12, 31), datetime.date(2017, 1, 1)]
    ds = DeviceDataset.from_radar_codes(c, dates=dates, ndomain=16)
    assert ds.timelist.tolist() == [365, 366, 1]
    idx = np.array(ds.valid_indices(1, 5, 20))
    ds.set_indices(idx)
    ixs = np.random.default_rng(5).integers(0, len(idx), 29)
    batch, cond = ds.gather(ixs)
    rb, rc = od.gather_real(h, idx, ixs, 16)
    assert np.array_equal(batch.cpu().numpy(), rb) and np.array_equal(cond.cpu().numpy(), rc)
    ds.check_flags()
    ds.set_extra_condition('doy')                              # the day of year of `dates`
    _, c3 = ds.gather(ixs)
    assert c3.shape == (29, 16, 16, 3) and ds.n_cond_channels == 3
    ref3 = od.extra_condition(rc, idx[ixs], 16, 'doy', ds.timelist).astype(np.float32)
    c3 = c3.cpu().numpy()
    assert np.array_equal(c3[..., 0], ref3[..., 0])
    np.testing.assert_allclose(c3[..., 1:], ref3[..., 1:], rtol=0, atol=1e-7)      # fp64 sin / cos rounded to fp32 (half an ulp of 1 = 6e-8)
    with pytest.raises(ValueError):
        DeviceDataset.from_radar_codes(c, ndomain=16).set_extra_condition('doy')       # no dates, no timelist


def test_device_file_formats(tmp_path):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    c, h, _, _ = rn.case(3, 37, 45, 12)
    ds = DeviceDataset.from_radar_codes(c)
    back = np.load(ds.save_npy(tmp_path / "x_tres1"), mmap_mode="r")
    assert back.dtype == np.float32 and np.array_equal(back, h, equal_nan=True)


def test_c_entries_reject_bad_arguments():
    L = lib()
    codes = torch.zeros((1, 288, 40, 48), dtype=torch.uint8, device="cuda")
    lut = torch.zeros(256, device="cuda")
    out = torch.zeros((1, 24, 40, 48), device="cuda")
    day = torch.zeros((1, 40, 48), device="cuda")
    valid = torch.zeros(64, dtype=torch.int32, device="cuda")
    null = ctypes.c_void_p(0)
    assert L.rdgan_data_radar_hourly(ptr(codes), ptr(lut), 1, 5, 40, 48, ptr(out), null, null, stream()) == -2
    assert L.rdgan_data_radar_hourly(ptr(codes), ptr(lut), 0, 12, 40, 48, ptr(out), null, null, stream()) == -2
    assert L.rdgan_data_radar_hourly(ptr(codes), ptr(lut), 1, 12, 40, 0, ptr(out), null, null, stream()) == -2
    assert L.rdgan_data_radar_hourly(ptr(codes), ptr(lut), 1, 12, 40, 48, ptr(out), null, null, stream()) == 0      # both optional outputs off
    assert L.rdgan_data_valid_tiles_daily(ptr(day), 1, 40, 48, 49, 16, 5.0, 20, ptr(valid), stream()) == -2         # ndomain > nx
    assert L.rdgan_data_valid_tiles_daily(ptr(day), 1, 40, 48, 41, 16, 5.0, 20, ptr(valid), stream()) == -2         # ndomain > ny
    assert L.rdgan_data_valid_tiles_daily(ptr(day), 1, 40, 48, 16, 0, 5.0, 20, ptr(valid), stream()) == -2
    assert L.rdgan_data_valid_tiles_daily(ptr(day), 1, 40, 48, 16, 16, 5.0, 20, ptr(valid), stream()) == 0
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0                       # lut of zeros
