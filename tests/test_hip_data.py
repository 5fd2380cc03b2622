"""-m gpu: device input pipeline (tile gather / normalisation, valid-tile scan) is BIT-IDENTICAL to the numpy
restatement of the reference's host code."""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import data_np as od
from tests.hip_util import lib, ptr, stream

pytestmark = pytest.mark.gpu


def _data(n_days=5, ny=70, nx=53, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.gamma(0.15, 3.0, (n_days, 24, ny, nx)).astype(np.float32)
    d[rng.random(d.shape) < 0.5] = 0.0                    # lots of dry hours, like radar data
    d[1, :, 10:14, 20:30] = np.nan                        # a patch of missing data on day 1
    return d


@pytest.mark.parametrize("nd,stride", [(16, 16), (16, 5), (32, 16)])
def test_valid_tile_scan_matches_reference_loop(nd, stride):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d = _data()
    ds = DeviceDataset(d, ndomain=nd)
    got = ds.valid_indices(stride=stride, tp_thresh_daily=5, n_thresh=20)
    ref = od.valid_indices(d, nd, stride, 5, 20)
    assert got == ref and len(ref) > 0
    assert not any(t == 1 and i < 14 and i + nd > 10 and j < 30 and j + nd > 20 for t, i, j in got)   # no box over the NaN patch


@pytest.mark.parametrize("nd", [16, 32])
def test_gather_is_bit_identical(nd):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d = _data(seed=1)
    idx = np.array(od.valid_indices(d, nd, 7, 5, 20))
    ds = DeviceDataset(d, idx, ndomain=nd)
    ixs = np.random.default_rng(2).integers(0, len(idx), 37)
    batch, cond = ds.gather(ixs)
    rb, rc = od.gather_real(d, idx, ixs, nd)
    assert batch.shape == (37, 24, nd, nd, 1) and cond.shape == (37, nd, nd, 1)
    assert np.array_equal(batch.cpu().numpy(), rb)
    assert np.array_equal(cond.cpu().numpy(), rc)
    np.testing.assert_allclose(batch.cpu().numpy().sum(axis=1), 1.0, rtol=1e-5)
    ds.check_flags()
    _, c2 = ds.gather(ixs, with_batch=False)
    assert np.array_equal(c2.cpu().numpy(), rc)
    np.random.seed(3)
    b3, c3 = ds.sample_real(8)
    np.random.seed(3)
    ix3 = np.random.randint(len(idx), size=8)
    assert np.array_equal(b3.cpu().numpy(), od.gather_real(d, idx, ix3, nd)[0])


def test_gather_flags_missing_data():
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d = _data(seed=4)
    ds = DeviceDataset(d, np.array([[1, 8, 18]]), ndomain=16)      # overlaps the NaN patch
    ds.gather([0])
    with pytest.raises(AssertionError):
        ds.check_flags()


# ------------------------------------------------------------------------------------------------------------------------
# Edges of the input pipeline: flag word, tiles flush with the array's last row / column, index bounds, the valid scan at its
# thresholds, more boxes than one launch holds, indexing past 2^31 elements, argument checks of the C entries.  Every comparison
# is exact: bits of the numpy restatement, or exact integer / sequential-fp32 torch forms on the device where the array is too
# large for the host.
# ------------------------------------------------------------------------------------------------------------------------
NORM = 127.4
LAUNCH_BOXES = 0xFFFFFF             # boxes per launch of k_valid_tiles; k_valid_tiles_daily: 4 per block, so 4 x this per sweep


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _assert_bits(got, ref):
    """NaN at the same places, every other value bit for bit (so -0.0 != 0.0 and inf == inf)"""
    got, ref = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(ref))
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn)
    assert np.array_equal(got.view(np.uint32)[~gn], ref.view(np.uint32)[~rn])


def _gather_ref(d, idx, ixs, nd):
    with np.errstate(divide="ignore", invalid="ignore"):
        return od.gather_real(d, np.asarray(idx), np.asarray(ixs), nd, NORM)


def _wet(n_days, ny, nx, seed):
    """radar-like hours (half of them dry), no pixel with a dry day: every fraction is finite and inside [0, 1]"""
    rng = np.random.default_rng(seed)
    d = rng.gamma(0.15, 3.0, (n_days, 24, ny, nx)).astype(np.float32)
    d[rng.random(d.shape) < 0.5] = 0.0
    d[:, 0] += np.float32(0.25)
    return d


# ---- 1. the flag word -------------------------------------------------------------------------------------------------
BIT2, BIT1, CLEAN = 0, 1, 2          # rows of the index array of _flag_case


def _flag_case():
    """(2, 24, 20, 19), nd 8.  Every pixel: 1 in hour 0, else 0 (fractions 1, 0, 0, ...).  Tile (0, 0, 0) holds one pixel with hours
    (-1, 2, 0, ...): daily sum 1, fractions -1 and 2, finite.  Tile (1, 12, 11), flush with the last row and column, holds one
    all-dry pixel: 0 / 0.  Tile (0, 12, 11) is clean."""
    d = np.zeros((2, 24, 20, 19), np.float32)
    d[:, 0] = 1.0
    d[0, :2, 3, 4] = (-1.0, 2.0)
    d[1, :, 17, 15] = 0.0
    return d, np.array([[0, 0, 0], [1, 12, 11], [0, 12, 11]])


@pytest.mark.parametrize("rows,word,message", [([BIT2], 2, "outside"), ([BIT1], 1, "NaN"), ([BIT2, BIT1, CLEAN], 3, "NaN")])
def test_flag_bits_alone_and_together(rows, word, message):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d, idx = _flag_case()
    ds = DeviceDataset(d, idx, ndomain=8)
    assert int(ds.flags.item()) == 0
    batch, cond = ds.gather(rows)
    rb, rc = _gather_ref(d, idx, rows, 8)
    _assert_bits(batch, rb)
    _assert_bits(cond, rc)
    assert np.isnan(rb).any() == bool(word & 1) and ((rb < 0) | (rb > 1)).any() == bool(word & 2)
    assert int(ds.flags.item()) == word
    with pytest.raises(AssertionError, match=message):
        ds.check_flags()
    assert int(ds.flags.item()) == 0
    ds.check_flags()                                           # the raise cleared the word


def test_flag_bits_add_up_over_calls_and_the_condition_alone_is_clean():
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d, idx = _flag_case()
    ds = DeviceDataset(d, idx, ndomain=8)
    for rows in ([BIT2], [BIT1], [BIT2, BIT1]):                # the daily sums are 1 and 0: finite, so nothing to flag
        none, cond = ds.gather(rows, with_batch=False)
        assert none is None
        _assert_bits(cond, _gather_ref(d, idx, rows, 8)[1])
        assert int(ds.flags.item()) == 0
        ds.check_flags()
    ds.gather([BIT2])
    assert int(ds.flags.item()) == 2
    ds.gather([BIT1])
    assert int(ds.flags.item()) == 3                           # two calls, one word
    ds.gather([CLEAN])
    assert int(ds.flags.item()) == 3
    with pytest.raises(AssertionError):
        ds.check_flags()
    ds.check_flags()


@pytest.mark.parametrize("bad", [BIT2, BIT1])
def test_flags_stick_until_checked(bad):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d, idx = _flag_case()
    ds = DeviceDataset(d, idx, ndomain=8)
    ds.gather([bad, CLEAN], True)
    ds.gather([CLEAN], False)
    ds.gather([CLEAN, CLEAN], True)
    with pytest.raises(AssertionError):
        ds.check_flags()
    ds.check_flags()
    ds.gather([CLEAN], True)
    ds.check_flags()


@pytest.mark.parametrize("bad", [BIT2, BIT1])
def test_flags_stick_over_the_calls_of_a_training_iteration(bad):
    """train(): sample_real n_disc times, sample_latent, then ONE check_flags.  The bad tile is in the first critic batch only."""
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d, idx = _flag_case()
    ds = DeviceDataset(d, idx[[bad]], ndomain=8)
    np.random.seed(0)
    ds.sample_real(4)
    ds.set_indices(idx[[CLEAN]])
    ds.sample_real(4)
    latent, cond = ds.sample_latent(4, 16)
    assert latent.shape == (4, 16) and cond.shape == (4, 8, 8, 1)
    with pytest.raises(AssertionError):
        ds.check_flags()
    ds.check_flags()
    ds.sample_real(4)
    ds.sample_latent(4, 16)
    ds.check_flags()


# ---- 2. tiles at the array's edges ------------------------------------------------------------------------------------
def _edge_indices(n_days, ny, nx, nd):
    """all four corners and the middle of each edge on the first and the last day (the far ones flush with the last row / column),
    and one tile inside on a middle day"""
    ys, xs = sorted({0, (ny - nd) // 2, ny - nd}), sorted({0, (nx - nd) // 2, nx - nd})
    out = [(t, y, x) for t in sorted({0, n_days - 1}) for y in ys for x in xs if len(ys) == 1 or len(xs) == 1
           or (y, x) != (ys[1], xs[1])]
    out.append((n_days // 2, ys[len(ys) // 2], xs[len(xs) // 2]))
    return np.array(out)


@pytest.mark.parametrize("nd,shape", [(8, (3, 21, 19)), (16, (3, 37, 23)), (32, (3, 45, 39)), (64, (3, 70, 67)),
                                      (16, (2, 16, 16)), (8, (2, 8, 8))])         # the last two: the whole plane is one tile
def test_gather_at_the_edges_of_the_array(nd, shape):
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    n_days, ny, nx = shape
    d = _wet(n_days, ny, nx, seed=10 + nd)
    idx = _edge_indices(n_days, ny, nx, nd)
    assert (n_days - 1, ny - nd, nx - nd) in [tuple(r) for r in idx] and (0, 0, 0) in [tuple(r) for r in idx]
    assert len(idx) == (17 if ny > nd else 3)
    ds = DeviceDataset(d, idx, ndomain=nd)
    last = int(np.nonzero((idx == (n_days - 1, ny - nd, nx - nd)).all(axis=1))[0][0])
    for ixs in (np.arange(len(idx)), np.array([last]), np.array([0, 0, last, last, 0, len(idx) - 1, last])):   # all; n = 1; repeats
        rb, rc = _gather_ref(d, idx, ixs, nd)
        batch, cond = ds.gather(ixs)
        assert batch.shape == (len(ixs), 24, nd, nd, 1) and cond.shape == (len(ixs), nd, nd, 1)
        _assert_bits(batch, rb)
        _assert_bits(cond, rc)
        none, c2 = ds.gather(ixs, with_batch=False)
        assert none is None
        _assert_bits(c2, rc)
    ds.check_flags()


# ---- 3. set_indices ---------------------------------------------------------------------------------------------------
def test_set_indices_bounds():
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    d = _wet(3, 20, 19, seed=3)
    nd = 8
    ds = DeviceDataset(d, ndomain=nd)
    ok = np.array([[2, 12, 11], [0, 0, 0], [2, 12, 0], [0, 0, 11]])            # ny - nd = 12, nx - nd = 11 are inside
    ds.set_indices(ok)
    before, n_before = ds.indices, ds.n_samples
    for bad, message in [([[0, 13, 0]], "outside"), ([[0, 0, 12]], "outside"), ([[3, 0, 0]], "outside"),
                         ([[-1, 0, 0]], "negative"), ([[0, -1, 0]], "negative"), ([[0, 0, -1]], "negative"),
                         ([[0, 0, 0], [1, 2, -1]], "negative"), ([[0, 0, 0], [-3, 13, 12]], "negative"),
                         (np.zeros((0, 3), np.int64), "empty"), ([], "shape"), (np.zeros((4, 2), np.int64), "shape"),
                         ([0, 0, 0], "shape")]:
        with pytest.raises(ValueError, match=message):
            ds.set_indices(bad)
        assert ds.indices is before and ds.n_samples == n_before           # nothing was uploaded, nothing to launch on
    with pytest.raises(ValueError, match="negative"):
        DeviceDataset(d, [[0, -1, 0]], ndomain=nd)
    ixs = np.arange(4)
    batch, cond = ds.gather(ixs)
    rb, rc = _gather_ref(d, ok, ixs, nd)
    _assert_bits(batch, rb)
    _assert_bits(cond, rc)
    ds.check_flags()


# ---- 4. the valid scan, both kernels ----------------------------------------------------------------------------------
def _scan_both(h, nd, stride, thresh, n_thresh):
    """od.valid_indices' list, after checking that k_valid_tiles (hourly array) and k_valid_tiles_daily (daily plane) both give it"""
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    ref = od.valid_indices(h, nd, stride, thresh, n_thresh)
    ds = DeviceDataset(h, ndomain=nd)
    assert ds.daily is None
    assert ds.valid_indices(stride, thresh, n_thresh) == ref
    assert ds.daily is None
    plane = ds.ensure_daily()
    _assert_bits(plane, np.stack([np.sum(h[t], axis=0) for t in range(h.shape[0])]))
    assert ds.valid_indices(stride, thresh, n_thresh) == ref and ds.daily is plane
    return ref


@pytest.mark.parametrize("ny,nx", [(20, 21), (21, 20), (20, 20), (21, 21)])
def test_valid_scan_box_flush_with_the_last_row_or_column(ny, nx):
    """nd 8, stride 4: range(0, 12, 4) leaves the box at 12 out, range(0, 13, 4) takes it.  Day 0 is wet, day 1 dry."""
    h = np.zeros((2, 24, ny, nx), np.float32)
    h[0, 5] = 6.0
    ref = _scan_both(h, 8, 4, 5, 20)
    want = [(0, i, j) for i in range(0, 9 + 4 * (ny == 21), 4) for j in range(0, 9 + 4 * (nx == 21), 4)]
    assert ref == want and len(want) == (3 + (ny == 21)) * (3 + (nx == 21))
    assert ((0, 12, 0) in ref) == (ny == 21) and ((0, 0, 12) in ref) == (nx == 21)


@pytest.mark.parametrize("nd,ny,nx,stride", [(16, 16, 40, 4), (16, 40, 16, 4), (16, 16, 16, 1), (24, 40, 23, 4), (24, 23, 40, 4)])
def test_valid_scan_without_a_box(nd, ny, nx, stride):
    """ny == nd: range(0, 0, stride) is empty (the reference never takes a box flush with the far edge); nd > nx: no box fits"""
    h = np.zeros((2, 24, ny, nx), np.float32)
    h[:, 5] = 6.0
    assert _scan_both(h, nd, stride, 5, 0) == []


def test_valid_scan_stride_beyond_the_array():
    """stride > ny: range(0, ny - nd, stride) is [0], so the one box at the origin is scanned (and no other)"""
    h = np.zeros((3, 24, 20, 19), np.float32)
    h[0, 5] = 6.0
    h[2, 5, :8, :8] = 6.0
    h[2, 5, 7, 7] = np.nan
    assert _scan_both(h, 8, 23, 5, 20) == [(0, 0, 0)]
    assert _scan_both(h, 8, 23, 5, 0) == [(0, 0, 0), (1, 0, 0)]


SCAN_STRIDE = {5: 3, 8: 4, 12: 5, 16: 16, 64: 7}


@pytest.mark.parametrize("nd", [5, 8, 12, 16, 64])
def test_valid_scan_thresholds(nd):
    """3 x 4 boxes a day; everything happens in the LAST box of the grid, whose pixels are counted in row-major order (25 and 144
    pixels: the last sweep of 64 lanes is partly filled).  Background 1 mm, wet pixel 1 + 5 = 6 > 5, 1 + 4 = 5 is not > 5.
      day 0: 20 wet pixels, the first 10 and the last 10 of the box         -> valid at n_thresh 20
      day 1: the same, but the first pixel is exactly 5                     -> 19: not valid
      day 2: 23 wet pixels, the last pixel of the box (its far corner) NaN  -> not valid, whatever n_thresh"""
    s, n_thresh = SCAN_STRIDE[nd], 20
    ny, nx = nd + 2 * s + 1, nd + 3 * s + 2
    i0, j0 = 2 * s, 3 * s
    assert list(range(0, ny - nd, s))[-1] == i0 and list(range(0, nx - nd, s))[-1] == j0
    h = np.zeros((3, 24, ny, nx), np.float32)
    h[:, 0] = 1.0
    at = lambda pix: (i0 + pix // nd, j0 + pix % nd)
    npx = nd * nd
    for day, wet in ((0, list(range(10)) + list(range(npx - 10, npx))), (1, list(range(1, 10)) + list(range(npx - 10, npx))),
                     (2, list(range(10)) + list(range(npx - 14, npx - 1)))):
        for pix in wet:
            h[(day, 3) + at(pix)] = 2.5
            h[(day, 17) + at(pix)] = 2.5
    h[(1, 3) + at(0)] = 4.0
    h[(2, 7) + at(npx - 1)] = np.nan
    daily = h.sum(axis=1)
    assert (daily[0] > 5).sum() == 20 and (daily[1] > 5).sum() == 19 and (daily[1] == 5).sum() == 1 and (daily[2] > 5).sum() == 23
    assert _scan_both(h, nd, s, 5, n_thresh) == [(0, i0, j0)]
    assert _scan_both(h, nd, s, 5, n_thresh - 1) == [(0, i0, j0), (1, i0, j0)]
    assert _scan_both(h, nd, s, 5, n_thresh + 1) == []
    every = [(t, i, j) for t in range(3) for i in range(0, ny - nd, s) for j in range(0, nx - nd, s)]
    assert len(every) == 36
    assert _scan_both(h, nd, s, 5, 0) == every[:-1]                               # only the box with the NaN is missing


# ---- 5. more boxes than one launch holds ------------------------------------------------------------------------------
def _box_counts(mask, nd, nbi, nbj):
    """(days, ny, nx) bool on the device -> exact number of set pixels in every stride-1 box, int32 (days, nbi, nbj): integer 2-D
    cumulative sum, four corners"""
    days, ny, nx = mask.shape
    s = torch.zeros((days, ny + 1, nx + 1), dtype=torch.int32, device=mask.device)
    s[:, 1:, 1:] = mask.to(torch.int32).cumsum(1, dtype=torch.int32).cumsum(2, dtype=torch.int32)
    return s[:, nd:nd + nbi, nd:nd + nbj] - s[:, :nbi, nd:nd + nbj] - s[:, nd:nd + nbi, :nbj] + s[:, :nbi, :nbj]


def _valid_ref(plane, nd, thresh, n_thresh):
    nbi, nbj = plane.shape[1] - nd, plane.shape[2] - nd              # len(range(0, ny - nd, 1))
    ok = (_box_counts(plane > thresh, nd, nbi, nbj) >= n_thresh) & (_box_counts(torch.isnan(plane), nd, nbi, nbj) == 0)
    return ok.to(torch.int32)


def test_valid_scan_daily_loops_past_one_grid():
    """310 x 472 x 472 = 69.1 M boxes of 8 x 8 at stride 1 > 4 x 0xFFFFFF = 67.1 M: the blocks of k_valid_tiles_daily go round again
    for the last 1.95 M boxes (days 301 to 309)"""
    t0 = time.perf_counter()
    n_days, ny, nx, nd, thresh, n_thresh = 310, 480, 480, 8, 5.0, 20
    nbi = nbj = ny - nd
    sweep = 4 * LAUNCH_BOXES
    assert n_days * nbi * nbj > sweep
    g = torch.Generator(device="cuda").manual_seed(5)
    plane = torch.zeros((n_days, ny, nx), device="cuda")
    for day in (1, 155, 305, 309):                                   # 35 % wet: 22.4 +- 3.8 of 64 pixels, either side of n_thresh
        plane[day] = torch.where(torch.rand((ny, nx), generator=g, device="cuda") < 0.35, 6.0, 0.0)
    plane[0, 10:40, 10:60] = 6.0
    plane[0, 100:108, 200:208] = 5.0                                 # not > 5
    plane[150, 200:300, 100:400] = 7.0
    plane[309, 440:, 430:] = 8.0                                     # the last day's last boxes are wet
    for day, y, x in ((0, 20, 30), (150, 250, 250), (155, 7, 7), (309, 470, 470), (309, 3, 400)):
        plane[day, y, x] = float("nan")
    valid = torch.full((n_days, nbi, nbj), -7, dtype=torch.int32, device="cuda")
    assert lib().rdgan_data_valid_tiles_daily(ptr(plane), n_days, ny, nx, nd, 1, thresh, n_thresh, ptr(valid), stream()) == 0
    ref = _valid_ref(plane, nd, thresh, n_thresh)
    assert torch.equal(valid, ref)
    flat = ref.view(-1)
    for part in (flat[:sweep], flat[sweep:], flat[-(nbi * nbj):]):   # valid and invalid boxes in the first sweep and beyond it
        assert bool(part.any()) and not bool(part.all())
    assert int(ref[309, nbi - 1, nbj - 1]) == 1 and int(ref[309, 471 - nd, 471 - nd]) == 0
    torch.cuda.synchronize()
    print(f"case 5a: {n_days * nbi * nbj} boxes, {int(flat.sum())} valid, {time.perf_counter() - t0:.2f} s")


def test_valid_indices_switches_to_the_daily_plane():
    """78 x 464 x 464 = 16.79 M boxes of 16 x 16 at stride 1 > 0xFFFFFF: more than one launch of k_valid_tiles holds"""
    from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
    t0 = time.perf_counter()
    n_days, ny, nx, nd, thresh, n_thresh = 78, 480, 480, 16, 5.0, 90
    assert n_days * (ny - nd) * (nx - nd) > LAUNCH_BOXES >= (n_days - 1) * (ny - nd) * (nx - nd)
    rng = np.random.default_rng(6)
    h = np.zeros((n_days, 24, ny, nx), np.float32)                   # mostly dry
    h[0, 3, 10:40, 10:60] = h[0, 17, 10:40, 10:60] = 3.0             # 6 a day
    h[0, 7, 20, 30] = np.nan
    h[40, 0, 100:130, 100:130] = h[40, 23, 100:130, 100:130] = 2.5   # 5 a day: not > 5
    h[41, 2] = np.where(rng.random((ny, nx)) < 0.35, 6.0, 0.0)       # 89.6 +- 7.6 of 256 pixels, either side of n_thresh
    h[41, 9] = rng.random((ny, nx), dtype=np.float32)                # (sums that round)
    h[77, 5, 440:, 430:] = 8.0
    ds = DeviceDataset(h, ndomain=nd)
    assert ds.daily is None
    got = ds.valid_indices(stride=1, tp_thresh_daily=thresh, n_thresh=n_thresh)
    assert ds.daily is not None
    s = ds.data[:, 0].clone()
    for hour in range(1, 24):
        s = s + ds.data[:, hour]                                     # np.sum(data[t], axis=0): in order, fp32
    assert torch.equal(torch.isnan(s), torch.isnan(ds.daily)) and torch.equal(torch.nan_to_num(s), torch.nan_to_num(ds.daily))
    assert int(torch.isnan(s).sum()) == 1
    ref = _valid_ref(s, nd, thresh, n_thresh)
    t, i, j = np.nonzero(ref.cpu().numpy())
    want = list(zip(t.tolist(), i.tolist(), j.tolist()))
    assert got == want
    days = {a for a, _, _ in want}
    assert days == {0, 41, 77} and (77, ny - nd - 1, nx - nd - 1) in want and (0, 10, 20) not in want and (0, 24, 44) in want
    n41 = sum(1 for a, _, _ in want if a == 41)
    assert 0 < n41 < (ny - nd) * (nx - nd)
    print(f"case 5b: {n_days * (ny - nd) * (nx - nd)} boxes, {len(want)} valid ({n41} on the random day), {time.perf_counter() - t0:.2f} s")


# ---- 6. past 2^31 elements --------------------------------------------------------------------------------------------
def test_input_array_past_two_to_the_31_elements():
    """(87383, 24, 32, 32) fp32, 8.6 GB, built on the device: element 2^31 lies inside day 87381, day 87382 lies wholly beyond"""
    t0 = time.perf_counter()
    L = lib()
    n_days, ny, nx, nd, stride = 87383, 32, 32, 16, 8
    per_day = 24 * ny * nx
    assert 87381 * per_day < 2 ** 31 < 87382 * per_day and n_days * per_day > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(7)
    data = torch.empty((n_days, 24, ny, nx), device="cuda")
    for d0 in range(0, n_days, 4096):                                # 56 % exact zeros, else uniform in [0, 1.75): daily sums 9.2 +- 2.7
        part = data[d0:d0 + 4096]
        r = torch.rand(part.shape, generator=g, device="cuda")
        part.copy_(torch.where(r < 0.5625, torch.zeros_like(r), (r - 0.5625) * 4))
        del r
    data[87381, 5, 4:9, 20:27] = float("nan")
    data[87382, :, 31, 31] = 0.0                                     # the very last pixel: a dry day, 0 / 0
    days = [0, 87380, 87381, 87382]
    host = data[days].cpu().numpy()
    assert (host == 0).mean() > 0.5 and np.isnan(host[2]).sum() == 35

    # gather: tiles on the four days, the last one ending on the array's last element
    local = np.array([(k, y, x) for k in range(4) for y, x in ((0, 0), (7, 9), (16, 16))])
    idx = local.copy()
    idx[:, 0] = np.array(days)[local[:, 0]]
    n = len(idx)
    idx_d = torch.from_numpy(idx.astype(np.int32)).cuda()
    batch = torch.full((n, 24, nd, nd, 1), -7.0, device="cuda")
    cond = torch.full((n, nd, nd, 1), -7.0, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.rdgan_data_gather(ptr(data), n_days, ny, nx, ptr(idx_d), n, nd, NORM, ptr(batch), ptr(cond), ptr(flags), stream()) == 0
    rb, rc = _gather_ref(host, local, np.arange(n), nd)
    _assert_bits(batch, rb)
    _assert_bits(cond, rc)
    assert int(flags.item()) == 1 and np.isnan(rb[-1]).any() and np.isnan(rb[6:9]).any() and not np.isnan(rb[:6]).any()
    cond.fill_(-7.0)
    assert L.rdgan_data_gather(ptr(data), n_days, ny, nx, ptr(idx_d), n, nd, NORM, None, ptr(cond), ptr(flags), stream()) == 0
    _assert_bits(cond, rc)

    # daily plane: the sequential fp32 sum, bit for bit
    plane = torch.full((n_days, ny, nx), -7.0, device="cuda")
    assert L.rdgan_data_daily_sum(ptr(data), n_days, ny, nx, ptr(plane), stream()) == 0
    s = data[:, 0].clone()
    for hour in range(1, 24):
        s = s + data[:, hour]
    nan = torch.isnan(s)
    assert torch.equal(nan, torch.isnan(plane)) and int(nan.sum()) == 35
    assert torch.equal(torch.nan_to_num(s).view(torch.int32), torch.nan_to_num(plane).view(torch.int32))
    del s, nan

    # valid scan: 4 boxes a day, 135 +- 8 of 256 pixels above 9 mm
    thresh, n_thresh = 9.0, 135
    assert len(range(0, ny - nd, stride)) == 2
    v_hourly = torch.full((n_days, 2, 2), -7, dtype=torch.int32, device="cuda")
    v_daily = torch.full((n_days, 2, 2), -7, dtype=torch.int32, device="cuda")
    assert L.rdgan_data_valid_tiles(ptr(data), n_days, ny, nx, nd, stride, thresh, n_thresh, ptr(v_hourly), stream()) == 0
    assert L.rdgan_data_valid_tiles_daily(ptr(plane), n_days, ny, nx, nd, stride, thresh, n_thresh, ptr(v_daily), stream()) == 0
    assert torch.equal(v_hourly, v_daily)
    n_valid = int(v_daily.sum())
    assert int(v_daily.min()) == 0 and int(v_daily.max()) == 1 and n_days < n_valid < 3 * n_days       # about half of them
    want = od.valid_indices(host, nd, stride, thresh, n_thresh)
    got = [(k, int(i) * stride, int(j) * stride) for k, day in enumerate(days) for i, j in zip(*np.nonzero(v_daily[day].cpu().numpy()))]
    assert got == want and 0 < len(want) < 16
    assert not any(k == 2 and i < 9 and j + nd > 20 for k, i, j in want)       # no box over the NaN patch of day 87381
    print(f"case 6 (input past 2^31): {n_days * per_day} elements, {n_valid} of {4 * n_days} boxes valid, {time.perf_counter() - t0:.2f} s")


def test_gather_output_past_two_to_the_31_elements():
    """nd 64: 21852 tiles x 24 x 64 x 64 = 2.148e9 fractions > 2^31, six indices repeated 3642 times"""
    t0 = time.perf_counter()
    nd, ny, nx = 64, 70, 67
    d = _wet(2, ny, nx, seed=8)
    pattern = np.array([(0, 0, 0), (1, ny - nd, nx - nd), (0, 3, 1), (1, 0, nx - nd), (0, ny - nd, 0), (1, 2, 2)])
    period, repeats = len(pattern), 3642
    n = period * repeats
    assert n * 24 * nd * nd > 2 ** 31
    data = torch.from_numpy(d).cuda()
    idx_d = torch.from_numpy(pattern.astype(np.int32)).cuda().repeat(repeats, 1).contiguous()
    batch = torch.empty((n, 24, nd, nd, 1), device="cuda")
    cond = torch.empty((n, nd, nd, 1), device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert lib().rdgan_data_gather(ptr(data), 2, ny, nx, ptr(idx_d), n, nd, NORM, ptr(batch), ptr(cond), ptr(flags), stream()) == 0
    rb, rc = _gather_ref(d, pattern, np.arange(period), nd)
    _assert_bits(batch[:period], rb)
    _assert_bits(cond[:period], rc)
    assert int(flags.item()) == 0 and not np.isnan(rb).any()
    b, c = batch.view(repeats, -1), cond.view(repeats, -1)
    for k0 in range(0, repeats, 256):                                # every repeat equals the first period (no NaN: == is enough)
        assert bool((b[k0:k0 + 256] == b[:1]).all()) and bool((c[k0:k0 + 256] == c[:1]).all()), k0
    print(f"case 6 (output past 2^31): {n * 24 * nd * nd} fractions, {time.perf_counter() - t0:.2f} s")


# ---- 7. argument checks of the C entries ------------------------------------------------------------------------------
def test_c_entries_return_minus_2_and_write_nothing():
    L = lib()
    n_days, ny, nx, nd, n = 2, 40, 48, 16, 3
    data = torch.ones((n_days, 24, ny, nx), device="cuda")
    idx = torch.tensor([[0, 0, 0], [1, 24, 32], [1, 3, 5]], dtype=torch.int32, device="cuda")
    batch = torch.full((n, 24, nd, nd, 1), -7.0, device="cuda")
    cond = torch.full((n, nd, nd, 1), -7.0, device="cuda")
    flags = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    plane = torch.full((n_days, ny, nx), -7.0, device="cuda")
    valid = torch.full((n_days, 24, 32), -7, dtype=torch.int32, device="cuda")       # stride 1: 24 x 32 boxes a day
    null = ctypes.c_void_p(0)

    def gather(data=ptr(data), n_days=n_days, ny=ny, nx=nx, idx=ptr(idx), n=n, nd=nd, batch=ptr(batch), cond=ptr(cond), flags=ptr(flags)):
        return L.rdgan_data_gather(data, n_days, ny, nx, idx, n, nd, NORM, batch, cond, flags, stream())

    def scan(data=ptr(data), n_days=n_days, ny=ny, nx=nx, nd=nd, stride=1, valid=ptr(valid)):
        return L.rdgan_data_valid_tiles(data, n_days, ny, nx, nd, stride, 5.0, 20, valid, stream())

    def daily(data=ptr(data), n_days=n_days, ny=ny, nx=nx, plane=ptr(plane)):
        return L.rdgan_data_daily_sum(data, n_days, ny, nx, plane, stream())

    def scan_daily(plane=ptr(plane), n_days=n_days, ny=ny, nx=nx, nd=nd, stride=1, valid=ptr(valid)):
        return L.rdgan_data_valid_tiles_daily(plane, n_days, ny, nx, nd, stride, 5.0, 20, valid, stream())

    extents = [dict(n_days=0), dict(n_days=-1), dict(ny=0), dict(nx=0), dict(ny=-40), dict(nx=-48)]
    boxes = [dict(nd=0), dict(nd=-16), dict(nd=ny + 1), dict(nd=nx + 1), dict(ny=nd - 1), dict(nx=nd - 1)]
    strides = [dict(stride=0), dict(stride=-1)]
    assert (LAUNCH_BOXES // (24 * 32) + 1) * 24 * 32 > LAUNCH_BOXES
    for fn_, cases in ((gather, extents + boxes + [dict(data=null), dict(idx=null), dict(cond=null), dict(flags=null), dict(n=0), dict(n=-3)]),
                       (scan, extents + boxes + strides + [dict(data=null), dict(valid=null),
                                                           dict(n_days=LAUNCH_BOXES // (24 * 32) + 1)]),         # 16 777 728 boxes
                       (daily, extents + [dict(data=null), dict(plane=null)]),
                       (scan_daily, extents + boxes + strides + [dict(plane=null), dict(valid=null)])):
        for kw in cases:
            assert fn_(**kw) == -2, (fn_.__name__, kw)
    torch.cuda.synchronize()
    for buf in (batch, cond, flags, plane, valid):
        assert bool((buf == -7).all())                                 # nothing was launched
    flags.zero_()
    assert gather(batch=null) == 0 and scan() == 0                     # (no fractions wanted: accepted)
    torch.cuda.synchronize()
    assert bool((batch == -7).all()) and bool((cond == float(np.float32(24.0) / np.float32(NORM))).all())
    assert not bool((valid == -7).any()) and int(flags.item()) == 0
    valid.fill_(-7)
    assert gather() == 0 and daily() == 0 and scan_daily() == 0
    torch.cuda.synchronize()
    assert bool((batch == float(np.float32(1.0) / np.float32(24.0))).all()) and bool((plane == 24.0).all())
    assert bool((valid == 1).all()) and int(flags.item()) == 0
