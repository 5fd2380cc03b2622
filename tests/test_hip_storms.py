"""-m gpu: storms of hourly fields (csrc/rdgan_storms.hip.h, pr_disagg_radar_gan_amd/storms.py) against the numpy restatement
(tests/storms_np.py, itself checked on the CPU by tests/test_storms_host.py).  Everything is an integer: label maps are compared
with torch.equal, states int64 against int64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, cells as CL, field as F, models, storms as SM, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import cells_np as cn
from tests import storms_np as sn
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

# one pixel, one ragged row, one tile, four tiles (the second row and column one pixel wide), ragged tiles: (ny, nx, days)
SHAPES = {"1x1": (1, 1, 3), "1x70": (1, 70, 3), "64x64": (64, 64, 2), "65x65": (65, 65, 2), "130x67": (130, 67, 1)}
THR3 = (0.1, 1.0, 5.0)


def check(x, thresholds, conn, reach, label_t=0, want=None, **kw):
    """state and labels of one add() of x against the yardstick -> the StormStructure"""
    want, lab = want or sn.storms_np(x, thresholds, conn, reach, want_labels=label_t)
    labels = torch.full(x.shape, -7, dtype=torch.int32, device="cuda")
    ss = SM.StormStructure(thresholds, conn, reach, **kw).add(dev(x), labels_out=labels, label_threshold=label_t)
    assert torch.equal(labels.cpu(), torch.from_numpy(lab))
    assert torch.equal(ss.state().cpu(), torch.from_numpy(sn.flat_state(want)))
    sn.check_identities(SM.split_state(ss.state().cpu().numpy(), len(thresholds)))
    return ss


@functools.lru_cache(maxsize=None)
def rain_like(ny, nx, days, seed):
    """(days, 24, ny, nx): a smoothed noise field above its 70 % quantile is wet, so the wet areas have a size and move and change
    slowly from hour to hour; gamma amounts of at least 0.2; one value exactly at a threshold.  Shared: copy before writing."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(days, 24, ny, nx))
    for _ in range(2):
        g = (g + np.roll(g, 1, 1) + np.roll(g, 1, 2) + np.roll(g, -1, 2) + np.roll(g, 1, 3) + np.roll(g, -1, 3)) / 6
    x = ((0.2 + rng.gamma(0.6, 3.0, g.shape)) * (g > np.quantile(g, 0.7))).astype(np.float32)
    x[0, 11, ny // 3, nx // 3] = np.float32(1.0)
    return x


@pytest.mark.parametrize("reach", [0, 1, 4])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_fields_against_restatement(name, conn, reach):
    ny, nx, days = SHAPES[name]
    check(rain_like(ny, nx, days, len(name)), THR3, conn, reach, label_t=1)


@pytest.mark.parametrize("reach", [0, 1, 4])
@pytest.mark.parametrize("conn", [4, 8])
def test_deep_trees_through_all_hours(conn, reach):
    """a serpentine and a spiral over the whole 130 x 70 plane (3 x 2 ragged tiles) in hour 0, each continued by a single pixel
    that steps back along the figure's last row through the other 23 hours"""
    ny, nx = 130, 70
    x = np.stack([sn.staircase(cn.serpentine(ny, nx), ny, nx), 2 * sn.staircase(cn.spiral(ny, nx), ny, nx)])
    s = check(x, (0.5,), conn, reach).result()
    if reach == 0:                                                  # hour 1 still lies on the figure, hour 2 beside hour 1
        assert s.storms.sum() == 2 * 23 and s.longest_duration[0, 2] == 2
    else:
        assert s.storms.tolist() == [[0, 0, 0, 2]] and s.duration_hist[0, 3, 23] == 2 and s.storms_per_day[0, 1] == 2


def test_all_wet_day_is_one_storm():
    x = np.full((24, 130, 130), 0.75, np.float32)
    size = 24 * 130 * 130
    assert size == 405600
    for conn, reach in ((8, 1), (4, 0)):
        ss = SM.StormStructure((0.5,), conn, reach).add(dev(x))
        o = SM.split_state(ss.state().cpu().numpy(), 1)
        assert sn.only_nonzero(o["storms"]) == {(0, 3): 1} and sn.only_nonzero(o["duration_hist"]) == {(0, 3, 23): 1}
        assert sn.only_nonzero(o["start_hour"]) == {(0, 3, 0): 1} and sn.only_nonzero(o["size_hist"]) == {(0, 3, 18): 1}
        assert sn.only_nonzero(o["size_sum"]) == {(0, 3): size} and sn.only_nonzero(o["size_sq_sum"]) == {(0, 3): size * size}
        assert sn.only_nonzero(o["size_by_duration"]) == {(0, 3, 23): size} and sn.only_nonzero(o["volume_by_duration"]) == {(0, 3, 23): size * 49152}
        assert sn.only_nonzero(o["storms_per_day"]) == {(0, 1): 1} and sn.only_nonzero(o["longest_duration"]) == {(0, 24): 1}
        assert np.all(o["wet_pixels"] == 130 * 130) and o["n_days"] == 1 and o["n_bad_pixels"] == 0
    want = sn.storms_np(x, (0.5,), 8, 1, want_labels=0)
    assert np.all(want[1] == 0)
    check(x, (0.5,), 8, 1, want=want)


@pytest.mark.parametrize("conn", [4, 8])
def test_stepping_pixel_and_inverting_checkerboard(conn):
    step = sn.stepping_pixel(5, 70)
    assert check(step, (0.5,), conn, 1).result().storms.sum() == 1
    assert check(step, (0.5,), conn, 0).result().storms.sum() == 24
    across = sn.stepping_pixel(90, 130, row=63, col=52)             # columns 52 .. 75: over the tile border at 64
    across[np.arange(24), 52 + np.arange(24), 100] = 1              # and one that steps down a column, rows 52 .. 75
    assert check(across, (0.5,), conn, 1).result().storms.sum() == 2
    board = sn.inverting_checkerboard(65, 67)
    n = int(board.sum())
    zero, one = check(board, (0.5,), conn, 0).result(), check(board, (0.5,), conn, 1).result()
    assert zero.storms.sum() == (n if conn == 4 else 24) and zero.longest_duration[0, 1] == 1
    assert one.storms.tolist() == [[0, 0, 0, 1]] and one.size_sum[0, 3] == n


def test_bad_values():
    """NaN, +inf and -inf are never wet, flag their neighbours' storms as space_edge, and are counted once"""
    bar = np.zeros((1, 24, 7, 11), np.float32)
    bar[0, 5:8, 3, 2:9] = 2.0
    assert check(bar, THR3, 8, 0).result().storms[:2].tolist() == [[1, 0, 0, 0]] * 2
    for badv in (np.nan, np.inf, -np.inf):
        bar[0, 6, 3, 5] = badv
        s = check(bar, THR3, 8, 0).result()
        assert s.n_bad_pixels == 1 and s.storms[:2].tolist() == [[0, 1, 0, 0]] * 2 and s.size_sum[0, 1] == 20 and s.storms[2].sum() == 0
    bar[0, 6, 3, 5], bar[0, 9, 1, 1] = 2.0, np.nan                  # a bad pixel of another hour is no neighbour
    assert check(bar, THR3, 8, 4).result().storms[0].tolist() == [1, 0, 0, 0]
    x = rain_like(130, 67, 1, 9).copy()
    for k, (y, c) in enumerate(((63, 63), (64, 64), (63, 64), (64, 0), (0, 63), (129, 66), (65, 33), (65, 62), (128, 1))):
        x[0, (3 * k) % 24, y, c] = (np.nan, np.inf, -np.inf)[k % 3]
        x[0, (3 * k + 1) % 24, y, c] = 7.0                           # wet above every threshold in the hour after
    for conn, reach in ((8, 1), (4, 4)):
        assert check(x, THR3, conn, reach, label_t=2).result().n_bad_pixels == 9


def test_grouping_strides_passes_and_thresholds():
    x = rain_like(65, 65, 3, 77)
    xd = dev(x)
    whole = SM.StormStructure(THR3, 8, 1).add(xd)
    assert torch.equal(whole.state().cpu(), torch.from_numpy(sn.flat_state(sn.storms_np(x, THR3, 8, 1))))
    parts = SM.StormStructure(THR3, 8, 1).add(xd[:1]).add(xd[1:2]).add(xd[2:])
    assert torch.equal(parts.state(), whole.state())
    la, lb = torch.empty(x.shape, dtype=torch.int32, device="cuda"), torch.empty(x.shape, dtype=torch.int32, device="cuda")
    one = SM.StormStructure(THR3, 8, 1, days_per_pass=1).add(xd, labels_out=la, label_threshold=2)
    two = SM.StormStructure(THR3, 8, 1, days_per_pass=2).add(xd, labels_out=lb, label_threshold=2)       # 3 = 2 + 1: a short last pass
    assert torch.equal(one.state(), whole.state()) and torch.equal(two.state(), whole.state()) and torch.equal(la, lb)
    assert torch.equal(la, SM.label_storms(xd, THR3[2]))
    assert torch.equal(SM.StormStructure(THR3, 8, 1).add(xd.view(1, 3, 24, 65, 65)).state(), whole.state())
    lead = torch.empty((1, 3, 24, 65, 65), dtype=torch.int32, device="cuda")
    assert torch.equal(SM.StormStructure(THR3, 8, 1).add(xd[None], labels_out=lead, label_threshold=2).state(), whole.state())
    assert torch.equal(lead[0], la)
    wide = torch.full((3, 24 * 65 * 65 + 52), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :24 * 65 * 65].view(3, 24, 65, 65)
    view.copy_(xd)
    assert view.stride(0) == 24 * 65 * 65 + 52
    assert torch.equal(SM.StormStructure(THR3, 8, 1).add(view).state(), whole.state())
    for conn, reach in ((4, 0), (8, 4)):
        ref = SM.StormStructure(THR3, conn, reach).add(xd).state().cpu().numpy()
        for t, thr in enumerate(THR3):
            single = SM.StormStructure((thr,), conn, reach).add(xd).state().cpu().numpy()
            assert np.array_equal(single[:SM.N_COUNTS], ref[t * SM.N_COUNTS:(t + 1) * SM.N_COUNTS]) and np.array_equal(single[-2:], ref[-2:])
    # numpy in: the same
    assert torch.equal(SM.StormStructure(THR3, 8, 1).add(x).state(), whole.state())
    assert torch.equal(SM.StormStructure(THR3, 8, 1).add(xd[:1]).add(x[1:]).state(), whole.state())      # numpy onto a state that exists
    assert np.array_equal(sn.flat_state(vars(SM.storm_structure(x, THR3, 8, 1, days_per_pass=1))), whole.state().cpu().numpy())
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2])


@pytest.mark.parametrize("conn", [4, 8])
def test_with_dry_odd_hours_storms_are_cells(conn):
    x = rain_like(130, 67, 1, 5).copy()
    x[:, 1::2] = 0.0
    x[0, 4, 64, 30] = np.nan
    for reach in (0, 4):
        s = SM.StormStructure(THR3, conn, reach).add(dev(x)).result()
        c = CL.CellStructure(THR3, conn).add(dev(x)).result()
        assert np.array_equal(s.storms.sum(axis=1), c.cells.sum(axis=(1, 2))) and s.storms.sum() > 100
        assert np.array_equal(s.duration_hist.sum(axis=1)[:, 0], s.storms.sum(axis=1)) and s.duration_hist[:, :, 1:].sum() == 0
        assert np.array_equal(s.size_hist.sum(axis=1)[:, :CL.N_BINS], c.area_hist.sum(axis=1)) and s.size_hist[:, :, CL.N_BINS:].sum() == 0
        assert np.array_equal(s.wet_pixels, c.wet_pixels) and s.n_bad_pixels == c.n_bad_pixels == 1
        # the space edge is the cell's edge flag; the day cuts the cells of hour 0 off as well (hour 23 is dry)
        assert np.array_equal(s.storms[:, 1] + s.storms[:, 3], c.cells[:, 1].sum(axis=1))
        assert np.array_equal(s.storms[:, 2] + s.storms[:, 3], c.cells[:, :, 0].sum(axis=1))
        assert np.array_equal(s.volume_by_duration.sum(axis=(1, 2)), c.volume_by_area.sum(axis=(1, 2)))


def test_label_storms():
    x = rain_like(65, 65, 2, 3)
    for conn, reach in ((8, 1), (4, 0), (4, 4)):
        assert torch.equal(SM.label_storms(dev(x), 1.0, conn, reach).cpu(), torch.from_numpy(sn.labels_np(x, 1.0, conn, reach)))
    assert torch.equal(SM.label_storms(x[1], 0.1).cpu(), torch.from_numpy(sn.labels_np(x[1], 0.1)))              # numpy in, one day
    labels = torch.full(x.shape, -7, dtype=torch.int32, device="cuda")
    SM.StormStructure(THR3, 8, 1).add(dev(x), labels_out=labels, label_threshold=2)
    assert torch.equal(labels.cpu(), torch.from_numpy(sn.labels_np(x, THR3[2])))
    ss = SM.StormStructure(THR3, 8, 1)
    for bad in (torch.zeros(x.shape, dtype=torch.int64, device="cuda"), torch.zeros(x.shape, dtype=torch.float32, device="cuda"),
                torch.zeros(x.shape[1:], dtype=torch.int32, device="cuda"), torch.zeros(x.shape, dtype=torch.int32),
                torch.zeros(x.shape + (2,), dtype=torch.int32, device="cuda")[..., 0], np.zeros(x.shape, np.int32)):
        with pytest.raises(ValueError):
            ss.add(dev(x), labels_out=bad)
    with pytest.raises(ValueError):
        ss.state()                                                  # nothing was added by the refused calls


def test_past_2_31_elements():
    """1366 days of 256 x 256: 24 * 65536 * 1366 > 2^31 floats (8.6 GB), built on the device and dry but for two storms in the last
    day; the label map of the whole array is written (another 8.6 GB, never filled before) and its last day is checked, so that
    both the offsets into the input and those into the labels pass 2^31.  The state must equal the yardstick's of the last day
    plus the closed form of the dry days."""
    n, ny, nx = 1366, 256, 256
    assert n * 24 * ny * nx > 2 ** 31
    x = torch.zeros((n, 24, ny, nx), dtype=torch.float32, device="cuda")
    last = np.zeros((1, 24, ny, nx), np.float32)
    for h in range(20, 24):
        last[0, h, 60:70, 40 + h:50 + h] = 2.0                       # 100 pixels that drift over the corner of four tiles
    last[0, 22, 255, 250:256] = 1.0                                 # 6 pixels that end at the very last pixel of hour 22
    last[0, 23, 7, 9] = np.nan
    x[n - 1].copy_(dev(last[0]))
    labels = torch.empty(x.shape, dtype=torch.int32, device="cuda")
    ss = SM.StormStructure((0.5,), 8, 1).add(x, labels_out=labels)
    want, lab = sn.storms_np(last, (0.5,), 8, 1, want_labels=0)
    assert torch.equal(labels[n - 1:].cpu(), torch.from_numpy(lab)) and int(labels[n - 2].max()) == -1
    want["n_days"] += n - 1
    want["storms_per_day"][0, 0] += n - 1
    want["longest_duration"][0, 0] += n - 1
    assert torch.equal(ss.state().cpu(), torch.from_numpy(sn.flat_state(want)))
    s = ss.result()
    assert s.n_days == n and s.n_bad_pixels == 1 and s.storms.tolist() == [[0, 1, 1, 0]] and s.duration_hist[0, 2, 3] == 1
    assert s.size_sum.tolist() == [[0, 6, 400, 0]] and s.volume_by_duration[0, 2, 3] == 800 * 65536 and s.longest_duration[0, 4] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_structure_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, one NaN pixel, a dry tile; `chunk` is one unit's wet tiles on both sides, as
    tests/test_hip_cells.py pins it, so that the hourly values the two sides see are the same"""
    S, thr = 5, (0.1, 0.5, 2.0)
    rng = np.random.default_rng(31)
    daily = (rng.gamma(0.8, 6.0, (40, 52)) * (rng.random((40, 52)) < 0.7)).astype(np.float32)
    daily[:16, :16] = 0.0
    daily[20, 30] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, dd, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, dd, S, latent=z, chunk=unit_tiles)
    assert info.n_nan_pixels == 1 and hourly.shape == (S, 24, 40, 52)
    want = SM.StormStructure(thr, 8, 1).add(hourly)
    assert torch.equal(want.state().cpu(), torch.from_numpy(sn.flat_state(sn.storms_np(hourly.cpu().numpy(), thr, 8, 1))))
    ws = want.result()
    assert ws.n_bad_pixels == S * 24 and ws.n_days == S and ws.storms[0].sum() > 0
    for scenario_chunk in (1, 3, 5):
        got = SM.storm_structure_field(generator, dd if scenario_chunk == 3 else daily, S, thr, latent=z, scenario_chunk=scenario_chunk,
                                       chunk=unit_tiles)
        assert np.array_equal(sn.flat_state(vars(got)), want.state().cpu().numpy()), scenario_chunk
    got = SM.storm_structure_field(generator, dd, S, thr, latent=z, scenario_chunk=3, connectivity=4, reach=0, days_per_pass=2)
    assert got.n_days == S and got.n_bad_pixels == S * 24 and (got.connectivity, got.reach) == (4, 0)
    sn.check_identities(vars(got))
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.storm_structure_field(daily, S, thr, reach=2, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert np.array_equal(sn.flat_state(vars(a)), SM.StormStructure(thr, 8, 2).add(hourly2).state().cpu().numpy())


def test_field_on_a_dry_day_draws_nothing():
    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    s = SM.storm_structure_field(NoGenerator(), np.zeros((20, 30), np.float32), 3, (0.1,))
    assert np.array_equal(np.random.get_state()[1], before)
    assert s.n_days == 3 and s.storms_per_day[0, 0] == 3 and s.longest_duration[0, 0] == 3 and s.storms.sum() == 0


def test_c_entries_refuse_bad_arguments_and_touch_nothing():
    lib = _lib.load()
    ny, nx = 5, 7
    one = lib.rdgan_storms_workspace_bytes(ny, nx, 1)
    assert one == 24 * 35 * 24 + 8 + 24 * 8 and lib.rdgan_storms_state_count(2) == 2 * 622 + 2
    x = dev(np.full((2, 24, ny, nx), 3.0, np.float32))
    counts = torch.zeros(2 * 622 + 2, dtype=torch.int64, device="cuda")
    labels = torch.full((2, 24, ny, nx), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros(2 * one // 8, dtype=torch.int64, device="cuda")
    thr = np.array([0.1, 1.0])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)

    def acc(xp=p(x), n=2, stride=24 * 35, ny=ny, nx=nx, th=thr, T=2, conn=8, reach=1, cp=p(counts), lp=p(labels), lt=0, wp=p(ws), nbytes=2 * one):
        return lib.rdgan_storms_accumulate(xp, n, stride, ny, nx, th.ctypes.data_as(ctypes.c_void_p), T, conn, reach, cp, lp, lt, wp, nbytes,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    for kw in (dict(ny=0), dict(nx=0), dict(ny=-3), dict(ny=4096, nx=2048), dict(reach=-1), dict(reach=5), dict(conn=0), dict(conn=6), dict(lt=2),
               dict(lt=-1), dict(nbytes=one - 1), dict(nbytes=0), dict(xp=null), dict(cp=null), dict(wp=null), dict(n=0), dict(stride=24 * 35 - 1),
               dict(T=0), dict(T=9), dict(th=np.array([1.0, 0.1]))):
        assert acc(**kw) == -2, kw
    torch.cuda.synchronize()
    assert not counts.any() and torch.all(labels == -7)
    assert acc(nbytes=one) == 0                                     # a workspace for one day: two passes
    want, lab = sn.storms_np(x.cpu().numpy(), thr, 8, 1, want_labels=0)
    assert torch.equal(counts.cpu(), torch.from_numpy(sn.flat_state(want))) and torch.equal(labels.cpu(), torch.from_numpy(lab))
