"""-m gpu: rain cells of hourly fields (csrc/rdgan_cells.hip.h, pr_disagg_radar_gan_amd/cells.py) against the numpy restatement
(tests/cells_np.py, itself checked on the CPU by tests/test_cells_host.py).  Everything is an integer: label maps are compared with
torch.equal, states int64 against int64."""
import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import cells as CL, field as F, models, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import cells_np as cn
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

SHAPES = {"5x7": (5, 7), "64x64": (64, 64), "65x65": (65, 65), "130x70": (130, 70), "256x256": (256, 256)}
THR3 = (0.1, 1.0, 5.0)


def check(x, thresholds, conn, label_t=0, xd=None, **kw):
    """state and labels of one add() of x against the yardstick -> the CellStructure"""
    want, lab = cn.cells_np(x, thresholds, conn, want_labels=label_t)
    xd = dev(x) if xd is None else xd
    labels = torch.full(x.shape, -7, dtype=torch.int32, device="cuda")
    cs = CL.CellStructure(thresholds, conn, **kw).add(xd, labels_out=labels, label_threshold=label_t)
    assert torch.equal(labels.cpu(), torch.from_numpy(lab))
    assert torch.equal(cs.state().cpu(), torch.from_numpy(cn.flat_state(want)))
    cn.check_identities(CL.split_state(cs.state().cpu().numpy(), len(thresholds)))
    return cs


def random_days(shape, seed, hours=(0, 7, 12, 23)):
    """(2, 24, ny, nx): gamma amounts at wet fractions 0.05, 0.41, 0.59 (the percolation thresholds of the two connectivities,
    where cells are large and tortuous) and 0.9 in four hours of each day, the other hours dry; NaN and inf pixels on and beside
    the tile borders, a value exactly at a threshold"""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    x = np.zeros((2, 24, ny, nx), np.float32)
    for d in range(2):
        for h, p in zip(hours, (0.05, 0.41, 0.59, 0.9)):
            x[d, h] = (0.2 + rng.gamma(0.6, 3.0, shape)) * (rng.random(shape) < p)
    for k, (y, c) in enumerate(((63, 63), (64, 64), (63, 64), (64, 0), (0, 63), (ny - 1, nx - 1), (ny // 2, nx // 2), (65, 62))):
        if y < ny and c < nx:
            x[k % 2, hours[1 + k % 3], y, c] = (np.nan, np.inf, -np.inf)[k % 3]
    x[0, hours[2], ny // 3, nx // 3] = np.float32(1.0)
    return x


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_random_fields_against_restatement(name, conn):
    x = random_days(SHAPES[name], len(name) + conn)
    check(x, (1.0,) if name == "256x256" else THR3, conn, label_t=0 if name == "256x256" else 1)


@pytest.mark.parametrize("conn", [4, 8])
def test_long_merge_chains(conn):
    """a spiral and a serpentine over the whole 130 x 70 plane (3 x 2 ragged tiles): one cell each, through every tile many
    times; the same on 65 x 65, where the second tile row and column are one pixel wide"""
    for ny, nx in ((130, 70), (65, 65)):
        x = np.zeros((2, 24, ny, nx), np.float32)
        x[0, 3], x[0, 4], x[1, 23] = cn.spiral(ny, nx), 2 * cn.serpentine(ny, nx), cn.spiral(nx, ny).T
        x[1, 0] = cn.serpentine(nx, ny).T * 3
        cs = check(x, (0.5,), conn)
        s = cs.result()
        assert s.cells.sum() == 4 and s.cells_per_plane[0, 1] == 4 and s.dry_planes[0] == 44


@pytest.mark.parametrize("conn", [4, 8])
def test_u_shape_corner_diagonal_and_planes_do_not_link(conn):
    ny, nx = 130, 70
    x = np.zeros((2, 24, ny, nx), np.float32)
    # a U whose arms lie in the tile (0, 0) and whose bottom lies in the tile below: two local components there become one
    x[0, 0, 10:70, 20], x[0, 0, 10:70, 40], x[0, 0, 69, 20:41] = 1.0, 1.0, 1.0
    # two pixels that touch only diagonally across the corner where four tiles meet, both ways
    x[0, 1, 63, 63], x[0, 1, 64, 64] = 1.0, 1.0
    x[0, 2, 63, 64], x[0, 2, 64, 63] = 1.0, 1.0
    # diagonal pairs across one border only
    x[0, 5, 63, 10], x[0, 5, 64, 11], x[0, 5, 20, 63], x[0, 5, 19, 64] = 1.0, 1.0, 1.0, 1.0
    # the wet last row of a plane above the wet first row of the next plane, and of the next day
    x[0, 9, ny - 1], x[0, 10, 0], x[0, 23, ny - 1], x[1, 0, 0] = 1.0, 1.0, 1.0, 1.0
    s = check(x, (0.5,), conn).result()
    two = 1 if conn == 8 else 2
    assert s.cell_count_by_hour()[0, :3].tolist() == [2, two, two]          # (hour 0: the U, and the first row of day 1)
    assert s.cell_count_by_hour()[0, :3].sum() == 2 + 2 * two and s.cell_count_by_hour()[0, 5] == 2 * two
    assert s.cell_count_by_hour()[0, [9, 10, 23]].tolist() == [1, 1, 1] and s.area_hist[0, 1, 6] == 4


@pytest.mark.parametrize("name", ["5x7", "65x65", "130x70"])
def test_checkerboard_all_wet_all_dry_and_threshold(name):
    ny, nx = SHAPES[name]
    x = np.zeros((2, 24, ny, nx), np.float32)
    x[0, 0], x[0, 1], x[1, 2] = cn.checkerboard(ny, nx), 1.0, 1.0 - cn.checkerboard(ny, nx)
    x[1, 3] = np.float32(0.5)                                       # a whole plane exactly at the threshold: dry
    x[1, 4] = np.nextafter(np.float32(0.5), np.float32(1.0))
    x[1, 5] = 3.0e9                                                 # above the 2^20 at which a pixel's volume saturates
    s4 = check(x, (0.5,), 4).result()
    s8 = check(x, (0.5,), 8).result()
    n0, n1 = (ny * nx + 1) // 2, ny * nx // 2
    assert s4.cells.sum() == n0 + n1 + 3 and s8.cells.sum() == 5 and s4.dry_planes[0] == s8.dry_planes[0] == 43
    assert s4.cells_per_plane[0, min(n0, 64)] >= 1 and s4.area_hist[0, :, 0].sum() == n0 + n1
    assert s8.volume_by_area[0].sum() == (n0 + n1 + ny * nx) * 65536 + ny * nx * (int(cn.quantum(x[1, 4, :1, 0])[0]) + 2 ** 36)


def test_grouping_strides_passes_and_thresholds():
    x = random_days((130, 70), 77)
    x = np.concatenate([x, random_days((130, 70), 78)[:1]])        # 3 days
    xd = dev(x)
    whole = CL.CellStructure(THR3, 8).add(xd)
    assert torch.equal(whole.state().cpu(), torch.from_numpy(cn.flat_state(cn.cells_np(x, THR3, 8))))
    parts = CL.CellStructure(THR3, 8).add(xd[:1]).add(xd[1:])
    assert torch.equal(parts.state(), whole.state())
    wide = torch.full((3, 24 * 130 * 70 + 52), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :24 * 130 * 70].view(3, 24, 130, 70)
    view.copy_(xd)
    assert view.stride(0) == 24 * 130 * 70 + 52
    assert torch.equal(CL.CellStructure(THR3, 8).add(view).state(), whole.state())
    la, lb = torch.empty(x.shape, dtype=torch.int32, device="cuda"), torch.empty(x.shape, dtype=torch.int32, device="cuda")
    one = CL.CellStructure(THR3, 8, planes_per_pass=1).add(xd, labels_out=la, label_threshold=2)
    five = CL.CellStructure(THR3, 8, planes_per_pass=5).add(xd, labels_out=lb, label_threshold=2)       # 72 = 14 x 5 + 2: a short last pass
    assert torch.equal(one.state(), whole.state()) and torch.equal(five.state(), whole.state()) and torch.equal(la, lb)
    assert torch.equal(la, CL.label_cells(xd, THR3[2]))
    for conn in (4, 8):
        ref = CL.CellStructure(THR3, conn).add(xd).state().cpu().numpy()
        for t, thr in enumerate(THR3):
            single = CL.CellStructure((thr,), conn).add(xd).state().cpu().numpy()
            assert np.array_equal(single[:CL.N_COUNTS], ref[t * CL.N_COUNTS:(t + 1) * CL.N_COUNTS]) and np.array_equal(single[-2:], ref[-2:])
    # numpy in: the same
    assert torch.equal(CL.CellStructure(THR3, 8).add(x).state(), whole.state())
    assert torch.equal(CL.CellStructure(THR3, 8).add(xd[:1]).add(x[1:]).state(), whole.state())       # numpy onto a state that exists
    with pytest.raises(ValueError):
        whole.add(xd[..., ::2])
    assert torch.equal(CL.label_cells(x[0], 1.0, 4).cpu(), torch.from_numpy(cn.labels_np(x[0], 1.0, 4)))


def test_past_2_31_elements():
    """1366 days of 256 x 256: 24 * 65536 * 1366 > 2^31 floats (8.6 GB), built on the device and dry but for a few cells in the
    last planes; only the last planes' labels and the state are checked.  The state of the whole array must equal the yardstick's
    of the last day plus the closed form of the dry planes; the labels are taken from a view of the last day inside the large
    array, so the label map of the whole array (another 8.6 GB) is not needed."""
    n, ny, nx = 1366, 256, 256
    assert n * 24 * ny * nx > 2 ** 31
    x = torch.zeros((n, 24, ny, nx), dtype=torch.float32, device="cuda")
    last = np.zeros((1, 24, ny, nx), np.float32)
    last[0, 22, 60:70, 60:70] = 2.0                                 # 100 pixels over the corner of four tiles, interior
    last[0, 23, 255, 250:256] = 1.0                                 # 6 pixels that end at the very last pixel
    last[0, 23, 100, 100] = 4.0
    last[0, 23, 7, 9] = np.nan
    x[n - 1].copy_(dev(last[0]))
    cs = CL.CellStructure((0.5,), 8).add(x)
    s = cs.result()
    want = cn.cells_np(last, (0.5,), 8)
    extra = (n - 1) * 24
    want["n_planes"] += extra
    want["cells_per_plane"][0, 0] += extra
    want["dry_planes"][0] += extra
    assert torch.equal(cs.state().cpu(), torch.from_numpy(cn.flat_state(want)))
    assert s.n_planes == n * 24 and s.n_bad_pixels == 1 and s.cells[0, 0, 22] == 1 and s.cells[0, :, 23].tolist() == [1, 1]
    assert s.area_hist[0, 0, 6] == 1 and s.area_hist[0, 1, 2] == 1 and s.volume_by_area[0, 0, 6] == 200 * 65536
    lab = CL.label_cells(x[n - 1:], 0.5)
    assert torch.equal(lab.cpu(), torch.from_numpy(cn.labels_np(last, 0.5, 8)))


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_structure_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, one NaN pixel, a dry tile; `chunk` is one unit's wet tiles on both sides, as
    tests/test_hip_temporal.py pins it, so that the hourly values the two sides see are the same"""
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
    want = CL.CellStructure(thr, 8).add(hourly)
    assert torch.equal(want.state().cpu(), torch.from_numpy(cn.flat_state(cn.cells_np(hourly.cpu().numpy(), thr, 8))))
    ws = want.result()
    assert ws.n_bad_pixels == S * 24 and ws.cells[0].sum() > 0
    for scenario_chunk in (1, 3, 5):
        got = CL.cell_structure_field(generator, dd if scenario_chunk == 3 else daily, S, thr, latent=z, scenario_chunk=scenario_chunk,
                                      chunk=unit_tiles)
        assert np.array_equal(cn.flat_state(vars(got)), want.state().cpu().numpy()), scenario_chunk
    # the default chunk: the generator's batches, and with them the last bits of the hourly values, differ with scenario_chunk
    for scenario_chunk in (1, 3):
        got = CL.cell_structure_field(generator, dd, S, thr, latent=z, scenario_chunk=scenario_chunk, connectivity=4)
        assert got.n_planes == S * 24 and got.n_bad_pixels == S * 24 and got.connectivity == 4
        cn.check_identities(vars(got))
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.cell_structure_field(daily, S, thr, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert np.array_equal(cn.flat_state(vars(a)), CL.CellStructure(thr, 8).add(hourly2).state().cpu().numpy())


def test_field_on_a_dry_day_draws_nothing():
    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    s = CL.cell_structure_field(NoGenerator(), np.zeros((20, 30), np.float32), 3, (0.1,))
    assert np.array_equal(np.random.get_state()[1], before)
    assert s.n_planes == 72 and s.dry_planes[0] == 72 and s.cells.sum() == 0 and np.all(s.wet_fraction_by_hour() == 0)
