"""-m gpu: the analog baseline (csrc/rdgan_analog.hip.h, pr_disagg_radar_gan_amd/analog.py) against the numpy restatement
(tests/analog_np.py, itself checked on the CPU by tests/test_analog_host.py).  The search and the picks are integers: compared for
equality.  The apply step is fp32: compared with the fp64 restatement to bounds derived from its roundings."""
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import analog as AN
from pr_disagg_radar_gan_amd.data_pipeline import DeviceDataset
from pr_disagg_radar_gan_amd.ensemble import crps_ensemble_device
from tests import analog_np as an
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                                               # the unit roundoff of fp32
ONE_SLICE = lambda Q, k: Q * AN.WAVES * k * 8                                # bytes of the lists of one slice


@functools.lru_cache(maxsize=None)
def rain_like(ny, nx, days, seed):
    """(days, 24, ny, nx): gamma amounts where a smoothed noise field is above its 70 % quantile, some values at quantisation ties.
    Shared: copy before writing."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(days, 24, ny, nx))
    for _ in range(2):
        g = (g + np.roll(g, 1, 1) + np.roll(g, 1, 2) + np.roll(g, -1, 2) + np.roll(g, 1, 3) + np.roll(g, -1, 3)) / 6
    x = ((0.2 + rng.gamma(0.6, 3.0, g.shape)) * (g > np.quantile(g, 0.7))).astype(np.float32)
    ties = rng.random(g.shape) < 0.05
    x[ties] = ((rng.integers(0, 8192, g.shape) + 0.5) / 1024).astype(np.float32)[ties]
    return x


def conditions(lib, Q, seed):
    """Q daily sums: library days scaled and perturbed, so that the nearest days are neither obvious nor all alike"""
    rng = np.random.default_rng(seed)
    base = lib[rng.integers(0, lib.shape[0], Q)].sum(axis=1)
    return (base * rng.uniform(0.5, 1.5, (Q, 1, 1)) + rng.gamma(0.5, 1.0, base.shape) * (rng.random(base.shape) < 0.3)).astype(np.float32)


def check(lib, cond, k, groups=None, qgroups=None, workspace_bytes=None, hourly=None, n_members=3, seed=11, weights="rank"):
    """search and picks of the device against the yardstick -> (library, neighbours, found), the latter two numpy"""
    library = AN.AnalogLibrary(dev(lib) if hourly is None else hourly, groups=groups)
    nb, dist, found = library.search(dev(cond), k=k, query_groups=qgroups, workspace_bytes=workspace_bytes)
    want = an.search(lib, cond, k, groups, qgroups)
    assert np.array_equal(nb.cpu().numpy(), want[0]) and nb.dtype == torch.int32
    assert np.array_equal(dist.cpu().numpy(), want[1]) and dist.dtype == torch.int64
    assert np.array_equal(found.cpu().numpy(), want[2]) and found.dtype == torch.int32
    _, void, total = an.library_features(lib)
    assert library.n_void == int(void.sum()) and np.array_equal(library.void.cpu().numpy(), void.astype(np.uint8))
    assert np.array_equal(library.totals.cpu().numpy()[~void], total[~void])
    _, picks = library.generate(dev(cond), n_members, k=k, seed=seed, weights=weights, query_groups=qgroups, return_picks=True)
    assert np.array_equal(picks.cpu().numpy(), an.picks(want[0], want[2], n_members, seed, weights)) and picks.dtype == torch.int32
    return library, want[0], want[2]


# the plane: neither a multiple of 4 nor of a wave; the training tile; the LDS maximum.  N: three blocks of 64 days; one day more
# than a block; less than a block.  Q: one more than the query tile.
SHAPES = {"3x5": (3, 5, 150, 17, 5), "16x16": (16, 16, 65, 17, 10), "64x64": (64, 64, 40, 9, 32)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_fields_against_restatement(name):
    ny, nx, N, Q, k = SHAPES[name]
    assert Q == AN.query_tile(ny * nx) + 1
    lib = rain_like(ny, nx, N, len(name)).copy()
    lib[N // 2] = 2047.5                                                                   # the largest feature everywhere: sums beyond 2^32
    cond = conditions(lib, Q, 3)
    cond[0] = 0.0
    cond[1] = 49151.0
    check(lib, cond, k)
    check(lib, cond, k, workspace_bytes=ONE_SLICE(Q, k), weights="uniform")               # one slice
    check(lib, cond, k, workspace_bytes=64 * ONE_SLICE(Q, k), seed=2 ** 40 + 5)           # a slice per block


def test_a_single_library_day_and_a_single_query():
    lib = rain_like(3, 5, 1, 1)
    check(lib, conditions(lib, 1, 0), 1)
    check(lib, conditions(lib, 4, 1), 32)                                                 # k above the library: -1 fill
    lib = rain_like(16, 16, 65, 5)
    check(lib, conditions(lib, 1, 2), 32)                                                 # Q = 1, k = 32


def test_slices_through_a_small_workspace():
    Q, k = 3, 4
    lib = rain_like(16, 16, 150, 7).copy()
    lib[64] = lib[3]                                                                      # a tie across two slices
    cond = conditions(lib, Q, 4)
    cond[0] = lib[3].sum(axis=0)
    for N, slices in ((65, 2), (129, 2), (150, 3), (150, 2), (150, 1)):                   # one day more than a slice; three slices; uneven slices
        check(lib[:N], cond, k, workspace_bytes=slices * ONE_SLICE(Q, k))
    check(lib, cond, k, workspace_bytes=3 * ONE_SLICE(Q, k) + 8)                          # a workspace that is no multiple of a slice
    _, nb, _ = check(lib, cond, 2, workspace_bytes=3 * ONE_SLICE(Q, 2))
    assert nb[0].tolist() == [3, 64]


def test_duplicates_voids_and_k_above_the_admissible_days():
    lib = rain_like(3, 5, 70, 9).copy()
    lib[[10, 20, 69]] = lib[5]                                                            # equal days: ties go to the smaller index
    lib[1, 4, 1, 2] = np.nan
    lib[2, 0, 0, 0] = -0.5
    lib[3, 23, 2, 4] = 2048.0
    lib[4] = 0.0
    lib[65, 7, 0, 1] = np.inf
    cond = conditions(lib, 5, 6)
    cond[0] = lib[5].sum(axis=0)
    library, nb, found = check(lib, cond, 4)
    assert nb[0].tolist() == [5, 10, 20, 69] and library.n_void == 5
    # 13 admissible days under k = 32
    few = lib[:17]
    _, nb, found = check(few, cond, 32)
    assert np.all(found == 13) and np.all(nb[:, 13:] == -1) and np.all(nb[:, :13] >= 0)
    # a library of void days only
    _, nb, found = check(lib[1:5], cond, 3)
    assert np.all(found == 0) and np.all(nb == -1)


def test_group_exclusion():
    lib = rain_like(16, 16, 70, 12)
    groups = (np.arange(70) // 7).astype(np.int32)                                        # ten "days" of seven tiles
    groups[63:] = -1
    cond = lib[[0, 8, 20, 66, 69]].sum(axis=1)
    qgroups = np.array([0, 1, -1, -1, 3], np.int32)
    _, nb, found = check(lib, cond, 6, groups, qgroups)
    assert not np.isin(nb[0], range(0, 7)).any() and not np.isin(nb[1], range(7, 14)).any()
    assert nb[2, 0] == 20 and nb[3, 0] == 66                                              # -1 is no group: nothing is skipped
    assert found.tolist() == [6] * 5
    # a query whose every candidate is excluded, beside one that keeps them all
    _, nb, found = check(lib[:7], cond[:2], 3, groups[:7], qgroups[:2])
    assert found.tolist() == [0, 3] and np.all(nb[0] == -1)
    # query groups without library groups are refused; library groups alone exclude nothing
    library = AN.AnalogLibrary(dev(lib), groups=groups)
    assert np.array_equal(library.search(dev(cond), k=6)[0].cpu().numpy(), an.search(lib, cond, 6)[0])
    # groups as int64 CUDA tensors
    nb = library.search(dev(cond), k=6, query_groups=torch.from_numpy(qgroups).long().cuda())[0]
    assert np.array_equal(nb.cpu().numpy(), an.search(lib, cond, 6, groups, qgroups)[0])


def test_masked_query_pixels():
    lib = rain_like(3, 5, 70, 15)
    cond = conditions(lib, 4, 8)
    cond[0, 0, 0], cond[0, 2, 4], cond[1, 1, 1], cond[2, 1, 3] = np.nan, -1.0, np.inf, 49152.0
    cond[3] = np.nan                                                                      # every pixel masked: distance 0 to every day
    _, nb, _ = check(lib, cond, 5)
    assert nb[3].tolist() == [0, 1, 2, 3, 4]
    lib = rain_like(64, 64, 40, 16)
    cond = conditions(lib, 2, 9)
    cond[0, ::3, 1::2] = np.nan
    check(lib, cond, 7)


@pytest.mark.parametrize("pad", (8, 3))                                                  # 16-byte loads; the scalar path on a plane that would allow them
def test_a_strided_library_view(pad):
    lib = rain_like(16, 16, 66, 18)
    wide = torch.full((66, 24 * 256 + pad), float("nan"), device="cuda")
    wide[:, :24 * 256] = dev(lib).reshape(66, -1)
    view = wide[:, :24 * 256].unflatten(1, (24, 16, 16))
    assert view.stride(0) == 24 * 256 + pad and view.data_ptr() == wide.data_ptr()
    cond = conditions(lib, 3, 10)
    library, nb, found = check(lib, cond, 4, hourly=view)
    out = library.generate(dev(cond), 2, k=4, seed=3)
    assert torch.equal(out, AN.AnalogLibrary(dev(lib)).generate(dev(cond), 2, k=4, seed=3))


def test_numpy_inputs_are_uploaded():
    lib = rain_like(3, 5, 70, 15)
    cond = conditions(lib, 4, 8)
    library = AN.AnalogLibrary(lib)
    nb, dist, found = library.search(cond, k=3)
    want = an.search(lib, cond, 3)
    assert nb.is_cuda and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((nb, dist, found), want))


def test_results_do_not_depend_on_the_split():
    lib = rain_like(16, 16, 150, 7)
    cond = conditions(lib, 20, 11)
    library = AN.AnalogLibrary(dev(lib))
    c = dev(cond)
    a = library.search(c, k=9)
    b = library.search(c, k=9, workspace_bytes=ONE_SLICE(20, 9))
    halves = [library.search(c[:7], k=9), library.search(c[7:], k=9, workspace_bytes=2 * ONE_SLICE(13, 9))]
    for x, y, h0, h1 in zip(a, b, *halves):
        assert torch.equal(x, y) and torch.equal(x, torch.cat([h0, h1]))
    bits = lambda t: t.view(torch.int32)
    whole, picks = library.generate(c, 5, k=9, seed=77, return_picks=True)
    first, p0 = library.generate(c, 2, k=9, seed=77, return_picks=True)
    rest, p1 = library.generate(c, 3, k=9, seed=77, first_member=2, return_picks=True)
    assert torch.equal(bits(whole), bits(torch.cat([first, rest], dim=1))) and torch.equal(picks, torch.cat([p0, p1], dim=1))
    tail, p2 = library.generate(c[7:], 5, k=9, seed=77, first_query=7, return_picks=True)
    assert torch.equal(bits(whole[7:]), bits(tail)) and torch.equal(picks[7:], p2)
    assert not torch.equal(picks, library.generate(c, 5, k=9, seed=78, return_picks=True)[1])


def check_apply(lib, cond, library=None, n_members=4, k=5, **kw):
    """generate against the fp64 restatement, to the bounds of the definition -> (out, picks, profile path) as numpy"""
    library = library or AN.AnalogLibrary(dev(lib))
    out, picks = library.generate(dev(cond), n_members, k=k, return_picks=True, **kw)
    out, picks = out.cpu().numpy().astype(np.float64), picks.cpu().numpy()
    want, dry = an.apply(lib, cond, picks)
    P = lib.shape[-2] * lib.shape[-1]
    assert np.array_equal(np.isnan(out), np.isnan(want))                                 # NaN exactly where the definition says
    err = np.abs(np.nan_to_num(out) - np.nan_to_num(want))
    mag = np.abs(np.nan_to_num(want))
    dry_h = np.broadcast_to(dry[:, :, None], out.shape)
    # the pixel path: the 23 additions of the donor's sum, a division, a product; the profile path: a sum of non-negative terms
    assert np.all(err[~dry_h] <= 26 * U * mag[~dry_h]), (err[~dry_h] / np.maximum(mag[~dry_h], 1e-300)).max() / U
    assert np.all(err[dry_h] <= 24 * P * U * mag[dry_h]), (err[dry_h] / np.maximum(mag[dry_h], 1e-300)).max() / U
    # the 24 hours sum to the condition
    total = out.sum(axis=2)
    c = np.broadcast_to(cond.astype(np.float64)[:, None], total.shape)
    ok = ~np.isnan(total)
    assert np.all(np.abs(total[ok] - c[ok]) <= 26 * U * c[ok])
    return out, picks, dry


@pytest.mark.parametrize("name", ("3x5", "16x16", "64x64"))
def test_apply_against_fp64(name):
    ny, nx, N, Q, k = SHAPES[name]
    lib = rain_like(ny, nx, N, len(name)).copy()
    lib[:, :, :, : nx // 2] *= (np.arange(N) % 3 != 0)[:, None, None, None]              # donors with a dry half
    lib[1, 4, 0, 0] = np.nan                                                              # a void day is no donor
    cond = conditions(lib, Q, 5) + np.float32(0.25)                                       # wet everywhere: the profile path runs
    cond[0, 0, 0], cond[1, ny - 1, nx - 1], cond[2, 1, 1] = np.nan, -2.0, 49152.0
    cond[3, 0, 1] = 0.0
    out, picks, dry = check_apply(lib, cond, k=min(k, 6), seed=21)
    assert dry.any() and not dry.all() and not np.isin(picks, 1).any()
    assert np.isnan(out[0, :, :, 0, 0]).all() and np.isnan(out[1, :, :, -1, -1]).all() and np.isnan(out[2, :, :, 1, 1]).all()
    assert np.all(out[3, :, :, 0, 1] == 0.0)


def test_apply_without_a_neighbour_is_nan_throughout():
    lib = rain_like(3, 5, 70, 9).copy()
    groups = np.zeros(70, np.int32)
    library = AN.AnalogLibrary(dev(lib), groups=groups)
    cond = conditions(lib, 2, 1)
    out, picks, _ = check_apply(lib, cond, library=library, query_groups=np.array([0, -1], np.int32), seed=4)
    assert np.isnan(out[0]).all() and np.all(picks[0] == -1) and not np.isnan(out[1]).any()


def test_leave_one_out_returns_the_day_itself_unless_grouped():
    # amounts in whole 1/1024 mm below 8 mm: the 24-hour sums are exact in fp32, so the condition is the donor's own sum
    lib = np.rint(np.minimum(rain_like(16, 16, 66, 18), 7.0) * 1024).astype(np.float32) / 1024
    real = dev(lib[:12])
    library = AN.AnalogLibrary(dev(lib))
    out = AN.generate_one_per_day(real, library, k=1)
    assert out.shape == (12, 24, 16, 16)
    got, want = out.cpu().numpy().astype(np.float64), lib[:12].astype(np.float64)
    d = np.broadcast_to(want.sum(axis=1, keepdims=True), want.shape)
    wet = d > 0                                                                           # (a dry pixel of a dry condition: 0 either way)
    assert np.all(np.abs(got - want)[wet] <= 26 * U * want[wet]) and np.all(got[~wet] == 0)
    assert np.array_equal(library.generate(real.sum(1), 1, k=1, return_picks=True)[1].cpu().numpy()[:, 0], np.arange(12))
    days = np.arange(66, dtype=np.int32)
    grouped = AN.AnalogLibrary(dev(lib), groups=days)
    _, picks = grouped.generate(real.sum(1), 1, k=1, query_groups=days[:12], return_picks=True)
    assert not np.any(picks.cpu().numpy()[:, 0] == np.arange(12))
    other = AN.generate_one_per_day(real, grouped, k=1, query_groups=days[:12])
    assert not torch.equal(other, out)
    assert torch.equal(AN.generate_one_per_day(lib[:12], library, k=1), out)             # numpy days


def test_crps_for_days_is_the_crps_of_generate():
    lib = rain_like(16, 16, 66, 18)
    real = dev(lib[60:63])
    groups = np.arange(66, dtype=np.int32)
    library = AN.AnalogLibrary(dev(lib), groups=groups)
    got = AN.crps_for_days(real, library, n_members=20, k=6, seed=9, weights="uniform", query_groups=groups[60:63])
    ens = library.generate(real.sum(1), 20, k=6, seed=9, weights="uniform", query_groups=groups[60:63])
    want = torch.stack([crps_ensemble_device(ens[i], real[i]) for i in range(3)]).mean(dim=(2, 3)).cpu().numpy()
    assert got.shape == (3, 24) and np.array_equal(got, want) and np.all(got >= 0) and np.any(got > 0)


def test_library_from_a_dataset():
    data = rain_like(40, 48, 4, 20)
    idx = np.array([(t, y, x) for t in range(4) for y in (0, 8, 24) for x in (0, 16, 32)], np.int32)
    ds = DeviceDataset(data, idx, ndomain=16)
    library = AN.AnalogLibrary.from_dataset(ds)
    tiles = np.stack([data[t, :, y:y + 16, x:x + 16] for t, y, x in idx])
    assert library.n == len(idx) and np.array_equal(library.hourly.cpu().numpy(), tiles)
    assert np.array_equal(library.groups.cpu().numpy(), idx[:, 0])
    cond = tiles[[2, 20]].sum(axis=1)
    nb = library.search(dev(cond), k=3, query_groups=np.array([0, 2], np.int32))[0].cpu().numpy()
    assert np.array_equal(nb, an.search(tiles, cond, 3, idx[:, 0], np.array([0, 2]))[0]) and not np.isin(idx[nb[0], 0], 0).any()
    np.random.seed(3)
    drawn = AN.AnalogLibrary.from_dataset(ds, n=7)
    np.random.seed(3)
    ixs = np.random.randint(len(idx), size=7)
    assert np.array_equal(drawn.hourly.cpu().numpy(), tiles[ixs]) and np.array_equal(drawn.groups.cpu().numpy(), idx[ixs, 0])
