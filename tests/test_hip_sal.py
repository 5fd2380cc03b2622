"""-m gpu: the SAL records of hourly fields (csrc/rdgan_sal.hip.h, pr_disagg_radar_gan_amd/sal.py) against the numpy restatement
(tests/sal_np.py, itself checked on the CPU by tests/test_sal_host.py).  The integer records are compared int64 against int64; V and r
within the bound derived at check(); every record bitwise across groupings."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import cells as CL, field as F, models, sal as SL, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import cells_np as cn, sal_np as sn
from tests.hip_util import dev, lib, ptr, stream

pytestmark = pytest.mark.gpu

SHAPES = {"64x64": (64, 64), "70x130": (70, 130), "129x65": (129, 65), "1x200": (1, 200), "1x1": (1, 1)}
THR3 = (0.1, 1.0, 5.0)
EPS = 2.0 ** -52


def ramp(ny, nx):
    """1 .. 2.5 mm, rising along both axes at different rates, in multiples of 1/1024 mm: the moments of a figure are not symmetric"""
    yy, xx = np.indices((ny, nx))
    return (1.0 + np.floor(1024.0 * (yy / max(ny, 1) + 0.5 * xx / max(nx, 1))) / 1024.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def days(name):
    """(2, 24, ny, nx): day 0 holds the figures scaled by the ramp (a spiral, a serpentine, a checkerboard -- at 4-connectivity
    ny nx / 2 objects), an all-wet and an all-dry plane, an object over the corner where four tiles meet, pixels at and above the
    clamp, negative values; day 1 random blobs of 0 .. 60 mm/h with NaN and inf pixels on and beside the tile borders"""
    ny, nx = SHAPES[name]
    rng = np.random.default_rng(ny * 1000 + nx)
    x = np.zeros((2, 24, ny, nx), np.float32)
    r = ramp(ny, nx)
    x[0, 0], x[0, 1], x[0, 2] = cn.spiral(ny, nx) * r, cn.serpentine(ny, nx) * r, cn.checkerboard(ny, nx) * r
    x[0, 3] = 6.0 * r                                               # all wet at every threshold; hour 4 stays all dry
    x[0, 5, max(0, min(60, ny - 1)):70, max(0, min(60, nx - 1)):70] = 7.25       # over (63|64, 63|64) where the plane has that corner
    x[0, 6] = -2.0 * cn.checkerboard(ny, nx)                        # negative: valid, dry, mass 0
    x[0, 6, ny // 2, nx // 2] = 3.0
    c = x[0, 7]
    c.flat[0], c.flat[-1], c.flat[c.size // 2] = np.float32(2048.0) - np.float32(1 / 1024), 2048.0, 3.0e9        # at the clamp, above, far above
    c.flat[c.size // 3] = -np.float32(3.0e9)
    for h in range(8, 24):
        x[0, h] = ((rng.random((ny, nx)) < 0.02 * (h - 7)) * r * (h - 6) / 4).astype(np.float32)      # speckle, ever denser
    for h in range(24):                                             # blobs: a smooth field cut at its upper part, amounts 0 .. 60
        f = rng.random((ny + 8, nx + 8))
        f = sum(np.roll(np.roll(f, dy, 0), dx, 1) for dy in range(-2, 3) for dx in range(-2, 3))[4:-4, 4:-4] / 25
        x[1, h] = np.where(f > np.quantile(f, 0.5 + 0.02 * h), 60.0 * rng.random((ny, nx)), 0.0).astype(np.float32)
    for k, (y, c) in enumerate(((63, 63), (64, 64), (63, 64), (64, 0), (0, 63), (ny - 1, nx - 1), (ny // 2, nx // 2), (0, 0))):
        if y < ny and c < nx and ny * nx > 1:
            x[1, 3 * k % 24, y, c] = (np.nan, np.inf, -np.inf)[k % 3]
    return x


@functools.lru_cache(maxsize=None)
def reference(name, conn):
    return sn.records_np(days(name), THR3, conn)


def same_records(a, b):
    """bitwise: the doubles compared as their 64 bits"""
    return (torch.equal(a.plane, b.plane) and torch.equal(a.objects, b.objects)
            and torch.equal(a.vr.view(torch.int64), b.vr.view(torch.int64)))


def check(got, want):
    """The integers equal; V and r within a relative (n_objects + 16) 2^-52 of the yardstick.  Derivation: each is a sum of
    n = n_objects non-negative terms divided by R.  The terms being non-negative, any order of summation -- the yardstick adds them
    one after the other in ascending label, the kernel in a fixed tree -- stays within (n - 1) 2^-53 relative of the exact sum of
    the computed terms, so two orders differ by at most (n - 1) 2^-52.  A term is a division (or two, and two subtractions, for r),
    a hypot, a product; the sum is divided once: on both sides the same IEEE operations on the same integers, so the terms differ
    only through hypot (a few ulp in either library), which with the final quotient the slack of 16 ulp covers.  A value the
    definition makes 0 (no object, or no mass) must be exactly 0."""
    g = got.cpu()
    assert np.array_equal(g.plane, want["plane"])
    assert np.array_equal(g.objects, want["objects"])
    n = want["objects"][..., 0].astype(np.float64)[..., None]
    err = np.abs(g.vr - want["vr"])
    worst = float(np.max(np.where(want["vr"] > 0, err / np.where(want["vr"] > 0, want["vr"], 1.0) / ((n + 16) * EPS), 0.0)))
    print(f"V, r: worst error {worst:.3f} of the bound, largest plane {int(n.max())} objects")
    assert np.all(err <= (n + 16) * EPS * want["vr"])
    assert np.all(g.vr[want["vr"] == 0] == 0)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_records_against_restatement(name, conn):
    x = days(name)
    want = reference(name, conn)
    if name in ("70x130", "129x65") and conn == 4:
        assert want["objects"][0, 2, 0, 0] >= 1000                  # the checkerboard: the sum order matters there
    got = SL.plane_records(dev(x), THR3, conn)
    assert got.plane.shape == (2, 24, 4) and got.objects.shape == (2, 24, 3, 3) and got.vr.shape == (2, 24, 3, 2)
    check(got, want)
    assert got.n_objects[0, 4].sum() == 0 and got.M0[0, 4] == 0 and got.n_wet[0, 3, 0] == x.shape[-1] * x.shape[-2]
    assert int(got.n_bad.sum()) == int((~np.isfinite(x)).sum())


@pytest.mark.parametrize("name", ["70x130", "1x200"])
def test_every_record_bitwise_across_groupings(name):
    x = days(name)
    ny, nx = SHAPES[name]
    xd = dev(x)
    whole = SL.plane_records(xd, THR3, 8)
    check(whole, reference(name, 8))
    for ppp in (1, 5, 48):                                          # 48 = 9 x 5 + 3: a short last pass
        assert same_records(SL.plane_records(xd, THR3, 8, planes_per_pass=ppp), whole), ppp
    a, b = SL.plane_records(xd[:1], THR3, 8), SL.plane_records(xd[1:], THR3, 8)
    for k in ("plane", "objects", "vr"):
        assert torch.equal(torch.cat([getattr(a, k), getattr(b, k)]).view(torch.int64), getattr(whole, k).view(torch.int64)), k
    wide = torch.full((2, 24 * ny * nx + 52), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, :24 * ny * nx].view(2, 24, ny, nx)
    view.copy_(xd)
    assert view.stride(0) == 24 * ny * nx + 52 and same_records(SL.plane_records(view, THR3, 8), whole)
    assert same_records(SL.plane_records(x, THR3, 8), whole)        # numpy in
    # a workspace larger than the call needs, as an earlier call may leave it: the entry is told more bytes than 7 planes take
    L = lib()
    nbytes = 7 * L.rdgan_sal_workspace_bytes(ny, nx, 1) + 4096
    ws = torch.full(((nbytes + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    plane = torch.full((2, 24, 4), -7, dtype=torch.int64, device="cuda")
    objects = torch.full((2, 24, 3, 3), -7, dtype=torch.int64, device="cuda")
    vr = torch.full((2, 24, 3, 2), -7.0, dtype=torch.float64, device="cuda")
    thr = np.asarray(THR3, np.float64)
    rc = L.rdgan_sal_records(ptr(xd), 2, 24 * ny * nx, ny, nx, thr.ctypes.data_as(ctypes.c_void_p), 3, 8, ptr(plane), ptr(objects), ptr(vr),
                             ptr(ws), nbytes, stream())
    assert rc == 0 and same_records(SL.PlaneRecords(plane, objects, vr, ny, nx, THR3, 8), whole)
    # thresholds one at a time: the same columns
    for t, th in enumerate(THR3):
        one = SL.plane_records(xd, (th,), 8)
        assert torch.equal(one.plane, whole.plane) and torch.equal(one.objects[..., 0, :], whole.objects[..., t, :])
        assert torch.equal(one.vr[..., 0, :].contiguous().view(torch.int64), whole.vr[..., t, :].contiguous().view(torch.int64))


@pytest.mark.parametrize("conn", [4, 8])
def test_objects_are_the_cells(conn):
    x = days("70x130")
    xd = dev(x)
    got = SL.plane_records(xd, THR3, conn)
    stats = CL.cell_structure(xd, THR3, conn)
    assert np.array_equal(got.n_objects.sum(dim=(0, 1)).cpu().numpy(), stats.cells.sum(axis=(1, 2)))
    assert np.array_equal(got.n_wet.sum(dim=0).cpu().numpy().T, stats.wet_pixels)
    for t, th in enumerate(THR3):
        lab = CL.label_cells(xd, th, conn)
        flat = lab.view(48, -1)
        assert torch.equal((flat >= 0).sum(dim=1), got.n_wet[..., t].reshape(48))
        roots = flat == torch.arange(flat.shape[1], device="cuda", dtype=torch.int32)[None]
        assert torch.equal(roots.sum(dim=1), got.n_objects[..., t].reshape(48))


def day_of(planes):
    """(1, 24, ny, nx): the given planes in the first hours, the other hours dry"""
    x = np.zeros((1, 24) + planes[0].shape, np.float32)
    for h, p in enumerate(planes):
        x[0, h] = p
    return x


def tol(n_objects):
    """S, A, L against a known answer: the relative bound (n + 16) 2^-52 on V and r carried through 2 (a - b) / (a + b), whose
    derivatives are at most 2 / (a + b) times a or b: 8 (n + 16) 2^-52 absolute covers it with the divisions by d"""
    return 8 * (n_objects + 16) * EPS


def test_known_answers():
    ny, nx = 70, 130
    d = np.sqrt(ny * ny + nx * nx)
    z = np.zeros((ny, nx), np.float32)
    rng = np.random.default_rng(8)
    # 0: a field against itself; 1: the same field doubled, below the clamp.  Every wet value is a multiple of 1/1024 mm in 1 .. 20,
    # so the wet mask of f at 0.5 is that of 2 f at 1.0 and at 0.5 alike: the one threshold list serves as the scaled one
    f = ((1 + np.floor(rng.random((ny, nx)) * 19 * 1024) / 1024) * (rng.random((ny, nx)) < 0.4)).astype(np.float32)
    # 2: one rectangle shifted by (3, 4)
    a2, b2 = z.copy(), z.copy()
    a2[20:30, 40:60], b2[23:33, 44:64] = 2.0, 2.0
    # 3: two equal objects against one of the same total mass at their common centre
    a3, b3 = z.copy(), z.copy()
    a3[30:34, 20:24], a3[30:34, 100:104], b3[30:34, 60:64] = 2.0, 2.0, 4.0
    # 4: a peaked object against a flat one of equal mass and footprint: 16 pixels, 15 x 1 + 1 x 17 = 32 = 16 x 2
    a4, b4 = z.copy(), z.copy()
    a4[10:14, 10:14], b4[10:14, 10:14] = 1.0, 2.0
    a4[11, 11] = 17.0
    # 5: dry against dry; 6: dry model against wet observation; 7: wet model against dry observation
    model = day_of([f, 2 * f, a2, a3, a4, z, z, b2])
    obs = day_of([f, f, b2, b3, b4, z, b2, z])
    thr = (0.5,)
    got = SL.sal_hourly(dev(model)[None], dev(obs), thr)
    assert got.S.shape == (1, 1, 24, 1)
    S, A, L1, L2, L = (getattr(got, c)[0, 0, :, 0] for c in SL.COMPONENTS)
    n0 = int(SL.plane_records(obs, thr).n_objects[0, 0, 0])
    assert S[0] == 0 and A[0] == 0 and L[0] == 0                    # identical: exactly
    assert abs(A[1] - 2 / 3) <= tol(0) and abs(S[1]) <= tol(n0) and abs(L[1]) <= tol(n0)
    assert abs(L1[2] - 5 / d) <= tol(1) and S[2] == 0 and A[2] == 0 and L2[2] == 0
    r_m = SL.plane_records(a3[None, None].repeat(24, 1), thr).cpu().r[0, 0, 0]
    assert L1[3] == 0 and r_m == 40.0 and abs(L2[3] - 2 * r_m / d) <= tol(2) and L2[3] > 0 and A[3] == 0 and S[3] == 0
    assert S[4] < 0 and A[4] == 0 and abs(S[4] - 2 * (32 / 17 - 16) / (32 / 17 + 16)) <= tol(1) and L1[4] > 0
    assert all(np.isnan(v[5]) for v in (S, A, L1, L2, L))
    assert A[6] == -2 and A[7] == 2 and all(np.isnan(v[h]) for v in (S, L1, L2, L) for h in (6, 7))
    assert not got.mask_mismatch.any()
    s = got.summary()
    assert s["A"]["undefined"][0] == pytest.approx(17 / 24) and s["S"]["by_hour"].shape == (24, 1)


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_sal_of_the_held_ensemble(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4, a dry tile and a NaN pixel in the observation; `chunk` is one unit's wet tiles on both
    sides, as tests/test_hip_cells.py pins it, so that the hourly values the two sides see are the same.  (The generator is the real
    one at its initial weights: tests/fake_engine.py stands in for the training engine and has no generator forward for fields.)"""
    S, thr = 8, (0.1, 0.5, 2.0)
    rng = np.random.default_rng(31)
    obs = (rng.gamma(0.8, 0.6, (24, 40, 52)) * (rng.random((24, 40, 52)) < 0.5)).astype(np.float32)
    obs[:, :16, :16] = 0.0
    obs[3, 20, 30] = np.nan
    od = dev(obs)
    daily = od.sum(dim=0)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, daily, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, daily, S, latent=z, chunk=unit_tiles)
    want = SL.sal_hourly(hourly, od, thr)
    assert want.S.shape == (S, 24, 3) and not want.mask_mismatch[:, 3].any() and want.mask_mismatch[:, 4].all() and np.isfinite(want.A).all()
    check(SL.plane_records(hourly, thr), sn.records_np(hourly.cpu().numpy(), thr, 8))
    for scenario_chunk in (1, 7, S):
        got = SL.sal_field(generator, od if scenario_chunk == 7 else obs, S, thr, latent=z, scenario_chunk=scenario_chunk, chunk=unit_tiles)
        for c in SL.COMPONENTS + ("mask_mismatch",):
            assert np.array_equal(getattr(got, c).view(np.int64 if c != "mask_mismatch" else bool),
                                  getattr(want, c).view(np.int64 if c != "mask_mismatch" else bool)), (scenario_chunk, c)
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.sal_scenarios_field(obs, 3, thr, scenario_chunk=2, connectivity=4)
    assert a.S.shape == (3, 24, 3) and a.connectivity == 4


def test_cabi_argument_checks_on_device_pointers():
    L = lib()
    ny, nx = 5, 7
    x = torch.zeros((1, 24, ny, nx), dtype=torch.float32, device="cuda")
    one = L.rdgan_sal_workspace_bytes(ny, nx, 1)
    ws = torch.zeros(one // 8 + 2, dtype=torch.int64, device="cuda")
    plane = torch.full((24 * 4 + 1,), -7, dtype=torch.int64, device="cuda")
    objects = torch.full((24 * 2 * 3 + 1,), -7, dtype=torch.int64, device="cuda")
    vr = torch.full((24 * 2 * 2 + 1,), -7.0, dtype=torch.float64, device="cuda")
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    thr = np.array([0.1, 1.0])
    null = ctypes.c_void_p(0)
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)

    def rec(x=ptr(x), n=1, stride=24 * 35, ny=ny, nx=nx, th=hp(thr), T=2, conn=8, plane=ptr(plane), obj=ptr(objects), vr=ptr(vr), ws=ptr(ws), nbytes=one):
        return L.rdgan_sal_records(x, n, stride, ny, nx, th, T, conn, plane, obj, vr, ws, nbytes, stream())

    for kw in (dict(x=null), dict(plane=null), dict(obj=null), dict(vr=null), dict(ws=null), dict(th=null), dict(x=off(x, 2)), dict(plane=off(plane, 4)),
               dict(obj=off(objects, 4)), dict(vr=off(vr, 4)), dict(ws=off(ws, 4)), dict(conn=0), dict(conn=6), dict(T=0), dict(T=9),
               dict(th=hp(np.array([1.0, 0.1]))), dict(nbytes=one - 1), dict(nbytes=0), dict(n=0), dict(stride=24 * 35 - 1),
               dict(ny=64, nx=1 << 18, stride=24 << 24, nbytes=1 << 40)):
        assert rec(**kw) == -2, kw
    torch.cuda.synchronize()
    assert (plane == -7).all() and (objects == -7).all() and (vr == -7).all()              # no output touched
    assert rec() == 0
    torch.cuda.synchronize()
    assert (plane[:-1] == 0).all() and plane[-1] == -7 and (objects[:-1] == 0).all() and objects[-1] == -7 and (vr[:-1] == 0).all() and vr[-1] == -7
