"""-m gpu: verification of field ensembles (csrc/rdgan_verify.hip.h, pr_disagg_radar_gan_amd/verification.py) against the numpy
restatement (tests/verify_np.py, itself checked on the CPU by tests/test_verification_host.py).  Every accumulated value is an
integer or an fp64 sum of integers below 2^53, so every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, models, verification as V, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import verify_np as vn
from tests.hip_util import dev, ptr, stream

pytestmark = pytest.mark.gpu

THR8 = (0.0, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0)
S = 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_CASES = {}


def case(lead, ny, nx):
    """(x (8, *lead, 24, ny, nx), obs): gamma hours with many exact zeros; one NaN observation pixel-hour, one NaN member value in
    member 5 (it arrives in the second add of 3 + 5), one wet position where all members equal the observation.  Built once."""
    key = (lead, ny, nx)
    if key not in _CASES:
        rng = np.random.default_rng(ny * 1000 + nx + len(lead))
        shape = lead + (24, ny, nx)
        draw = lambda sh: (rng.gamma(0.4, 3.0, sh) * (rng.random(sh) < 0.45)).astype(np.float32)
        x, o = draw((S,) + shape), draw(shape)
        first = (0,) * len(lead)
        o[first + (3, 0, nx // 2)] = np.nan
        x[(5,) + first + (7, ny - 1, nx - 1)] = np.nan
        o[first + (11, ny // 2, 0)] = np.float32(1.25)
        x[(slice(None),) + first + (11, ny // 2, 0)] = np.float32(1.25)
        _CASES[key] = (x, o)
    return _CASES[key]


def host(state):
    return tuple(t.cpu().numpy() for t in state)


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("lead,ny,nx", [((), 5, 67), ((2,), 5, 67), ((), 1, 1), ((2,), 1, 1)])
def test_accumulate_against_restatement(lead, ny, nx, T):
    x, o = case(lead, ny, nx)
    thr = THR8 if T == 8 else (1.0,)
    want = vn.state(x, o, thr)
    assert want[3].sum() == 2 and np.all(want[2][(0,) * len(lead) + (11, ny // 2, 0)] == S)
    xd, od = dev(x), dev(o)
    Pn = o.size
    at_once = V.EnsembleVerifier(od, thr).add(xd)
    split = V.EnsembleVerifier(o, thr).add(xd[:3]).add(xd[3:])
    wide = torch.full((S, Pn + 3), -5.0, device="cuda")              # member stride P + 3: odd, so the rows are not 16-byte aligned
    wide[:, :Pn] = xd.view(S, Pn)
    view = wide[:, :Pn].view((S,) + o.shape)
    assert view.stride(0) == Pn + 3 and not view.is_contiguous()
    strided = V.EnsembleVerifier(od, thr).add(view)
    from_numpy = V.EnsembleVerifier(od, thr).add(wide.cpu().numpy()[:, :Pn].reshape((S,) + o.shape))      # made dense on the host
    assert at_once.n_members == split.n_members == strided.n_members == from_numpy.n_members == S
    with pytest.raises(ValueError, match="on the host"):
        at_once.add(view.cpu())
    for name, ver in (("8 at once", at_once), ("3 + 5", split), ("stride P + 3", strided), ("numpy view", from_numpy)):
        got = host(ver.state())
        assert got[0].shape == (T,) + o.shape and got[0].dtype == np.int32 and got[3].dtype == np.uint8
        for k, what in enumerate(("exceed", "below", "equal", "bad")):
            assert np.array_equal(got[k], want[k]), (name, what)
    with pytest.raises(ValueError):
        at_once.add(dev(np.zeros((4089,) + o.shape, np.float32)) if Pn <= 48 else xd[:, ..., :-1])


@pytest.mark.parametrize("seed", [0, 12345678901234567])
@pytest.mark.parametrize("n_bins", [2, 9])
def test_reduce_against_restatement(seed, n_bins):
    x, o = case((2,), 5, 67)
    thr = (0.1, 1.0, 5.0)
    ver = V.EnsembleVerifier(o, thr).add(dev(x))
    st = vn.state(x, o, thr)
    want = vn.reduce(o, st, S, thr, n_bins, seed)
    a = ver.result(scales=(1,), n_bins=n_bins, seed=seed)
    b = ver.result(scales=(1,), n_bins=n_bins, seed=seed)
    assert a.n_members == S and a.n_valid == o.size - 2 and a.thresholds == tuple(float(np.float32(t)) for t in thr)
    for k, name in enumerate(("rank_hist", "reliability", "brier_sums")):
        got = getattr(a, name)
        assert got.dtype == np.int64 and np.array_equal(got, want[k]), name
        assert np.array_equal(got, getattr(b, name)), name
    assert a.rank_hist.sum() == o.size - 2
    other = ver.result(scales=(1,), n_bins=n_bins, seed=seed + 1)
    assert not np.array_equal(other.rank_hist, a.rank_hist) and np.array_equal(other.brier_sums, a.brier_sums)


def test_reduce_one_member():
    x, o = case((), 5, 67)
    ver = V.EnsembleVerifier(o, (0.1, 1.0)).add(dev(x[:1]))
    a = ver.result(scales=(1,), n_bins=2, seed=3)
    want = vn.reduce(o, vn.state(x[:1], o, (0.1, 1.0)), 1, (0.1, 1.0), 2, 3)
    assert np.array_equal(a.rank_hist, want[0]) and np.array_equal(a.reliability, want[1]) and np.array_equal(a.brier_sums, want[2])
    assert a.rank_hist.shape == (24, 2)
    with pytest.raises(ValueError):
        ver.result(n_bins=3)


def test_reduce_4096_members_on_64_positions():
    """the C entries themselves: 64 positions are no whole day (plane 1: hour = p % 24), 4096 members fill the widest histogram"""
    lib = _lib.load()
    n, Pn, thr = 4096, 64, np.array([0.1, 1.0, 5.0])
    rng = np.random.default_rng(64)
    x = (rng.gamma(0.4, 3.0, (n, Pn)) * (rng.random((n, Pn)) < 0.45)).astype(np.float32)
    o = (rng.gamma(0.4, 3.0, Pn) * (rng.random(Pn) < 0.45)).astype(np.float32)
    o[:4] = (0.0, 0.05, 30.0, np.nan)
    st = vn.state(x, o, thr)
    xd, od = dev(x), dev(o)
    exceed = torch.zeros((3, Pn), dtype=torch.int32, device="cuda")
    below, equal = torch.zeros(Pn, dtype=torch.int32, device="cuda"), torch.zeros(Pn, dtype=torch.int32, device="cuda")
    bad = torch.zeros(Pn, dtype=torch.uint8, device="cuda")
    hp = thr.ctypes.data_as(ctypes.c_void_p)
    for s0, s1 in ((0, 1000), (1000, 4096)):
        assert lib.rdgan_verify_accumulate(ptr(xd[s0:s1]), s1 - s0, Pn, Pn, ptr(od), hp, 3, ptr(exceed), ptr(below), ptr(equal), ptr(bad),
                                           stream()) == 0
    for got, want in zip(host((exceed, below, equal, bad)), st):
        assert np.array_equal(got, want)
    assert st[2][0] > 1000                                           # the dry position ties with a thousand dry members
    for n_bins in (2, 64):
        rank = torch.full((24, n + 1), -1, dtype=torch.int64, device="cuda")
        rel = torch.full((3, 24, n_bins, 3), -1, dtype=torch.int64, device="cuda")
        brier = torch.full((3, 24, 4), -1, dtype=torch.int64, device="cuda")
        assert lib.rdgan_verify_reduce(ptr(od), ptr(exceed), ptr(below), ptr(equal), ptr(bad), Pn, 1, n, hp, 3, n_bins, 77, ptr(rank),
                                       ptr(rel), ptr(brier), stream()) == 0
        want = vn.reduce(o.reshape(Pn, 1, 1), tuple(a.reshape(a.shape[:-1] + (Pn, 1, 1)) for a in st), n, thr, n_bins, 77)
        assert np.array_equal(rank.cpu().numpy(), want[0]) and np.array_equal(rel.cpu().numpy(), want[1])
        assert np.array_equal(brier.cpu().numpy(), want[2]) and want[0].sum() == Pn - 1


@pytest.mark.parametrize("lead,ny,nx,T,scales", [((2,), 5, 67, 8, (1, 3, 9)), ((), 5, 67, 1, (1, 3, 9)),
                                                 ((), 20, 70, 2, (1, 3, 5, 9, 17, 33, 65))])
def test_fss_against_restatement(lead, ny, nx, T, scales):
    x, o = case(lead, ny, nx)
    o = o.copy()
    o[(0,) * len(lead) + (6, 0, 1)] = np.nan                         # a bad pixel beside the edge, in a corner box of every width
    o[(0,) * len(lead) + (6, 1, 0)] = np.float32(7.0)
    thr = THR8 if T == 8 else (0.1, 1.0)[:T]
    ver = V.EnsembleVerifier(o, thr).add(dev(x))
    st = vn.state(x, o, thr)
    want = vn.fss_sums(o, st[0], st[3], S, thr, scales)
    assert want.max() < 2.0 ** 53 and want[0, :, :, 1].min() > 0
    a = ver.result(scales=scales, n_bins=9)
    b = ver.result(scales=scales, n_bins=9)
    assert a.scales == scales and a.fss_sums.dtype == np.float64 and a.fss_sums.shape == (T, len(scales), 24, 2)
    assert same_bits(a.fss_sums, want) and same_bits(a.fss_sums, b.fss_sums)
    assert same_bits(a.fss(), vn.fss(want.sum(axis=2))) and same_bits(a.fss(by_hour=True), vn.fss(want))
    bs, base, bss = a.brier()
    wbs, wbase, wbss = vn.brier_score(vn.reduce(o, st, S, thr, 9, 0)[2].sum(axis=1), S)
    assert same_bits(bs, wbs) and same_bits(base, wbase) and same_bits(bss, wbss)


def test_verify_hourly_is_the_verifier():
    x, o = case((), 5, 67)
    a = V.verify_hourly(dev(x), dev(o), (0.1, 1.0), scales=(1, 3), n_bins=5, seed=9)
    b = V.verify_hourly(x, o, (0.1, 1.0), scales=(1, 3), n_bins=5, seed=9)
    st = vn.state(x, o, (0.1, 1.0))
    want = vn.reduce(o, st, S, (0.1, 1.0), 5, 9)
    for got in (a, b):
        assert np.array_equal(got.rank_hist, want[0]) and np.array_equal(got.reliability, want[1])
        assert same_bits(got.fss_sums, vn.fss_sums(o, st[0], st[3], S, (0.1, 1.0), (1, 3)))


def test_positions_past_2_31():
    """one member, one threshold, 24 x 9460 x 9460 > 2^31 positions, built on the device from index patterns:
    obs = hour + x % 5, member = obs + s(y), s = -1 on even rows, +1 on odd ones, 0 on the first and the last row; threshold 10.5.
    Accumulate and reduce only; totals from counting the patterns, and the last positions one by one."""
    ny = nx = 9460
    Pn = 24 * ny * nx
    assert Pn > 2 ** 31
    hv = torch.arange(24, dtype=torch.float32, device="cuda").view(24, 1, 1)
    xv = (torch.arange(nx, device="cuda") % 5).to(torch.float32).view(1, 1, nx)
    sy = np.where(np.arange(ny) % 2 == 0, -1.0, 1.0).astype(np.float32)
    sy[0] = sy[-1] = 0.0
    obs = torch.empty((24, ny, nx), dtype=torch.float32, device="cuda")
    torch.add(hv.expand(24, ny, 1), xv, out=obs)
    member = torch.empty((1, 24, ny, nx), dtype=torch.float32, device="cuda")
    torch.add(obs, dev(sy).view(1, ny, 1), out=member[0])
    obs.view(-1)[Pn - 2] = float("nan")
    ver = V.EnsembleVerifier(obs, (10.5,)).add(member)
    exceed, below, equal, bad = ver.state()
    # counts per (hour, row class, x % 5)
    n_x = np.bincount(np.arange(nx) % 5, minlength=5)
    n_s = {-1.0: int((sy == -1).sum()), 0.0: 2, 1.0: int((sy == 1).sum())}
    assert int(below.sum()) == 24 * nx * n_s[-1.0] and int(equal.sum()) == 24 * nx * 2 - 1 and int(bad.sum()) == 1
    want_exceed = sum(n_s[s] * n_x[r] for h in range(24) for s in n_s for r in range(5) if h + r + s > 10.5)
    assert int(exceed.sum()) == want_exceed
    tail = lambda t: t.view(-1)[Pn - 3:].cpu().numpy().tolist()
    assert tail(bad) == [0, 1, 0] and tail(below) == [0, 0, 0] and tail(equal) == [1, 0, 1] and tail(exceed) == [1, 1, 1]
    assert below.view(-1)[Pn - nx - 1].item() == (1 if sy[ny - 2] < 0 else 0)          # the last pixel of the row before: past 2^31 too
    lib = _lib.load()
    rank = torch.empty((24, 2), dtype=torch.int64, device="cuda")
    rel = torch.empty((1, 24, 2, 3), dtype=torch.int64, device="cuda")
    brier = torch.empty((1, 24, 4), dtype=torch.int64, device="cuda")
    thr = np.array([10.5])
    assert lib.rdgan_verify_reduce(ptr(obs), ptr(exceed), ptr(below), ptr(equal), ptr(bad), Pn, ny * nx, 1,
                                   thr.ctypes.data_as(ctypes.c_void_p), 1, 2, 5, ptr(rank), ptr(rel), ptr(brier), stream()) == 0
    rank, rel, brier = rank.cpu().numpy(), rel.cpu().numpy(), brier.cpu().numpy()
    valid = np.full(24, ny * nx, np.int64)
    valid[23] -= 1
    assert np.array_equal(rank.sum(axis=1), valid) and np.array_equal(brier[0, :, 0], valid)
    # ranks: 1 where the member lies below, 0 where above, the hash's top bit on the two tied rows (the last one lies past 2^31)
    for h in (0, 23):
        tied = np.concatenate([(h * ny + y) * nx + np.arange(nx, dtype=np.int64) for y in (0, ny - 1)])
        if h == 23:
            tied = tied[tied != Pn - 2]
        ones = int((vn.b24(5, tied) >> 23).sum())
        assert rank[h, 1] == nx * n_s[-1.0] + ones and tied.max() > (2 ** 31 if h == 23 else 0)
    for h in range(24):
        e_x = np.array([h + r > 10.5 for r in range(5)])             # the observed event by x % 5
        n_e = int((n_x * e_x).sum()) * ny - (1 if h == 23 else 0)      # (the NaN position would have been an event: 23 + 3 > 10.5)
        c1 = sum(n_s[s] * n_x[r] for s in n_s for r in range(5) if h + r + s > 10.5) - (1 if h == 23 else 0)
        ce = sum(n_s[s] * n_x[r] for s in n_s for r in range(5) if h + r + s > 10.5 and h + r > 10.5) - (1 if h == 23 else 0)
        assert brier[0, h].tolist() == [valid[h], n_e, ce, c1], h
        assert rel[0, h, 1].tolist() == [c1, ce, c1] and rel[0, h, 0, 0] == valid[h] - c1 and rel[0, h, 0, 2] == 0


def test_cabi_bad_arguments_leave_the_outputs_untouched():
    lib = _lib.load()
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    x, o = case((2,), 5, 67)
    Pn, T = o.size, 2
    xd, od = dev(x), dev(o)
    thr, wd = np.array([0.1, 1.0]), np.array([1, 3, 9], np.int32)
    i32 = lambda *sh: torch.full(sh, -7, dtype=torch.int32, device="cuda")
    exceed, below, equal = i32(T, Pn), i32(Pn), i32(Pn)
    bad = torch.full((Pn,), 77, dtype=torch.uint8, device="cuda")
    rank = torch.full((24, S + 1), -7, dtype=torch.int64, device="cuda")
    rel = torch.full((T, 24, 5, 3), -7, dtype=torch.int64, device="cuda")
    brier = torch.full((T, 24, 4), -7, dtype=torch.int64, device="cuda")
    fss = torch.full((T, 3, 24, 2), -7.0, dtype=torch.float64, device="cuda")
    need = lib.rdgan_verify_fss_workspace_bytes(5, 67, T, 3)
    assert need > 0
    ws = torch.full((need // 8 + 1,), -7, dtype=torch.int64, device="cuda")

    def acc(members=ptr(xd), n=S, stride=Pn, P=Pn, obs=ptr(od), th=hp(thr), T=T, exceed=ptr(exceed), below=ptr(below), equal=ptr(equal),
            bad=ptr(bad)):
        return lib.rdgan_verify_accumulate(members, n, stride, P, obs, th, T, exceed, below, equal, bad, stream())

    def red(obs=ptr(od), exceed=ptr(exceed), bad=ptr(bad), P=Pn, plane=5 * 67, S=S, th=hp(thr), T=T, n_bins=5, rank=ptr(rank),
            rel=ptr(rel), brier=ptr(brier)):
        return lib.rdgan_verify_reduce(obs, exceed, ptr(below), ptr(equal), bad, P, plane, S, th, T, n_bins, 0, rank, rel, brier, stream())

    def fs(obs=ptr(od), exceed=ptr(exceed), bad=ptr(bad), days=2, ny=5, nx=67, S=S, th=hp(thr), T=T, w=hp(wd), W=3, out=ptr(fss),
           ws=ptr(ws), nbytes=need):
        return lib.rdgan_verify_fss(obs, exceed, bad, days, ny, nx, S, th, T, w, W, out, ws, nbytes, stream())

    unsorted, negative = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0]))
    for kw in (dict(members=null), dict(obs=null), dict(exceed=null), dict(below=null), dict(equal=null), dict(bad=null), dict(th=null),
               dict(n=0), dict(n=4097), dict(stride=Pn - 1), dict(P=0), dict(T=0), dict(T=9), dict(th=unsorted), dict(th=negative)):
        assert acc(**kw) == -2, kw
    for kw in (dict(obs=null), dict(exceed=null), dict(bad=null), dict(rank=null), dict(rel=null), dict(brier=null), dict(th=null),
               dict(S=0), dict(S=4097), dict(n_bins=1), dict(n_bins=S + 2), dict(T=0), dict(T=9), dict(plane=0), dict(plane=7), dict(P=0),
               dict(th=unsorted), dict(th=negative)):
        assert red(**kw) == -2, kw
    for kw in (dict(obs=null), dict(exceed=null), dict(bad=null), dict(out=null), dict(ws=null), dict(th=null), dict(w=null), dict(days=0),
               dict(ny=0), dict(nx=0), dict(S=0), dict(S=4097), dict(T=0), dict(T=9), dict(W=0), dict(W=9), dict(nbytes=need - 1),
               dict(w=hp(np.array([1, 4, 9], np.int32))), dict(w=hp(np.array([3, 1, 9], np.int32))), dict(S=4096, w=hp(np.array([1, 3, 129], np.int32))),
               dict(th=unsorted), dict(th=negative)):
        assert fs(**kw) == -2, kw
    torch.cuda.synchronize()
    for t, v in ((exceed, -7), (below, -7), (equal, -7), (bad, 77), (rank, -7), (rel, -7), (brier, -7), (fss, -7.0), (ws, -7)):
        assert bool((t == v).all())                                  # nothing was launched
    for t in (exceed, below, equal, bad):
        t.zero_()
    assert acc() == 0 and red() == 0 and fs() == 0
    torch.cuda.synchronize()
    st = vn.state(x, o, thr)
    assert np.array_equal(exceed.cpu().numpy().reshape(st[0].shape), st[0]) and np.array_equal(bad.cpu().numpy().reshape(o.shape), st[3])
    want = vn.reduce(o, st, S, thr, 5, 0)
    assert np.array_equal(rank.cpu().numpy(), want[0]) and np.array_equal(rel.cpu().numpy(), want[1])
    assert np.array_equal(brier.cpu().numpy(), want[2])
    assert same_bits(fss.cpu().numpy(), vn.fss_sums(o, st[0], st[3], S, thr, (1, 3, 9)))


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def _observed():
    """(2, 24, 20, 30) hours: day 0 wet with one NaN pixel-hour (its daily sum, and with it all 24 scenario hours, are NaN), day 1 dry"""
    rng = np.random.default_rng(77)
    obs = (rng.gamma(0.5, 2.0, (2, 24, 20, 30)) * (rng.random((2, 24, 20, 30)) < 0.5)).astype(np.float32)
    obs[1] = 0.0
    obs[0, 5, 3, 4] = np.nan
    return obs


def _same_verification(a, b):
    return (a.thresholds == b.thresholds and a.scales == b.scales and a.n_members == b.n_members and a.n_valid == b.n_valid
            and np.array_equal(a.rank_hist, b.rank_hist) and np.array_equal(a.reliability, b.reliability)
            and np.array_equal(a.brier_sums, b.brier_sums) and same_bits(a.fss_sums, b.fss_sums))


def test_verify_field_equals_verify_hourly_of_disaggregate(generator, monkeypatch):
    n, thr, scales = 6, (0.1, 0.5, 2.0), (1, 3, 9)
    obs = _observed()
    od = dev(obs)
    z = np.random.default_rng(78).normal(size=(n, 2, 100)).astype(np.float32)
    hourly, info = F.disaggregate(generator, od.sum(dim=-3), n, latent=z)
    assert info.n_nan_pixels == 1 and hourly.shape == (n, 2, 24, 20, 30)
    want = V.verify_hourly(hourly, od, thr, scales=scales, n_bins=7, seed=4)
    assert want.n_members == n and want.n_valid == obs.size - 24     # the NaN pixel is bad in all its hours
    assert want.brier_sums[0, :, 1].sum() > 0 and want.rank_hist.sum() == want.n_valid
    # the state of the held ensemble is the restatement's
    st = vn.state(hourly.cpu().numpy(), obs, thr)
    assert np.array_equal(want.brier_sums, vn.reduce(obs, st, n, thr, 7, 4)[2])
    for scenario_chunk in (4, 6):
        for chunk in (3, 1024):
            got = V.verify_field(generator, od if chunk == 3 else obs, n, thr, scales=scales, n_bins=7, rank_seed=4, latent=z,
                                 scenario_chunk=scenario_chunk, chunk=chunk)
            assert _same_verification(got, want), (scenario_chunk, chunk)
    # a seeded device generator: all scenarios' latent vectors drawn once, as disaggregate draws them, whatever the chunks
    hourly3, _ = F.disaggregate(generator, od.sum(dim=-3), n, seed=3)
    assert not torch.equal(hourly3, hourly)
    want3 = V.verify_hourly(hourly3, od, thr, scales=scales, n_bins=7, seed=4)
    for scenario_chunk in (4, 16):
        got = V.verify_field(generator, od, n, thr, scales=scales, n_bins=7, rank_seed=4, seed=3, scenario_chunk=scenario_chunk, chunk=5)
        assert _same_verification(got, want3), scenario_chunk
    # the reference-style entry: numpy in, the latent noise from the global numpy RNG
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.verify_scenarios_field(obs, n, thr, scales=scales, n_bins=7, rank_seed=4, scenario_chunk=4)
    np.random.seed(5)
    b = V.verify_field(generator, obs, n, thr, scales=scales, n_bins=7, rank_seed=4, norm_scale=P.norm_scale)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, od.sum(dim=-3), n, norm_scale=P.norm_scale)
    assert _same_verification(a, b) and _same_verification(a, V.verify_hourly(hourly2, od, thr, scales=scales, n_bins=7, seed=4))


def test_verify_field_on_a_dry_day_draws_nothing():
    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    obs = np.zeros((24, 20, 30), np.float32)
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    v = V.verify_field(NoGenerator(), obs, 3, (0.1,), scales=(1,), n_bins=4)
    assert np.array_equal(np.random.get_state()[1], before)           # as disaggregate: without a wet tile no latent is drawn
    assert v.n_valid == obs.size and v.rank_hist.sum(axis=0).sum() == obs.size and np.all(v.brier_sums[0, :, 1:] == 0)
    assert np.isnan(v.fss()[0, 0]) and v.brier()[0][0] == 0.0
