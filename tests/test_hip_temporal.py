"""-m gpu: temporal structure of hourly fields (csrc/rdgan_temporal.hip.h, pr_disagg_radar_gan_amd/temporal.py) against the numpy
restatement (tests/temporal_np.py, itself checked on the CPU by tests/test_temporal_host.py).  Counts are compared for equality; an
fp64 sum of N non-negative terms within N 2^-52 relative (each of two orders is within (N - 1) 2^-53 of the exact sum), and for
equality on inputs that are multiples of 1/8 below 32, whose sums are exact."""
import ctypes

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, models, temporal as TS, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import temporal_np as tn
from tests.hip_util import dev, ptr, stream

pytestmark = pytest.mark.gpu

THR8 = (0.0, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0)
COUNTS = ("wet_hours", "longest_wet", "wet_spell", "dry_spell", "first_wet", "last_wet", "trans")
SUMS = ("moments", "lag", "wet_amount")
EPS = 2.0 ** -52


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def draw(shape, p_wet, seed):
    """gamma hours, wet with probability p_wet (p_wet = 1: every hour above every threshold of THR8)"""
    rng = np.random.default_rng(seed)
    x = (rng.gamma(0.6, 3.0, shape) * (rng.random(shape) < p_wet)).astype(np.float32)
    return x + np.float32(25.0) if p_wet == 1.0 else x


def spoil(x):
    """values exactly at thresholds, -0.0, a NaN series and an inf series, where the shape has room"""
    f = x.reshape(-1, 24, x.shape[-2] * x.shape[-1])
    q = f.shape[2] - 1
    f[0, 3, 0], f[0, 4, 0], f[0, 5, 0], f[0, 6, q] = 0.5, 2.0, -0.0, 0.1
    f[-1, 7, q] = np.nan
    if f.shape[0] * f.shape[2] > 2:
        f[0, 23, q // 2 + 1] = np.inf
    return x


def agree(got, want, T, K, exact=False):
    """got: TemporalStats; want: dict of the restatement"""
    assert got.n_valid == want["n_valid"] and got.n_bad == want["n_bad"]
    for name in COUNTS:
        assert np.array_equal(getattr(got, name), want[name]), name
    n = tn.terms(want, T, K)
    for name in SUMS:
        g, w = getattr(got, name), want[name]
        if exact:
            assert same_bits(g, w), name
        else:
            assert np.all(np.abs(g - w) <= n[name] * EPS * np.abs(w)), (name, np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))


def test_one_series_by_hand():
    x = np.zeros((1, 24, 1, 1), np.float32)
    x[0, [0, 1, 5, 22, 23], 0, 0] = (1.0, 2.0, 0.5, 3.0, 0.25)          # masks: > 0.25 -> hours 0, 1, 5, 22; > 1 -> hours 1, 22
    s = TS.temporal_structure(x, (0.25, 1.0), max_lag=2)
    assert s.n_valid == 1 and s.n_bad == 0
    assert s.wet_hours[0, 4] == 1 and s.wet_hours[1, 2] == 1 and s.wet_hours.sum() == 2
    assert s.longest_wet[0, 2] == 1 and s.longest_wet[1, 1] == 1
    assert s.wet_spell[0].tolist() == [[2] + [0] * 23, [0, 1] + [0] * 22]           # interior: 5 and 22; at the edge: 0 .. 1
    assert s.wet_spell[1, 0, 0] == 2 and s.wet_spell[1].sum() == 2
    assert s.dry_spell[0, 0, 2] == 1 and s.dry_spell[0, 0, 15] == 1 and s.dry_spell[0, 1, 0] == 1 and s.dry_spell[0].sum() == 3
    assert s.dry_spell[1, 1, 0] == 2 and s.dry_spell[1, 0, 19] == 1 and s.dry_spell[1].sum() == 3
    assert s.first_wet[0, 0] == 1 and s.last_wet[0, 22] == 1 and s.first_wet[1, 1] == 1 and s.last_wet[1, 22] == 1
    assert s.trans[0, 0].tolist() == [[0, 0], [0, 1]] and s.trans[0, 1].tolist() == [[0, 0], [1, 0]] and s.trans[0, 4].tolist() == [[0, 1], [0, 0]]
    assert s.trans[0, 22].tolist() == [[0, 0], [1, 0]] and s.trans[1, 0].tolist() == [[0, 1], [0, 0]] and np.all(s.trans.sum(axis=(2, 3)) == 1)
    assert s.moments[:, 0].sum() == 6.75 and s.moments[1].tolist() == [2.0, 4.0]
    assert s.lag.tolist() == [1.0 * 2.0 + 3.0 * 0.25, 0.0]
    assert s.wet_amount[0, [0, 1, 5, 22, 23]].tolist() == [1.0, 2.0, 0.5, 3.0, 0.0] and s.wet_amount[1].sum() == 5.0


@pytest.mark.parametrize("T,K", [(1, 1), (4, 6), (8, 12)])
@pytest.mark.parametrize("layout", ["odd", "vec", "16x16", "shifted", "strided"])
def test_against_restatement(layout, T, K):
    """(3, 24, 5, 7): odd plane, the scalar path; (2, 24, 4, 8): 16-byte loads; (5, 24, 16, 16); the (2, 24, 4, 8) array as a view
    shifted by one float, which must take the scalar path; a leading stride above 24 plane.  Wet probabilities 0 .. 1."""
    shape = {"odd": (3, 24, 5, 7), "vec": (2, 24, 4, 8), "16x16": (5, 24, 16, 16), "shifted": (2, 24, 4, 8), "strided": (3, 24, 4, 8)}[layout]
    thr = THR8[:T] if T > 1 else (0.5,)
    for p_wet in (0.0, 0.05, 0.5, 0.95, 1.0):
        x = spoil(draw(shape, p_wet, int(p_wet * 100) + shape[0]))
        if layout == "shifted":
            buf = torch.zeros(x.size + 4, dtype=torch.float32, device="cuda")
            xd = buf[1:1 + x.size].view(shape)
            xd.copy_(dev(x))
            assert xd.data_ptr() % 16 == 4
        elif layout == "strided":
            wide = torch.full((shape[0], 24 * 32 + 40), float("nan"), dtype=torch.float32, device="cuda")
            xd = wide[:, :24 * 32].view(shape)
            xd.copy_(dev(x))
            assert xd.stride(0) == 24 * 32 + 40
        else:
            xd = dev(x)
        agree(TS.TemporalStructure(thr, K).add(xd).result(), tn.temporal_np(x, thr, K), T, K)


@pytest.mark.parametrize("K", [7, 11])
@pytest.mark.parametrize("layout", ["odd", "vec"])
def test_fewer_lags_than_the_instance_forms(layout, K):
    """K = 7 .. 11 runs the 12-lag instances, which form 12 lags and keep the first K: the sums behind them must not shift"""
    shape = (3, 24, 5, 7) if layout == "odd" else (2, 24, 4, 8)
    x = spoil(draw(shape, 0.5, K))
    agree(TS.temporal_structure(dev(x), THR8[1:3], max_lag=K), tn.temporal_np(x, THR8[1:3], K), 2, K)


def test_views_a_stride_cannot_express_are_refused():
    """a crop, a step or a transposed plane, at rank 3 as at rank 4: ValueError, and the state is untouched"""
    day = dev(draw((24, 20, 24), 0.5, 1))
    four = dev(draw((3, 24, 8, 12), 0.5, 2))
    ts = TS.TemporalStructure((0.1,)).add(four)
    before = [t.clone() for t in ts.state()]
    for bad in (day[:, 6:14, 4:16], day[..., ::2], day.transpose(1, 2)[:, :8, :12], four[:, :, 2:6], four[..., 3:], four.transpose(2, 3),
                four[:, :, ::2, ::2]):
        with pytest.raises(ValueError):
            TS.TemporalStructure((0.1,)).add(bad)
        if tuple(bad.shape[-2:]) == (8, 12):
            with pytest.raises(ValueError):
                ts.add(bad)
    assert all(torch.equal(a, b) for a, b in zip(ts.state(), before))
    # the dense copy of such a view is what the view means
    crop = day[:, 6:14, 4:16]
    agree(TS.temporal_structure(crop.contiguous(), (0.1,)), tn.temporal_np(crop.cpu().numpy(), (0.1,), 6), 1, 6)


def test_single_run_masks_against_closed_forms():
    x, runs = tn.single_run_days()
    s = TS.temporal_structure(x, (0.5,), max_lag=1)
    want = tn.single_run_closed_form(runs)
    for name in COUNTS:
        assert np.array_equal(getattr(s, name)[0], want[name]), name
    assert s.n_valid == 304 and s.n_bad == 0


@pytest.mark.parametrize("exact", [True, False])
def test_grouping(exact):
    """(23, 24, 12, 20) added at once and in groups of 1, 7 and 15: equal counts; equal sums on multiples of 1/8 below 32, sums
    within N 2^-52 on generic non-negative input; two identical sequences of calls give identical bits"""
    T, K, thr = 4, 6, THR8[:4]
    x = draw((23, 24, 12, 20), 0.3, 5)
    if exact:
        x = np.minimum(np.round(x * 8) / 8, np.float32(31.875)).astype(np.float32)
    xd = dev(x)
    whole = TS.TemporalStructure(thr, K).add(xd)
    want = tn.temporal_np(x, thr, K)
    agree(whole.result(), want, T, K, exact=exact)
    n = tn.terms(want, T, K)
    assert torch.equal(TS.TemporalStructure(thr, K).add(xd[:9]).add(x[9:]).state()[0], whole.state()[0])       # numpy onto a state that exists
    for g in (1, 7, 15):
        runs = []
        for _ in range(2):
            ts = TS.TemporalStructure(thr, K)
            for i in range(0, 23, g):
                ts.add(xd[i:i + g])
            runs.append(ts)
        assert torch.equal(runs[0].state()[0], runs[1].state()[0]) and same_bits(runs[0].state()[1].cpu().numpy(), runs[1].state()[1].cpu().numpy())
        assert torch.equal(runs[0].state()[0], whole.state()[0]), g
        got, ref = runs[0].result(), whole.result()
        for name in SUMS:
            a, b = getattr(got, name), getattr(ref, name)
            assert same_bits(a, b) if exact else np.all(np.abs(a - b) <= n[name] * EPS * np.abs(b)), (g, name)


def test_more_series_than_one_pass_of_the_grid():
    """THREADS * MAX_BLOCKS = 262144 threads is one pass of the largest grid; an odd plane takes the scalar path, one series per
    thread, so 513 * 515 = 264195 series need every workgroup (1024 LDS tables merge) and a second trip of the loop for some"""
    ny, nx = 513, 515
    assert ny * nx > TS.THREADS * TS.MAX_BLOCKS and (ny * nx) % 2 == 1
    x = spoil(draw((1, 24, ny, nx), 0.2, 9))
    agree(TS.temporal_structure(dev(x), THR8[:2], max_lag=3), tn.temporal_np(x, THR8[:2], 3), 2, 3)
    # and a few workgroups of the 16-byte path with a ragged last one
    x = spoil(draw((5, 24, 33, 40), 0.4, 10))
    assert 5 * 33 * 40 // 4 > 6 * TS.THREADS
    agree(TS.temporal_structure(dev(x), THR8[:2], max_lag=3), tn.temporal_np(x, THR8[:2], 3), 2, 3)


def test_past_2_31_elements():
    """1366 zero days of 256 x 256: 24 * 65536 * 1366 > 2^31 floats (8.6 GB), with planted series in the first day, in the last
    day and at the very last pixel; the expectation is the closed form for dry series corrected by the planted ones, no numpy pass
    over the array.  A counter past 2^32 needs more than 2^32 series, i.e. 2^32 * 96 bytes = 412 GB: out of reach of any card, so
    the 64-bit merge is covered by the layout alone."""
    n, ny, nx = 1366, 256, 256
    plane = ny * nx
    assert n * 24 * plane > 2 ** 31
    x = torch.zeros((n, 24, ny, nx), dtype=torch.float32, device="cuda")
    planted = {(0, 5): {3: 2.0, 4: 1.0}, (n - 1, 17): {0: 4.0}, (n - 1, plane - 1): {22: 1.5, 23: 2.5}, (n - 1, plane - 2): {9: float("nan")}}
    for (i, q), hours in planted.items():
        for h, v in hours.items():
            x.view(n, 24, plane)[i, h, q] = v
    assert (n - 1) * 24 * plane + 23 * plane + plane - 1 > 2 ** 31
    s = TS.temporal_structure(x, (0.5,), max_lag=2)
    N = n * plane
    assert s.n_bad == 1 and s.n_valid == N - 1
    assert s.wet_hours[0].tolist() == [N - 4, 1, 2] + [0] * 22 and s.longest_wet[0].tolist() == [N - 4, 1, 2] + [0] * 22
    assert s.wet_spell[0, 0, 1] == 1 and s.wet_spell[0, 1, 0] == 1 and s.wet_spell[0, 1, 1] == 1 and s.wet_spell[0].sum() == 3
    assert s.dry_spell[0, 1, 23] == N - 4 and s.dry_spell[0, 1, 2] == 1 and s.dry_spell[0, 1, 18] == 1 and s.dry_spell[0, 1, 22] == 1
    assert s.dry_spell[0, 1, 21] == 1 and s.dry_spell[0].sum() == N - 4 + 4
    assert s.first_wet[0, [3, 0, 22]].tolist() == [1, 1, 1] and s.last_wet[0, [4, 0, 23]].tolist() == [1, 1, 1]
    assert np.all(s.trans[0].sum(axis=(1, 2)) == N - 1) and s.trans[0, 3, 1, 1] == 1 and s.trans[0, 22, 1, 1] == 1 and s.trans[0, 0, 1, 0] == 1
    assert s.trans[0, :, 1, 1].sum() == 2 and s.trans[0, :, 0, 1].sum() == 2 and s.trans[0, :, 1, 0].sum() == 2
    assert s.moments[:, 0].tolist() == [4.0, 0, 0, 2.0, 1.0] + [0] * 17 + [1.5, 2.5] and s.moments[23, 1] == 6.25
    assert s.lag.tolist() == [2.0 + 3.75, 0.0] and s.wet_amount[0].tolist() == s.moments[:, 0].tolist()


def test_cabi_bad_arguments_leave_the_outputs_untouched():
    lib = _lib.load()
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    x = draw((3, 24, 4, 8), 0.5, 3)
    xd = dev(x)
    thr = np.array([0.1, 1.0])
    T, K, plane = 2, 6, 32
    counts = torch.full((T * TS.N_COUNTS + 2,), -7, dtype=torch.int64, device="cuda")
    sums = torch.full((TS.n_sums(T, K),), -7.0, dtype=torch.float64, device="cuda")
    need = lib.rdgan_temporal_workspace_bytes(3, plane, T, K)
    assert need > 0
    ws = torch.full((need // 8 + 1,), -7, dtype=torch.int64, device="cuda")

    def acc(x=ptr(xd), n=3, stride=24 * plane, plane=plane, th=hp(thr), T=T, K=K, counts=ptr(counts), sums=ptr(sums), ws=ptr(ws), nbytes=need):
        return lib.rdgan_temporal_accumulate(x, n, stride, plane, th, T, K, counts, sums, ws, nbytes, stream())

    unsorted, negative = hp(np.array([1.0, 0.1])), hp(np.array([-0.1, 1.0]))
    for kw in (dict(T=0), dict(T=9), dict(K=0), dict(K=13), dict(stride=24 * plane - 1), dict(n=0), dict(plane=0), dict(nbytes=need - 1),
               dict(x=null), dict(th=null), dict(counts=null), dict(sums=null), dict(ws=null), dict(th=unsorted), dict(th=negative)):
        assert acc(**kw) == -2, kw
    for a in ((0, plane, T, K), (3, 0, T, K), (3, plane, 0, K), (3, plane, 9, K), (3, plane, T, 0), (3, plane, T, 13)):
        assert lib.rdgan_temporal_workspace_bytes(*a) == -2, a
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((sums == -7.0).all()) and bool((ws == -7).all())           # nothing was launched
    counts.zero_(); sums.zero_()
    assert acc() == 0
    torch.cuda.synchronize()
    agree(TS.stats_from_state(counts.cpu().numpy(), sums.cpu().numpy(), thr, K), tn.temporal_np(x, thr, K), T, K)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_field_equals_structure_of_disaggregate(generator, monkeypatch):
    """40 x 52 at ndomain 16, overlap 4: 12 tiles, one NaN pixel (one bad series per scenario), a dry tile.  The generator's fp32
    output depends in its last bits on the batch it runs in (tests/test_hip_field.py::test_chunking compares with a tolerance), so
    `chunk` is one unit's wet tiles on both sides: every generator batch is then one (scenario, day) whatever scenario_chunk is,
    and the hourly values the two sides see are the same."""
    S, thr, K = 7, (0.1, 0.5, 2.0), 6
    rng = np.random.default_rng(31)
    daily = (rng.gamma(0.8, 6.0, (40, 52)) * (rng.random((40, 52)) < 0.7)).astype(np.float32)
    daily[:16, :16] = 0.0
    daily[20, 30] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(32).normal(size=(S, 1, 100)).astype(np.float32)
    unit_tiles = F.disaggregate(generator, dd, 1, latent=z[:1])[1].n_active
    hourly, info = F.disaggregate(generator, dd, S, latent=z, chunk=unit_tiles)
    assert info.n_nan_pixels == 1 and 0 < info.n_active == unit_tiles < info.n_tiles and hourly.shape == (S, 24, 40, 52)
    want = TS.temporal_structure(hourly, thr, K)
    ref = tn.temporal_np(hourly.cpu().numpy(), thr, K)
    agree(want, ref, 3, K)
    assert want.n_bad == S and want.wet_hours[0, 1:].sum() > 0
    n = tn.terms(ref, 3, K)
    for scenario_chunk in (1, 3, 7):
        got = TS.temporal_structure_field(generator, dd if scenario_chunk == 3 else daily, S, thr, max_lag=K, latent=z,
                                          scenario_chunk=scenario_chunk, chunk=unit_tiles)
        assert got.n_valid == want.n_valid and got.n_bad == want.n_bad
        for name in COUNTS:
            assert np.array_equal(getattr(got, name), getattr(want, name)), (scenario_chunk, name)
        for name in SUMS:
            a, b = getattr(got, name), getattr(want, name)
            assert np.all(np.abs(a - b) <= n[name] * EPS * np.abs(b)), (scenario_chunk, name, np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
    # the default chunk, where the generator batches differ with scenario_chunk: the hourly values then differ as
    # tests/test_hip_field.py grants the whole path across batch splits -- every value within rtol 2e-5 and atol 1e-8 max|x| -- so
    # a sum of n non-negative values moves by at most rtol |sum| + n atol, and a sum of products x y by twice that times max|x|
    # (first order).  wet_amount and the counts may move by whole terms where a value crosses a threshold: not compared.
    rtol, atol = 2e-5, 1e-8 * float(np.nanmax(hourly.cpu().numpy()))
    xmax = max(1.0, float(np.nanmax(hourly.cpu().numpy())))
    one = TS.temporal_structure(F.disaggregate(generator, dd, S, latent=z)[0], thr, K)
    for scenario_chunk in (1, 3):
        got = TS.temporal_structure_field(generator, dd, S, thr, max_lag=K, latent=z, scenario_chunk=scenario_chunk)
        assert got.n_valid == one.n_valid and got.n_bad == one.n_bad == S
        assert np.all(np.abs(got.moments[:, 0] - one.moments[:, 0]) <= rtol * one.moments[:, 0] + n["moments"][:, 0] * atol)
        assert np.all(np.abs(got.moments[:, 1] - one.moments[:, 1]) <= 2 * (rtol * one.moments[:, 1] + n["moments"][:, 1] * atol * xmax))
        assert np.all(np.abs(got.lag - one.lag) <= 2 * (rtol * one.lag + n["lag"] * atol * xmax))
    # the reference-style entry: numpy in, the latent noise from the global numpy RNG; one chunk, so the batches are disaggregate's
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.temporal_structure_field(daily, S, thr, max_lag=K, scenario_chunk=S)
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    b = TS.temporal_structure(hourly2, thr, K)
    assert a.n_valid == b.n_valid and same_bits(a.moments, b.moments)
    for name in COUNTS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_field_on_a_dry_day_draws_nothing():
    class NoGenerator:
        ndomain, n_cond_channels = 16, 1
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    s = TS.temporal_structure_field(NoGenerator(), np.zeros((20, 30), np.float32), 3, (0.1,))
    assert np.array_equal(np.random.get_state()[1], before)           # as disaggregate: without a wet tile no latent is drawn
    assert s.n_valid == 3 * 600 and s.wet_hours[0, 0] == 1800 and s.dry_spell[0, 1, 23] == 1800 and np.all(s.trans[0, :, 0, 0] == 1800)
    assert np.all(s.moments == 0) and np.all(np.isnan(s.autocorrelation()))
