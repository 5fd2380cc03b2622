"""-m gpu: the distribution kernels (rdgan_dist.hip.h) against the reference's own recorded run (tests/golden/ks_*_reference*.npz, made
by tests/golden/make_ks_fixture.py from the CSV / KSpval files the reference's evaluation wrote), against the fp64 mirrors
(tests/dist_np.py), and the two experiment entry points against the per-piece functions they batch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import dist_np as dn

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P_RTOL = 2.3e-15                    # tests/test_distribution_host.py: 10 x the worst error of the host's exact p-value on the 480 recorded ones
EPS = 2.0 ** -52
Q_RTOL = 8 * EPS                    # quartiles, iqr, notches: either lerp form is three fp64 roundings of fp32-exact operands
FENCE_MARGIN = 1e-9                 # no datum may lie this close (relative) to a whisker fence: far above Q_RTOL, far below the 1.2e-5 of the recorded columns
SAMPLE_PAIRS = (0, 10, 16)


def _d():
    from pr_disagg_radar_gan_amd import distribution
    return distribution


def _fields(rng, shape, dry):
    x = (rng.standard_exponential(shape, dtype=np.float32) * np.float32(1.5)) ** 2
    x[rng.random(shape, dtype=np.float32) < dry] = 0.0
    return x


def test_library_exports_the_distribution_symbols():
    from pr_disagg_radar_gan_amd import _lib
    lib = _lib.load()
    for name in ("rdgan_ks_2samp", "rdgan_box_stats", "rdgan_ecdf_workspace_bytes", "rdgan_ecdf_grid"):
        assert name in _lib.SIGNATURES and isinstance(getattr(lib, name), ctypes._CFuncPtr)
    assert lib.rdgan_ecdf_workspace_bytes(512) == 514 * 8 and lib.rdgan_ecdf_workspace_bytes(4097) == -2


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's recorded run
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ks_equals_the_reference_run():
    """The 72 recorded columns: |i - j| EQUAL to the statistic of the reference's run, p within P_RTOL of the p-values it wrote."""
    D = _d()
    ref = np.load(os.path.join(GOLDEN, "ks_pvalues_reference.npz"))
    worst = 0.0
    for k in SAMPLE_PAIRS:
        x = np.load(os.path.join(GOLDEN, f"ks_samples_reference_{k:04d}.npz"))["samples"]
        assert x.shape == (2, 1000, 24) and x.dtype == np.float32
        counts, d = D.ks_statistic_device(x[0], x[1])
        counts = counts.cpu().numpy()[0]
        h = np.abs(counts[:, 0] - counts[:, 1])
        assert np.array_equal(h, ref["h"][k]), (k, h, ref["h"][k])
        stat, p = D.ks_2samp(x[0], x[1])
        assert stat.shape == p.shape == (24,) and np.array_equal(stat, d.cpu().numpy()[0])
        assert np.array_equal(stat, np.abs(counts[:, 0] / 1000 - counts[:, 1] / 1000))
        err = np.abs(p / ref["p"][k] - 1)
        worst = max(worst, err.max())
        print(f"pair {k:04d}: h {h.min()} .. {h.max()}, p {p.min():.3e} .. {p.max()!r}, worst relative error of p {err.max():.2e}")
        assert err.max() <= P_RTOL
    print(f"worst relative error of the 72 p-values: {worst:.2e} (limit {P_RTOL})")


def _assert_box(got, b, c, want, n, x64):
    for f in ("whislo", "whishi", "n_fliers_lo", "n_fliers_hi", "n"):
        assert getattr(got, f)[b, c] == want[f], (f, b, c, getattr(got, f)[b, c], want[f])
    for f in ("q1", "med", "q3", "iqr", "cilo", "cihi"):
        g, w = getattr(got, f)[b, c], want[f]
        assert abs(g - w) <= Q_RTOL * abs(w), (f, b, c, g, w)
    # two fp64 sums of the same n values in different orders: each within (n - 1) 2^-53 sum|x| of the exact sum, so the means differ
    # by at most 2^-52 sum|x| (n >= 2; never above the summation bound n 2^-53 sum|x|); one value: exact
    assert abs(got.mean[b, c] - want["mean"]) <= (EPS * np.abs(x64).sum() if n > 1 else 0.0)


def test_boxplot_stats_equal_the_reference_columns():
    """The 144 recorded columns against matplotlib's recorded values and the mirror."""
    D = _d()
    for k in SAMPLE_PAIRS:
        z = np.load(os.path.join(GOLDEN, f"ks_samples_reference_{k:04d}.npz"))
        x, box = z["samples"], z["box"]
        got = D.boxplot_stats(x)
        assert got.q1.shape == (2, 24) and tuple(got.sorted.shape) == (2, 1000, 24)
        srt = got.sorted.cpu().numpy()
        assert np.array_equal(srt, np.sort(x, axis=1))
        for b in range(2):
            for c in range(24):
                mirror = dn.box_stats(x[b, :, c])
                assert mirror["margin"] > FENCE_MARGIN, (k, b, c, mirror["margin"])
                recorded = dict(zip(dn.STAT_FIELDS, box[b, c]))
                for f in dn.STAT_FIELDS:                              # the mirror itself equals matplotlib, but for the mean's order
                    assert mirror[f] == recorded[f] or (f == "mean" and abs(mirror[f] - recorded[f]) < 1e-15), (f, mirror[f], recorded[f])
                _assert_box(got, b, c, recorded, 1000, x[b, :, c].astype(np.float64))
                _assert_box(got, b, c, mirror, 1000, x[b, :, c].astype(np.float64))
                as_dict = got.column(b, c)                            # the dict boxplot_stats returns
                assert set(as_dict) == {"mean", "q1", "med", "q3", "iqr", "whislo", "whishi", "cilo", "cihi", "fliers"}
                for f in ("whislo", "whishi"):
                    assert as_dict[f] == mirror[f] == recorded[f]
                for f in ("mean", "q1", "med", "q3", "iqr", "cilo", "cihi"):
                    assert as_dict[f] == getattr(got, f)[b, c]
                assert np.array_equal(as_dict["fliers"], got.fliers(b, c)) and len(as_dict["fliers"]) == recorded["n_fliers_lo"] + recorded["n_fliers_hi"]
                fl = got.fliers(b, c)
                assert np.array_equal(fl, np.concatenate([srt[b, :int(recorded["n_fliers_lo"]), c],
                                                          srt[b, 1000 - int(recorded["n_fliers_hi"]):, c]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# KS against the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_ks(D, a, b):
    counts, d = D.ks_statistic_device(a, b)
    want_c, want_d = dn.ks_columns(a, b)
    got_c, got_d = counts.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(got_c, want_c), (a.shape, b.shape, np.argwhere(got_c != want_c)[:4])
    assert np.array_equal(got_d, want_d, equal_nan=True)
    n, m = a.shape[1], b.shape[1]
    ok = got_c[..., 0] >= 0
    assert np.array_equal(got_d[ok], np.abs(got_c[..., 0][ok] / n - got_c[..., 1][ok] / m))
    again_c, again_d = D.ks_statistic_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    assert torch.equal(again_c, counts) and torch.equal(again_d.view(torch.int64), d.view(torch.int64))
    return got_c, got_d


@pytest.mark.parametrize("shape", [(1, 1), (3, 24), (20, 24)])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 7), (7, 2), (7, 7), (1000, 1000), (1000, 1001), (1001, 7), (10000, 10000), (1, 16384),
                                 (16384, 16384), (10000, 16384)])
def test_ks_matches_mirror(n, m, shape):
    D = _d()
    B, C = shape
    rng = np.random.default_rng(100000 * n + 10 * m + B)
    dry = 0.3 + 0.3 * ((n % 7) / 6.0)                                # 30-60 % exact zeros
    a, b = _fields(rng, (B, n, C), dry), _fields(rng, (B, m, C), 0.45)
    if n > 1 and m > 1:
        b[0, : m // 2, 0] = a[0, n // 2, 0]                          # one shared value repeated across both samples
        a[0, : n // 3, 0] = a[0, n // 2, 0]
    _check_ks(D, a, b)


def test_ks_special_columns():
    D = _d()
    rng = np.random.default_rng(3)
    n = 1000
    a = _fields(rng, (1, n, 6), 0.4)
    b = _fields(rng, (1, n, 6), 0.4)
    b[0, :, 0] = a[0, ::-1, 0]                                       # identical samples, another order: D = 0
    b[0, :, 1] = a[0, :, 1] + a[0, :, 1].max() + 1.0                 # disjoint: D = 1
    a[0, :, 2] = 0.25
    b[0, :, 2] = 0.25                                                # one value in both: D = 0
    b[0, :, 3] = -1.0 - b[0, :, 3]                                   # disjoint the other way, negative values
    a[0, 17, 4] = np.nan                                             # a NaN column
    counts, d = _check_ks(D, a, b)
    assert d[0, 0] == 0.0 and d[0, 1] == 1.0 and d[0, 2] == 0.0 and d[0, 3] == 1.0
    assert np.isnan(d[0, 4]) and tuple(counts[0, 4]) == (-1, -1) and np.isnan(d).sum() == 1
    stat, p = D.ks_2samp(a, b)
    assert p[0, 0] == 1.0 and p[0, 2] == 1.0 and p[0, 1] < 1e-300 and np.isnan(p[0, 4]) and np.isnan(stat[0, 4])
    s1, p1 = D.ks_2samp(a[0, :, 5], b[0, :, 5])                      # 1-D input: two floats
    assert isinstance(s1, float) and (s1, p1) == (stat[0, 5], p[0, 5])
    s2, p2 = D.ks_2samp(a[0, :, 5], b[0, :700, 5])                   # n != m: the asymptotic form
    assert p2 == D.ks_pvalue_asymptotic(1000, 700, s2) and 0 < p2 <= 1
    b[0, 3, 5] = np.nan                                              # a NaN in the second sample
    assert np.isnan(D.ks_2samp(a, b)[0][0, 5])


# ---------------------------------------------------------------------------------------------------------------------------------
# box statistics against the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
def _good_seed(first, make):
    """the first seed from `first` on whose columns all keep FENCE_MARGIN from their fences (judged by the mirror alone)"""
    for seed in range(first, first + 50):
        x = make(np.random.default_rng(seed))
        mirrors = [[dn.box_stats(x[b, :, c]) for c in range(x.shape[2])] for b in range(x.shape[0])]
        if all(m["margin"] > FENCE_MARGIN for row in mirrors for m in row):
            return x, mirrors
    raise AssertionError("no seed keeps every column clear of its fences")


@pytest.mark.parametrize("n", [5, 7, 300, 1000, 1001, 10000, 16384])
def test_boxplot_stats_match_mirror(n):
    D = _d()
    B, C = (3, 24) if n <= 1001 else (2, 5)

    def make(rng):
        x = _fields(rng, (B, n, C), 0.2)                             # fewer than a quarter zeros: the iqr is positive
        x[0, :, 0] = rng.standard_normal(n).astype(np.float32)       # a symmetric column with fliers on both sides
        return x
    x, mirrors = _good_seed(1000 * n, make)
    got = D.boxplot_stats(x)
    assert np.array_equal(got.sorted.cpu().numpy(), np.sort(x, axis=1))
    for b in range(B):
        for c in range(C):
            _assert_box(got, b, c, mirrors[b][c], n, x[b, :, c].astype(np.float64))
    for c in range(C):
        col = np.sort(x[0, :, c])
        m = mirrors[0][c]
        assert np.array_equal(got.fliers(0, c), np.concatenate([col[col < m["whislo"]], col[col > m["whishi"]]]))
    again = D.boxplot_stats(torch.from_numpy(x).cuda(), keep_sorted=False)
    assert again.sorted is None
    for f in dn.STAT_FIELDS:
        assert np.array_equal(getattr(again, f), getattr(got, f)), f          # bit-identical on a repeat, with or without the sorted output


def test_boxplot_stats_degenerate_columns():
    D = _d()
    for n in (1, 2, 3, 4):                                           # the degenerate quartile cases
        x = np.array([[3.5, 0.25, 7.0, 1.0][:n], [2.0, 2.0, 2.0, 2.0][:n], [0.1, 0.7, 0.3, 1e-3][:n]], np.float32).T[None]
        got = D.boxplot_stats(x)
        for c in range(3):
            m = dn.box_stats(x[0, :, c])
            assert m["margin"] > FENCE_MARGIN
            _assert_box(got, 0, c, m, n, x[0, :, c].astype(np.float64))
    x = np.full((2, 500, 3), 0.75, np.float32)                       # all-equal columns: iqr 0, whiskers on the value, no fliers
    x[1, 5, 2] = np.nan
    got = D.boxplot_stats(x)
    ok = np.ones((2, 3), bool)
    ok[1, 2] = False
    for f in ("mean", "q1", "med", "q3", "whislo", "whishi", "cilo", "cihi"):
        assert np.all(getattr(got, f)[ok] == 0.75), f
    assert np.all(got.iqr[ok] == 0) and np.all(got.n_fliers_lo[ok] == 0) and np.all(got.n_fliers_hi[ok] == 0) and np.all(got.n == 500)
    for f in dn.STAT_FIELDS[1:]:
        assert np.isnan(getattr(got, f)[1, 2]), f                    # the NaN column
    assert np.isnan(got.sorted[1, :, 2].cpu().numpy()).all() and not np.isnan(got.sorted[1, :, 1].cpu().numpy()).any()
    assert got.fliers(0, 0).shape == (0,) and got.fliers(1, 2).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------------------
# ECDF
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid(rng, T, x):
    """T ascending thresholds: up to three, data values; otherwise three quarters log-spaced and a quarter data values"""
    vals = np.unique(x[~np.isnan(x)])
    if T <= 3:
        return np.sort(rng.choice(vals, T, replace=False)).astype(np.float32)
    g = np.unique(np.concatenate([_d().log_grid(1e-3, 40.0, T - T // 4), rng.choice(vals, T // 4)]))
    return np.unique(np.concatenate([g, np.linspace(41.0, 50.0, T - len(g))]).astype(np.float32))


@pytest.mark.parametrize("T", [1, 2, 512, 4096])
@pytest.mark.parametrize("N", [1, 1023, 2 ** 20 + 3])
def test_ecdf_on_grid_matches_mirror(N, T):
    D = _d()
    rng = np.random.default_rng(7 * N + T)
    x = _fields(rng, (N,), 0.45)
    if N > 100:
        x[rng.integers(0, N, 5)] = np.nan                            # counted apart
        x[rng.integers(0, N, 5)] = -2.0                              # below the first threshold ...
        x[rng.integers(0, N, 5)] = 1e6                               # ... and above the last
    grid = _grid(rng, T, x) if N > 100 else np.linspace(0.0, 3.0, T).astype(np.float32)
    assert len(grid) == T and np.all(np.diff(grid) > 0)
    if N > 100 and T >= 512:
        assert np.isin(grid, x).sum() >= min(T // 8, 100)            # values equal to thresholds
    want, above, n_nan = dn.ecdf_counts(x, grid)
    for data in (x, torch.from_numpy(x).cuda(), torch.from_numpy(np.concatenate([[9.0], x]).astype(np.float32)).cuda()[1:]):
        counts, n_above, got_nan, n = D.ecdf_counts_device(data, grid)         # the last: a view that is not 16-byte aligned
        assert np.array_equal(counts.cpu().numpy(), want) and (n_above, got_nan, n) == (above, n_nan, N)
    counts, y = D.ecdf_on_grid(x, grid)
    assert counts.dtype == np.int64 and np.array_equal(counts, want)
    if N - n_nan > 0:
        assert np.array_equal(y, want / (N - n_nan))


def test_ecdf_at_the_reference_size():
    """10 000 days x 24 x 16 x 16 = 61 440 000 pixels (generate_and_evaluate.py:451), built on the device; the expected counts come
    from the device's exact sort, searched on the host."""
    D = _d()
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.empty(61440000, dtype=torch.float32, device="cuda").exponential_(0.7, generator=g) ** 2
    x[torch.rand(x.shape, generator=g, device="cuda") < 0.5] = 0.0
    x[12345] = float("nan")
    grid = np.unique(np.concatenate([[0.0], D.log_grid(1e-3, 60.0, 512), x[:50].cpu().numpy()])).astype(np.float32)   # with data values
    counts, y = D.ecdf_on_grid(x, grid)
    xs, ys = D.ecdf(x[100000:1100000])                               # (clear of the NaN)
    assert np.array_equal(xs.cpu().numpy(), np.sort(x[100000:1100000].cpu().numpy())) and ys[-1].item() == 1.0
    srt = torch.sort(x).values.cpu().numpy()                         # NaN sorts last
    want = np.searchsorted(srt[:-1], grid, side="right")
    assert np.array_equal(counts, want) and counts[0] > 30000000
    assert np.array_equal(y, want / 61439999)
    again, _ = D.ecdf_on_grid(x, grid)
    assert np.array_equal(again, counts)


def test_ecdf_sorts():
    D = _d()
    rng = np.random.default_rng(2)
    a = _fields(rng, (300, 24), 0.4)
    x, y = D.ecdf(a)
    assert np.array_equal(x.cpu().numpy(), np.sort(a.ravel())) and np.array_equal(y.cpu().numpy(), np.arange(1, a.size + 1) / a.size)
    x2, y2 = D.ecdf(torch.from_numpy(a).cuda())
    assert torch.equal(x, x2) and torch.equal(y, y2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two experiments
# ---------------------------------------------------------------------------------------------------------------------------------
def _real_days(rng, D, nd=16):
    return (rng.gamma(0.3, 2.0, (D, 24, nd, nd)) + 1e-3).astype(np.float32)


def _gen():
    from pr_disagg_radar_gan_amd import gan_train_cwgangp_pixelnorm as T
    T.configure(ndomain=16)
    return T.create_generator(seed=2)


def test_daily_cycle_end_to_end(tmp_path):
    D = _d()
    from pr_disagg_radar_gan_amd import ensemble
    reals = _real_days(np.random.default_rng(0), 40)
    _, ameans = ensemble.generate_one_per_condition(_gen(), reals, seed=3)
    res = D.daily_cycle(ameans)
    assert set(res) == set(D.AMEAN_KEYS)
    for key in D.AMEAN_KEYS:
        one = D.boxplot_stats(ameans[key])
        for f in dn.STAT_FIELDS:
            assert getattr(res[key], f).shape == (1, 24) and np.array_equal(getattr(res[key], f), getattr(one, f)), (key, f)
        assert torch.equal(res[key].sorted, one.sorted)
        m = dn.box_stats(ameans[key][:, 5])
        assert res[key].whishi[0, 5] == m["whishi"] and res[key].n_fliers_hi[0, 5] == m["n_fliers_hi"]
    path = tmp_path / "ameans.csv"
    D.write_ameans_csv(str(path), ameans)
    lines = path.read_text().splitlines()
    assert lines[0] == ",fraction,precip,typ,hour" and len(lines) == 1 + 24 * 2 * 40
    assert lines[1] == f"0,{str(ameans['fraction_gen'][0, 0])},{str(ameans['gen'][0, 0])},generated,1"
    assert lines[41] == f"0,{str(ameans['fraction_real'][0, 0])},{str(ameans['real'][0, 0])},real,1"
    assert lines[-1] == f"39,{str(ameans['fraction_real'][39, 23])},{str(ameans['real'][39, 23])},real,24"
    assert np.float32(lines[1].split(",")[1]) == ameans["fraction_gen"][0, 0]


def test_conditional_distribution_check_end_to_end(tmp_path):
    D = _d()
    from pr_disagg_radar_gan_amd import ensemble
    gen = _gen()
    rng = np.random.default_rng(4)
    conds = [(rng.gamma(0.5, 0.1, (16, 16, 1)).astype(np.float32), rng.gamma(0.5, 0.4, (16, 16, 1)).astype(np.float32)) for _ in range(3)]
    n = 200
    latent = rng.standard_normal((n, 100)).astype(np.float32)
    single = [D.conditional_distribution_check(gen, c1, c2, n_members=n, latent=latent) for c1, c2 in conds]
    for (c1, c2), res in zip(conds, single):
        e1, e2, _ = ensemble.generate_same_noise_pair(gen, c1, c2, n_members=n, latent=latent)
        f1, f2 = e1.mean(dim=(2, 3)), e2.mean(dim=(2, 3))
        assert res.fractions1.shape == (n, 24) and np.array_equal(res.fractions1, f1.cpu().numpy()) and np.array_equal(res.fractions2, f2.cpu().numpy())
        stat, p = D.ks_2samp(f1, f2)
        assert res.pvalue.shape == (24,) and np.array_equal(res.statistic, stat) and np.array_equal(res.pvalue, p)
        want_c, want_d = dn.ks_columns(res.fractions1[None], res.fractions2[None])
        assert np.array_equal(res.statistic, want_d[0])
        for box, f in ((res.box1, f1), (res.box2, f2)):
            one = D.boxplot_stats(f)
            for fld in dn.STAT_FIELDS:
                assert getattr(box, fld).shape == (1, 24) and np.array_equal(getattr(box, fld), getattr(one, fld)), fld
            fr = f.cpu().numpy()
            for hour in (0, 7, 23):                                  # the accessors the box plot of G:600 needs, on a single-pair result
                m = dn.box_stats(fr[:, hour])
                col = np.sort(fr[:, hour])
                want_fl = np.concatenate([col[col < m["whislo"]], col[col > m["whishi"]]])
                assert np.array_equal(box.fliers(0, hour), want_fl)
                as_dict = box.column(0, hour)
                assert set(as_dict) == {"mean", "q1", "med", "q3", "iqr", "whislo", "whishi", "cilo", "cihi", "fliers"}
                assert as_dict["whislo"] == m["whislo"] and as_dict["whishi"] == m["whishi"] and as_dict["med"] == box.med[0, hour]
                assert np.array_equal(as_dict["fliers"], want_fl)
        assert np.array_equal(res.latent, latent)                    # both ensembles share the latent block
    # the same latent under the same condition gives the same ensemble: D = 0, p = 1 in every hour
    same = D.conditional_distribution_check(gen, conds[0][0], conds[0][0], n_members=n, latent=latent)
    assert np.all(same.statistic == 0) and np.all(same.pvalue == 1) and np.array_equal(same.fractions1, same.fractions2)
    # without a latent it is drawn once from the global numpy RNG
    np.random.seed(9)
    drawn = D.conditional_distribution_check(gen, conds[0][0], conds[0][1], n_members=n)
    np.random.seed(9)
    assert np.array_equal(drawn.latent, np.random.normal(size=(n, 100)).astype(np.float32))
    # P pairs in one launch against P single calls
    batched = D.conditional_distribution_checks(gen, conds, n_members=n, latent=latent)
    assert batched.pvalue.shape == (3, 24) and batched.fractions1.shape == (3, n, 24)
    for k, res in enumerate(single):
        assert np.array_equal(batched.pvalue[k], res.pvalue) and np.array_equal(batched.statistic[k], res.statistic)
        assert np.array_equal(batched.fractions1[k], res.fractions1) and np.array_equal(batched.fractions2[k], res.fractions2)
        for fld in dn.STAT_FIELDS:
            assert np.array_equal(getattr(batched.box1, fld)[k], getattr(res.box1, fld)[0]), fld
            assert np.array_equal(getattr(batched.box2, fld)[k], getattr(res.box2, fld)[0]), fld
        for hour in (0, 11, 23):
            assert np.array_equal(batched.box1.fliers(k, hour), res.box1.fliers(0, hour))
            assert np.array_equal(batched.box2.fliers(k, hour), res.box2.fliers(0, hour))
            assert np.array_equal(batched.box2.column(k, hour)["fliers"], res.box2.column(0, hour)["fliers"])
    # the reference's two files
    single[1].write_csv(str(tmp_path / "one.csv"))
    batched.write_csv(str(tmp_path / "batched.csv"), pair=1)
    text = (tmp_path / "one.csv").read_text()
    assert text == (tmp_path / "batched.csv").read_text()
    lines = text.splitlines()
    assert lines[0] == ",fraction,cond,hour" and len(lines) == 1 + 24 * 2 * n
    assert lines[1] == f"0,{str(single[1].fractions1[0, 0])},1,1" and lines[n + 1] == f"0,{str(single[1].fractions2[0, 0])},2,1"
    assert lines[-1] == f"{n - 1},{str(single[1].fractions2[n - 1, 23])},2,24"
    batched.write_pvalues(str(tmp_path / "p.txt"), pair=2)
    assert np.array_equal(np.loadtxt(str(tmp_path / "p.txt")), batched.pvalue[2])
    with pytest.raises(ValueError):
        batched.write_csv(str(tmp_path / "x.csv"))
