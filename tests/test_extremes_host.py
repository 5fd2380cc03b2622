"""CPU tests of the extremes module: the numpy restatement (tests/extremes_np.py) against closed forms, the torch formulas of
ExtremeStats against the restatement on host tensors, and every ValueError of the Python layer, which fires before any device call
(this machine has no device: reaching one would raise RdganError instead)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import extremes as EX
from tests import extremes_np as en


def stats_of(samples, B=None, return_sorted=True):
    """ExtremeStats on host tensors from lists of samples in units (one position each, one series), through the restatement's sums"""
    B = B or max(len(s) for s in samples)
    table = np.full((1, B, len(samples)), -1, np.int64)
    for m, s in enumerate(samples):
        table[0, :len(s), m] = s
    n, A, srt = en.lmoment_sums_np(table)
    return EX.ExtremeStats(None, torch.from_numpy(n), torch.from_numpy(A), 1.0, torch.from_numpy(srt) if return_sorted else None, None), n, A, srt


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 50, 128])
def test_sums_of_1_to_n_give_the_closed_forms(n):
    _, nn, A, srt = stats_of([list(range(n, 0, -1))])
    assert nn[0, 0] == n and srt[0, :, 0].tolist() == list(range(1, n + 1))
    A0, A1, A2 = (int(v) for v in A[0, 0])
    # in rationals: l1 = (n + 1) / 2, l2 = (n + 1) / 6, l3 = 0
    b0 = Fraction(A0, n)
    assert b0 == Fraction(n + 1, 2)
    if n >= 2:
        b1 = Fraction(A1, n * (n - 1))
        assert 2 * b1 - b0 == Fraction(n + 1, 6)
    if n >= 3:
        assert 6 * Fraction(A2, n * (n - 1) * (n - 2)) - 6 * b1 + b0 == 0
    l1, l2, t3 = en.lmoments_np(nn, A, 1.0)
    assert l1[0, 0] == (n + 1) / 2
    assert (abs(l2[0, 0] - (n + 1) / 6) <= 1e-15 * (n + 1) / 6) if n >= 2 else np.isnan(l2[0, 0])
    # l3 = 0 up to the rounding of its terms 6 b2 = 1.5 (n + 1), 6 b1 = 2 (n + 1), b0: some 6 roundings of 2 (n + 1) 2^-53 at most,
    # over l2 = (n + 1) / 6: |t3| <= 72 * 2^-53 = 8e-15
    assert (abs(t3[0, 0]) <= 8e-15) if n >= 3 else np.isnan(t3[0, 0])


def test_equal_values_and_short_samples():
    st, n, A, _ = stats_of([[5000] * 6, [7], [3, 9], [], [4, 4, 10]])
    for l1, l2, t3 in (en.lmoments_np(n, A, 1.0), tuple(t.numpy() for t in st.lmoments())):
        assert l1[0].tolist()[:3] == [5000.0, 7.0, 6.0] and np.isnan(l1[0, 3])
        assert l2[0, 0] == 0.0 and np.isnan(l2[0, 1]) and l2[0, 2] == 3.0 and np.isnan(l2[0, 3])
        assert np.isnan(t3[0, :4]).all() and np.isfinite(t3[0, 4])
    loc, scale = (t.numpy() for t in st.gumbel())
    assert np.isnan(loc[0, [0, 1, 3]]).all() and np.isnan(scale[0, [0, 1, 3]]).all()      # l2 = 0, n = 1, n = 0
    assert scale[0, 2] == 3.0 / math.log(2.0) and loc[0, 2] == 6.0 - en.EULER_GAMMA * scale[0, 2]
    g = [t.numpy() for t in st.gev()]
    assert all(np.isnan(a[0, :4]).all() and np.isfinite(a[0, 4]) for a in g)             # n = 2 is too few for the GEV
    for dist in ("gumbel", "gev"):
        rl = st.return_levels((2, 10), dist).numpy()
        assert rl.shape == (2, 1, 5) and np.isnan(rl[:, 0, [0, 1, 3]]).all() and np.isfinite(rl[:, 0, 4]).all()
    emp = st.return_levels((2, 3.9, 4.1), "empirical").numpy()
    assert emp[0, 0].tolist()[:3] == [5000.0, 7.0, 6.0] and np.isnan(emp[0, 0, 3]) and emp[0, 0, 4] == 4.0
    at = (1.0 - 1.0 / 3.9) * 4                                                           # 2.97: between x_(2) = 4 and x_(3) = 10
    assert emp[1, 0, 0] == 5000.0 and np.isnan(emp[1, 0, 1:4]).all() and abs(emp[1, 0, 4] - (4 + (at - 2) * 6)) < 1e-12
    assert np.isnan(emp[2, 0, 1:]).all()                                                # F = 0.756 lies above n / (n + 1) = 0.75


def test_torch_formulas_equal_the_restatement():
    rng = np.random.default_rng(3)
    samples = [sorted(rng.integers(0, 200000, rng.integers(3, 40)).tolist()) for _ in range(60)]
    st, n, A, srt = stats_of(samples)
    st.unit = 1024.0
    T = (2, 10, 50)
    for got, want in zip(st.lmoments(), en.lmoments_np(n, A)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-13)
    l1, l2, t3 = en.lmoments_np(n, A)
    for got, want in zip(st.gumbel() + st.gev(), en.gumbel_np(l1, l2) + en.gev_np(l1, l2, t3)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12)
    for dist in EX.DISTS:
        np.testing.assert_allclose(st.return_levels(T, dist).numpy(), en.return_levels_np(n, A, T, dist, srt), rtol=1e-12, equal_nan=True)


def test_gumbel_return_level_is_the_closed_form():
    a, b = 31.5, 7.25
    for T in (1.5, 2, 10, 50, 1000):
        want = a - b * math.log(-math.log(1.0 - 1.0 / T))
        assert abs(en.quantile_np(a, b, 0.0, T) - want) <= 1e-14 * abs(want)
        got = float(EX.quantile_level(torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64),
                                      torch.tensor(0.0, dtype=torch.float64), T))
        assert abs(got - want) <= 1e-14 * abs(want)


def test_gev_joins_its_gumbel_limit_at_the_switch():
    """t3 on either side of the switch |k| = 1e-6: parameters and return levels differ by O(k), far below 1e-5"""
    ln23 = math.log(2.0) / math.log(3.0)

    def t3_of(k):                                                    # the inverse of k = 7.8590 c + 2.9554 c^2, c = 2 / (3 + t3) - ln2 / ln3
        c = (-7.8590 + math.sqrt(7.8590 ** 2 + 4 * 2.9554 * k)) / (2 * 2.9554)
        return 2.0 / (c + ln23) - 3.0

    l1, l2 = 40.0, 9.0
    for sign in (1.0, -1.0):
        inner, outer = t3_of(sign * 0.9e-6), t3_of(sign * 1.1e-6)
        a, b = en.gev_np(l1, l2, inner), en.gev_np(l1, l2, outer)
        assert a[2] == 0.0 and abs(b[2] - sign * 1.1e-6) < 1e-9
        t = lambda v: torch.tensor(v, dtype=torch.float64)
        ta, tb = EX.gev_params(t(l1), t(l2), t(inner)), EX.gev_params(t(l1), t(l2), t(outer))
        assert float(ta[2]) == 0.0 and abs(float(tb[2]) - b[2]) < 1e-15
        for T in (2, 10, 50, 1000):
            qa, qb = en.quantile_np(*a, T), en.quantile_np(*b, T)
            assert abs(qa - qb) < 1e-5 * abs(qa)
            # torch against numpy: the same operations inside the switch; outside it the two lgamma(1 + k) may differ by a few
            # 2^-53 in absolute terms, which (1 - Gamma(1 + k)) / k turns into 4 * 2^-53 / 1.1e-6 = 4e-10 in relative ones
            assert abs(float(EX.quantile_level(*ta, T)) - qa) < 1e-13 * abs(qa) and abs(float(EX.quantile_level(*tb, T)) - qb) < 4e-10 * abs(qb)


def test_block_maxima_np_on_a_day_worked_by_hand():
    x = np.zeros((3, 24, 1, 2), np.float32)
    x[0, 5:8, 0, 0] = (1.0, 2.0, 4.0)
    x[1, 23, 0, 0] = 3.0
    x[2, 0, 0, 0] = 5.0                                              # day 2 follows day 1, but no window crosses midnight
    x[1, 3, 0, 1] = np.nan
    bmax, ndays, nvoid = en.block_maxima_np(x, [0, 1, 1], 3, (1, 2, 24))
    assert bmax[:, :, 0, 0].tolist() == [[4096, 6144, 7168], [5120, 5120, 5120], [-1, -1, -1]]
    assert bmax[:, 0, 0, 1].tolist() == [0, 0, -1] and ndays[:, 0].tolist() == [[1, 1], [2, 1], [0, 0]] and nvoid[:, 0].tolist() == [[0, 0], [0, 1], [0, 0]]
    q, bad = en.quantise(np.array([np.nan, np.inf, -1.0, 2048.0, 2047.999, 0.5 / 1024, 1.5 / 1024], np.float32))
    assert bad.tolist() == [True] * 4 + [False] * 3 and q[4:].tolist() == [2047 * 1024 + 1023, 0, 2]


def test_block_maxima_of_depths_keeps_minus_one():
    depths = torch.tensor([[5, -1], [7, -1], [-1, 3], [2, 9]], dtype=torch.int64)
    out = EX.block_maxima_of_depths(depths, [2, 2, 0, 0], 4)
    assert out.tolist() == [[2, 9], [-1, -1], [7, -1], [-1, -1]]
    out = EX.block_maxima_of_depths(depths.view(4, 2, 1), torch.tensor([0, 1, 0, 1]), 2)
    assert out.shape == (2, 2, 1) and out[:, :, 0].tolist() == [[5, 3], [7, 9]]
    for bad in (dict(block=[0, 1, 2]), dict(block=[0, 1, 2, 4]), dict(block=[0.0, 1.0, 2.0, 3.0]), dict(depths=depths.to(torch.int32))):
        with pytest.raises(ValueError):
            EX.block_maxima_of_depths(**{**dict(depths=depths, block=[0, 1, 2, 3], n_blocks=4), **bad})


def test_every_value_error_fires_before_any_device_call():
    x = np.zeros((3, 24, 2, 2), np.float32)
    bm = EX.BlockMaxima((1, 24), 4)
    for block in ([0, 1, 4], [0, -1, 1], [0, 1], [0, 1, 2, 3], [[0, 1, 2]], [0.0, 1.0, 2.0], torch.tensor([0, 1, 5])):
        with pytest.raises(ValueError):
            bm.add(x, block)
    for windows in ((), (0, 1), (1, 25), (3, 3), (6, 1), tuple(range(1, 10)), (1.5,)):
        with pytest.raises(ValueError):
            EX.BlockMaxima(windows, 4)
        with pytest.raises(ValueError):
            EX.extremes(x, [0, 1, 2], 4, windows)
    for kw in (dict(n_blocks=0), dict(n_blocks=2.0), dict(n_blocks=4, days_per_run=0), dict(n_blocks=4, days_per_run=4097)):
        with pytest.raises(ValueError):
            EX.BlockMaxima((1,), **kw)
    with pytest.raises(ValueError):
        bm.add(torch.zeros((3, 24, 2, 2)), [0, 1, 2])                # a torch tensor on the host
    with pytest.raises(ValueError):
        bm.add(np.zeros((3, 23, 2, 2), np.float32), [0, 1, 2])
    with pytest.raises(ValueError):
        EX.BlockMaxima((1, 2), 1 << 20).add(np.zeros((1, 24, 64, 64), np.float32), [0])       # NB K P above 2^31
    with pytest.raises(ValueError):
        bm.state()
    # extremes: n_blocks = series * B, B <= 128
    for kw in (dict(n_blocks=4, series=3), dict(n_blocks=258, series=2), dict(n_blocks=4, series=0), dict(n_blocks=4, min_days=-1)):
        with pytest.raises(ValueError):
            EX.extremes(x, [0, 1, 2], **{**dict(windows=(1,)), **kw})
    # lmoment_sums
    table = np.arange(24, dtype=np.int64).reshape(2, 3, 4)
    big = table.copy()
    big[1, 2, 3] = 1 << 40
    for kw in (dict(table=np.zeros((1, 129, 2), np.int64)), dict(table=big), dict(table=table.astype(np.float64)), dict(table=torch.from_numpy(table)),
               dict(table=table[0]), dict(table=np.zeros((1, 0, 2), np.int64)), dict(table=table, ndays=np.ones((2, 3, 5), np.int32)),
               dict(table=table, ndays=np.ones((2, 3, 4))), dict(table=table, min_days=-1), dict(table=table, min_days=1.5)):
        with pytest.raises(ValueError):
            EX.lmoment_sums(**kw)
    # ExtremeStats
    st = stats_of([[1, 2, 3, 4]], return_sorted=False)[0]
    for T in (1, 0.5, (2, 1.0), (), np.nan, np.inf):
        with pytest.raises(ValueError):
            st.return_levels(T)
    with pytest.raises(ValueError):
        st.return_levels((2,), "weibull")
    with pytest.raises(ValueError):
        st.return_levels((2,), "empirical")                          # no sorted maxima
    wide = EX.ExtremeStats(None, torch.full((4097, 1), 4, dtype=torch.int32), torch.ones((4097, 1, 3), dtype=torch.int64), 1.0, None, None)
    with pytest.raises(ValueError):
        wide.band((2,), (0.5,))
    for probs in ((), (1.5,), (0.5, -0.1)):
        with pytest.raises(ValueError):
            st.band((2,), probs)
    two = EX.ExtremeStats(None, torch.full((2, 1), 4, dtype=torch.int32), torch.ones((2, 1, 3), dtype=torch.int64), 1.0, None, None)
    for kw in (dict(obs=two), dict(obs=None), dict(probs=(0.5,)), dict(probs=(0.9, 0.1)), dict(T=1.0)):
        with pytest.raises(ValueError):
            EX.compare(**{**dict(obs=st, gen=two, T=(2,)), **kw})


class _Gen:
    ndomain = 16
    n_cond_channels = 1


def test_extremes_field_checks_its_arguments_on_the_host(monkeypatch):
    daily = np.ones((4, 16, 16), np.float32)
    ok = dict(gen=_Gen(), daily=daily, n_scenarios=3, block=[0, 0, 1, 1], n_blocks_per_member=2, windows=(1, 24))
    for kw in (dict(block=[0, 1, 2, 1]), dict(block=[0, 0, 1]), dict(n_blocks_per_member=129), dict(n_blocks_per_member=0), dict(windows=(24, 1)),
               dict(n_scenarios=0), dict(scenario_chunk=0), dict(min_days=-1), dict(daily=np.ones((4, 8, 16), np.float32)),
               dict(daily=torch.ones((4, 16, 16))), dict(latent_mode="x")):
        with pytest.raises(ValueError):
            EX.extremes_field(**{**ok, **kw})
    from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
    monkeypatch.setattr(P, "gen", _Gen())
    with pytest.raises(ValueError):
        P.extremes_field(daily, 3, [0, 1, 2, 1], 2)
