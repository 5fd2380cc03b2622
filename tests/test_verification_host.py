"""Host side of the verification of field ensembles (pr_disagg_radar_gan_amd/verification.py): the numpy restatement
(tests/verify_np.py) against brute-force loops and closed forms, its tie, bin and NaN rules, additivity of the state, the host
methods of Verification, the argument errors of every Python entry (raised before the device is touched) and -2 from every C
entry.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, verification as V
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import verify_np as vn

THR = (0.1, 1.0, 5.0)


def gamma_case(seed, S=6, shape=(2, 24, 4, 7)):
    """gamma hours with many exact zeros, in members and observation alike"""
    rng = np.random.default_rng(seed)
    draw = lambda sh: (rng.gamma(0.4, 3.0, sh) * (rng.random(sh) < 0.45)).astype(np.float32)
    return draw((S,) + shape), draw(shape)


def test_package_exports_the_module():
    import pr_disagg_radar_gan_amd
    assert pr_disagg_radar_gan_amd.verification is V


def test_hash_restates_the_header_constants():
    """fixed words of the mixer (computed by hand from rdgan_rng.h's definition with Python integers)"""
    def mix(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
        return x
    for seed, p in ((0, 0), (1, 5), (2 ** 40 + 17, 2 ** 33 + 3), (2 ** 64 - 1, 2 ** 40 - 1)):
        key = (mix((seed & 0xFFFFFFFF) ^ mix((seed >> 32) ^ 0x9E3779B9)) + 8 * 0x85EBCA6B) & 0xFFFFFFFF
        mk = mix(key ^ mix((p & 0xFFFFFFFF) ^ mix((p >> 32) ^ 0x9E3779B9)))
        assert int(vn.b24(seed, np.array([p], dtype=np.int64))[0]) == mix(mix(0) ^ mk) >> 8


def test_restatement_against_brute_force():
    x, o = gamma_case(1)
    x[3, 1, 7, 2, 5] = np.nan
    o[0, 3, 0, 0] = np.nan
    widths, n_bins, seed, S = (1, 3, 9), 4, 11, x.shape[0]          # width 9 is wider than the 4 x 7 field
    st, rank_hist, rel, brier, fsum = vn.verify(x, o, THR, widths, n_bins, seed)
    exceed, below, equal, bad = st
    thr = np.asarray(THR, np.float32)
    D, _, ny, nx = o.shape
    rh = np.zeros_like(rank_hist); rl = np.zeros_like(rel); br = np.zeros_like(brier); fs = np.zeros_like(fsum)
    p = 0
    for d in range(D):
        for h in range(24):
            for y in range(ny):
                for xx in range(nx):
                    col, ob = x[:, d, h, y, xx], o[d, h, y, xx]
                    isbad = np.isnan(ob) or np.isnan(col).any()
                    assert bad[d, h, y, xx] == isbad
                    with np.errstate(invalid="ignore"):
                        nb, ne = int((col < ob).sum()), int((col == ob).sum())
                    assert below[d, h, y, xx] == nb and equal[d, h, y, xx] == ne
                    if not isbad:
                        r = nb + ((int(vn.b24(seed, np.array([p]))[0]) * (ne + 1)) >> 24)
                        rh[h, r] += 1
                        for t in range(3):
                            c, e = int((col > thr[t]).sum()), int(ob > thr[t])
                            assert exceed[t, d, h, y, xx] == c
                            rl[t, h, c * n_bins // (S + 1)] += (1, e, c)
                            br[t, h] += (1, e, c * e, c * c)
                    p += 1
    assert np.array_equal(rh, rank_hist) and np.array_equal(rl, rel) and np.array_equal(br, brier)
    ok = (bad == 0)
    for t in range(3):
        C = np.where(ok, exceed[t], 0).astype(np.int64)
        E = np.where(ok, np.nan_to_num(o) > thr[t], 0).astype(np.int64)
        for i, w in enumerate(widths):
            r = w // 2
            for d in range(D):
                for h in range(24):
                    for y in range(ny):
                        for xx in range(nx):
                            bc = be = 0
                            for yy in range(max(y - r, 0), min(y + r, ny - 1) + 1):
                                for xb in range(max(xx - r, 0), min(xx + r, nx - 1) + 1):
                                    bc += C[d, h, yy, xb]; be += E[d, h, yy, xb]
                            fs[t, i, h] += ((bc - S * be) ** 2, bc ** 2 + (S * be) ** 2)
    assert np.array_equal(fs, fsum)


def test_members_equal_to_the_observation():
    _, o = gamma_case(2)
    S = 5
    x = np.broadcast_to(o, (S,) + o.shape)
    st, rank_hist, rel, brier, fsum = vn.verify(x, o, THR, (1, 3, 5), 6, 0)
    assert not st[1].any() and np.all(st[2] == S)
    r = vn.ranks(st[1], st[2], 0)
    assert r.min() >= 0 and r.max() <= S and rank_hist.sum() == o.size
    bs, base, bss = vn.brier_score(brier.sum(axis=1), S)
    assert np.all(bs == 0)
    f = vn.fss(fsum.sum(axis=2))
    assert np.all(f[~np.isnan(f)] == 1.0) and np.all(fsum[..., 0] == 0)
    v = V.Verification(THR, (1, 3, 5), S, o.size, rank_hist, rel, brier, fsum)
    assert np.all(v.brier()[0] == 0) and np.array_equal(v.fss(), f, equal_nan=True)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_displaced_one_pixel_event(k):
    """forecast (all S members) at (10, 10), observed at (10, 10 + k), boxes never clipped: a pixel's box holds the forecast pixel
    for w^2 pixels, the observed one for w^2, both for w max(w - k, 0): num = S^2 (2 w^2 - 2 w max(w - k, 0)), den = 2 S^2 w^2, so
    FSS = max(w - k, 0) / w"""
    S, widths = 3, (1, 3, 5, 9)
    o = np.zeros((24, 21, 25), np.float32)
    x = np.zeros((S,) + o.shape, np.float32)
    o[7, 10, 10 + k] = 2.0
    x[:, 7, 10, 10] = 2.0
    st = vn.state(x, o, (1.0,))
    fsum = vn.fss_sums(o, st[0], st[3], S, (1.0,), widths)
    for i, w in enumerate(widths):
        ov = w * max(w - k, 0)
        assert fsum[0, i, 7].tolist() == [S * S * (2 * w * w - 2 * ov), 2 * S * S * w * w]
        assert vn.fss(fsum)[0, i, 7] == 1.0 - (2 * w * w - 2 * ov) / (2 * w * w)
        if w <= k:
            assert vn.fss(fsum)[0, i, 7] == 0.0
    assert np.all(fsum[0, :, 6] == 0) and np.isnan(vn.fss(fsum)[0, 0, 6])          # an hour without any event: 0 / 0
    assert vn.fss(fsum)[0, 2, 7] == pytest.approx(max(5 - k, 0) / 5)


def test_rank_between_distinct_members():
    x = np.array([0.5, 4.0, 1.5, 3.0, 0.1, 2.0], np.float32).reshape(6, 1, 1, 1) * np.ones((6, 24, 1, 1), np.float32)
    o = np.full((24, 1, 1), 1.75, np.float32)                      # between the 3rd (1.5) and the 4th (2.0)
    st = vn.state(x, o, (1.0,))
    for seed in range(5):
        assert np.all(vn.ranks(st[1], st[2], seed) == 3)
    rank_hist, _, _ = vn.reduce(o, st, 6, (1.0,), 2, 0)
    assert np.all(rank_hist[:, 3] == 1) and rank_hist.sum() == 24


def test_tied_ranks_stay_in_range_and_fill_the_bins():
    """2^16 dry positions, S = 8 dry members: every rank is a draw from 0 .. 8.  The seed was picked on the CPU so that the
    restatement passes; chi-square against the 99.9 % point for 8 degrees of freedom (26.124)."""
    S, n = 8, 1 << 16
    below, equal = np.zeros(n, np.int32), np.full(n, S, np.int32)
    r = vn.ranks(below, equal, seed=0)
    assert r.min() == 0 and r.max() == S
    counts = np.bincount(r, minlength=S + 1)
    chi2 = float(((counts - n / (S + 1)) ** 2 / (n / (S + 1))).sum())
    print("chi2", chi2)
    assert chi2 < 26.124
    below2, equal2 = np.full(n, 2, np.int32), np.full(n, 3, np.int32)            # partial ties: 2 below, 3 equal
    r2 = vn.ranks(below2, equal2, seed=0)
    assert r2.min() == 2 and r2.max() == 5
    assert not np.array_equal(vn.ranks(below, equal, seed=1), r)               # the seed matters
    assert np.array_equal(vn.ranks(below[100:200], equal[100:200], 0, first=100), r[100:200])      # ... and the position, nothing else


def test_bin_formula_at_its_ends():
    o = np.full((24, 1, 3), 2.0, np.float32)
    for S, n_bins in ((10, 11), (10, 4), (1, 2), (63, 64)):
        x = np.zeros((S,) + o.shape, np.float32)
        x[:, :, 0, 1] = 3.0                                         # c = 0, S, 0 at the three pixels
        st = vn.state(x, o, (1.0,))
        _, rel, _ = vn.reduce(o, st, S, (1.0,), n_bins, 0)
        assert rel[0, :, 0, 0].tolist() == [2] * 24 and rel[0, :, n_bins - 1].tolist() == [[1, 1, S]] * 24
        assert rel[0].sum(axis=(0, 1)).tolist() == [72, 72, 24 * S]
    S = n_bins_less_one = 5                                         # S = n_bins - 1: bin == c
    x = np.zeros((S, 24, 1, 6), np.float32)
    for c in range(6):
        x[:c, :, 0, c] = 3.0
    o6 = np.zeros((24, 1, 6), np.float32)
    _, rel, _ = vn.reduce(o6, vn.state(x, o6, (1.0,)), S, (1.0,), n_bins_less_one + 1, 0)
    assert rel[0, 0, :, 0].tolist() == [1] * 6 and rel[0, 0, :, 2].tolist() == list(range(6))


def test_nan_rules():
    x, o = gamma_case(4, S=4, shape=(24, 2, 3))
    o[5, 1, 2] = np.nan
    x[2, 9, 0, 1] = np.nan
    x[[0, 3], 9, 0, 1] = 0.0
    x[1, 9, 0, 1] = 7.0
    exceed, below, equal, bad = vn.state(x, o, THR)
    assert bad.sum() == 2 and bad[5, 1, 2] == 1 and bad[9, 0, 1] == 1
    assert below[5, 1, 2] == 0 and equal[5, 1, 2] == 0              # a NaN observation: every comparison is false
    assert exceed[2, 9, 0, 1] == 1                                  # the NaN member counts nowhere, the others still do
    rank_hist, rel, brier = vn.reduce(o, (exceed, below, equal, bad), 4, THR, 5, 0)
    assert rank_hist.sum() == o.size - 2 and np.all(brier[:, :, 0].sum(axis=1) == o.size - 2)
    assert rank_hist[5].sum() == 5 and rank_hist[9].sum() == 5
    fs = vn.fss_sums(o, exceed, bad, 4, THR, (1,))
    x2, o2 = x.copy(), o.copy()
    x2[:, 9, 0, 1] = 0.0; o2[9, 0, 1] = 0.0; x2[:, 5, 1, 2] = 0.0; o2[5, 1, 2] = 0.0      # a bad position is a dry one to the FSS
    st2 = vn.state(x2, o2, THR)
    assert np.array_equal(fs, vn.fss_sums(o2, st2[0], st2[3], 4, THR, (1,)))


def test_state_is_additive():
    x, o = gamma_case(5, S=8)
    x[6, 0, 3, 1, 1] = np.nan
    whole = vn.state(x, o, THR)
    parts = vn.add_states(vn.state(x[:3], o, THR), vn.state(x[3:], o, THR))
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))


def test_verification_host_methods():
    x, o = gamma_case(6, S=6)
    widths = (1, 3)
    _, rank_hist, rel, brier, fsum = vn.verify(x, o, THR, widths, 7, 3)
    v = V.Verification(THR, widths, 6, int(brier[0, :, 0].sum()), rank_hist, rel, brier, fsum)
    assert v.rank_histogram().shape == (7,) and v.rank_histogram().sum() == o.size
    assert np.array_equal(v.rank_histogram(by_hour=True), rank_hist)
    bs, base, bss = v.brier()
    # against the definition: the mean of (c / S - e)^2
    st = vn.state(x, o, THR)
    for t, th in enumerate(np.asarray(THR, np.float32)):
        pr, e = st[0][t] / 6.0, (o > th).astype(np.float64)
        assert bs[t] == pytest.approx(((pr - e) ** 2).mean(), rel=1e-12)
        assert base[t] == pytest.approx(e.mean(), rel=1e-12)
        assert bss[t] == pytest.approx(1 - ((pr - e) ** 2).mean() / (e.mean() * (1 - e.mean())), rel=1e-12)
    assert v.brier(by_hour=True)[0].shape == (3, 24)
    fc, ob, n = v.reliability_curve(1)
    assert n.sum() == o.size and fc.shape == (7,) and np.nanmax(fc) <= 1.0 and np.nanmin(ob) >= 0.0
    assert v.fss().shape == (3, 2) and v.fss(by_hour=True).shape == (3, 2, 24)
    assert np.array_equal(v.fss(), vn.fss(fsum.sum(axis=2)), equal_nan=True)
    with pytest.raises(ValueError):
        v.reliability_curve(3)
    dry = V.Verification((1.0,), (1,), 2, 0, np.zeros((24, 3), np.int64), np.zeros((1, 24, 2, 3), np.int64),
                         np.zeros((1, 24, 4), np.int64), np.zeros((1, 1, 24, 2)))
    assert np.isnan(dry.brier()[0][0]) and np.isnan(dry.brier()[2][0]) and np.isnan(dry.fss()[0, 0])


@pytest.mark.parametrize("bad", [(), (1,) * 9, (-0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (1.0, np.nan), (1.0, np.inf), (1e39,), ((1.0,),),
                                 (1.0, 1.0 + 1e-9), "ab"])
def test_check_event_thresholds_refuses(bad):
    with pytest.raises(ValueError):
        V.check_event_thresholds(bad)


def test_check_event_thresholds_rounds_once():
    t = V.check_event_thresholds((0, 0.1, 1))
    assert t.dtype == np.float64 and t.tolist() == [0.0, float(np.float32(0.1)), 1.0]


@pytest.mark.parametrize("bad", [(), (1,) * 9, (2,), (0, 1), (-1, 1), (3, 3), (5, 3), (1.5,), ((1,),), (np.nan,), (100001,)])
def test_check_scales_refuses(bad):
    with pytest.raises(ValueError):
        V.check_scales(bad)


def test_check_scales_bound():
    assert V.check_scales((1, 3.0, 65), 4096).tolist() == [1, 3, 65]
    assert V.check_scales((127,), 4096).dtype == np.int32           # 4096 * 127^2 < 2^26
    with pytest.raises(ValueError):
        V.check_scales((129,), 4096)                                # 4096 * 129^2 >= 2^26
    assert V.check_scales((8191,), 1).tolist() == [8191]
    with pytest.raises(ValueError):
        V.check_scales((8193,), 1)


class _Gen:
    ndomain, n_cond_channels = 16, 1


def _bare_verifier(shape=(24, 3, 4), n_members=0, T=1):
    """an EnsembleVerifier as its constructor leaves it, without the device: for the checks add() and result() make first"""
    v = V.EnsembleVerifier.__new__(V.EnsembleVerifier)
    v.thr, v.shape, v.n_members = np.ones(T), shape, n_members
    v.P, v.ny, v.nx = int(np.prod(shape)), shape[-2], shape[-1]
    return v


def test_python_entries_refuse_bad_arguments_before_the_device():
    o = np.zeros((24, 20, 30), np.float32)
    for obs in (np.zeros((23, 4, 4)), np.zeros((4, 4)), np.zeros((24, 0, 4)), torch.zeros(24, 4, 4), np.zeros((24, 2, 2), dtype="U1")):
        with pytest.raises(ValueError):
            V.EnsembleVerifier(obs, (1.0,))
    with pytest.raises(ValueError):
        V.EnsembleVerifier(o, (1.0, 0.5))
    v = _bare_verifier()
    for members in (np.zeros((2, 24, 3, 5), np.float32), np.zeros((24, 3, 4), np.float32), torch.zeros(2, 24, 3, 4, dtype=torch.float64),
                    torch.zeros(2, 24, 4, 3).transpose(2, 3), np.zeros((0, 24, 3, 4), np.float32), np.zeros((4097, 24, 1, 1), np.float32)):
        with pytest.raises(ValueError):
            (v if members.shape[-1] != 1 else _bare_verifier((24, 1, 1))).add(members)
    with pytest.raises(ValueError, match="at most 4096"):
        _bare_verifier(n_members=4090).add(np.zeros((7, 24, 3, 4), np.float32))
    with pytest.raises(ValueError, match="no member"):
        v.result()
    full = _bare_verifier(n_members=10)
    for kw in (dict(scales=(2,)), dict(n_bins=1), dict(n_bins=12), dict(n_bins=2.5), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5),
               dict(scales=(2601,))):
        with pytest.raises(ValueError):
            full.result(**kw)
    with pytest.raises(ValueError):
        _bare_verifier(n_members=100).result(n_bins=65)
    ens = np.zeros((3,) + o.shape, np.float32)
    for args, kw in (((ens, o[:, :19], (1.0,)), {}), ((ens, o, ()), {}), ((o, o, (1.0,)), {}), ((ens, o, (1.0,)), dict(n_bins=5)),
                     ((ens, o, (1.0,)), dict(n_bins=4, scales=(4,))), ((ens, o, (1.0,)), dict(n_bins=4, rank_seed=0)),
                     ((ens, o, (1.0,)), dict(n_bins=4, seed=-3)), ((ens, o, (1.0,)), {})):
        with pytest.raises(ValueError):
            V.verify_hourly(*args, **kw)
    good = dict(gen=_Gen(), observed=o, n_scenarios=4, thresholds=(1.0,), n_bins=4)
    for kw in (dict(thresholds=(1.0, 1.0)), dict(n_scenarios=0), dict(n_scenarios=4097), dict(scales=(1, 2)), dict(n_bins=6),
               dict(rank_seed=-1), dict(scenario_chunk=0), dict(observed=o[:, :15]), dict(observed=o[0]), dict(observed=o[None, None]),
               dict(observed=torch.zeros(24, 20, 30)), dict(daily=np.zeros((20, 31), np.float32)), dict(overlap=9),
               dict(latent_mode="each"), dict(latent=np.zeros((4, 2, 100), np.float32)), dict(chunk=0), dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            V.verify_field(**{**good, **kw})
    if not torch.cuda.is_available():                               # valid arguments reach the device: there is no CPU fallback
        with pytest.raises(_lib.RdganError):
            V.EnsembleVerifier(o, (1.0,))
        with pytest.raises(_lib.RdganError):
            V.verify_hourly(ens, o, (1.0,), n_bins=4)
        with pytest.raises(_lib.RdganError):
            V.verify_field(**good)


def test_host_torch_tensors_are_refused():
    """a torch tensor on the host is no input of add(): its copy to the device would be dense, and the strides of a view of a wider
    buffer (a member stride above P) would no longer describe it.  numpy arrays are made dense on the host first."""
    v = _bare_verifier()
    dense = torch.zeros(2, 24, 3, 4)
    wide = torch.zeros(2, 24 * 3 * 4 + 3)[:, :24 * 3 * 4].view(2, 24, 3, 4)
    assert wide.stride(0) == 24 * 3 * 4 + 3
    for members in (dense, wide):
        with pytest.raises(ValueError, match="on the host"):
            v.add(members)
    assert v.n_members == 0
    with pytest.raises(ValueError, match="on the host"):
        V.verify_hourly(torch.zeros(3, 24, 20, 30), np.zeros((24, 20, 30), np.float32), (1.0,), n_bins=4)


def test_pretrained_entry_checks_before_loading_anything(monkeypatch):
    monkeypatch.setattr(P, "gen", _Gen())
    o = np.zeros((24, 20, 30), np.float32)
    for kw in (dict(thresholds=(2.0, 1.0)), dict(scales=(2,)), dict(n_bins=40), dict(overlap=10), dict(latent_mode="x")):
        with pytest.raises(ValueError):
            P.verify_scenarios_field(**{**dict(observed=o, n_scenarios=5, thresholds=(1.0,), n_bins=6), **kw})
    with pytest.raises(ValueError):
        P.verify_scenarios_field(o[:, :10], 5, (1.0,), n_bins=6)


def test_c_entries_refuse_bad_arguments():
    """-2 before any HIP call: checkable without a GPU.  The device pointers are never followed."""
    lib = _lib.load()
    d = ctypes.c_void_p(1 << 20)                                    # stands for a device pointer (16-byte aligned)
    null = ctypes.c_void_p(0)
    thr = np.array([0.1, 1.0], np.float64)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def acc(members=d, n=4, stride=480, P=480, obs=d, th=thr, T=2, exceed=d, below=d, equal=d, bad=d):
        return lib.rdgan_verify_accumulate(members, n, stride, P, obs, hp(th) if th is not None else null, T, exceed, below, equal, bad, null)

    for kw in (dict(members=null), dict(obs=null), dict(exceed=null), dict(below=null), dict(equal=null), dict(bad=null), dict(th=None),
               dict(n=0), dict(n=4097), dict(P=0), dict(stride=479), dict(T=0), dict(T=9), dict(th=np.array([1.0, 1.0])),
               dict(th=np.array([2.0, 1.0])), dict(th=np.array([-1.0, 1.0])), dict(th=np.array([0.0, np.nan])),
               dict(th=np.array([0.0, np.inf])), dict(th=np.array([1.0, 1.0 + 1e-12])), dict(members=ctypes.c_void_p((1 << 20) + 2))):
        assert acc(**kw) == -2, kw

    def red(obs=d, exceed=d, below=d, equal=d, bad=d, P=480, plane=20, S=4, th=thr, T=2, n_bins=5, rank=d, rel=d, brier=d):
        return lib.rdgan_verify_reduce(obs, exceed, below, equal, bad, P, plane, S, hp(th) if th is not None else null, T, n_bins, 0, rank,
                                       rel, brier, null)

    for kw in (dict(obs=null), dict(exceed=null), dict(below=null), dict(equal=null), dict(bad=null), dict(rank=null), dict(rel=null),
               dict(brier=null), dict(th=None), dict(S=0), dict(S=4097), dict(n_bins=1), dict(n_bins=6), dict(S=100, n_bins=65), dict(T=0),
               dict(T=9), dict(plane=0), dict(P=0), dict(P=481), dict(plane=7), dict(plane=481), dict(th=np.array([1.0, 0.5]))):
        assert red(**kw) == -2, kw

    assert lib.rdgan_verify_fss_workspace_bytes(5, 67, 2, 3) == 24 * 2 * 2 * 3 * 2 * 8 + 2 * 24 * 2 * 5 * 67 * 4
    for args in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 9, 1), (5, 5, 1, 0), (5, 5, 1, 9)):
        assert lib.rdgan_verify_fss_workspace_bytes(*args) == -2, args
    wd = np.array([1, 3, 9], np.int32)
    need = lib.rdgan_verify_fss_workspace_bytes(5, 67, 2, 3)

    def fss(obs=d, exceed=d, bad=d, days=2, ny=5, nx=67, S=8, th=thr, T=2, w=wd, W=3, out=d, ws=d, nbytes=need):
        return lib.rdgan_verify_fss(obs, exceed, bad, days, ny, nx, S, hp(th) if th is not None else null, T,
                                    hp(w) if w is not None else null, W, out, ws, nbytes, null)

    for kw in (dict(obs=null), dict(exceed=null), dict(bad=null), dict(out=null), dict(ws=null), dict(th=None), dict(w=None), dict(days=0),
               dict(ny=0), dict(nx=0), dict(S=0), dict(S=4097), dict(T=0), dict(T=9), dict(W=0), dict(W=9), dict(nbytes=need - 1),
               dict(w=np.array([1, 2, 9], np.int32)), dict(w=np.array([3, 1, 9], np.int32)), dict(w=np.array([1, 3, 3], np.int32)),
               dict(w=np.array([-1, 3, 9], np.int32)), dict(S=4096, w=np.array([1, 3, 129], np.int32)),
               dict(th=np.array([1.0, 1.0])), dict(ws=ctypes.c_void_p((1 << 20) + 4))):
        assert fss(**kw) == -2, kw
