"""CPU tests of whole-field disaggregation (pr_disagg_radar_gan_amd/field.py): the tile plan and its weights against the rules and
the numpy restatement (tests/field_np.py), the argument errors raised before any device call, and the restatement's own mass
conservation around a fake generator."""
import itertools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F
from pr_disagg_radar_gan_amd import weights as W
from tests import field_np as fn

ULP_BELOW_ONE = 2.0 ** -24


def _axis_cases():
    for nd in (8, 16):
        for overlap in (0, 1, 4, nd // 2):
            for L in (nd, nd + 1, 2 * nd - overlap, 2 * nd - overlap + 2, 37, 64):
                yield L, nd, overlap


@pytest.mark.parametrize("L,nd,overlap", sorted(set(_axis_cases())))
def test_axis_plan_properties(L, nd, overlap):
    plan = F.tile_plan(L, nd, nd, overlap)               # y axis of length L, x axis a single tile
    o = plan.y_origins.tolist()
    assert o == fn.origins_1d(L, nd, overlap)
    s = nd - overlap
    regular = [k * s for k in range(L) if k * s + nd <= L]
    assert o[:len(regular)] == regular and o[-1] == L - nd and len(o) in (len(regular), len(regular) + 1)
    assert plan.x_origins.tolist() == [0] and plan.n_tiles == len(o)
    cover = fn.cover_1d(L, nd, o)
    for y in range(L):
        idx, w = plan.ytab_idx[y], plan.ytab_w[y]
        k = int((idx >= 0).sum())
        assert 1 <= k <= 3                               # every coordinate is covered, by at most 3 tiles
        assert np.all(idx[k:] == -1) and np.all(w[k:] == 0)
        tiles = idx[:k].tolist()
        assert tiles == sorted(tiles) == [i for i, oo in enumerate(o) if oo <= y < oo + nd]
        assert [(i, ww) for i, ww in zip(tiles, w[:k])] == [(i, np.float32(ww)) for i, ww in cover[y]]      # the restatement's, rounded once
        assert w.dtype == np.float32 and np.all(w[:k] > 0)
        assert abs(float(np.sum(w[:k].astype(np.float64))) - 1.0) <= k * ULP_BELOW_ONE
        if k == 1:
            assert w[0] == np.float32(1.0)
    assert np.all(plan.xtab_idx[:, 0] == 0) and np.all(plan.xtab_w[:, 0] == 1.0)
    if overlap == 0 and L % nd == 0:                     # a partition
        assert o == list(range(0, L, nd))
        assert np.all((plan.ytab_idx >= 0).sum(1) == 1) and np.all(plan.ytab_w[:, 0] == 1.0)


def test_triple_cover_case():
    plan = F.tile_plan(16, 30, 16, 4)
    assert plan.x_origins.tolist() == [0, 12, 14] and plan.y_origins.tolist() == [0]
    assert (plan.n_ty, plan.n_tx, plan.n_tiles) == (1, 3, 3)
    assert plan.origins().tolist() == [[0, 0], [0, 12], [0, 14]]
    n_cover = (plan.xtab_idx >= 0).sum(1)
    assert n_cover.tolist() == [1] * 12 + [2] * 2 + [3] * 2 + [2] * 12 + [1] * 2
    # x = 14: tile 0 (p = min(15, 2) = 2), tile 1 (p = min(3, 14) = 3), tile 2 (p = min(1, 16) = 1)
    assert plan.xtab_idx[14].tolist() == [0, 1, 2]
    assert plan.xtab_w[14].tolist() == [np.float32(2 / 6), np.float32(3 / 6), np.float32(1 / 6)]
    # x = 20: tile 1 (p = min(9, 8) = 8), tile 2 (p = min(7, 10) = 7)
    assert plan.xtab_idx[20].tolist() == [1, 2, -1]
    assert plan.xtab_w[20].tolist() == [np.float32(8 / 15), np.float32(7 / 15), 0.0]


def test_plan_2d_order_and_restatement():
    plan, ref = F.tile_plan(20, 30, 16, 4), fn.Plan(20, 30, 16, 4)
    assert plan.y_origins.tolist() == [0, 4] and plan.n_tiles == ref.n_tiles == 6
    assert plan.origins().tolist() == [list(ref.origin(t)) for t in range(6)]            # y-major


class _Gen:
    ndomain, n_cond_channels = 16, 1


def test_value_errors_before_any_device_call(monkeypatch):
    def no_gpu():
        raise AssertionError("an argument error must be raised before the device is touched")
    monkeypatch.setattr(F, "require_gpu", no_gpu)
    ok = np.ones((20, 30), np.float32)
    for bad in (np.ones((15, 30), np.float32), np.ones((20, 15), np.float32), np.ones((2, 20, 15), np.float32)):
        with pytest.raises(ValueError):
            F.disaggregate(_Gen(), bad, 2)
    for overlap in (-1, 9):
        with pytest.raises(ValueError):
            F.disaggregate(_Gen(), ok, 2, overlap=overlap)
        with pytest.raises(ValueError):
            F.tile_plan(20, 30, 16, overlap)
    with pytest.raises(ValueError):
        F.tile_plan(15, 30, 16, 4)
    T = F.tile_plan(20, 30, 16, 4).n_tiles
    for mode, shape in (("shared", (2, 100)), ("shared", (2, 1, T, 100)), ("shared", (3, 1, 100)), ("independent", (2, 1, 100)),
                        ("independent", (2, 1, T + 1, 100)), ("shared", (2, 1, 99))):
        with pytest.raises(ValueError):
            F.disaggregate(_Gen(), ok, 2, latent_mode=mode, latent=np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        F.disaggregate(_Gen(), ok, 2, latent_mode="per-pixel")
    for nc in (2, 3):
        g = _Gen()
        g.n_cond_channels = nc
        with pytest.raises(ValueError):
            F.disaggregate(g, ok, 2)
    with pytest.raises(ValueError):
        F.disaggregate(_Gen(), np.ones((1, 1, 20, 30), np.float32), 2)
    with pytest.raises(ValueError):
        F.disaggregate(_Gen(), torch.ones(20, 30), 2)                  # a CPU tensor is neither numpy nor on the device
    with pytest.raises(ValueError):
        F.blend_device(torch.zeros(2, 24, 16, 16), np.zeros((1, T + 1), np.int32), F.tile_plan(20, 30, 16, 4), torch.zeros(1, 20, 30))
    with pytest.raises(ValueError):
        F.blend_device(torch.zeros(2, 24, 16, 16), np.full((1, T), 2, np.int32), F.tile_plan(20, 30, 16, 4), torch.zeros(1, 20, 30))


def test_no_gpu_means_rdgan_error(monkeypatch):
    if not torch.cuda.is_available():
        with pytest.raises(_lib.RdganError):
            F.disaggregate(_Gen(), np.ones((20, 30), np.float32), 2)
        with pytest.raises(_lib.RdganError):
            F.blend_device(torch.zeros(2, 24, 16, 16), np.zeros((1, 6), np.int32), F.tile_plan(20, 30, 16, 4), torch.zeros(1, 20, 30))
        from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
        monkeypatch.setattr(P, "gen", _Gen())
        with pytest.raises(_lib.RdganError):
            P.generate_scenarios_field(np.ones((20, 30)), 2)


def _fake_predict(inputs):
    """softmax-like fake generator (the _FakeGen of tests/test_host_api.py with a dependence on the condition): fractions that sum to
    1 over the hours at every pixel"""
    latent, cond = inputs
    n = latent.shape[0]
    assert latent.shape == (n, 100) and cond.shape == (n, 16, 16, 1) and not np.isnan(cond).any()
    w = 1.0 + 0.1 * np.tanh(latent[:, :24].astype(np.float64))[:, :, None, None] + 0.05 * np.sin(cond[:, None, :, :, 0] * np.arange(24)[None, :, None, None])
    return (w / w.sum(1, keepdims=True))[..., None]


def test_restatement_conserves_mass():
    rng = np.random.default_rng(0)
    daily = fn.example_field(rng)
    plan = fn.Plan(20, 30, 16, 4)
    counts = fn.scan(daily, plan)
    active = counts[..., 0] > 0
    assert 0 < active.sum() < active.size and counts[..., 1].sum() > 0 and not counts[..., 2].any()
    assert active[1, 0] and not active[1, 3]                                       # the lone wet pixel keeps tile (0, 0) alive
    for mode, zshape in (("shared", (3, 2, 100)), ("independent", (3, 2, plan.n_tiles, 100))):
        out, n_active = fn.disaggregate(_fake_predict, daily, rng.normal(size=zshape).astype(np.float32), plan, W.NORM_SCALE, mode)
        assert out.shape == (3, 2, 24, 20, 30) and n_active == int(active.sum())
        nan = np.isnan(daily)
        assert np.array_equal(np.isnan(out), np.broadcast_to(nan[None, :, None], out.shape))
        assert np.all(out[np.broadcast_to((daily == 0)[None, :, None], out.shape)] == 0)
        total = np.where(nan[None], 0.0, out.sum(axis=2))
        want = np.where(nan, 0.0, daily.astype(np.float64))[None]
        np.testing.assert_allclose(total, np.broadcast_to(want, total.shape), rtol=1e-12, atol=0)


def test_group_units():
    assert F._group_units([3, 3, 3, 3], 6) == [(0, 2), (2, 4)]
    assert F._group_units([3, 3, 3], 3) == [(0, 1), (1, 2), (2, 3)]
    assert F._group_units([5, 0, 5, 1], 4) == [(0, 1), (1, 2), (2, 3), (3, 4)]         # a unit larger than the chunk stands alone
    assert F._group_units([0, 0], 1024) == [(0, 2)]
    for rows, chunk in itertools.product(([1, 2, 3, 4, 5], [4, 4, 4], [0, 7, 0, 7]), (1, 4, 8, 100)):
        g = F._group_units(rows, chunk)
        assert g[0][0] == 0 and g[-1][1] == len(rows) and all(a[1] == b[0] for a, b in zip(g, g[1:]))
        assert all(u1 - u0 == 1 or sum(rows[u0:u1]) <= chunk for u0, u1 in g)
