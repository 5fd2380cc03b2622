"""-m gpu: the least-cost assignment (csrc/rdgan_assign.hip.h, sequence.optimal_matching, chain*(matching="optimal")) against its
numpy restatement (tests/assign_np.py, itself checked on the CPU by tests/test_assign_host.py).  Every case asserts the certificate
on the device result first -- a permutation with feasible duals that are tight on it is optimal, whatever the mirror says -- and then
equality of perm, u, v and total with the mirror.  Everything is an integer: every comparison is an equality."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, field as F, models, sequence as SQ, weights as W
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import assign_np as an
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

TOP = (1 << 40) - 1
THREADS = 256                                                                             # RD_ASG_THREADS


@functools.lru_cache(maxsize=None)
def classes(S):
    """(costs (3, S, S): random 0 .. 3 (heavy ties), random up to 2^40 - 1 (the 64-bit paths and the packed key), a planted
    permutation of zeros in a field of ones; the planted permutation; the mirror's answer).  Shared: not written to."""
    rng = np.random.default_rng(100 + S)
    pi = rng.permutation(S)
    planted = np.ones((S, S), np.int64)
    planted[np.arange(S), pi] = 0
    C = np.stack([rng.integers(0, 4, (S, S)), rng.integers(0, TOP + 1, (S, S)), planted]).astype(np.int64)
    return C, pi, an.optimal_matching(C)


@functools.lru_cache(maxsize=None)
def adversarial(S):
    """a constant matrix and i + j, where every permutation is optimal and the tie rules alone decide; (i + 1)(j + 1), whose unique
    optimum is the anti-diagonal and whose every insertion walks every matched column"""
    i = np.arange(S, dtype=np.int64)
    C = np.stack([np.full((S, S), 7, np.int64), np.add.outer(i, i), np.outer(i + 1, i + 1)])
    return C, an.optimal_matching(C)


def solve_and_check(C, want, costs=None):
    """optimal_matching on the device: the certificate per boundary, then perm, u, v and total against the mirror"""
    perm, total, u, v = SQ.optimal_matching(dev(C, torch.int64) if costs is None else costs, return_duals=True)
    B, S = C.shape[:2]
    assert perm.dtype == torch.int32 and total.dtype == u.dtype == v.dtype == torch.int64 and perm.is_cuda
    assert tuple(perm.shape) == tuple(u.shape) == tuple(v.shape) == (B, S) and tuple(total.shape) == (B,)
    perm, total, u, v = perm.cpu().numpy(), total.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy()
    for b in range(B):
        assert an.check_certificate(C[b], perm[b], u[b], v[b]) == total[b], b
    for name, got, ref in zip(("perm", "total", "u", "v"), (perm, total, u, v), want[:4]):
        assert np.array_equal(got, ref), name
    return perm, total


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 3])
def test_cost_classes(S):
    """around one wave, around the workgroup's 256 threads, and 515: thread 0 .. 2 own three live columns, the others two, and
    every thread idle slots"""
    C, pi, want = classes(S)
    perm, total = solve_and_check(C, want)
    assert perm[2].tolist() == pi.tolist() and total[2] == 0                              # the planted permutation, recovered
    assert torch.equal(SQ.optimal_matching(dev(C, torch.int64)), torch.from_numpy(perm).cuda())   # (without the duals: perm alone)


@pytest.mark.parametrize("S", [1, 3, 64, THREADS + 1])
def test_adversarial_classes(S):
    C, want = adversarial(S)
    perm, total = solve_and_check(C, want)
    assert perm[0].tolist() == perm[1].tolist() == list(range(S)) and perm[2].tolist() == list(range(S))[::-1]
    assert want[4].tolist() == [S * (S + 1) // 2] * 3                                     # the most search steps there can be


def test_boundaries_are_indexed_by_the_grid():
    S = 65
    rng = np.random.default_rng(9)
    C = np.concatenate([classes(S)[0], rng.integers(0, 1000, (2, S, S)).astype(np.int64)])
    C[4] = C[4].T + 5
    want = an.optimal_matching(C)
    solve_and_check(C, want)
    for b in range(5):
        solve_and_check(C[b:b + 1], [w[b:b + 1] for w in want])
    assert len({tuple(q) for q in want[0].tolist()}) == 5                                 # five different answers


def test_non_contiguous_costs():
    S = 65
    C, _, want = classes(S)
    wide = torch.full((3, S + 3, 2 * S + 1), -1, dtype=torch.int64, device="cuda")
    wide[:, 2:S + 2, 1:2 * S:2] = dev(C, torch.int64)
    view = wide[:, 2:S + 2, 1:2 * S:2]
    assert not view.is_contiguous()
    solve_and_check(C, want, costs=view)
    assert (wide[:, :2] == -1).all() and (wide[:, :, ::2] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
def planted_series(S=8, D=4, ny=6, nx=6, seed=7):
    """distinct random fields; day d + 1's member pi_d(s) starts with exactly the field day d's member s ends with"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(1, 2000, (S, D, 24, ny, nx)) / 32.0).astype(np.float32)              # exact in 1/32 mm, all distinct fields
    pis = [rng.permutation(S) for _ in range(D - 1)]
    for d, pi in enumerate(pis):
        x[pi, d + 1, 0] = x[np.arange(S), d, 23]
    return x, np.stack(pis)


FIELDS = [f.name for f in dataclasses.fields(SQ.ChainResult)]


def same(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if not (isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)):
                return False
        elif x != y:
            return False
    return True


def test_chain_optimal_recovers_planted_series():
    x, pis = planted_series()
    S, D = x.shape[:2]
    xd = dev(x)
    r = SQ.chain(xd, matching="optimal")
    assert r.matching == "optimal" and np.array_equal(r.perm, pis) and r.perm.dtype == np.int32
    assert not r.matched.any() and r.matched.shape == (D - 1,)
    assert r.greedy_matched is not None and r.greedy_matched.shape == (D - 1,) and not r.greedy_matched.any()
    series = SQ.reorder(xd, r.order)
    assert torch.equal(series[:, :-1, 23], series[:, 1:, 0])                              # hour 23 is the next day's hour 0
    g = SQ.chain(xd)
    assert g.matching == "greedy" and g.greedy_matched is None
    assert all(np.array_equal(getattr(g, f), getattr(r, f)) for f in ("order", "perm", "path", "n_valid", "random", "diagonal", "matched", "path_cost"))


def test_chain_optimal_is_never_worse_than_greedy():
    S, D = 40, 5
    rng = np.random.default_rng(23)
    x = (rng.gamma(0.6, 3.0, (S, D, 24, 5, 7)) * (rng.random((S, D, 24, 5, 7)) < 0.5)).astype(np.float32)
    xd = dev(x)
    r, g = SQ.chain(xd, matching="optimal"), SQ.chain(xd, matching="greedy")
    assert (r.matched <= r.greedy_matched).all() and (r.matched < r.greedy_matched).any()
    assert np.array_equal(r.greedy_matched, g.matched) and not np.array_equal(r.perm, g.perm)
    e = SQ.SeamEdges().add(xd)
    costs, n_valid = SQ.seam_costs(e)
    C = costs.cpu().numpy()
    want = an.optimal_matching(C)
    assert np.array_equal(r.perm, want[0]) and np.array_equal(r.order, SQ.series_order(want[0]))
    assert np.allclose(r.matched, want[1] / S / (32 * n_valid.cpu().numpy()), rtol=1e-12)
    assert same(SQ.chain_edges(e, "optimal"), r)


def test_chain_default_is_greedy_field_by_field():
    x, _ = planted_series(S=5, D=3, seed=11)
    x[:, :, 23] = np.random.default_rng(12).integers(0, 3, x[:, :, 23].shape) / 32.0      # few distinct costs: ties
    xd = dev(x)
    a, b = SQ.chain(xd), SQ.chain(xd, matching="greedy")
    assert same(a, b) and a.matching == "greedy" and a.greedy_matched is None
    e = SQ.SeamEdges().add(xd)
    assert same(SQ.chain_edges(e), a) and same(SQ.chain_edges(e, matching="greedy"), a)


@pytest.fixture(scope="module")
def generator():
    return models.Generator(W.init_generator(np.random.default_rng(21), 16), 16)


def test_chain_field_optimal_equals_chain_of_disaggregate(generator, monkeypatch):
    """as tests/test_hip_sequence.py builds its *_field case: 3 wet days of a 20 x 24 plane at ndomain 16, overlap 4, 4 scenarios;
    `chunk` is one unit's tiles on both sides, the batching for which evaluate_field promises equal values"""
    S, D = 4, 3
    rng = np.random.default_rng(41)
    daily = (0.1 + rng.gamma(0.8, 6.0, (D, 20, 24))).astype(np.float32)
    daily[1, 3, 5] = np.nan
    dd = dev(daily)
    z = np.random.default_rng(42).normal(size=(S, D, 100)).astype(np.float32)
    info = F.disaggregate(generator, dd, 1, latent=z[:1])[1]
    hourly, _ = F.disaggregate(generator, dd, S, latent=z, chunk=info.n_tiles)
    want = SQ.chain(hourly, matching="optimal")
    assert want.matching == "optimal" and want.greedy_matched is not None and (want.matched <= want.greedy_matched).all()
    C = SQ.seam_costs(SQ.SeamEdges().add(hourly))[0].cpu().numpy()
    assert np.array_equal(want.perm, an.optimal_matching(C)[0])
    for scenario_chunk in (1, 3, 4):
        got = SQ.chain_field(generator, dd if scenario_chunk == 3 else daily, S, scenario_chunk=scenario_chunk, latent=z, chunk=info.n_tiles,
                             matching="optimal")
        assert same(got, want), scenario_chunk
    monkeypatch.setattr(P, "gen", generator)
    np.random.seed(5)
    a = P.chain_scenarios_field(daily, S, scenario_chunk=S, matching="optimal")
    np.random.seed(5)
    hourly2, _ = F.disaggregate(generator, dd, S, norm_scale=P.norm_scale)
    assert same(a, SQ.chain(hourly2, matching="optimal"))


def test_c_entry_refuses_bad_arguments_and_touches_nothing():
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S = 5
    C = dev(classes(65)[0][:, :S, :S], torch.int64)
    perm = torch.full((3, S), -3, dtype=torch.int32, device="cuda")
    u, v = torch.full((3, S), -3, dtype=torch.int64, device="cuda"), torch.full((3, S), -3, dtype=torch.int64, device="cuda")
    total = torch.full((3,), -3, dtype=torch.int64, device="cuda")
    call = lambda c=C.data_ptr(), B=3, S=S, p=perm.data_ptr(), u_=u.data_ptr(): lib.rdgan_assign(c, B, S, p, u_, v.data_ptr(), total.data_ptr(), st)
    for kw in (dict(B=0), dict(B=65536), dict(S=0), dict(S=4097), dict(S=4096, B=129), dict(c=0), dict(p=0), dict(c=C.data_ptr() + 4),
               dict(u_=u.data_ptr() + 4), dict(p=perm.data_ptr() + 2)):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert (perm == -3).all() and (u == -3).all() and (v == -3).all() and (total == -3).all()
    assert call() == 0
    assert an.check_certificate(C[1].cpu().numpy(), perm[1].cpu().numpy(), u[1].cpu().numpy(), v[1].cpu().numpy()) == int(total[1])
