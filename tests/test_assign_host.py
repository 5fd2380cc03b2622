"""CPU: the numpy restatement of the least-cost assignment (tests/assign_np.py) against brute force over all
permutations, its own certificate, scipy where it imports and an answer worked out by hand; the argument checks of the new Python
surface of pr_disagg_radar_gan_amd/sequence.py and of the C entry; header against _lib.py and the kernel's constants."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, sequence as SQ
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import assign_np as an
from tests import sequence_np as sn
from tests.test_sequence_host import NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = (1 << 40) - 1


def random_costs(rng, S, top):
    return rng.integers(0, top + 1, (S, S)).astype(np.int64)


def test_mirror_against_brute_force():
    rng = np.random.default_rng(0)
    sizes = set()
    for n in range(200):
        S = int(rng.integers(1, 8))
        C = random_costs(rng, S, 3 if n < 100 else TOP)                                   # heavy ties, then the 64-bit range
        perm, u, v, steps = an.assign(C)
        assert an.check_certificate(C, perm, u, v) == an.brute_force(C), n
        assert S <= steps <= S * (S + 1) // 2 and perm.dtype == np.int32
        sizes.add(S)
    assert sizes == set(range(1, 8))


@pytest.mark.parametrize("S", [1, 2, 3, 17, 63, 64, 65])
def test_mirror_certificate(S):
    rng = np.random.default_rng(S)
    ij = np.add.outer(np.arange(S), np.arange(S)).astype(np.int64)
    planted = np.ones((S, S), np.int64)
    pi = rng.permutation(S)
    planted[np.arange(S), pi] = 0
    for C in (random_costs(rng, S, 3), random_costs(rng, S, TOP), np.full((S, S), 7, np.int64), ij, np.full((S, S), TOP, np.int64), planted,
              np.outer(np.arange(1, S + 1), np.arange(1, S + 1)).astype(np.int64)):
        perm, u, v, _ = an.assign(C)
        an.check_certificate(C, perm, u, v)
        assert max(np.abs(u).max(), np.abs(v).max()) < S * (1 << 40)
    perm, u, v, steps = an.assign(planted)
    assert perm.tolist() == pi.tolist() and an.check_certificate(planted, perm, u, v) == 0
    # every permutation is optimal on a constant matrix and on i + j: the tie rules alone decide, and they give the identity
    assert an.assign(np.full((S, S), 7, np.int64))[0].tolist() == list(range(S)) and an.assign(ij)[0].tolist() == list(range(S))
    # (i + 1)(j + 1): the unique optimum is the anti-diagonal, and every insertion walks every matched column
    perm, _, _, steps = an.assign(np.outer(np.arange(1, S + 1), np.arange(1, S + 1)).astype(np.int64))
    assert perm.tolist() == list(range(S))[::-1] and steps == S * (S + 1) // 2


def test_mirror_totals_against_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(5)
    for n in range(50):
        C = random_costs(rng, 40, (3, 1000, TOP)[n % 3])
        perm, u, v, _ = an.assign(C)
        rows, cols = lsa(C)
        assert an.check_certificate(C, perm, u, v) == int(C[rows, cols].sum()), n


def test_greedy_is_not_optimal_by_hand():
    C = np.array([[1, 2], [2, 100]], np.int64)
    greedy = sn.greedy_sorted(C)
    assert greedy.tolist() == [0, 1] and int(C[np.arange(2), greedy].sum()) == 101
    perm, u, v, steps = an.assign(C)
    # row 0 takes column 0 (u0 = 1); row 1 finds column 0 at 2, then through row 0 column 1 at 2 + (2 - 1) = 3: u = (2, 3), v = (-1, 0)
    assert perm.tolist() == [1, 0] and u.tolist() == [2, 3] and v.tolist() == [-1, 0] and steps == 3
    assert an.check_certificate(C, perm, u, v) == 4 == an.brute_force(C)
    perm, total, u, v, steps = an.optimal_matching(np.stack([C, C.T, np.zeros((2, 2), np.int64)]))
    # (all equal: row 1 meets column 0 first, the smaller index, though it is taken -- a constant matrix costs S (S + 1) / 2 steps)
    assert total.tolist() == [4, 4, 0] and perm.tolist() == [[1, 0], [1, 0], [0, 1]] and steps.tolist() == [3, 3, 3]
    with pytest.raises(AssertionError):
        an.check_certificate(C, greedy, u[0], v[0])
    with pytest.raises(AssertionError):
        an.check_certificate(C, perm[0], u[0] + 1, v[0])                                  # infeasible
    with pytest.raises(AssertionError):
        an.check_certificate(C, perm[0], u[0] - 1, v[0])                                  # not tight
    with pytest.raises(AssertionError):
        an.check_certificate(C, np.array([0, 0]), u[0], v[0])


def test_argument_errors():
    for costs in (torch.zeros((2, 3, 4), dtype=torch.int64), torch.zeros((1, 3, 3)), torch.zeros((1, 3, 3), dtype=torch.int32),
                  torch.zeros((3, 3), dtype=torch.int64), torch.zeros((0, 3, 3), dtype=torch.int64), np.zeros((1, 3, 3), np.int64),
                  torch.zeros((1, 3, 3), dtype=torch.int64), torch.zeros((1, 1, 1), dtype=torch.int64).expand(1, 4097, 4097),
                  torch.zeros((1, 1, 1), dtype=torch.int64).expand(65536, 1, 1)):
        for kw in ({}, dict(return_duals=True)):
            with pytest.raises(ValueError):                                               # (among them: int64 and square, but on the host)
                SQ.optimal_matching(costs, **kw)
    assert SQ.MATCHINGS == ("greedy", "optimal") and [SQ.check_matching(m) for m in SQ.MATCHINGS] == list(SQ.MATCHINGS)

    class Gen:
        ndomain, n_cond_channels = 16, 1

    for bad in ("hungarian", "Optimal", "", None, 1, b"optimal"):
        with pytest.raises(ValueError, match="matching"):
            SQ.check_matching(bad)
        with pytest.raises(ValueError, match="matching"):                                 # before the days are counted, before the device
            SQ.chain_edges(NoDevice(), bad)
        with pytest.raises(ValueError, match="matching"):
            SQ.chain(np.zeros((2, 2, 24, 3, 4), np.float32), matching=bad)
        with pytest.raises(ValueError, match="matching"):
            SQ.chain_field(Gen(), np.zeros((2, 20, 20)), 3, matching=bad)
        with pytest.raises(ValueError, match="matching"):
            P.chain_scenarios_field(np.zeros((2, 20, 20), np.float32), 3, matching=bad)
    for m in SQ.MATCHINGS:                                                                # the other checks still come first
        with pytest.raises(ValueError):
            SQ.chain_edges(NoDevice(D=1), m)
        with pytest.raises(ValueError):
            SQ.chain_field(Gen(), np.zeros((1, 20, 20)), 3, matching=m)


def test_chain_result_keeps_its_constructions():
    fields = [f.name for f in dataclasses.fields(SQ.ChainResult)]
    assert fields[-2:] == ["matching", "greedy_matched"] and fields[-4:-2] == ["observed", "observed_within"]
    res = SQ.ChainResult(*([None] * 2), np.zeros(3, np.int64), 0, *([None] * 5), plane_shape=(3, 4))
    assert res.matching == "greedy" and res.greedy_matched is None


def test_cabi_argument_checks():
    """the entry refuses a bad argument before it touches the device: callable without one"""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # 16-byte aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)

    def assign(c=good, B=3, S=5, perm=good, u=good, v=good, total=good):
        return lib.rdgan_assign(c, B, S, perm, u, v, total, st)

    for kw in (dict(c=null), dict(perm=null), dict(u=null), dict(v=null), dict(total=null), dict(c=by(4)), dict(u=by(4)), dict(v=by(4)),
               dict(total=by(4)), dict(perm=by(2)), dict(B=0), dict(B=-1), dict(B=65536), dict(S=0), dict(S=-1), dict(S=4097), dict(S=4096, B=129)):
        assert assign(**kw) == -2, kw


def test_header_and_lib_agree_on_the_entry():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "int*": "c_void_p", "long long*": "c_void_p", "const long long*": "c_void_p"}
    name = "rdgan_assign"
    assert [n for n in _lib.SIGNATURES if "assign" in n] == [name]
    assert isinstance(getattr(_lib.load(), name), ctypes._CFuncPtr)
    m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
    assert m
    res, args = _lib.SIGNATURES[name]
    params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
    assert params == ["const long long*", "long", "long", "int*", "long long*", "long long*", "long long*", "void*"]
    assert res.__name__ == ctype[m.group(1)] and [a.__name__ for a in args] == [ctype[p] for p in params]


def test_kernel_constants():
    csrc = os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc")
    text = "".join(open(os.path.join(csrc, h)).read() for h in ("rdgan_sequence.hip.h", "rdgan_assign.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", "").replace("ll", ""))
    S, T, bits = value("RD_SEQ_MAXS"), value("RD_ASG_THREADS"), value("RD_ASG_KEYBITS")
    assert S == SQ.MAX_MEMBERS == 1 << bits and S // T == 16 and T % 64 == 0
    assert S * SQ.MAX_COST <= 1 << (64 - bits) and SQ.MAX_COST == an.MAX_COST               # minv << 12 | j stays inside 64 bits
    assert value("RD_ASG_INF") == an.INF > S * SQ.MAX_COST
    assert "static_assert" in text.split("RD_ASG_INF")[1]
