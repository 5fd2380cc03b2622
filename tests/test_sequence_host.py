"""CPU: the numpy restatement of the seam definitions (tests/sequence_np.py) against answers worked out by hand, its sorted walk
against its rounds of locally dominant pairs; the argument checks of pr_disagg_radar_gan_amd/sequence.py and of the C entries;
header against _lib.py and the kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _hourly, _lib, sequence as SQ
from tests import sequence_np as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_edge_features_by_hand():
    x = np.zeros((2, 2, 24, 1, 6), np.float32)
    # x * 32 on .5 exactly: 0.015625 * 32 = 0.5 -> 0 (even), 0.046875 * 32 = 1.5 -> 2, 0.078125 * 32 = 2.5 -> 2; 2047.99 clamps
    x[0, 0, 0, 0] = (0.015625, 0.046875, 0.078125, 2047.99, 1.0, 2047.0)
    x[1, 0, 0, 0] = (np.nan, -1.0, np.inf, 2048.0, -0.0, 0.25)
    x[0, 1, 23, 0, 2] = 3.0
    x[0, 0, 11, 0, 0] = 7.0                                                               # not an edge hour: never seen
    feat, bad = sn.edge_features(x)
    assert feat.dtype == np.uint16 and feat.shape == (2, 2, 2, 6) and bad.shape == (2, 2, 6)
    assert feat[0, 0, 0].tolist() == [0, 2, 2, 65535, 32, 65504] and feat[1, 0, 0].tolist() == [0, 0, 0, 0, 0, 8]
    assert bad[0, 0].tolist() == [True, True, True, True, False, False] and not bad[0, 1].any() and not bad[1].any()
    assert feat[0, 1, 1].tolist() == [0, 0, 96, 0, 0, 0]
    feat2, _ = sn.edge_features(x, first_hour=11, last_hour=0)
    assert feat2[0, 0, 0, 0] == 224 and feat2[0, 0, 1].tolist() == feat[0, 0, 0].tolist()


def test_costs_and_masks_by_hand():
    feat = np.zeros((2, 3, 2, 4), np.uint16)
    feat[0, 0, 1], feat[1, 0, 1] = (1, 2, 3, 4), (10, 0, 0, 65535)                        # the last edges of day 0
    feat[0, 1, 0], feat[1, 1, 0] = (1, 2, 3, 0), (0, 0, 5, 0)                             # the first edges of day 1
    bad = np.zeros((3, 2, 4), bool)
    bad[1, 0, 3] = True                                                                   # masks pixel 3 at boundary 0
    bad[1, 1, :] = True                                                                   # masks boundary 1 whole
    costs, n_valid = sn.seam_costs(feat, bad)
    assert n_valid.tolist() == [3, 0] and costs[0].tolist() == [[0, 1 + 2 + 2], [9 + 2 + 3, 10 + 5]] and not costs[1].any()
    c0, nv0 = sn.seam_costs(feat, bad, shift=0)                                           # hour pairs within days 0, 1, 2
    assert nv0.tolist() == [4, 0, 4] and c0[0, 1, 0] == 10 + 65535 and c0.shape == (3, 2, 2)
    one, _ = sn.seam_costs(feat, bad, 1, feat[:1], bad)
    assert one.shape == (2, 2, 1) and one[0, :, 0].tolist() == [0, 14]


def test_min_plus_ties_and_large_costs():
    C = np.array([[[5, 1, 1], [5, 1, 0], [4, 1, 1]], [[2, 2, 9], [2, 2, 9], [0, 1, 9]]], np.int64)
    acc, back = sn.min_plus(C)
    assert acc[1].tolist() == [4, 1, 0] and back[0].tolist() == [2, 0, 1]                  # column 1: three equal, the smallest i
    assert acc[2].tolist() == [0, 1, 9] and back[1].tolist() == [2, 2, 2]
    path, total = sn.best_path(C)
    assert path.tolist() == [1, 2, 0] and total == 0
    path, total = sn.best_path(np.zeros((3, 4, 4), np.int64))                             # all equal: member 0 throughout
    assert path.tolist() == [0, 0, 0, 0] and total == 0
    big = np.full((8, 2, 2), (1 << 40) - 1, np.int64)
    big[:, 1, 1] -= 1
    path, total = sn.best_path(big)
    assert path.tolist() == [1] * 9 and total == 8 * ((1 << 40) - 2)


def test_matching_by_hand():
    assert sn.greedy_sorted(np.zeros((5, 5), np.int64)).tolist() == [0, 1, 2, 3, 4]        # a constant matrix: the identity
    C = np.array([[1, 0, 5], [0, 0, 5], [5, 5, 0]], np.int64)
    # keys ascending: (0, 1), (1, 0), (1, 1), (2, 2), ...: greedy takes (0, 1), (1, 0), (2, 2) -- total 0, where the diagonal costs 1
    assert sn.greedy_sorted(C).tolist() == [1, 0, 2]
    S = 64
    ij = np.add.outer(np.arange(S), np.arange(S)).astype(np.int64)
    perm, rounds = sn.greedy_rounds(ij)
    assert perm.tolist() == list(range(S)) and rounds == S                                # one pair a round: the bound is attained
    perm, rounds = sn.greedy_rounds(np.array([[(1 << 40) - 1]], np.int64))
    assert perm.tolist() == [0] and rounds == 1
    assert sn.keys(np.array([[(1 << 40) - 1]], np.int64))[0, 0] == np.uint64(((1 << 40) - 1) << 24)


def test_sorted_walk_equals_locally_dominant_rounds():
    rng = np.random.default_rng(0)
    most = 0
    for n in range(200):
        S = int(rng.integers(1, 13))
        C = rng.integers(0, int(rng.integers(1, 5)), (S, S)).astype(np.int64)              # values 0 .. 3 at most: heavy ties
        a, (b, rounds) = sn.greedy_sorted(C), sn.greedy_rounds(C)
        assert np.array_equal(a, b) and sorted(a.tolist()) == list(range(S)) and 1 <= rounds <= S, n
        most = max(most, rounds)
    assert most > 1


def test_series_order_and_reorder():
    perm = np.array([[1, 2, 0], [0, 2, 1]], np.int32)
    order = sn.series_order(perm)
    assert order.tolist() == [[0, 1, 2], [1, 2, 0], [2, 1, 0]]
    assert np.array_equal(SQ.series_order(perm), order) and torch.equal(SQ.series_order(torch.from_numpy(perm)), torch.from_numpy(order))
    assert all(sorted(row) == [0, 1, 2] for row in order.tolist())
    x = np.arange(3 * 3 * 2).reshape(3, 3, 2)
    y = sn.reorder(x, order)
    assert y[0, :, 0].tolist() == [x[0, 0, 0], x[1, 1, 0], x[2, 2, 0]]
    for bad in (np.zeros(3, np.int32), np.zeros((2, 3)), torch.zeros(2, 3)):
        with pytest.raises(ValueError):
            SQ.series_order(bad)


class NoDevice(SQ.SeamEdges):
    """a SeamEdges as far as the host checks go: S members of D days of a plane, nothing on a device"""

    def __init__(self, S=3, D=4, plane=(3, 4), **kw):
        super().__init__(**kw)
        self.n_members, self.n_days, self.plane_shape, self.device = S, D, plane, torch.device("cpu")


def test_argument_errors():
    for kw in (dict(first_hour=24), dict(first_hour=-1), dict(last_hour=24), dict(last_hour=-1), dict(first_hour=1.0), dict(last_hour=True),
               dict(first_hour=None)):
        with pytest.raises(ValueError):
            SQ.SeamEdges(**kw)
        with pytest.raises(ValueError):
            SQ.chain(np.zeros((2, 2, 24, 3, 4), np.float32), **kw)
    e = SQ.SeamEdges(11, 12)
    assert (e.first_hour, e.last_hour, e.n_members) == (11, 12, 0)
    for bad in (np.zeros((24, 3, 4)), np.zeros((2, 2, 2, 24, 3, 4)), np.zeros((2, 23, 3, 4)), np.zeros((0, 2, 24, 3, 4)), torch.zeros(2, 24, 3, 4),
                np.zeros((2, 24, 3, 4), dtype=complex), np.broadcast_to(np.float32(0), (4097, 2, 24, 1, 1)),
                np.broadcast_to(np.float32(0), (1, 65536, 24, 1, 1))):
        with pytest.raises(ValueError):
            SQ.SeamEdges().add(bad)
    pinned = NoDevice()
    for bad in (np.zeros((2, 4, 24, 3, 5), np.float32), np.zeros((2, 4, 24, 4, 3), np.float32), np.zeros((2, 3, 24, 3, 4), np.float32),
                np.broadcast_to(np.float32(0), (4094, 4, 24, 3, 4))):
        with pytest.raises(ValueError):                                                   # another plane, other days, 3 + 4094 members
            pinned.add(bad)
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: no CPU fallback
        with pytest.raises(_lib.RdganError):
            SQ.SeamEdges().add(np.zeros((2, 2, 24, 3, 4), np.float32))
    for args in ((None,), (SQ.SeamEdges(),), (NoDevice(), 1, NoDevice(plane=(4, 3))), (NoDevice(), 1, NoDevice(D=5)), (NoDevice(), 1, "x"),
                 (NoDevice(), 4), (NoDevice(), -1), (NoDevice(), 1.0), (NoDevice(), 1, None, 0), (NoDevice(), 1, None, 1.5), (NoDevice(), 1, None, 2 ** 24 + 1), (NoDevice(S=4096, D=130), 1, NoDevice(S=4096, D=130))):
        with pytest.raises(ValueError):
            SQ.seam_costs(*args)
    for costs in (torch.zeros((2, 3, 4), dtype=torch.int64), torch.zeros((1, 3, 3)), torch.zeros((1, 3, 3), dtype=torch.int32),
                  torch.zeros((3, 3), dtype=torch.int64), torch.zeros((0, 3, 3), dtype=torch.int64), np.zeros((1, 3, 3), np.int64),
                  torch.zeros((1, 3, 3), dtype=torch.int64), torch.zeros((1, 1, 1), dtype=torch.int64).expand(1, 4097, 4097),
                  torch.zeros((1, 1, 1), dtype=torch.int64).expand(65536, 1, 1)):
        for fn in (SQ.greedy_matching, SQ.best_path, SQ.min_plus):
            with pytest.raises(ValueError):                                               # (among them: int64 and square, but on the host)
                fn(costs)
    with pytest.raises(ValueError):
        SQ.chain_edges(NoDevice(D=1))
    for args in ((np.zeros((3, 2)), np.zeros((2, 3), np.int64)), (torch.zeros(3, 2), np.zeros((2, 3), np.int64))):
        with pytest.raises(ValueError):
            SQ.reorder(*args)
    res = SQ.ChainResult(*([None] * 2), np.zeros(3, np.int64), 0, *([None] * 5), plane_shape=(3, 4))
    for args in ((None, np.zeros((3, 24, 3, 4))), (res, np.zeros((2, 24, 3, 4))), (res, np.zeros((3, 24, 3, 5))), (res, np.zeros((1, 3, 24, 3, 4))),
                 (res, np.zeros((3, 24, 3, 4)), [True]), (res, np.zeros((3, 24, 3, 4)), [1, 0])):
        with pytest.raises(ValueError):
            SQ.compare(*args)

    class Gen:
        ndomain, n_cond_channels = 16, 1

    for kw in (dict(daily=np.zeros((20, 20))), dict(daily=np.zeros((1, 20, 20))), dict(n_scenarios=0), dict(n_scenarios=4097), dict(scenario_chunk=0),
               dict(first_hour=24), dict(last_hour=-1), dict(latent_mode="none"), dict(daily=np.zeros((2, 8, 20)))):
        with pytest.raises(ValueError):
            SQ.chain_field(**{**dict(gen=Gen(), daily=np.zeros((2, 20, 20)), n_scenarios=3), **kw})


def test_cabi_argument_checks():
    """the five C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    ws = lib.rdgan_seq_workspace_bytes
    assert ws(1, 1) == 32 and ws(100, 29) == 29 * 2600 and ws(4096, 65535) == 65535 * 26 * 4096 and ws(3, 2) == 2 * 80
    for a in ((0, 1), (4097, 1), (1, 0), (1, 65536), (-1, -1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # 16-byte aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)

    def edges(x=good, n=6, stride=24 * 15, ny=3, nx=5, D=3, h0=0, h1=23, f=good, bad=good):
        return lib.rdgan_seq_edges(x, n, stride, ny, nx, D, h0, h1, f, bad, st)

    for kw in (dict(x=null), dict(f=null), dict(bad=null), dict(x=by(2)), dict(f=by(8)), dict(bad=by(2)), dict(n=0), dict(n=7), dict(D=0), dict(D=65536),
               dict(ny=0), dict(nx=0), dict(ny=4097, nx=4096, stride=24 * 4097 * 4096), dict(stride=24 * 15 - 1), dict(h0=-1), dict(h0=24), dict(h1=-1),
               dict(h1=24), dict(n=4097, D=1)):
        assert edges(**kw) == -2, kw

    def costs(fa=good, ba=good, sa=3, fb=good, bb=good, sb=5, D=4, plane=15, shift=1, splits=0, c=good, nv=good):
        return lib.rdgan_seq_costs(fa, ba, sa, fb, bb, sb, D, plane, shift, splits, c, nv, st)

    for kw in (dict(fa=null), dict(ba=null), dict(fb=null), dict(bb=null), dict(c=null), dict(nv=null), dict(fa=by(8)), dict(fb=by(8)), dict(ba=by(2)),
               dict(bb=by(2)), dict(c=by(4)), dict(nv=by(4)), dict(sa=0), dict(sa=4097), dict(sb=0), dict(sb=4097), dict(D=0), dict(D=65536), dict(plane=0),
               dict(plane=2 ** 24 + 1), dict(shift=-1), dict(shift=4), dict(splits=-1), dict(sa=4096, sb=4096, D=130)):
        assert costs(**kw) == -2, kw

    def minplus(c=good, B=3, S=5, acc=good, back=good):
        return lib.rdgan_seq_minplus(c, B, S, acc, back, st)

    for kw in (dict(c=null), dict(acc=null), dict(back=null), dict(c=by(4)), dict(acc=by(4)), dict(back=by(2)), dict(B=0), dict(B=65536), dict(S=0),
               dict(S=4097), dict(S=4096, B=129)):
        assert minplus(**kw) == -2, kw

    def match(c=good, B=3, S=5, init=1, rounds=2, perm=good, free=good, w=good, nbytes=3 * 136):
        return lib.rdgan_seq_match(c, B, S, init, rounds, perm, free, w, nbytes, st)

    for kw in (dict(c=null), dict(perm=null), dict(free=null), dict(w=null), dict(c=by(4)), dict(w=by(4)), dict(perm=by(2)), dict(free=by(2)), dict(B=0),
               dict(B=65536), dict(S=0), dict(S=4097), dict(S=4096, B=129, nbytes=1 << 40), dict(init=2), dict(init=-1), dict(rounds=-1), dict(rounds=4097),
               dict(nbytes=3 * 136 - 1), dict(nbytes=0), dict(nbytes=-8)):
        assert match(**kw) == -2, kw


def test_header_and_lib_agree_on_the_sequence_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "int*": "c_void_p", "long long*": "c_void_p",
             "const long long*": "c_void_p", "unsigned short*": "c_void_p", "const unsigned short*": "c_void_p", "unsigned int*": "c_void_p",
             "const unsigned int*": "c_void_p"}
    names = ("rdgan_seq_workspace_bytes", "rdgan_seq_edges", "rdgan_seq_costs", "rdgan_seq_minplus", "rdgan_seq_match")
    assert tuple(sorted(n for n in _lib.SIGNATURES if n.startswith("rdgan_seq_"))) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_seq_\w+)\(", header, re.M)))) == tuple(sorted(names))
    lib = _lib.load()
    for name in names:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)


def test_python_constants_are_the_kernel_header_s():
    csrc = os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc")
    text = "".join(open(os.path.join(csrc, h)).read() for h in ("rdgan_sequence.hip.h", "rdgan_hourly_host.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (SQ.MAX_MEMBERS, SQ.UNIT, SQ.MAX_DAYS, SQ.MAX_COSTS, SQ.MAX_PLANE, SQ.NHOURS) == tuple(
        value(m) for m in ("RD_SEQ_MAXS", "RD_SEQ_UNIT", "RD_SEQ_MAXDAYS", "RD_SEQ_MAXCOSTS", "RD_HOURLY_MAXPLANE", "RD_HOURS"))
    assert SQ.MAX_MEMBERS == _hourly.MAX_MEMBERS == sn.MAX_MEMBERS == 1 << 12 and (sn.UNIT, sn.FEATMAX) == (SQ.UNIT, value("RD_SEQ_FEATMAX"))
    assert SQ.MAX_COST == (value("RD_SEQ_FEATMAX") + 1) * SQ.MAX_PLANE == 1 << 40
    # the 32-bit sums of a pair cannot wrap between two flushes; a tile's LDS is the two padded panels
    assert value("RD_SEQ_FLUSH") * value("RD_SEQ_CHUNK") * 8 * value("RD_SEQ_FEATMAX") < 2 ** 32
    assert value("RD_SEQ_LDU") == value("RD_SEQ_TILE") + 1 and value("RD_SEQ_THREADS") * 16 == value("RD_SEQ_TILE") ** 2
    assert [SQ.padded_plane(p) for p in (1, 8, 9, 35)] == [8, 8, 16, 40] and [SQ.bad_words(p) for p in (1, 32, 33, 70000)] == [1, 1, 2, 2188]
