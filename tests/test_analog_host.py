"""CPU: the numpy restatement of the analog definitions (tests/analog_np.py) in its two forms against each other and against
answers worked out by hand; the argument checks of pr_disagg_radar_gan_amd/analog.py and of the C entries; header against _lib.py
and the kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, analog as AN
from tests import analog_np as an

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_case(seed, N=23, Q=5, ny=3, nx=4):
    rng = np.random.default_rng(seed)
    lib = (rng.gamma(0.5, 4.0, (N, 24, ny, nx)) * (rng.random((N, 24, ny, nx)) < 0.4)).astype(np.float32)
    lib[3] = lib[1]                                                                       # a duplicate day: a tie
    lib[5, 2, 0, 0] = np.nan
    lib[6, 0, 1, 1] = -1.0
    lib[7, 9, 2, 3] = 2048.0
    lib[8] = 0.0                                                                          # all dry
    cond = lib[rng.integers(0, N, Q)].sum(axis=1) * rng.uniform(0.5, 2.0, (Q, 1, 1)).astype(np.float32)
    cond[0] = lib[1].sum(axis=0)
    cond[1, 0, 0] = np.nan
    cond[2, 1, 2] = 2048.0 * 24
    return lib, cond.astype(np.float32)


def test_sort_and_running_top_k_agree():
    for seed in range(3):
        lib, cond = small_case(seed)
        groups, qgroups = np.arange(23) % 4, np.array([0, 1, -1, 3, 5])
        for k in (1, 4, 32):
            for g, qg in ((None, None), (groups, qgroups)):
                a = an.search(lib, cond, k, g, qg)
                b = an.search_running(lib, cond, k, g, qg)
                c = an.search_running(lib, cond, k, g, qg, order=np.random.default_rng(seed).permutation(23))
                for x, y, z in zip(a, b, c):
                    assert np.array_equal(x, y) and np.array_equal(x, z)
        nb, dist, found = an.search(lib, cond, 32)
        assert np.all(found == 23 - 4)                                                    # four void days
        assert not np.isin(nb, (5, 6, 7, 8)).any()
        assert nb[0, :2].tolist() == [1, 3] and dist[0, 0] == dist[0, 1]                  # the duplicate: the smaller index first
        assert np.all(nb[:, 19:] == -1) and np.all(dist[:, 19:] == -1)
        assert np.all(np.diff(dist[:, :19], axis=1) >= 0)
        nb, _, found = an.search(lib, cond, 32, groups, qgroups)
        assert found.tolist() == [19 - 5, 19 - 5, 19, 19 - 4, 19]                          # groups 0, 1, 3 hold 6, 6, 5 days, one void each
        assert not np.isin(nb[0][nb[0] >= 0] % 4, 0).any() and not np.isin(nb[3][nb[3] >= 0] % 4, 3).any()


def test_keys_by_hand():
    lib = np.zeros((3, 24, 1, 2), np.float32)
    lib[0, 0, 0] = (4.0, 0.0)                                                             # D = 4096, 0: e = 64, 0
    lib[1, :, 0, 0] = 1.0 / 24                                                            # 24 rint(1024 / 24) = 24 * 43 = 1032: e = 32
    lib[1, 3, 0, 1] = 9.0                                                                 # e = 96
    lib[2, 5, 0] = (4.0, np.inf)
    e, void, total = an.library_features(lib)
    assert e.tolist() == [[64, 0], [32, 96], [64, 0]] and void.tolist() == [False, False, True] and total.tolist() == [4096, 1032 + 9216, 4096]
    cond = np.array([[[4.0, 0.0]], [[1.0, np.nan]], [[-1.0, 49152.0]]], np.float32)
    eq, masked = an.query_features(cond)
    assert eq.tolist() == [[64, 0], [32, 0], [0, 0]] and masked.tolist() == [[False, False], [False, True], [True, True]]
    keys = an.all_keys(lib, cond)
    assert keys[0].tolist() == [0, ((32 * 32 + 96 * 96) << 24) + 1, an.NONE]
    assert keys[1].tolist() == [(32 * 32) << 24, 1, an.NONE]                               # the masked pixel adds nothing
    assert keys[2].tolist() == [0, 1, an.NONE]                                            # every pixel masked: distance 0 to all
    nb, dist, found = an.search(lib, cond, 2)
    assert nb.tolist() == [[0, 1], [1, 0], [0, 1]] and dist.tolist() == [[0, 10240], [0, 1024], [0, 0]] and found.tolist() == [2, 2, 2]


def test_integer_square_root():
    r = np.arange(0, 8193, dtype=np.int64)
    sq = r * r
    assert np.array_equal(an.isqrt(sq), r) and np.array_equal(an.isqrt(sq[1:] - 1), r[1:] - 1) and np.array_equal(an.isqrt(sq + 1)[1:], r[1:])
    assert an.isqrt(np.array([0, 1, 2, 3, 4, 2 ** 26 - 1, 2 ** 26])).tolist() == [0, 1, 1, 1, 2, 8191, 8192]
    assert an.isqrt(np.arange(0, 70000)).tolist() == [int(np.floor(np.sqrt(v))) for v in range(70000)]


def test_rank_table_and_picks():
    assert an.rank_table(4).tolist() == [1048576, 1048576 + 524288, 1048576 + 524288 + 349525, 1048576 + 524288 + 349525 + 262144]
    c = an.rank_table(32)
    assert np.all(np.diff(c) > 0) and c[-1] < 2 ** 23
    # the words 0 and 2^32 - 1 pick the first and the last rank; the shares follow 1 / rank
    for f in (1, 2, 5, 32):
        assert an.pick_rank(0, f, "rank") == 0 and an.pick_rank(2 ** 32 - 1, f, "rank") == f - 1
        assert an.pick_rank(0, f, "uniform") == 0 and an.pick_rank(2 ** 32 - 1, f, "uniform") == f - 1
    words = np.arange(0, 2 ** 32, 2 ** 20 + 12345)
    share = np.bincount([an.pick_rank(int(w), 3, "rank") for w in words], minlength=3) / len(words)
    assert np.allclose(share, np.array([6, 3, 2]) / 11, atol=2e-3)
    share = np.bincount([an.pick_rank(int(w), 3, "uniform") for w in words], minlength=3) / len(words)
    assert np.allclose(share, 1 / 3, atol=2e-3)
    # a pick depends on (seed, member, query) only
    nb, found = np.arange(12, dtype=np.int32).reshape(3, 4), np.array([4, 0, 2], np.int32)
    whole = an.picks(nb, found, 6, seed=5)
    assert np.array_equal(whole[:, 2:], an.picks(nb, found, 4, seed=5, first_member=2))
    assert np.array_equal(whole[1:], an.picks(nb[1:], found[1:], 6, seed=5, first_query=1))
    assert np.all(whole[1] == -1) and np.isin(whole[0], nb[0]).all() and np.isin(whole[2], nb[2, :2]).all()
    assert not np.array_equal(whole, an.picks(nb, found, 6, seed=6))
    # the member key is the RainFARM one on another stream: a 64-bit member
    assert an.member_key(1, 2 ** 32) != an.member_key(1, 0) and an.pick_bits(1, 0, 0) != an.pick_bits(1, 0, 1)


def test_apply_by_hand():
    lib = np.zeros((2, 24, 1, 2), np.float32)
    lib[0, 2, 0, 0], lib[0, 5, 0, 0] = 1.0, 3.0                                           # the second pixel of day 0 is dry
    lib[1, :, 0, :] = 0.5
    cond = np.array([[[8.0, 2.0]], [[np.nan, 12.0]]], np.float32)
    out, dry = an.apply(lib, cond, np.array([[0, 1], [0, -1]]))
    assert dry.tolist() == [[[[False, True]], [[False, False]]], [[[False, True]], [[False, False]]]]
    assert out[0, 0, :, 0, 0].tolist() == [0, 0, 2.0] + [0, 0, 6.0] + [0] * 18            # the pixel's own fractions
    assert out[0, 0, :, 0, 1].tolist() == [0, 0, 0.5] + [0, 0, 1.5] + [0] * 18            # the day's areal profile, 1/4 and 3/4
    assert np.allclose(out[0, 1], cond[0] / 24)
    assert np.isnan(out[1, 0, :, 0, 0]).all() and out[1, 0, :, 0, 1].tolist() == [0, 0, 3.0] + [0, 0, 9.0] + [0] * 18
    assert np.isnan(out[1, 1]).all()


class NoDevice(AN.AnalogLibrary):
    """an AnalogLibrary as far as the host checks go: five days of 3 x 4 pixels, no groups, nothing on a device"""

    def __init__(self):
        self.plane_shape, self.n, self.groups, self.device = (3, 4), 5, None, torch.device("cpu")


def test_argument_errors():
    good = np.zeros((5, 24, 3, 4), np.float32)
    for bad in (np.zeros((24, 3)), np.zeros((5, 23, 3, 4)), np.zeros((0, 24, 3, 4)), np.zeros((2, 24, 3, 4), dtype=complex), torch.zeros(2, 24, 3, 4),
                np.broadcast_to(np.float32(0), (2, 24, 65, 64))):
        with pytest.raises(ValueError):
            AN.AnalogLibrary(bad)
    for groups in (np.zeros(4, np.int32), np.zeros(5), np.zeros((5, 1), np.int32), np.array([0, 1, 2, 3, 2 ** 31]), np.zeros(5, bool),
                   torch.zeros(5), torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError):
            AN.AnalogLibrary(good, groups=groups)
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: no CPU fallback
        with pytest.raises(_lib.RdganError):
            AN.AnalogLibrary(good, groups=np.arange(5))
    lib = NoDevice()
    cond = np.zeros((2, 3, 4), np.float32)
    for kw in (dict(cond=np.zeros((3, 4))), dict(cond=np.zeros((2, 4, 3))), dict(cond=np.zeros((0, 3, 4))), dict(cond=torch.zeros(2, 3, 4)), dict(k=0),
               dict(k=33), dict(k=2.0), dict(k=True), dict(query_groups=np.zeros(2, np.int32)), dict(query_groups=np.zeros(3)), dict(workspace_bytes=0),
               dict(workspace_bytes=2 * 8 * 10 * 8 - 1), dict(workspace_bytes=1.5)):
        with pytest.raises(ValueError):
            lib.search(**{**dict(cond=cond), **kw})
    for kw in (dict(n_members=0), dict(n_members=65536), dict(n_members=1.0), dict(k=0), dict(weights="linear"), dict(weights=1), dict(seed=-1),
               dict(seed=2 ** 64), dict(first_member=-1), dict(first_query=-1), dict(first_query=2 ** 32 - 1), dict(cond=np.zeros((2, 3, 5))),
               dict(query_groups=np.zeros(2, np.int32))):
        with pytest.raises(ValueError):
            lib.generate(**{**dict(cond=cond, n_members=3), **kw})
    real = np.zeros((2, 24, 3, 4), np.float32)
    for fn in (AN.generate_one_per_day, AN.crps_for_days):
        for args in ((real, None), (np.zeros((2, 24, 3, 5)), lib), (np.zeros((24, 3, 4)), lib), (torch.zeros(2, 24, 3, 4), lib)):
            with pytest.raises(ValueError):
                fn(*args)
        for kw in (dict(k=0), dict(weights="best"), dict(seed=-1), dict(query_groups=np.zeros(2, np.int32)), dict(query_groups=np.zeros(3, np.int32))):
            with pytest.raises(ValueError):
                fn(real, lib, **kw)
    with pytest.raises(ValueError):
        AN.crps_for_days(real, lib, n_members=0)
    with pytest.raises(ValueError):
        AN.AnalogLibrary.from_dataset(type("D", (), {"indices": None})())
    assert AN.check_weights("rank") == 1 and AN.check_weights("uniform") == 0 and AN.check_k(32) == 32
    assert [AN.query_tile(p) for p in (1, 15, 256, 2048, 2049, 4096)] == [16, 16, 16, 16, 8, 8] and AN.padded_plane(15) == 16


def test_cabi_argument_checks():
    """the four C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    ws = lib.rdgan_analog_workspace_bytes
    assert ws(1, 1, 1) == 64 and ws(1000, 10, 16) == 1000 * 16 * 8 * 10 * 8 and ws(2 ** 18, 32, 1) == 2 ** 18 * 8 * 32 * 8
    for a in ((0, 1, 1), (2 ** 18 + 1, 1, 1), (1, 0, 1), (1, 33, 1), (1, 1, 0), (1, 1, 2 ** 18 + 1), (-1, -1, -1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # 16-byte aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)

    def feat(x=good, n=2, stride=24 * 15, ny=3, nx=5, hourly=1, f=good, m=null, tot=good, void=good, nv=good):
        return lib.rdgan_analog_features(x, n, stride, ny, nx, hourly, f, m, tot, void, nv, st)

    for kw in (dict(x=null), dict(f=null), dict(tot=null), dict(void=null), dict(nv=null), dict(m=good), dict(x=by(2)), dict(f=by(8)), dict(tot=by(4)),
               dict(nv=by(4)), dict(n=0), dict(n=2 ** 24), dict(ny=0), dict(nx=0), dict(ny=65, nx=64, stride=24 * 65 * 64), dict(ny=4097, nx=1, stride=24 * 4097),
               dict(stride=24 * 15 - 1), dict(hourly=0), dict(hourly=0, m=good, tot=null, void=null, nv=null, stride=16), dict(hourly=0, m=by(8), tot=null,
               void=null, nv=null, stride=15), dict(hourly=0, m=good, tot=null, void=null, nv=null, stride=15, n=2 ** 18 + 1),
               dict(hourly=0, m=good, tot=good, void=null, nv=null, stride=15)):
        assert feat(**kw) == -2, kw

    def search(f=good, void=good, lg=null, n=70, plane=15, qf=good, qm=good, qg=null, Q=3, k=4, nb=good, dist=good, found=good, w=good, nbytes=3 * 8 * 4 * 8):
        return lib.rdgan_analog_search(f, void, lg, n, plane, qf, qm, qg, Q, k, nb, dist, found, w, nbytes, st)

    for kw in (dict(f=null), dict(void=null), dict(qf=null), dict(qm=null), dict(nb=null), dict(dist=null), dict(found=null), dict(w=null), dict(f=by(8)),
               dict(qf=by(8)), dict(qm=by(4)), dict(dist=by(4)), dict(w=by(4)), dict(nb=by(2)), dict(found=by(2)), dict(lg=by(2)), dict(qg=by(2)), dict(n=0),
               dict(n=2 ** 24), dict(plane=0), dict(plane=4097), dict(Q=0), dict(Q=2 ** 18 + 1), dict(k=0), dict(k=33), dict(nbytes=3 * 8 * 4 * 8 - 1),
               dict(nbytes=0), dict(nbytes=-8)):
        assert search(**kw) == -2, kw

    def apply(x=good, n=7, stride=24 * 15, ny=3, nx=5, cond=good, Q=3, q0=0, nb=good, found=good, k=4, S=2, m0=0, seed=1, weights=1, out=good, picks=good):
        return lib.rdgan_analog_apply(x, n, stride, ny, nx, cond, Q, q0, nb, found, k, S, m0, seed, weights, out, picks, st)

    for kw in (dict(x=null), dict(cond=null), dict(nb=null), dict(found=null), dict(out=null), dict(picks=null), dict(x=by(2)), dict(cond=by(2)), dict(out=by(2)),
               dict(picks=by(1)), dict(n=0), dict(n=2 ** 24), dict(ny=0), dict(ny=65, nx=64), dict(stride=24 * 15 - 1), dict(Q=0), dict(Q=2 ** 18 + 1), dict(q0=-1),
               dict(q0=2 ** 32 - 2), dict(k=0), dict(k=33), dict(S=0), dict(S=65536), dict(m0=-1), dict(weights=2), dict(weights=-1)):
        assert apply(**kw) == -2, kw


def test_header_and_lib_agree_on_the_analog_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "float*": "c_void_p", "const int*": "c_void_p",
             "int*": "c_void_p", "long long*": "c_void_p", "unsigned short*": "c_void_p", "const unsigned short*": "c_void_p",
             "unsigned char*": "c_void_p", "const unsigned char*": "c_void_p", "unsigned long long": "c_ulong"}
    names = ("rdgan_analog_workspace_bytes", "rdgan_analog_features", "rdgan_analog_search", "rdgan_analog_apply")
    assert tuple(sorted(n for n in _lib.SIGNATURES if "analog" in n)) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_analog_\w+)\(", header, re.M)))) == tuple(sorted(names))
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
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_analog.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (AN.MAX_PLANE, AN.MAX_LIBRARY, AN.MAX_QUERIES, AN.MAX_K, AN.MAX_MEMBERS, AN.BLOCK, AN.WAVES, AN.NHOURS) == tuple(
        value(m) for m in ("RD_AN_MAXP", "RD_AN_MAXN", "RD_AN_MAXQ", "RD_AN_MAXK", "RD_AN_MAXS", "RD_AN_BLOCK", "RD_AN_WAVES", "RD_HOURS"))
    assert (AN.WEIGHTS["uniform"], AN.WEIGHTS["rank"]) == (value("RD_AN_UNIFORM"), value("RD_AN_RANK"))
    assert (AN.query_tile(256), AN.query_tile(4096), 2048) == (value("RD_AN_QT_SMALL"), value("RD_AN_QT_LARGE"), value("RD_AN_QT_SPLIT"))
    assert value("RD_AN_THREADS") == 64 * AN.WAVES and value("RD_AN_WIDEN") * 8 * 8191 ** 2 < 2 ** 32 and AN.UNIT == 1024
    # the LDS of a workgroup stays inside a compute unit's 160 KB at both ends of the plane range
    assert AN.query_tile(4096) * AN.padded_plane(4096) * 4 <= 128 * 1024 and AN.query_tile(2048) * 2048 * 4 <= 128 * 1024
    rng_h = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_rng.h")).read()
    assert re.search(r"^#define RD_STREAM_ANALOG 9u", rng_h, re.M) and AN.STREAM_ANALOG == an.STREAM_ANALOG == 9
