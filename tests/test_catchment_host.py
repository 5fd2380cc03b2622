"""CPU: the catchment map of pr_disagg_radar_gan_amd/catchments.py (lists, chunks, argument checks), its derived quantities, the
numpy restatement of the definitions (tests/catchment_np.py) against answers worked out by hand, and the header against _lib.py
and the kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, catchments as CT
from pr_disagg_radar_gan_amd import raindisagg_gan_pretrained as P
from tests import catchment_np as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#  0  0  1  1
#  0  0  1  1
# -1  2  2  2
REGIONS = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [-1, 2, 2, 2]])


def only(a):
    a = np.asarray(a)
    return {tuple(int(i) for i in idx): int(a[tuple(idx)]) for idx in np.argwhere(a != 0)}


def test_lists_and_chunks_of_labels_and_of_the_equivalent_masks():
    a = CT.CatchmentMap(regions=REGIONS)
    assert a.n_catch == 3 and a.plane_shape == (3, 4) and a.npix.tolist() == [4, 4, 3] and a.offsets.tolist() == [0, 4, 8, 11]
    assert a.pixels.tolist() == [0, 1, 4, 5, 2, 3, 6, 7, 9, 10, 11] and a.chunks.tolist() == [[0, 0, 4], [1, 4, 4], [2, 8, 3]]
    assert (a.npix.dtype, a.pixels.dtype, a.chunks.dtype, a.offsets.dtype) == (np.int32, np.int32, np.int32, np.int64)
    b = CT.CatchmentMap(masks=np.stack([REGIONS == c for c in range(3)]))
    for name in ("npix", "offsets", "pixels", "chunks"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert [m.tolist() for m in cn.members_of(regions=REGIONS)] == [[0, 1, 4, 5], [2, 3, 6, 7], [9, 10, 11]]
    # a larger map: stripes, so that the lists are not contiguous, and catchments of more than one chunk
    rng = np.random.default_rng(3)
    regions = rng.integers(-1, 5, (37, 41))
    regions[:30, 3] = 4                                                                   # (no label is missing)
    a = CT.CatchmentMap(regions=regions)
    b = CT.CatchmentMap(masks=np.stack([regions == c for c in range(5)]))
    for name in ("npix", "offsets", "pixels", "chunks"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    members = cn.members_of(regions=regions)
    assert [a.pixels[a.offsets[c]:a.offsets[c + 1]].tolist() for c in range(5)] == [m.tolist() for m in members]
    CT.check_chunks(a.chunks, a.offsets, a.pixels, 37 * 41)
    assert a.chunks[:, 2].max() == CT.CHUNK and len(a.chunks) == sum(-(-len(m) // CT.CHUNK) for m in members)
    assert np.array_equal(np.bincount(a.chunks[:, 0], weights=a.chunks[:, 2]).astype(np.int64), a.npix)


def test_chunks_at_their_edges():
    for sizes in ((1,), (255, 256, 257), (512, 1, 513)):
        off = np.concatenate([[0], np.cumsum(sizes)])
        ch = CT.make_chunks(off)
        CT.check_chunks(ch, off, np.zeros(off[-1], np.int32), 1)
        assert [ch[ch[:, 0] == c][:, 2].tolist() for c in range(len(sizes))] == [[256] * (s // 256) + ([s % 256] if s % 256 else []) for s in sizes]
    off, pix = np.array([0, 3, 6]), np.arange(6)
    good = np.array([[0, 0, 3], [1, 3, 3]])
    CT.check_chunks(good, off, pix, 6)
    for bad in ([[0, 0, 4], [1, 4, 2]], [[0, 0, 3], [1, 3, 2]], [[0, 0, 3], [2, 3, 3]], [[0, 0, 0], [1, 3, 3]], [[0, 0, 2], [0, 2, 1], [1, 4, 2]],
                [[1, 3, 3], [0, 0, 3]]):
        with pytest.raises(ValueError):
            CT.check_chunks(np.array(bad), off, pix, 6)
    with pytest.raises(ValueError):
        CT.check_chunks(good, off, pix, 5)                                                # the entry 5 lies outside a plane of 5
    with pytest.raises(ValueError):
        CT.check_chunks(np.array([[0, 0, 257]]), np.array([0, 257]), np.zeros(257), 1)


def test_overlapping_masks_list_a_shared_pixel_twice():
    masks = np.zeros((2, 3, 4), bool)
    masks[0] = True                                                                       # the basin
    masks[1, 1:, 2:] = True                                                               # a sub-basin
    m = CT.CatchmentMap(masks=masks, names=("gauge", "upper"))
    assert m.npix.tolist() == [12, 4] and m.pixels.tolist() == list(range(12)) + [6, 7, 10, 11] and m.n_entries == 16
    assert m.names == ("gauge", "upper")


def test_valid_removes_pixels_and_an_emptied_catchment_is_refused_by_name():
    valid = np.ones((3, 4), bool)
    valid[0, 0] = valid[2, 3] = valid[2, 0] = False
    m = CT.CatchmentMap(regions=REGIONS, valid=valid)
    assert m.npix.tolist() == [3, 4, 2] and m.pixels.tolist() == [1, 4, 5, 2, 3, 6, 7, 9, 10]
    assert np.array_equal(m.pixels, CT.CatchmentMap(masks=np.stack([REGIONS == c for c in range(3)]), valid=valid).pixels)
    assert [v.tolist() for v in cn.members_of(regions=REGIONS, valid=valid)] == [[1, 4, 5], [2, 3, 6, 7], [9, 10]]
    valid[2] = False
    with pytest.raises(ValueError, match="catchment 2 .*'south'.* is empty"):
        CT.CatchmentMap(regions=REGIONS, valid=valid, names=("west", "east", "south"))
    with pytest.raises(ValueError, match="catchment 2 is empty"):
        CT.CatchmentMap(masks=np.stack([REGIONS == c for c in range(3)]), valid=valid)


def test_map_argument_errors():
    masks = np.stack([REGIONS == c for c in range(3)])
    gap = np.where(REGIONS == 1, 3, REGIONS)                                              # labels 0, 2, 3: catchment 1 is empty
    for kw in (dict(), dict(regions=REGIONS, masks=masks), dict(regions=np.where(REGIONS < 0, -2, REGIONS)), dict(regions=gap),
               dict(regions=np.full((3, 4), -1)), dict(regions=REGIONS.astype(np.float32)), dict(regions=REGIONS[0]), dict(regions=REGIONS == 1),
               dict(regions=np.zeros((0, 4), np.int64)), dict(masks=masks.astype(np.int8)), dict(masks=masks[0]), dict(masks=np.zeros((0, 3, 4), bool)),
               dict(masks=np.concatenate([masks, np.zeros((1, 3, 4), bool)])), dict(regions=REGIONS, valid=np.ones((4, 3), bool)),
               dict(regions=REGIONS, valid=np.ones((3, 4))), dict(masks=masks, valid=np.ones(12, bool)), dict(regions=REGIONS, names=("a", "b")),
               dict(regions=np.broadcast_to(np.int8(0), (4097, 4096))),                   # a plane above 2^24 pixels
               dict(regions=np.arange(65536).reshape(256, 256)),                         # 65536 catchments
               dict(masks=np.broadcast_to(np.True_, (5, 4096, 4096)))):                  # 5 x 2^24 entries: above 2^26
        with pytest.raises(ValueError):
            CT.CatchmentMap(**kw)
    with pytest.raises(ValueError, match="catchment 1 is empty"):
        CT.CatchmentMap(regions=gap)
    assert CT.CatchmentMap(regions=np.arange(65535).reshape(255, 257)).n_catch == 65535


class NoGenerator:
    ndomain, n_cond_channels = 16, 1


def test_argument_errors_with_no_device(monkeypatch):
    cmap = CT.CatchmentMap(regions=REGIONS)
    ok = dict(windows=(1, 3), levels=(1.0,))
    bad_lists = (dict(windows=()), dict(windows=(3, 1)), dict(windows=(1, 1)), dict(windows=(0, 1)), dict(windows=(25,)), dict(windows=tuple(range(1, 10))),
                 dict(windows=(1.0,)), dict(windows=(True,)), dict(windows=3), dict(levels=(2.0, 1.0)), dict(levels=(1.0, 1.0)), dict(levels=(-0.5,)),
                 dict(levels=(np.nan,)), dict(levels=(np.inf,)), dict(levels=(2048.0 * 24 + 1,)), dict(levels=tuple(range(17))), dict(levels="x"),
                 dict(levels=3.0))
    for kw in bad_lists + (dict(cmap=REGIONS), dict(cmap=None)):
        with pytest.raises(ValueError):
            CT.CatchmentRainfall(**{"cmap": cmap, **ok, **kw})
    for days in (0, 65536, 2.5, True):
        with pytest.raises(ValueError):
            CT.CatchmentRainfall(cmap, **ok, workspace_days=days)
    cr = CT.CatchmentRainfall(cmap, **ok)
    for bad in (np.zeros((24, 5)), np.zeros((23, 3, 4)), np.zeros((2, 25, 3, 4)), np.zeros((0, 24, 3, 4)), np.zeros((24, 3, 4), dtype=complex),
                torch.zeros(24, 3, 4), np.zeros((24, 4, 3), np.float32), np.zeros((24, 3, 5), np.float32)):      # the last two: not the map's plane
        with pytest.raises(ValueError):
            cr.add(bad)
    x = np.zeros((2, 24, 3, 4), np.float32)
    for kw in (dict(series_out=torch.zeros(2, 3, 24, dtype=torch.int64)), dict(depths_out=torch.zeros(2, 3, 2, dtype=torch.int64))):       # on the host
        with pytest.raises(ValueError):
            cr.add(x, **kw)
    with pytest.raises(ValueError):
        cr.state()
    for kw in (dict(return_series=True), dict(return_depths=True), dict()):
        with pytest.raises(ValueError):
            CT.catchment_rainfall(torch.zeros(24, 3, 4), cmap, (1,), **kw)
        with pytest.raises(ValueError):
            CT.catchment_rainfall(np.zeros((24, 4, 4), np.float32), cmap, (1,), **kw)
    for bad in (np.zeros((2, 3, 24), np.int64), torch.zeros(2, 3, 24, dtype=torch.int64)):                        # not on the device
        with pytest.raises(ValueError):
            CT.series_mm(bad, cmap)
    assert cr.reset() is cr and cr.plane_shape is None
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: there is no CPU fallback
        for kw in (dict(), dict(return_series=True, return_depths=True)):
            with pytest.raises(_lib.RdganError):
                CT.catchment_rainfall(x, cmap, **ok, **kw)

    big = CT.CatchmentMap(regions=np.arange(20 * 30).reshape(20, 30) % 7)
    good = dict(daily=np.zeros((20, 30), np.float32), n_scenarios=3, cmap=big, **ok)
    bad_field = bad_lists + (dict(cmap=cmap), dict(cmap=None), dict(n_scenarios=0), dict(scenario_chunk=0), dict(overlap=9), dict(latent_mode="each"),
                             dict(daily=np.zeros((2, 2, 20, 30), np.float32)), dict(daily=np.zeros((20, 31), np.float32)))
    for kw in bad_field + (dict(daily=torch.zeros(20, 30)), dict(workspace_days=0), dict(chunk=0), dict(norm_scale=0.0)):
        with pytest.raises(ValueError):
            CT.catchment_rainfall_field(**{**good, "gen": NoGenerator(), **kw})
    monkeypatch.setattr(P, "gen", NoGenerator())
    for kw in bad_field:
        with pytest.raises(ValueError):
            P.catchment_rainfall_field(**{**good, **kw})


def test_restatement_against_answers_by_hand():
    """The 3 x 4 plane above, one day, windows (1, 2, 24), levels 1 and 2 mm of catchment mean.
    Catchment 0 (4 pixels): 0.5 mm on every pixel in the hours 3, 4, 10 and 11, so P = 4 * 512 = 2048 there.  k = 1: 2048, four
    hours tie, the earliest is 3.  k = 2: hours 3-4 and 10-11 both give 4096, the tie goes to h0 = 3; 4096 == 1024 * 4 pixels sits
    exactly on the 1 mm level: reached.  k = 24: 8192 == 2048 * 4, exactly the 2 mm level: both reached; h0 = 0.
    Catchment 1 (4 pixels): 1 mm on pixel 2 in the hours 5 and 7, a NaN on pixel 7 in hour 6.  Hour 6 is void.  k = 1: 1024 at
    h0 = 5.  k = 2: the windows from 5 and from 6 hold hour 6 and are void; from 4 (hours 4-5) and from 7 (hours 7-8) give 1024,
    the earlier is 4.  k = 24 holds hour 6: void.  1024 is below 1 mm * 4 pixels: no level.
    Catchment 2 (3 pixels): no rain: dry for every window, counted, in level_count[0], in no start hour.
    Pixel 8 lies in no catchment: its inf changes nothing."""
    x = np.zeros((1, 24, 3, 4), np.float32)
    x[0, [3, 4, 10, 11], :2, :2] = 0.5
    x[0, [5, 7], 0, 2] = 1.0
    x[0, 6, 1, 3] = np.nan
    x[0, 0, 2, 0] = np.inf
    o, series, depths = cn.catchment_np(x, cn.members_of(regions=REGIONS), (1, 2, 24), (1.0, 2.0))
    assert depths.tolist() == [[[2048, 4096, 8192], [1024, 1024, -1], [0, 0, 0]]]
    assert only(series[0, 0]) == {(3,): 2048, (4,): 2048, (10,): 2048, (11,): 2048}
    assert only(series[0, 1]) == {(5,): 1024, (6,): -1, (7,): 1024} and not series[0, 2].any()
    assert only(o["start_hour"]) == {(0, 0, 3): 1, (0, 1, 3): 1, (0, 2, 0): 1, (1, 0, 5): 1, (1, 1, 4): 1}
    assert only(o["level_count"]) == {(0, 0, 0): 1, (0, 1, 1): 1, (0, 2, 2): 1, (1, 0, 0): 1, (1, 1, 0): 1, (2, 0, 0): 1, (2, 1, 0): 1, (2, 2, 0): 1}
    assert o["n_void"].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]] and o["n_dry"].tolist() == [[0] * 3, [0] * 3, [1] * 3]
    assert o["n_days"].tolist() == [[1, 1, 1], [1, 1, 0], [1, 1, 1]] and o["n_bad"] == 1 and o["n_days_total"] == 1
    assert np.array_equal(o["sum_A"], np.maximum(depths[0], 0)) and np.array_equal(o["max_A"], o["sum_A"])
    cn.check_identities(o)
    # one unit below the level is not reached: 0.5 mm less one unit on one pixel in one hour
    x[0, 3, 0, 0] = 511 / 1024
    o, _, depths = cn.catchment_np(x, cn.members_of(regions=REGIONS), (1, 2, 24), (1.0, 2.0))
    assert depths[0, 0].tolist() == [2048, 4096, 8191] and only(o["start_hour"][0]) == {(0, 4): 1, (1, 10): 1, (2, 0): 1}
    assert only(o["level_count"][0]) == {(0, 0): 1, (1, 1): 1, (2, 1): 1}
    # with the pixel of the NaN dropped by `valid`, catchment 1 has no void hour; a pixel in two catchments counts in both
    valid = np.ones((3, 4), bool)
    valid[1, 3] = False
    o, series, depths = cn.catchment_np(x, cn.members_of(regions=REGIONS, valid=valid), (1, 2, 24), ())
    assert depths[0, 1].tolist() == [1024, 1024, 2048] and o["n_bad"] == 0 and series[0, 1, 6] == 0
    masks = np.stack([np.ones((3, 4), bool), REGIONS == 1])
    o, series, depths = cn.catchment_np(x, cn.members_of(masks=masks), (24,), ())
    assert o["n_bad"] == 3 and depths.tolist() == [[[-1], [-1]]]                          # the inf once, the NaN twice
    # ties to even and the bad-value rule, as in the areal yardstick
    assert cn.quantise(np.array([0.5, 1.5, 2.5], np.float32) / 1024)[0].tolist() == [0, 2, 2]
    assert cn.quantise(np.array([np.nan, -np.inf, -1e-9, 2048.0, 2047.9999, -0.0], np.float32))[1].tolist() == [True, True, True, True, False, False]


def hand_state():
    """C = 2 catchments of 4 and 2 pixels, K = 1 window, L = 2 levels (1, 4 mm): four days; the second catchment has one void day"""
    o = cn.empty_state(2, 1, 2)
    o["n_days_total"], o["n_bad"] = 4, 7
    o["n_days"][:, 0], o["n_void"][:, 0], o["n_dry"][:, 0] = (4, 3), (0, 1), (1, 1)
    o["level_count"][0, 0], o["level_count"][1, 0] = (1, 1, 2), (2, 1, 0)
    o["start_hour"][0, 0, [0, 5]], o["start_hour"][1, 0, [0, 6]] = (1, 2), (1, 1)
    o["sum_A"][:, 0], o["max_A"][:, 0] = (48 * 1024, 6 * 1024), (24 * 1024, 4 * 1024)
    return o


def test_derived_quantities_on_a_hand_made_state():
    s = CT.stats_from_state(cn.flat_state(hand_state()), (4, 2), (3,), (1.0, 4.0), names=("a", "b"))
    assert s.windows == (3,) and s.levels == (1.0, 4.0) and s.n_days_total == 4 and s.n_bad == 7 and s.names == ("a", "b")
    # 48 mm-pixels over 4 days and 4 pixels; 6 over 3 days and 2 pixels
    assert np.allclose(s.mean_depth(), [[3.0], [1.0]]) and np.allclose(s.max_depth(), [[6.0], [2.0]])
    assert np.allclose(s.exceedance(), [[[0.75, 0.5]], [[1 / 3, 0.0]]])
    assert only(s.start_hour_distribution() * 6) == {(0, 0, 0): 2, (0, 0, 5): 4, (1, 0, 0): 3, (1, 0, 6): 3}
    none = CT.stats_from_state(np.zeros(CT.state_count(2, 1, 2), np.int64), (4, 2), (3,), (1.0, 4.0))
    for q in (none.mean_depth(), none.max_depth(), none.exceedance(), none.start_hour_distribution()):
        assert np.all(np.isnan(q))
    assert none.exceedance().shape == (2, 1, 2) and none.start_hour_distribution().shape == (2, 1, 24)
    assert CT.stats_from_state(np.zeros(CT.state_count(2, 1, 0), np.int64), (4, 2), (3,), ()).exceedance().shape == (2, 1, 0)
    for npix in ((4,), (4, 0), ()):
        with pytest.raises(ValueError):
            CT.stats_from_state(cn.flat_state(hand_state()), npix, (3,), (1.0, 4.0))
    # compare
    c = CT.compare(s, s)
    assert all(np.all(c[k] == 0) for k in ("mean_depth", "exceedance", "tv_start_hour")) and c["exceedance"].shape == (2, 1, 2)
    o2 = hand_state()
    o2["start_hour"][0, 0, [0, 5]] = (2, 1)
    o2["sum_A"][0, 0] = 64 * 1024
    c = CT.compare(s, CT.stats_from_state(cn.flat_state(o2), (4, 2), (3,), (1.0, 4.0)))
    assert np.allclose(c["tv_start_hour"], [[1 / 3], [0.0]]) and c["mean_depth"].tolist() == [[-1.0], [0.0]]
    flat = cn.flat_state(hand_state())
    for other in (CT.stats_from_state(flat, (4, 2), (4,), (1.0, 4.0)), CT.stats_from_state(flat, (4, 2), (3,), (1.0, 5.0)),
                  CT.stats_from_state(flat, (4, 3), (3,), (1.0, 4.0)), None):
        with pytest.raises(ValueError):
            CT.compare(s, other)


def test_state_count_and_layout_round_trip():
    C, K, L = 3, 2, 2
    rec = L + 30
    assert CT.state_count(C, K, L) == C * K * rec + 2 and CT.state_count(65535, 8, 16) == 65535 * 8 * 46 + 2
    flat = np.arange(CT.state_count(C, K, L))
    d = CT.split_state(flat, C, K, L)
    assert d["level_count"][0, 1].tolist() == [rec, rec + 1, rec + 2] and d["start_hour"][0, 0, 0] == L + 1 and d["start_hour"][0, 0, 23] == L + 24
    assert [int(d[k][0, 0]) for k in ("sum_A", "max_A", "n_days", "n_void", "n_dry")] == list(range(L + 25, L + 30))
    assert d["n_dry"][2, 1] == C * K * rec - 1 and d["n_days_total"] == C * K * rec and d["n_bad"] == C * K * rec + 1
    assert np.array_equal(cn.flat_state(d), flat)                                         # the yardstick's order is the module's
    with pytest.raises(ValueError):
        CT.split_state(np.zeros(5), 1, 1, 0)


def test_cabi_argument_checks():
    """the three C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    count = lib.rdgan_catchment_state_count
    assert [count(*a) for a in ((1, 1, 0), (65535, 8, 16), (3, 2, 2), (0, 1, 0), (65536, 1, 0), (1, 0, 0), (1, 9, 0), (1, 1, -1), (1, 1, 17))] == \
        [32, 65535 * 8 * 46 + 2, CT.state_count(3, 2, 2), -2, -2, -2, -2, -2, -2]
    ws = lib.rdgan_catchment_workspace_bytes
    assert ws(1, 1) == 288 and ws(3, 5) == 15 * 288 and ws(65535, 65535) == 65535 * 65535 * 288
    for a in ((0, 1), (65536, 1), (3, 0), (3, 65536), (-1, 1)):
        assert ws(*a) == -2, a
    buf = (ctypes.c_double * 64)()
    good_p = ctypes.c_void_p(ctypes.addressof(buf))                                       # 8-byte aligned, never read: every call below is refused
    odd_p = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    four_p = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    null = ctypes.c_void_p(0)
    ip = lambda *v: np.array(v, np.int32).ctypes.data_as(ctypes.c_void_p)
    dp = lambda *v: np.array(v, np.float64).ctypes.data_as(ctypes.c_void_p)

    def acc(x=good_p, n=1, stride=24 * 12, ny=3, nx=4, chunks=good_p, n_chunks=3, pixels=good_p, E=11, npix=good_p, C=3, k=ip(1, 3), K=2,
            lv=dp(1.0, 2.0), L=2, counts=good_p, series=null, depths=null, ws=good_p, nbytes=3 * 288):
        return lib.rdgan_catchment_accumulate(x, n, stride, ny, nx, chunks, n_chunks, pixels, E, npix, C, k, K, lv, L, counts, series, depths, ws,
                                              nbytes, ctypes.c_void_p(0))

    for kw in (dict(x=null), dict(chunks=null), dict(pixels=null), dict(npix=null), dict(counts=null), dict(ws=null), dict(k=null), dict(lv=null),
               dict(x=odd_p), dict(chunks=odd_p), dict(pixels=odd_p), dict(npix=odd_p), dict(counts=four_p), dict(series=four_p), dict(depths=four_p),
               dict(ws=four_p), dict(n=0), dict(n=-1), dict(ny=0), dict(nx=0), dict(ny=-3), dict(ny=4097, nx=4096), dict(n=2 ** 40),
               dict(stride=24 * 12 - 1), dict(C=0), dict(C=-1), dict(C=65536), dict(C=12), dict(E=2), dict(E=2 ** 26 + 1), dict(n_chunks=2),
               dict(n_chunks=12), dict(n_chunks=2 ** 19 + 1, E=2 ** 20), dict(K=0), dict(K=9), dict(k=ip(3, 1)), dict(k=ip(1, 1)), dict(k=ip(0, 1)),
               dict(k=ip(1, 25)), dict(L=-1), dict(L=17), dict(lv=dp(2.0, 1.0)), dict(lv=dp(1.0, 1.0)), dict(lv=dp(-1.0, 1.0)), dict(lv=dp(np.nan, 1.0)),
               dict(lv=dp(1.0, np.inf)), dict(lv=dp(1.0, 49153.0)), dict(nbytes=3 * 288 - 1), dict(nbytes=0), dict(nbytes=-5)):
        assert acc(**kw) == -2, kw


def test_header_lib_and_kernel_constants_agree():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "const double*": "c_void_p",
             "const int*": "c_void_p", "long long*": "c_void_p"}
    names = ("rdgan_catchment_state_count", "rdgan_catchment_workspace_bytes", "rdgan_catchment_accumulate")
    assert tuple(sorted(n for n in _lib.SIGNATURES if "catchment" in n)) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_catchment_\w+)\(", header, re.M)))) == tuple(sorted(names))
    for name in names:
        m = re.search(r"^(\w+) " + name + r"\(([^)]*)\);", header, re.M | re.S)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        params = [" ".join(p.split()[:-1]) for p in m.group(2).replace("\n", " ").split(",")]
        assert res.__name__ == ctype[m.group(1)] and len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ctype[p], (name, p, a)
    # the record the header lists is the one of the constants, L = 0
    block = header[header.index("Catchment rainfall of hourly fields"):]
    listed = dict((name, int(off or 0)) for off, name in re.findall(r"^ \*\s+(?:L \+ (\d+)|0)\s+(\w+)", block, re.M)[:7])
    offsets = (0, CT._START, CT._SUM_A, CT._MAX_A, CT._NDAYS, CT._NVOID, CT._NDRY)
    assert listed == {name: (off + 1 if name != "level_count" else 0) for name, off in zip(cn.ORDER, offsets)}
    assert f"C * K * (L + {CT.N_FIXED + 1}) + 2" in header
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_catchment.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    assert (CT.CHUNK, CT.MAX_CATCHMENTS, CT.MAX_PLANE, CT.MAX_ENTRIES, CT.MAX_PASS, CT.MAX_GROUPS, CT.N_FIXED, CT.NHOURS) == tuple(
        value(m) for m in ("RD_CT_CHUNK", "RD_CT_MAXCATCH", "RD_HOURLY_MAXPLANE", "RD_CT_MAXENTRIES", "RD_CT_MAXPASS", "RD_CT_MAXGROUPS", "RD_CT_FIXED",
                           "RD_HOURS"))
    assert offsets[1:] == tuple(value(m) for m in ("RD_CT_START", "RD_CT_SUM_A", "RD_CT_MAX_A", "RD_CT_NDAYS", "RD_CT_NVOID", "RD_CT_NDRY"))
    assert value("RD_CT_MAXCHUNKS") > CT.MAX_ENTRIES // CT.CHUNK + CT.MAX_CATCHMENTS and value("RD_CT_CHUNK") == value("RD_CT_THREADS")
    from pr_disagg_radar_gan_amd import areal as AR
    assert (value("RD_CT_MAXK"), value("RD_CT_MAXL")) == (AR.MAX_WINDOWS, AR.MAX_LEVELS)
