"""CPU: the numpy restatement of the cascade definitions (tests/cascade_np.py) in its two forms against each other and against counts
written out by hand; the model's thresholds and fallback chain; the argument checks of pr_disagg_radar_gan_amd/cascade.py and of
the C entries; header against _lib.py and the kernel's constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _lib, cascade as C, multivariate as MV
from tests import cascade_np as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO, START, ENCL, END = range(4)


def day(**hours):
    """one pixel-day (1, 24, 1, 1): day(h0=1.0, h5=0.25) has 1 mm in hour 0 and 0.25 mm in hour 5"""
    x = np.zeros((1, 24, 1, 1), np.float32)
    for k, v in hours.items():
        x[0, int(k[1:]), 0, 0] = v
    return x


def counts(state, NV=3):
    """the non-zero counters of a state by name: {("type", level, pos, vclass, kind): n, ("weight", level, pos, vclass, bin): n,
    ("pattern", vclass, mask): n, ("w2", vclass, mask, bin): n, ("w3a" | "w3b", vclass, bin): n, ("n_days" | "n_bad" | "n_dry",): n}"""
    off, out = cn.offsets(NV), {}
    for i in np.flatnonzero(state):
        i, n = int(i), int(state[i])
        if i >= off["tail"]:
            out[(("n_days", "n_bad", "n_dry")[i - off["tail"]],)] = n
        elif i >= off["w3a"]:
            name, j = ("w3a", i - off["w3a"]) if i < off["w3b"] else ("w3b", i - off["w3b"])
            out[(name, j // 32, j % 32)] = n
        elif i >= off["w2"]:
            j = i - off["w2"]
            out[("w2", j // 256, j // 32 % 8, j % 32)] = n
        elif i >= off["pattern"]:
            j = i - off["pattern"]
            out[("pattern", j // 8, j % 8)] = n
        else:
            name, width, j = ("type", 3, i) if i < off["weight"] else ("weight", 32, i - off["weight"])
            row, k = divmod(j, width)
            out[(name, row // (4 * NV), row // NV % 4, row % NV, k)] = n
    return out


# With the default edges (0.1, 1.0) mm/h the integer thresholds are 102 and 1024 per hour: a 2 h box is of class 1 from 204 units and
# of class 2 from 2048; a 4 h box from 408 and 4096; an 8 h box from 816 and 8192; the day from 2448 and 24576.
HAND = [
    # 1 mm in hour 0: every node passes all of it to its first half (1/0); isolated at every level
    (day(h0=1.0), {("pattern", 0, 1): 1, ("type", 0, ISO, 1, 1): 1, ("type", 1, ISO, 1, 1): 1, ("type", 2, ISO, 1, 1): 1}),
    # 1 mm in hour 1: the 2 h box's first half is dry (0/1)
    (day(h1=1.0), {("pattern", 0, 1): 1, ("type", 0, ISO, 1, 1): 1, ("type", 1, ISO, 1, 1): 1, ("type", 2, ISO, 1, 0): 1}),
    # 0.25 and 0.75 mm in hours 0 and 1: x/(1-x) at the 2 h box, bin 256 * 32 / 1024 = 8
    (day(h0=0.25, h1=0.75), {("pattern", 0, 1): 1, ("type", 0, ISO, 1, 1): 1, ("type", 1, ISO, 1, 1): 1, ("type", 2, ISO, 1, 2): 1,
                             ("weight", 2, ISO, 1, 8): 1}),
    # six wet hours 0 .. 5 of 1 mm: the 2 h boxes 0, 1, 2 are starting, enclosed, ending (2048 units: class 2, halves equal: bin 16); the
    # 4 h boxes hold 4096 (class 2, starting, bin 16) and 2048 (class 1, ending, all in the first half); the 8 h box holds 6144 (class
    # 1, isolated, 4096 * 32 / 6144 = 21); the day 6144 >= 2448: class 1, pattern 1
    (day(h0=1, h1=1, h2=1, h3=1, h4=1, h5=1),
     {("pattern", 1, 1): 1, ("type", 0, ISO, 1, 2): 1, ("weight", 0, ISO, 1, 21): 1, ("type", 1, START, 2, 2): 1, ("weight", 1, START, 2, 16): 1,
      ("type", 1, END, 1, 1): 1, ("type", 2, START, 2, 2): 1, ("weight", 2, START, 2, 16): 1, ("type", 2, ENCL, 2, 2): 1,
      ("weight", 2, ENCL, 2, 16): 1, ("type", 2, END, 2, 2): 1, ("weight", 2, END, 2, 16): 1}),
    # 1 mm in hour 0 and 2 mm in hour 8: pattern 3, the first wet third's bin 1024 * 32 / 3072 = 10; the 8 h boxes are starting and
    # ending; below them every box is isolated.  The box of 2048 units is of class 1 at 8 h and 4 h and of class 2 at 2 h.
    (day(h0=1.0, h8=2.0),
     {("pattern", 1, 3): 1, ("w2", 1, 3, 10): 1, ("type", 0, START, 1, 1): 1, ("type", 0, END, 1, 1): 1, ("type", 1, ISO, 1, 1): 2,
      ("type", 2, ISO, 1, 1): 1, ("type", 2, ISO, 2, 1): 1}),
    # the first and the last third wet: pattern 5; the 8 h boxes are both isolated
    (day(h7=0.5, h23=0.5),
     {("pattern", 0, 5): 1, ("w2", 0, 5, 16): 1, ("type", 0, ISO, 0, 0): 2, ("type", 1, ISO, 1, 0): 2, ("type", 2, ISO, 1, 0): 2}),
    # three wet thirds: 1, 1 and 2 mm in hours 0, 8, 16: b1 = 1024 * 32 / 4096 = 8, b2 = 1024 * 32 / 3072 = 10; starting, enclosed, ending
    (day(h0=1.0, h8=1.0, h16=2.0),
     {("pattern", 1, 7): 1, ("w3a", 1, 8): 1, ("w3b", 1, 10): 1, ("type", 0, START, 1, 1): 1, ("type", 0, ENCL, 1, 1): 1,
      ("type", 0, END, 1, 1): 1, ("type", 1, ISO, 1, 1): 3, ("type", 2, ISO, 1, 1): 2, ("type", 2, ISO, 2, 1): 1}),
]


def test_counts_by_hand():
    total = {}
    for x, expect in HAND:
        got = counts(cn.accumulate(x))
        assert got.pop(("n_days",)) == 1 and got == expect, (x.ravel().tolist(), got, expect)
        assert np.array_equal(cn.accumulate(x), cn.accumulate_scalar(x))
        for k, v in expect.items():
            total[k] = total.get(k, 0) + v
    # all of them as one array, with a dry day and one bad day of each kind: the counts add up
    bad = [day(h3=np.nan), day(h3=np.inf), day(h3=-1.0), day(h3=2048.0)]
    every = np.concatenate([x for x, _ in HAND] + [day()] + bad)
    total.update({("n_days",): len(HAND) + 5, ("n_dry",): 1, ("n_bad",): 4})
    assert counts(cn.accumulate(every)) == total
    assert counts(cn.accumulate(day(h3=np.float32(2047.9999)))) [("n_days",)] == 1 and ("n_bad",) not in counts(cn.accumulate(day(h3=2047.0)))
    # every position class and every type occurs among the hand-made days
    assert {k[2] for k in total if k[0] == "type"} == {ISO, START, ENCL, END} and {k[4] for k in total if k[0] == "type"} == {0, 1, 2}


def test_the_two_forms_agree_on_random_days():
    rng = np.random.default_rng(3)
    x = (rng.gamma(0.5, 2.0, (7, 24, 3, 5)) * (rng.random((7, 24, 3, 5)) < 0.3)).astype(np.float32)
    x[1] = 0.0
    x[2, 5, 1, 1], x[3, 0, 0, 0], x[3, 1, 0, 0] = np.nan, -1.0, np.inf
    for edges in ((), (0.5,), (0.1, 1.0), (0.01, 0.05, 0.1, 0.5, 1.0, 2.0, 5.0)):
        a, b = cn.accumulate(x, edges), cn.accumulate_scalar(x, edges)
        assert np.array_equal(a, b) and len(a) == cn.state_size(len(edges)) == C.state_size(len(edges))
        NV, off = len(edges) + 1, cn.offsets(len(edges) + 1)
        assert a[off["tail"]:].tolist() == [7 * 15, 2, 15] and a[off["pattern"]:off["w2"]].sum() == 7 * 15 - 17
        # a type-2 count is a weight count; a two- or three-wet pattern is a w2 or w3 count
        assert a[off["weight"]:off["pattern"]].sum() == a[:off["weight"]].reshape(-1, 3)[:, 2].sum()
        pat = a[off["pattern"]:off["w2"]].reshape(NV, 8)
        assert pat[:, 0].sum() == 0 and a[off["w3a"]:off["w3b"]].sum() == a[off["w3b"]:off["tail"]].sum() == pat[:, 7].sum()
        assert a[off["w2"]:off["w3a"]].sum() == pat[:, [3, 5, 6]].sum()
    assert C.offsets(3) == cn.offsets(3)


def test_thresholds_and_fallback_chain():
    assert cn.cumulative([1, 0, 3]) == [1 << 22, 1 << 22, 1 << 24] and cn.cumulative([0, 0, 7]) == [0, 0, 1 << 24]
    assert cn.cumulative([1, 1, 1]) == [(1 << 24) // 3, (2 << 24) // 3, 1 << 24]
    state = sum(cn.accumulate(x) for x, _ in HAND)
    table, fallbacks = cn.build_model(state, 2)
    assert np.array_equal(table, C.thresholds_from_state(state, 2)) and table.dtype == np.uint32
    off, t = cn.offsets(3), table.astype(np.int64)
    rows = [(off["type"], off["weight"], 3), (off["weight"], off["pattern"], 32), (off["pattern"], off["w2"], 8), (off["w2"], off["tail"], 32)]
    for a, b, width in rows:                                                              # every row: non-decreasing, the last 2^24
        r = t[a:b].reshape(-1, width)
        assert np.all(np.diff(r, axis=1) >= 0) and np.all(r[:, -1] == 1 << 24) and r.min() >= 0
    type_row = lambda L, pos, v: t[((L * 4 + pos) * 3 + v) * 3:((L * 4 + pos) * 3 + v) * 3 + 3].tolist()
    weight_row = lambda L, pos, v: t[off["weight"] + ((L * 4 + pos) * 3 + v) * 32:off["weight"] + ((L * 4 + pos) * 3 + v + 1) * 32].tolist()
    # its own counts: level 2, isolated, class 1 saw 0/1 three times, 1/0 four times, x/(1-x) once
    assert type_row(2, ISO, 1) == cn.cumulative([3, 4, 1]) and ("type", (2, ISO, 1)) not in fallbacks
    # step 1: level 2, enclosed, class 1 is empty; pooled over the positions it is the isolated row
    assert fallbacks[("type", (2, ENCL, 1))] == 1 and type_row(2, ENCL, 1) == type_row(2, ISO, 1)
    # step 2: level 0, class 2 is empty at every position; pooled over positions and classes: 0/1 twice, 1/0 eight times, x/(1-x) once
    assert fallbacks[("type", (0, ISO, 2))] == 2 and type_row(0, ISO, 2) == cn.cumulative([2, 8, 1])
    # step 3: a state with one sample has no x/(1-x) split at all: every weight row is bin 16
    lone, lone_fb = cn.build_model(cn.accumulate(HAND[0][0]), 2)
    assert lone_fb[("weight", (1, END, 0))] == 3 and lone_fb[("w2", (1, 3))] == 3 and lone_fb[("type", (0, ENCL, 2))] == 2
    w = lone[off["weight"]:off["weight"] + 32].astype(np.int64).tolist()
    assert w == [0] * 16 + [1 << 24] * 16 and np.array_equal(lone, C.thresholds_from_state(cn.accumulate(HAND[0][0]), 2))
    assert weight_row(1, START, 2) == [0] * 16 + [1 << 24] * 16                           # its own single sample happens to be bin 16 too
    # the day's rows pool over the volume classes: class 2 saw no day
    assert fallbacks[("pattern", (2, 0))] == 1 and t[off["pattern"] + 16:off["pattern"] + 24].tolist() == cn.cumulative([0, 4, 0, 1, 0, 1, 0, 1])
    # an all-dry state is refused, by both
    dry = cn.accumulate(np.zeros((2, 24, 2, 2), np.float32))
    for build in (lambda: cn.build_model(dry, 2), lambda: C.thresholds_from_state(dry, 2), lambda: C.CascadeModel(dry),
                  lambda: C.thresholds_from_state(state[:-1], 2), lambda: C.thresholds_from_state(-state, 2)):
        with pytest.raises(ValueError):
            build()
    p = C.CascadeModel(state).probabilities()
    assert p["type"].shape == (3, 4, 3, 3) and p["weight"].shape == (3, 4, 3, 32) and p["pattern"].shape == (3, 8) and p["w2"].shape == (3, 8, 32)
    assert all(np.allclose(v.sum(axis=-1), 1.0, atol=1e-6) and v.min() >= 0 for v in p.values())
    assert np.allclose(p["type"][2, ISO, 1], [3 / 8, 4 / 8, 1 / 8], atol=1e-7)
    assert all(np.array_equal(v, cn.probabilities(table, 2)[k]) for k, v in p.items())


def test_generation_rules_by_hand():
    """the mirror's generation on models whose every draw is forced"""
    # calibrated on "1 mm in hour 0" alone: pattern 1, and every level hands all to the first half
    model, _ = cn.build_model(cn.accumulate(HAND[0][0]), 2)
    cond = np.array([[[0.0, 1.0 / 1024, 3.5, np.nan, -1.0, np.inf, 16384.0, np.float32(16383.999)]]], np.float32)
    out, units = cn.generate(model, (0.1, 1.0), cond, 2, seed=1)
    assert out.shape == units.shape == (1, 2, 24, 1, 8) and out.dtype == np.float32 and units.dtype == np.int32
    assert units[0, :, :, 0, 0].tolist() == [[0] * 24] * 2 and units[0, :, :, 0, 1].tolist() == [[1] + [0] * 23] * 2
    assert units[0, 0, :, 0, 2].tolist() == [3584] + [0] * 23 and out[0, 0, 0, 0, 2] == 3.5
    assert np.all(units[0, :, :, 0, 3:7] == -1) and np.isnan(out[0, :, :, 0, 3:7]).all()
    assert units[0, 1, 0, 0, 7] == (1 << 24) - 1 and out[0, 1, 0, 0, 7] == np.float32(16383.999)
    # calibrated on the six wet hours: 8 h box x/(1-x) in bin 21, the 4 h boxes bin 16 or 1/0, the 2 h boxes bin 16
    model, _ = cn.build_model(cn.accumulate(HAND[3][0]), 2)
    out, units = cn.generate(model, (0.1, 1.0), np.full((1, 1, 1), 6.0, np.float32), 50, seed=2)
    u = units[0, :, :, 0, 0].astype(np.int64)
    assert np.all(u.sum(axis=1) == 6144) and np.all(u[:, 8:] == 0) and np.all(u[:, :4].sum(axis=1) * 32 // 6144 == 21)
    assert np.all(u[:, 6:8] == 0) and np.all(u[:, 4:6].sum(axis=1) > 0)                      # hours 4 .. 7: an ending 4 h box of class 1: 1/0
    # V = 1: the 8 h and 2 h rows (pooled: x/(1-x) alone) have no mass on 0/1 and 1/0 and go evenly by the draw's top bit; the 4 h row,
    # pooled, is 1/0 and x/(1-x) in equal parts, of which 1/0 alone is left: the unit lands in hour 0, 1, 4 or 5
    out, units = cn.generate(model, (0.1, 1.0), np.full((1, 1, 1), 1.0 / 1024, np.float32), 400, seed=3)
    share = units[0, :, :, 0, 0].astype(np.int64).sum(axis=0) / 400
    assert np.all(units.sum(axis=2) == 1) and share[[2, 3, 6, 7]].sum() + share[8:].sum() == 0
    assert np.all(np.abs(share[[0, 1, 4, 5]] - 1 / 4) < 5 * np.sqrt(3 / 16 / 400))
    # the split itself
    assert cn.split(np.array([1000]), np.array([16]), np.array([0]), np.array([999])).tolist() == [500]
    assert cn.split(np.array([1000]), np.array([0]), np.array([0]), np.array([999])).tolist() == [1]             # never 0 ...
    assert cn.split(np.array([1000]), np.array([31]), np.array([(1 << 24) - 1]), np.array([999])).tolist() == [999]      # ... nor all
    assert cn.split(np.array([(1 << 24) - 1]), np.array([31]), np.array([(1 << 24) - 1]), np.array([1 << 24])).tolist() == [(1 << 24) - 2]
    # a pick depends on (seed, member, query, block) only
    rng = np.random.default_rng(5)
    x = (rng.gamma(0.5, 2.0, (12, 24, 3, 4)) * (rng.random((12, 24, 3, 4)) < 0.4)).astype(np.float32)
    model, _ = cn.build_model(cn.accumulate(x), 2)
    cond = x[:3].sum(axis=1)
    whole = cn.generate(model, (0.1, 1.0), cond, 4, seed=7)[1]
    assert np.array_equal(whole[:, 2:], cn.generate(model, (0.1, 1.0), cond, 2, seed=7, first_member=2)[1])
    assert np.array_equal(whole[1:], cn.generate(model, (0.1, 1.0), cond[1:], 4, seed=7, first_query=1)[1])
    assert not np.array_equal(whole, cn.generate(model, (0.1, 1.0), cond, 4, seed=8)[1])
    assert np.array_equal(whole.astype(np.int64).sum(axis=2), np.broadcast_to(np.rint(cond * 1024).astype(np.int64)[:, None], (3, 4, 3, 4)))
    same = np.broadcast_to(cond[:, :1, :1], cond.shape)
    tile = cn.generate(model, (0.1, 1.0), same, 2, seed=7, patch=4)[1]
    assert np.all(tile == tile[..., :1, :1])
    two = cn.generate(model, (0.1, 1.0), same, 2, seed=7, patch=2)[1]
    assert np.all(two[..., :2, :2] == two[..., :1, :1]) and np.all(two[..., 2:, 2:] == two[..., 2:3, 2:3]) and not np.all(two == two[..., :1, :1])
    assert cn.member_key(1, 2 ** 32, 0) != cn.member_key(1, 0, 0) and cn.member_key(1, 0, 1) != cn.member_key(1, 1, 0)


class NoDevice(C.CascadeModel):
    """a CascadeModel as far as the host checks go"""

    def __init__(self):
        super().__init__(sum(cn.accumulate(x) for x, _ in HAND))


def test_argument_errors():
    for edges in ((1.0, 0.1), (0.1, 0.1), (0.1, 0.10001), (0.0,), (-1.0,), (np.nan,), (np.inf,), (3000.0,), tuple(range(1, 9)), "0.1", 0.1, (True,), ("a",)):
        with pytest.raises(ValueError):
            C.CascadeCalibrator(edges)
    assert C.check_edges(())[1].tolist() == [] and C.check_edges((0.1, 1.0))[1].tolist() == [102, 1024] == cn.edge_units((0.1, 1.0))
    assert C.check_edges([2048.0])[1].tolist() == [1 << 21] and C.check_edges(np.array([0.001, 0.002]))[1].tolist() == [1, 2]
    good = np.zeros((5, 24, 3, 4), np.float32)
    for bad in (np.zeros((24, 3)), np.zeros((5, 23, 3, 4)), np.zeros((0, 24, 3, 4)), np.zeros((2, 24, 3, 4), dtype=complex), torch.zeros(2, 24, 3, 4),
                np.broadcast_to(np.float32(0), (1, 24, 4097, 4096))):
        with pytest.raises(ValueError):
            C.CascadeCalibrator().add(bad)
        with pytest.raises(ValueError):
            C.calibrate(bad)
    with pytest.raises(ValueError):
        C.CascadeCalibrator().state()
    with pytest.raises(ValueError):
        C.calibrate(good, edges=(2.0, 1.0))
    if not torch.cuda.is_available():                                                     # valid arguments reach the device: no CPU fallback
        with pytest.raises(_lib.RdganError):
            C.CascadeCalibrator().add(good)
        with pytest.raises(_lib.RdganError):
            NoDevice().generate(np.zeros((2, 3, 4), np.float32), 3)
    model = NoDevice()
    cond = np.zeros((2, 3, 4), np.float32)
    for kw in (dict(cond=np.zeros((3, 4))), dict(cond=np.zeros((0, 3, 4))), dict(cond=torch.zeros(2, 3, 4)), dict(cond=np.zeros((2, 3, 0))),
               dict(cond=np.broadcast_to(np.float32(0), (1, 4097, 4096))), dict(cond=np.broadcast_to(np.float32(0), (2 ** 18 + 1, 1, 1))),
               dict(n_members=0), dict(n_members=65536), dict(n_members=1.0), dict(n_members=True), dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5),
               dict(first_member=-1), dict(first_member=2 ** 62 + 1), dict(first_query=-1), dict(first_query=2 ** 32 - 1), dict(patch=0), dict(patch=-1),
               dict(patch=1.0), dict(patch=2 ** 24 + 1), dict(return_units=1), dict(out=np.zeros((2, 3, 24, 3, 4), np.float32)),
               dict(out=torch.zeros(2, 3, 24, 3, 4))):
        with pytest.raises(ValueError):
            model.generate(**{**dict(cond=cond, n_members=3), **kw})
    real = np.zeros((2, 24, 3, 4), np.float32)
    for fn in (C.generate_one_per_day, C.crps_for_days):
        for args in ((real, None), (real, "model"), (np.zeros((2, 23, 3, 4)), model), (np.zeros((24, 3, 4)), model), (torch.zeros(2, 24, 3, 4), model)):
            with pytest.raises(ValueError):
                fn(*args)
        for kw in (dict(seed=-1), dict(patch=0), dict(patch=2.0)):
            with pytest.raises(ValueError):
                fn(real, model, **kw)
    for n in (0, 65536):
        with pytest.raises(ValueError):
            C.crps_for_days(real, model, n_members=n)
    with pytest.raises(ValueError):
        C.CascadeModel.from_dataset(type("D", (), {"indices": None})())
    with pytest.raises(ValueError):
        C.CascadeModel.from_dataset(type("D", (), {"indices": None})(), edges=(1.0, 0.5))
    with pytest.raises(ValueError):
        C.CascadeModel(model.state, edges=(0.1,))                                          # the state of two edges
    reals = np.ones((2, 24, 8, 8), np.float32)
    for kw in (dict(cascade="model"), dict(cascade=model.state), dict(cascade=model, cascade_patch=0), dict(cascade_patch=1.5)):
        with pytest.raises(ValueError):
            MV.multivariate_experiment(None, reals, reals, **kw)


def test_save_and_load(tmp_path):
    rng = np.random.default_rng(9)
    x = (rng.gamma(0.5, 2.0, (6, 24, 2, 3)) * (rng.random((6, 24, 2, 3)) < 0.4)).astype(np.float32)
    edges = (0.05, 0.5, 2.0)
    model = C.CascadeModel(cn.accumulate(x, edges), edges)
    path = str(tmp_path / "cascade.npz")
    model.save(path)
    back = C.CascadeModel.load(path)
    assert back.edges == model.edges == edges and np.array_equal(back.state, model.state) and np.array_equal(back.table, model.table)
    assert back.edge_units.tolist() == model.edge_units.tolist() == cn.edge_units(edges) and back.n_classes == 4
    assert (back.n_days, back.n_bad, back.n_dry) == tuple(int(v) for v in model.state[-3:]) and back.n_days == 36
    assert np.array_equal(back.table, cn.build_model(cn.accumulate(x, edges), 3)[0])


def test_cabi_argument_checks():
    """the three C entries refuse a bad argument before they touch the device: callable without one"""
    lib = _lib.load()
    size = lib.rdgan_cascade_state_size
    assert [size(n) for n in range(8)] == [748 * (n + 1) + 3 for n in range(8)] and size(2) == C.state_size(2) < 3000
    assert size(-1) == -2 and size(8) == -2
    buf = (ctypes.c_double * 64)()
    good = ctypes.c_void_p(ctypes.addressof(buf) + 16 - ctypes.addressof(buf) % 16)       # 16-byte aligned, never read: every call is refused
    by = lambda off: ctypes.c_void_p(good.value + off)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)
    ints = lambda *v: (ctypes.c_int * max(len(v), 1))(*v)
    two = ints(102, 1024)

    def acc(x=good, n=2, stride=24 * 15, ny=3, nx=5, edges=two, ne=2, state=good):
        return lib.rdgan_cascade_accumulate(x, n, stride, ny, nx, edges, ne, state, st)

    for kw in (dict(x=null), dict(state=null), dict(x=by(2)), dict(state=by(4)), dict(n=0), dict(n=-1), dict(ny=0), dict(nx=0), dict(ny=4097, nx=4096, stride=24 * 4097 * 4096),
               dict(ny=2 ** 24 + 1, nx=1, stride=24 * (2 ** 24 + 1)), dict(stride=24 * 15 - 1), dict(n=2 ** 40 // (24 * 15) + 1), dict(stride=2 ** 50), dict(ne=-1),
               dict(ne=8), dict(edges=null), dict(edges=ints(1024, 102)), dict(edges=ints(102, 102)), dict(edges=ints(0, 5)), dict(edges=ints(5, 2 ** 21 + 1)),
               dict(edges=ints(-3, 5))):
        assert acc(**kw) == -2, kw

    def gen(model=good, edges=two, ne=2, cond=good, Q=3, q0=0, ny=3, nx=5, S=2, m0=0, seed=1, patch=1, out=good, units=null):
        return lib.rdgan_cascade_generate(model, edges, ne, cond, Q, q0, ny, nx, S, m0, seed, patch, out, units, st)

    for kw in (dict(model=null), dict(cond=null), dict(out=null), dict(model=by(2)), dict(cond=by(2)), dict(out=by(2)), dict(units=by(1)), dict(ne=-1), dict(ne=8),
               dict(edges=null), dict(edges=ints(1024, 102)), dict(edges=ints(0, 1)), dict(Q=0), dict(Q=2 ** 18 + 1), dict(q0=-1), dict(q0=2 ** 32 - 2), dict(ny=0),
               dict(nx=0), dict(ny=4097, nx=4096), dict(S=0), dict(S=65536), dict(m0=-1), dict(m0=2 ** 62 + 1), dict(patch=0), dict(patch=-2), dict(patch=2 ** 24 + 1),
               dict(Q=2 ** 18, S=65535, ny=64, nx=64)):
        assert gen(**kw) == -2, kw


def test_header_and_lib_agree_on_the_cascade_entries():
    header = open(os.path.join(ROOT, "include", "rdgan.h")).read()
    ctype = {"long": "c_long", "int": "c_int", "void*": "c_void_p", "const float*": "c_void_p", "float*": "c_void_p", "const int*": "c_void_p",
             "int*": "c_void_p", "long long*": "c_void_p", "const unsigned*": "c_void_p", "unsigned long long": "c_ulong"}
    names = ("rdgan_cascade_state_size", "rdgan_cascade_accumulate", "rdgan_cascade_generate")
    assert tuple(sorted(n for n in _lib.SIGNATURES if "cascade" in n)) == tuple(sorted(names))
    assert tuple(sorted(set(re.findall(r"^\w+ (rdgan_cascade_\w+)\(", header, re.M)))) == tuple(sorted(names))
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
    text = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_cascade.hip.h")).read()
    text += "".join(open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", h)).read() for h in ("rdgan_hourly_host.h", "rdgan_hourly.hip.h"))
    value = lambda name: eval(re.search(r"^#define " + name + r"\s+(\S.*?)\s*(//.*)?$", text, re.M).group(1).replace("L", ""))
    names = ("RD_HOURS", "RD_CS_NB", "RD_CS_NP", "RD_CS_NL", "RD_CS_NT", "RD_CS_MAXE", "RD_CS_PER_CLASS", "RD_CS_TAIL", "RD_CS_MAXEDGE", "RD_HOURLY_MAXPLANE",
             "RD_HOURLY_MAXELEMS", "RD_CS_MAXQ", "RD_CS_MAXS", "RD_CS_MAXCOND")
    ours = (C.NHOURS, C.NB, C.NP, C.NL, C.NT, C.MAX_EDGES, C.PER_CLASS, C.TAIL, C.MAX_EDGE, C.MAX_PLANE, C.MAX_ELEMS, C.MAX_QUERIES, C.MAX_MEMBERS, C.MAX_COND)
    assert ours == tuple(value(n) for n in names)
    assert ours[:8] + (C.MAX_COND,) == (cn.NHOURS, cn.NB, cn.NP, cn.NL, cn.NT, cn.MAX_EDGES, cn.PER_CLASS, cn.TAIL, cn.MAX_COND)
    assert value("RD_CS_NODE_DAY2") == cn.NODE_DAY2 == 22 and C.UNIT == cn.UNIT == 1024
    assert C.PER_CLASS == C.NL * C.NP * (C.NT + C.NB) + 8 + 8 * C.NB + 2 * C.NB
    # the LDS of a workgroup at the most classes, and the 32-bit counters of a workgroup: 12 increments a pixel-day at the most
    assert C.state_size(C.MAX_EDGES) * 4 <= 64 * 1024
    assert 12 * (C.MAX_ELEMS // 24 // value("RD_CS_ACC_MAXBLOCKS") + 4 * value("RD_CS_THREADS")) < 2 ** 32
    assert C.MAX_PLANE * 32 * 4 <= 2 ** 31                                                 # a draw's counter
    rng_h = open(os.path.join(ROOT, "pr_disagg_radar_gan_amd", "csrc", "rdgan_rng.h")).read()
    assert re.search(r"^#define RD_STREAM_CASCADE 10u", rng_h, re.M) and C.STREAM_CASCADE == cn.STREAM_CASCADE == 10
