"""CPU: the one admission of hourly arrays (pr_disagg_radar_gan_amd/_hourly.py) and everything built on it -- the five
accumulators of HourlyAccumulator (temporal, cells, storms, areal, space-time) and the one-call functions that allocate an output
before they add (label_cells, label_storms, areal_extremes with return_depths) -- refuse the same inputs, with ValueError, before
any device call, and let a good input through to it; and the per-pass arithmetic of each accumulator, against the numbers the
expressions in the five modules gave before the base class existed."""
import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _hourly as H, _lib, areal as AR, cells as CL, spacetime as ST, storms as SM, temporal as TS

# one of each accumulator, with parameters under which the 4 x 5 and 6 x 8 planes of the rows below are admissible
ACCUMULATORS = (lambda: TS.TemporalStructure((0.1,)), lambda: CL.CellStructure((0.1,)), lambda: SM.StormStructure((0.1,)),
                lambda: AR.ArealExtremes((1,), (1, 3)), lambda: ST.SpaceTimeStructure((0.1,), radius=1))


class AsIfOnDevice(torch.Tensor):
    """a host tensor that answers is_cuda with True: its shape and strides stand in for a device tensor's, so the layout rules are
    reached without a GPU (views of it keep the class)"""
    is_cuda = True


def _rows():
    """(input, a piece of the message): everything an hourly input must not be"""
    day = torch.zeros(24, 60, 64).as_subclass(AsIfOnDevice)
    four = torch.zeros(5, 24, 6, 8).as_subclass(AsIfOnDevice)
    five = torch.zeros(4, 3, 24, 6, 8).as_subclass(AsIfOnDevice)
    rows = [(torch.zeros(24, 4, 5), "on the host"), (torch.zeros(2, 24, 4, 5)[::2], "on the host"),
            (np.zeros((24, 4, 5), dtype=complex), "array of numbers"), (np.zeros((24, 4, 5), dtype="U1"), "array of numbers"),
            (torch.zeros(24, 4, 5, dtype=torch.float64).as_subclass(AsIfOnDevice), "float32"),
            (np.zeros((24, 5)), "shape"), (np.zeros((23, 4, 5)), "shape"), (np.zeros((2, 25, 4, 5)), "shape"),
            (np.zeros((0, 24, 4, 5)), "empty"), (np.zeros((24, 0, 5), np.float32), "empty"), (four[:0], "empty")]
    # what a stride argument cannot express (the list of test_temporal_host.test_tensor_layout_refuses_what_a_stride_cannot_express)
    rows += [(day[::2], "shape"), (day.transpose(0, 1), "shape")]       # (these two no longer hold 24 hours: the shape check has them)
    rows += [(t, "contiguous|leading stride") for t in (
        day[:, 10:50, 10:50], day[..., ::2], day.transpose(1, 2), day[:, :, 3:],
        four[:, :, 1:5, 2:6], four[..., ::2], four.transpose(2, 3), four[:, ::2].repeat_interleave(2, 1)[:, :, :, 1:],
        five[:, :2], five[:, ::2], five.transpose(0, 1), four.expand(2, 5, 24, 6, 8), four[:1].expand(3, 24, 6, 8))]
    return rows, four


def test_every_entry_refuses_the_same_inputs_before_the_device(monkeypatch):
    def device_call(*a, **k):
        raise AssertionError("the device was reached")
    for mod in (H, CL, SM, AR):                     # the accumulators' add reaches it in _hourly, the one-call functions in their modules
        monkeypatch.setattr(mod, "require_gpu", device_call)
    monkeypatch.setattr(_lib, "load", device_call)
    rows, four = _rows()
    assert all(isinstance(t, AsIfOnDevice) and t.is_cuda for t, m in rows if "contig" in m)
    entries = (("admit", lambda x: H.admit(x)),) + tuple((f"{make().__class__.__name__}.add", lambda x, make=make: make().add(x))
                                                          for make in ACCUMULATORS)
    entries += (("label_cells", lambda x: CL.label_cells(x, 0.1)), ("label_storms", lambda x: SM.label_storms(x, 0.1)),
                ("areal_extremes", lambda x: AR.areal_extremes(x, (1,), (1, 3), return_depths=True)))
    assert len(entries) == 9
    for name, entry in entries:
        for i, (bad, message) in enumerate(rows):
            with pytest.raises(ValueError, match=message):
                entry(bad)
                pytest.fail(f"{name} admitted row {i}")
    # the same entries let a good input through: to the device call for the accumulators, to its layout for admit
    good = four[::2]
    for name, entry in entries[1:]:
        for x in (np.zeros((2, 24, 4, 5)), good):
            with pytest.raises(AssertionError, match="the device was reached"):
                entry(x)
    x, from_host, shape, n, day_stride = H.admit(np.zeros((2, 3, 24, 4, 5), np.int16))
    assert from_host and shape == (2, 3, 24, 4, 5) and (n, day_stride) == (6, 480)
    x, from_host, shape, n, day_stride = H.admit(good)
    assert x is good and not from_host and shape == (3, 24, 6, 8) and (n, day_stride) == (3, 2304)


def test_the_plane_shape_of_the_first_call_holds(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the device was reached"))
    second = (np.zeros((24, 4, 6), np.float32), torch.zeros(3, 24, 5, 4).as_subclass(AsIfOnDevice))
    for make in ACCUMULATORS:
        acc = make()
        acc.plane_shape = (4, 5)                                    # as after a first add
        for x in second:
            with pytest.raises(ValueError, match="since the first call"):
                acc.add(x)
    for x in second:
        with pytest.raises(ValueError, match="since the first call"):
            H.admit(x, (4, 5))
    assert H.admit(np.zeros((7, 24, 4, 5)), (4, 5))[3] == 7          # more days of the same plane are welcome


# (per_pass argument, plane, {n days: units of a pass}); the numbers are worked out by hand from the expressions each module's add
# held before HourlyAccumulator: 2^24 // 63 = 266305, 2^24 // 4550 = 3687, 2^24 // (24 * 63) = 11096, 2^24 // (24 * 4550) = 153,
# 2^22 // 63 = 66576, 2^22 // 4550 = 921, 2^28 // 63 = 4260880, 2^28 // 4550 = 58996 -- none of which binds below 3 days, so the
# 2048 x 2048 rows are there for the default: 2^24 // 2^22 = 4 planes, 2^24 // (24 * 2^22) = 0 -> 1 day, 2^22 // 2^22 = 1 day, 2^28 //
# 2^22 = 64 planes -> 48
PASS_UNITS = {
    "cells": (lambda per: CL.CellStructure((0.1,), planes_per_pass=per), [          # planes: min(per or default, 24 n, 65535)
        (None, (9, 7), {1: 24, 3: 72}), (None, (70, 65), {1: 24, 3: 72}), (None, (2048, 2048), {1: 4, 3: 4}),
        (1, (9, 7), {1: 1, 3: 1}), (1, (70, 65), {1: 1, 3: 1}), (100, (9, 7), {1: 24, 3: 72}), (100, (70, 65), {1: 24, 3: 72}),
        (50, (9, 7), {1: 24, 3: 50})]),
    "storms": (lambda per: SM.StormStructure((0.1,), days_per_pass=per), [          # days: min(per or default, n, 2730)
        (None, (9, 7), {1: 1, 3: 3}), (None, (70, 65), {1: 1, 3: 3}), (None, (2048, 2048), {1: 1, 3: 1}),
        (1, (9, 7), {1: 1, 3: 1}), (1, (70, 65), {1: 1, 3: 1}), (5, (9, 7), {1: 1, 3: 3}), (5, (70, 65), {1: 1, 3: 3}),
        (2, (70, 65), {1: 1, 3: 2})]),
    "areal": (lambda per: AR.ArealExtremes((1,), (1, 3), workspace_days=per), [     # days: min(per or default, n, 65535)
        (None, (9, 7), {1: 1, 3: 3}), (None, (70, 65), {1: 1, 3: 3}), (None, (2048, 2048), {1: 1, 3: 1}),
        (1, (9, 7), {1: 1, 3: 1}), (1, (70, 65), {1: 1, 3: 1}), (5, (9, 7), {1: 1, 3: 3}), (5, (70, 65), {1: 1, 3: 3}),
        (2, (70, 65), {1: 1, 3: 2})]),
    "spacetime": (lambda per: ST.SpaceTimeStructure((0.1,), radius=1, planes_per_pass=per), [   # planes, in whole days, one day at least
        (None, (9, 7), {1: 24, 3: 72}), (None, (70, 65), {1: 24, 3: 72}), (None, (2048, 2048), {1: 24, 3: 48}),
        (24, (9, 7), {1: 24, 3: 24}), (24, (70, 65), {1: 24, 3: 24}), (100, (9, 7), {1: 24, 3: 72}), (100, (70, 65), {1: 24, 3: 72}),
        (71, (70, 65), {1: 24, 3: 48}), (48, (9, 7), {1: 24, 3: 48})]),
}


@pytest.mark.parametrize("name", sorted(PASS_UNITS))
def test_pass_units_are_the_expressions_the_modules_held(name):
    make, table = PASS_UNITS[name]
    for per, (ny, nx), want in table:
        acc = make(per)
        assert {n: acc._pass_units(n, ny, nx) for n in want} == want, (name, per, ny, nx)


def test_pass_units_of_temporal_and_the_smallest_pass_arguments():
    assert TS.TemporalStructure((0.1,))._pass_units(3, 9, 7) is None          # one launch over the whole array: no passes
    # an explicit per-pass of 1 is the least a caller can ask for, 24 planes (one day) for space-time
    for make, _ in PASS_UNITS.values():
        with pytest.raises(ValueError):
            make(0)
    with pytest.raises(ValueError):
        ST.SpaceTimeStructure((0.1,), planes_per_pass=23)


def test_upload_or_refusal_once_the_state_exists():
    """to_state_device on the host: a numpy array becomes dense float32 on the state's device, a tensor elsewhere is refused"""
    a = np.arange(2 * 24 * 2 * 3, dtype=np.int64).reshape(2, 24, 2, 3)[::-1]
    t = H.to_state_device(a, True, torch.device("cpu"))
    assert t.dtype == torch.float32 and t.is_contiguous() and np.array_equal(t.numpy(), a.astype(np.float32))
    assert H.to_state_device(t, False, torch.device("cpu")) is t
    with pytest.raises(ValueError, match="lies on cpu, the state on meta"):
        H.to_state_device(t, False, torch.device("meta"))


def test_the_numpy_quantiser_against_literals():
    """tests/hourly_np.quantise, the yardstick of the fixed-point depth in four restatements, pinned to values worked out by hand:
    the fp32 product rounds ties to even, the range is 0 <= x < 2048 with -0.0 inside it, and NaN and both infinities are bad"""
    from tests import hourly_np as hn
    below = np.nextafter(np.float32(2048), np.float32(0))
    x = np.array([0.5 / 1024, 1.5 / 1024, 2.5 / 1024, below, 2048.0, -0.0, -1e-30, np.nan, np.inf, -np.inf], np.float32)
    q, bad = hn.quantise(x)
    assert bad.tolist() == [False, False, False, False, True, False, True, True, True, True]
    # (2048 - 2^-13) * 1024 = 2^21 - 1/8 is exact in fp32 and rounds up to 2^21
    assert q[:3].tolist() == [0, 2, 2] and q[5] == 0 and q[3] == 2048 * 1024 and q[bad].tolist() == [0] * 5
    assert q.dtype == np.int64 and hn.quantise(np.float32(2048.0), 2048 * 24)[1] == False and hn.quantise(np.float32(49152.0), 2048 * 24)[1] == True  # noqa: E712
    assert hn.levels_q((0.0, 0.00048828125, 0.00146484375, 49152.0)) == [0, 0, 2, 49152 * 1024]        # fp64 product, ties to even
    assert (hn.UNIT, hn.MAX_DEPTH) == (H.UNIT, H.MAX_DEPTH) == (1024, 2048)
