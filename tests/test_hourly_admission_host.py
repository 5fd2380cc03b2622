"""CPU: the one admission of hourly arrays (pr_disagg_radar_gan_amd/_hourly.py) and the two accumulators built on it refuse the
same inputs, with ValueError, before any device call."""
import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import _hourly as H, _lib, cells as CL, temporal as TS


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
    for mod in (TS, CL):
        monkeypatch.setattr(mod, "require_gpu", device_call)
    monkeypatch.setattr(_lib, "load", device_call)
    rows, four = _rows()
    assert all(isinstance(t, AsIfOnDevice) and t.is_cuda for t, m in rows if "contig" in m)
    entries = (("admit", lambda x: H.admit(x)), ("TemporalStructure.add", lambda x: TS.TemporalStructure((0.1,)).add(x)),
               ("CellStructure.add", lambda x: CL.CellStructure((0.1,)).add(x)), ("label_cells", lambda x: CL.label_cells(x, 0.1)))
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
    for acc in (TS.TemporalStructure((0.1,)), CL.CellStructure((0.1,))):
        acc.plane_shape = (4, 5)                                    # as after a first add
        for x in second:
            with pytest.raises(ValueError, match="since the first call"):
                acc.add(x)
    for x in second:
        with pytest.raises(ValueError, match="since the first call"):
            H.admit(x, (4, 5))
    assert H.admit(np.zeros((7, 24, 4, 5)), (4, 5))[3] == 7          # more days of the same plane are welcome


def test_upload_or_refusal_once_the_state_exists():
    """to_state_device on the host: a numpy array becomes dense float32 on the state's device, a tensor elsewhere is refused"""
    a = np.arange(2 * 24 * 2 * 3, dtype=np.int64).reshape(2, 24, 2, 3)[::-1]
    t = H.to_state_device(a, True, torch.device("cpu"))
    assert t.dtype == torch.float32 and t.is_contiguous() and np.array_equal(t.numpy(), a.astype(np.float32))
    assert H.to_state_device(t, False, torch.device("cpu")) is t
    with pytest.raises(ValueError, match="lies on cpu, the state on meta"):
        H.to_state_device(t, False, torch.device("meta"))
