"""What the evaluations of hourly arrays share on the host: how an array (..., 24, ny, nx) is admitted -- kind, shape, layout --
before any device call, and the two small quotients their statistics use."""
import numpy as np
import torch

NHOURS = 24
MAX_MEMBERS = 4096                                                           # RD_MS_MAXS, RD_VF_MAXS


def hourly_shape(shape, what="hourly"):
    shape = tuple(int(n) for n in shape)
    if len(shape) < 3 or shape[-3] != NHOURS or min(shape) < 1:
        raise ValueError(f"{what}: expected shape (..., 24, ny, nx) with no empty axis, got {shape}")
    return shape


def tensor_layout(shape, strides):
    """(n, day_stride) of a tensor of shape (..., 24, ny, nx) with these strides (in elements), as rdgan_temporal_accumulate reads
    it: the last three axes must be dense, whatever the rank; the leading axes must flatten to one axis of stride day_stride >= 24
    ny nx, which a single leading axis does with any stride (a view of a wider buffer) and several do only when they are dense
    among themselves.  Anything a stride argument cannot express -- a crop, a step, a transposed plane -- is a ValueError."""
    shape, strides = tuple(int(m) for m in shape), tuple(int(st) for st in strides)
    expect = 1
    for m, st in zip(reversed(shape[-3:]), reversed(strides[-3:])):
        if m != 1 and st != expect:
            raise ValueError("hourly: the hour, row and column axes must be contiguous (a crop, a step or a transpose is not)")
        expect *= m
    day = expect
    lead = [(m, st) for m, st in zip(shape[:-3], strides[:-3]) if m != 1]
    n = int(np.prod(shape[:-3], dtype=np.int64))
    if not lead:
        return n, day
    stride = lead[-1][1]
    if stride < day:
        raise ValueError(f"hourly: the leading stride {stride} is below the size of a day {day}")
    expect = stride
    for m, st in reversed(lead):
        if st != expect:
            raise ValueError("hourly: several leading axes must be contiguous among themselves")
        expect *= m
    return n, stride


def member_layout(x):
    """(S, P, member_stride, shape) of x (S, *shape): every axis behind the first must be contiguous, the first may have any stride
    >= P (a view of a wider buffer)"""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("x: expected a tensor of shape (S, *shape)")
    S, shape = int(x.shape[0]), tuple(int(n) for n in x.shape[1:])
    P = int(np.prod(shape, dtype=np.int64))
    if not 1 <= S <= MAX_MEMBERS:
        raise ValueError(f"the number of members must lie in 1 .. {MAX_MEMBERS}, got {S}")
    if P < 1:
        raise ValueError(f"x holds no position: shape {tuple(x.shape)}")
    expect = 1
    for n, st in zip(reversed(shape), reversed(x.stride()[1:])):
        if n != 1 and st != expect:
            raise ValueError("x: the axes behind the member axis must be contiguous")
        expect *= n
    stride = int(x.stride(0)) if S > 1 else P
    if stride < P:
        raise ValueError(f"x: the member stride {stride} is below the number of positions {P}")
    return S, P, stride, shape


def admit_array(a, what="hourly"):
    """Kind and shape of an hourly input, host code: a float32 CUDA tensor is taken as it is, anything else as a numpy array of
    numbers; a torch tensor on the host is refused.  -> (the tensor or array, from_host, shape)"""
    from_host = not isinstance(a, torch.Tensor)
    if from_host:
        a = np.asarray(a)
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{what}: expected an array of numbers")
    elif not a.is_cuda:                                # (a host view's strides would not survive the copy to the device)
        raise ValueError(f"{what}: expected a CUDA tensor or a numpy array, got a torch tensor on the host")
    elif a.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32")
    return a, from_host, hourly_shape(a.shape, what)


def admit(hourly, plane_shape=None):
    """admit_array, the plane shape an accumulator has pinned (None: not yet), and the layout the accumulate entries read: a
    numpy array will be uploaded dense, a tensor must pass tensor_layout.  -> (hourly, from_host, shape, n, day_stride)"""
    hourly, from_host, shape = admit_array(hourly)
    if plane_shape is not None and shape[-2:] != tuple(plane_shape):
        raise ValueError(f"hourly: the plane shape is {tuple(plane_shape)} since the first call, got {shape[-2:]}")
    if from_host:
        n, day_stride = int(np.prod(shape[:-3], dtype=np.int64)), NHOURS * shape[-2] * shape[-1]
    else:
        n, day_stride = tensor_layout(shape, hourly.stride())
    return hourly, from_host, shape, n, day_stride


def to_state_device(a, from_host, device, what="hourly"):
    """The step behind admission once the state exists: a host array goes to the state's device as dense float32, a tensor must
    lie there already"""
    if from_host:
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    if a.device != device:
        raise ValueError(f"{what} lies on {a.device}, the state on {device}")
    return a


def div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.asarray(b) != 0, np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64), np.nan)


def tv(a, b):
    with np.errstate(invalid="ignore"):
        return 0.5 * np.abs(a - b).sum(axis=-1)
