"""Host-side plumbing every module that calls the library shares: pointers and streams for ctypes, arrays brought to the device,
workspace sizes, whole-number and flag arguments.  Host code; nothing here touches the device but device_f32's upload."""
import ctypes

import numpy as np
import torch

from . import _lib


def ptr(t):
    """the device pointer of a tensor, null for None"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def host_ptr(a):
    """the pointer of a numpy array, read by the library before the call returns"""
    return a.ctypes.data_as(ctypes.c_void_p)


def stream(t):
    """the current stream of the tensor's device"""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def device_f32(a, name, device=None):
    """a CUDA tensor where it lies, as contiguous float32; anything else through numpy to `device` (default "cuda"); a torch
    tensor on the host is a ValueError"""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError(f"{name}: expected a CUDA tensor or a numpy array")
        return a.detach().to(torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device or "cuda")


def workspace_bytes(lib, entry, *args):
    """the size the library's `entry` returns for these arguments; a negative one is an RdganError"""
    nbytes = int(getattr(lib, entry)(*args))
    if nbytes < 0:
        raise _lib.RdganError(f"{entry} failed with code {nbytes}")
    return nbytes


def whole_number(value, lo, hi, what, whole_floats=False):
    """int(value) for an int or numpy integer in lo .. hi -- no bool, and no float unless whole_floats admits the whole-valued
    ones; ValueError otherwise"""
    ok = isinstance(value, (int, np.integer)) and not isinstance(value, bool)
    if whole_floats and isinstance(value, (float, np.floating)):
        ok = float(value).is_integer()
    if not (ok and lo <= int(value) <= hi):
        raise ValueError(f"{what} must be a whole number in {lo} .. {hi}, got {value!r}")
    return int(value)


def flag(value, name):
    """bool(value) for a bool or numpy bool; ValueError otherwise"""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {value!r}")
    return bool(value)
