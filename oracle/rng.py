"""Counter-based RNG shared by the oracle and the HIP path (test infrastructure).

The reference draws dropout masks (gan_train_cwgangp_pixelnorm.py:289-301) and the
RandomWeightedAverage alpha (…:223) from TensorFlow's stateful global RNG, which is never
seeded, so no bit pattern is pinned by the reference.  Both sides of the parity tests use
this stateless definition instead (mirrored in csrc/rdgan_rng.h):

    key(seed, stream) = mix(lo32(seed) ^ mix(hi32(seed) ^ 0x9E3779B9)) + stream * 0x85EBCA6B
    bits(idx)         = mix(mix(idx) ^ key)                       (all uint32, wrapping)
    uniform(idx)      = (bits >> 8) * 2**-24            in [0, 1)
    keep(idx)         = byte (idx & 3) of bits(idx >> 2) >= 64      P(keep) = 192/256 = 0.75 for rate 0.25
                        (one hash word decides four consecutive elements: the kernels' epilogues hold four consecutive
                        channels per lane and pay the hash once per quad)

``mix`` is the lowbias32 integer finaliser.  ``idx`` is the flat NDHWC element index of the
tensor the mask is applied to (for the critic step: the 3B batch [real; fake; interpolated]).
"""
import numpy as np

STREAM_D1, STREAM_D2, STREAM_D3, STREAM_D4, STREAM_ALPHA = 1, 2, 3, 4, 5
DROP_THRESHOLD = 64  # 0.25 * 2**8: one byte of the hash word per element
DROP_SCALE = np.float32(1.0) / np.float32(0.75)


def mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def make_key(seed, stream):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo = np.uint32(seed & 0xFFFFFFFF)
    hi = np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        k = mix32(lo ^ mix32(hi ^ np.uint32(0x9E3779B9)))
        k = np.uint32((int(k) + int(stream) * 0x85EBCA6B) & 0xFFFFFFFF)
    return k


def bits(seed, stream, n, start=0):
    idx = np.arange(start, start + n, dtype=np.uint64).astype(np.uint32)
    return mix32(mix32(idx) ^ make_key(seed, stream))


def uniform(seed, stream, n, start=0):
    """float32 uniforms in [0,1) for element indices start..start+n-1."""
    return (bits(seed, stream, n, start) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_scale_mask(seed, stream, shape, start=0):
    """float32 mask holding 0 or 1/0.75 (inverted dropout, rate 0.25) of the given shape.
    seed == 0 means dropout off (all ones) -- the ``predict`` path of the reference.
    start: flat index of the mask's first element in the whole tensor (a sample range of a larger batch)."""
    n = int(np.prod(shape))
    if seed == 0:
        return np.ones(shape, np.float32)
    idx = np.arange(start, start + n, dtype=np.uint64)
    w0 = int(start) >> 2
    words = bits(seed, stream, ((int(start) + n + 3) >> 2) - w0, start=w0)[(idx >> np.uint64(2)).astype(np.int64) - w0]
    byte = (words >> (np.uint32(8) * (idx & np.uint64(3)).astype(np.uint32))) & np.uint32(0xFF)
    keep = byte >= np.uint32(DROP_THRESHOLD)
    return np.where(keep, DROP_SCALE, np.float32(0)).astype(np.float32).reshape(shape)


# The same definitions in torch int64 arithmetic, for masks generated on a GPU (the fp64 device oracle at the benchmarked
# batch sizes).  Every product is split so that no intermediate leaves the int64 range; bit-equal to the numpy form
# (tests/test_oracle_chunked.py).
def _mul32_t(x, c):
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & 0xFFFFFFFF


def mix32_t(x):
    """mix32 of an int64 torch tensor holding uint32 values"""
    x = x ^ (x >> 16)
    x = _mul32_t(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32_t(x, 0x846CA68B)
    return x ^ (x >> 16)


def bits_t(seed, stream, n, start=0, device=None):
    import torch
    idx = torch.arange(start, start + n, dtype=torch.int64, device=device) & 0xFFFFFFFF
    return mix32_t(mix32_t(idx) ^ int(make_key(seed, stream)))


def dropout_scale_mask_t(seed, stream, shape, start=0, device=None, dtype=None):
    """dropout_scale_mask as a torch tensor generated on `device` (default dtype float32)"""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    n = int(np.prod(shape))
    if seed == 0:
        return torch.ones(shape, dtype=dtype, device=device)
    idx = torch.arange(start, start + n, dtype=torch.int64, device=device)
    words = mix32_t(mix32_t((idx >> 2) & 0xFFFFFFFF) ^ int(make_key(seed, stream)))
    keep = ((words >> (8 * (idx & 3))) & 0xFF) >= DROP_THRESHOLD
    return torch.where(keep, torch.tensor(float(DROP_SCALE), dtype=torch.float32, device=device),
                       torch.zeros((), dtype=torch.float32, device=device)).to(dtype).reshape(shape)
