"""The one numpy definition of the fixed-point depth that the restatements of the hourly evaluations share (analog_np, areal_np,
cascade_np, catchment_np): a depth counts whole units of 1 / 1024 mm.  tests/test_hourly_admission_host.py pins it against literals."""
import numpy as np

UNIT = 1024
MAX_DEPTH = 2048


def quantise(x, limit=MAX_DEPTH):
    """x float32 -> (q int64, bad bool): q = rint(x * 1024), the product in fp32, ties to even, 0 where bad; bad where x is NaN,
    +-inf, negative or >= limit"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        bad = ~((x >= 0) & (x < limit))
        q = np.rint(np.where(bad, np.float32(0), x) * np.float32(UNIT)).astype(np.int64)
    return q, bad


def levels_q(levels):
    """levels in mm -> whole units: rint(level * 1024), the product in fp64"""
    return [int(np.rint(np.float64(v) * float(UNIT))) for v in levels]
