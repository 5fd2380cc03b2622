"""numpy restatement of the radar ingest (csrc/rdgan_radar.hip.h), with explicit loops so that the order of every fp32 sum is
unambiguous, and the synthetic radar codes the tests share.

Reference: convert_smhi_radardata.py:38-44 (code -> mm per frame; the table itself is data_pipeline.radar_lut, checked against the
fp64 formula in tests/test_radar_host.py), reformat_data.py:72-91 (frames -> hours with skipna=False, -> (days, 24, ny, nx))."""
import functools

import numpy as np


def lut_f64(scale=0.4, offset=-30.0, a=200.0, b=1.5, minutes=5):
    """the formula of convert_smhi_radardata.py:41-43 in float64, for the codes 0..254"""
    c = np.arange(255, dtype=np.float64)
    return ((10 ** ((c * scale + offset) / 10)) / a) ** (1 / b) * minutes / 60


def make_codes(n_days, ny, nx, fph=12, seed=0):
    """uint8 (n_days, 24 fph, ny, nx): zeros, 5 % drizzle codes 1..79, one 20 x 20 rain block of codes ~ N(150, 12) for six hours on
    every day but day 1, and code 255 at the first and at the last frame of an hour, at the very last element, and on a 4 x 10 patch
    across two hours of day 2.  Needs n_days >= 3, ny, nx > 30."""
    rng = np.random.default_rng(seed)
    fpd = 24 * fph
    c = np.zeros((n_days, fpd, ny, nx), np.uint8)
    rng.random(c.shape)                                    # (a draw that is not used: the counts recorded in the tests were taken behind it)
    drizzle = rng.random(c.shape) < 0.05
    c[drizzle] = rng.integers(1, 80, size=int(drizzle.sum()), dtype=np.uint8)
    for d in range(n_days):
        if d == 1:
            continue                                       # a dry day
        y0, x0 = rng.integers(0, ny - 20), rng.integers(0, nx - 20)
        h0 = rng.integers(0, 18) * fph
        blk = rng.normal(150, 12, (6 * fph, 20, 20)).clip(0, 254).astype(np.uint8)
        c[d, h0:h0 + 6 * fph, y0:y0 + 20, x0:x0 + 20] = blk
    c[0, 0, 3, 5] = 255                                    # first frame of an hour
    c[0, fph - 1, 4, 6] = 255                              # last frame of an hour
    c[2, fpd - 1, ny - 1, nx - 1] = 255                    # the very last element
    c[2, 5 * fph:7 * fph, 10:14, 20:30] = 255              # a missing patch across two hours
    return c


PATCH = (2, 10, 14, 20, 30)            # day, y0, y1, x0, x1 of the missing patch


def hourly(codes, lut, fph):
    """hourly[d,h] = ((lut[c0] + lut[c1]) + lut[c2]) + ... over the fph frames of hour h, in order, fp32"""
    n, fpd, ny, nx = codes.shape
    assert fpd == 24 * fph and lut.dtype == np.float32
    out = np.empty((n, 24, ny, nx), np.float32)
    for h in range(24):
        acc = lut[codes[:, h * fph]]
        for k in range(1, fph):
            acc = acc + lut[codes[:, h * fph + k]]
        out[:, h] = acc
    return out


def daily(hourly_arr):
    """daily[d] = ((hourly[d,0] + hourly[d,1]) + ...) over h = 0..23, fp32"""
    acc = hourly_arr[:, 0].copy()
    for h in range(1, 24):
        acc = acc + hourly_arr[:, h]
    return acc


@functools.lru_cache(maxsize=None)
def case(n_days, ny, nx, fph=12, seed=0):
    """(codes, hourly, daily, n_missing) of make_codes with data_pipeline.radar_lut(): computed once per shape, shared, read-only"""
    from pr_disagg_radar_gan_amd.data_pipeline import radar_lut
    c = make_codes(n_days, ny, nx, fph, seed)
    h = hourly(c, radar_lut(), fph)
    d = daily(h)
    for a in (c, h, d):
        a.setflags(write=False)
    return c, h, d, int(np.isnan(h).sum())
