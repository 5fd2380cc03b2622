"""-m gpu: the one workspace rule of HourlyAccumulator (pr_disagg_radar_gan_amd/_hourly.py): the buffer only grows, and an entry
is told the bytes its call needs, not the size of the buffer.  3 days, then 1 day -- for which the buffer of the first call is
larger than needed -- then 3 days on one accumulator give the state of the 7 days added at once to a fresh one: bit for bit for the
integer states, and for temporal's fp64 sums within the reordering bound of tests/test_hip_temporal.py (N 2^-52 relative for a
sum of N non-negative terms).  70 x 65 crosses the 64-pixel tiles of the label and box kernels, 9 x 7 lies inside one."""
import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import areal as AR, cells as CL, spacetime as ST, storms as SM, temporal as TS
from tests import temporal_np as tn
from tests.hip_util import dev

pytestmark = pytest.mark.gpu

SUMS, EPS = ("moments", "lag", "wet_amount"), 2.0 ** -52           # as tests/test_hip_temporal.py has them (test_grouping's bound)
THR, K = (0.1, 2.0), 2
INTEGER = {"cells": lambda: CL.CellStructure(THR, 8), "storms": lambda: SM.StormStructure(THR, 8, 1),
           "areal": lambda: AR.ArealExtremes((1, 3), (1, 3), (1.0, 5.0)), "spacetime": lambda: ST.SpaceTimeStructure(THR, 2, 2)}


def three_one_three(make, xd):
    acc = make().add(xd[:3])
    held = acc._ws.numel()
    acc.add(xd[3:4])
    assert acc._ws.numel() == held                                  # the buffer stays: larger than the one-day call needs
    return acc.add(xd[4:]), held


@pytest.mark.parametrize("plane", [(70, 65), (9, 7)])
def test_a_buffer_larger_than_the_call_needs_changes_nothing(plane):
    rng = np.random.default_rng(plane[0])
    shape = (7, 24) + plane
    xd = dev((rng.gamma(0.6, 3.0, shape) * (rng.random(shape) < 0.3)).astype(np.float32))
    for name, make in INTEGER.items():
        got, held = three_one_three(make, xd)
        assert make().add(xd[3:4])._ws.numel() < held, name         # (what one day alone asks for)
        assert torch.equal(got.state(), make().add(xd).state()), name
    got, _ = three_one_three(lambda: TS.TemporalStructure(THR, K), xd)
    whole = TS.TemporalStructure(THR, K).add(xd)
    assert torch.equal(got.state()[0], whole.state()[0])
    a, b = got.result(), whole.result()
    n = tn.terms(dict(n_valid=b.n_valid), len(THR), K)
    for s in SUMS:
        assert np.all(np.abs(getattr(a, s) - getattr(b, s)) <= n[s] * EPS * np.abs(getattr(b, s))), s
