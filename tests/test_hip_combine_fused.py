"""-m gpu: option "combine_dx_fused" (fp32 storage, shared-centre backward): the PixelNorm/LeakyReLU backward kernels form
dx + (dE[d] - dE[d+1]) themselves instead of reading a dx that k_combine_dx has combined in a pass of its own.  Same expression,
same order, nothing else changes: the generator step must be equal BIT FOR BIT with the option on and off."""
import numpy as np
import pytest
import torch

from oracle import rdgan_torch as ot
from pr_disagg_radar_gan_amd import Engine
from tests.hip_util import dev
from tests.test_hip_step import _params

pytestmark = pytest.mark.gpu


# ndomain 16: blocks 3 and 2 run the shared-centre backward (k_pn_lrelu_bwd_pairs<32> at 3 -> 2, k_pn_lrelu_bwd<64, 0> at 2 -> 1).
# ndomain 8: the smallest accepted geometry, hour planes of 4 x 4 and 2 x 2 pixels -- a workgroup of 256 threads spans several
# planes (and, at 2 -> 1, several samples), so the plane / sample decoding of the dE rows is exercised across its lanes.
@pytest.mark.parametrize("nd,B", [(16, 2), (16, 3), (8, 2), (8, 3)])
def test_gen_step_is_bit_identical_with_combine_dx_fused(nd, B):
    eng = Engine(ndomain=nd, max_batch=B)
    try:
        g, d = _params(nd, 81)
        x, cond, z = ot.synthetic_batch(B, nd, 800 + B)
        gs, ds = eng.to_slab(g), eng.to_slab(d)
        res = {}
        for on in (0, 1):
            eng.set_option("combine_dx_fused", on)
            res[on] = eng.gen_grad(ds, gs, dev(z), dev(cond), 41).clone()
            assert torch.equal(res[on], eng.gen_grad(ds, gs, dev(z), dev(cond), 41))       # run-to-run deterministic
        n = eng.n_gen
        assert bool(torch.isfinite(res[1]).all()) and float(res[1][:n].abs().max()) > 0
        assert float(res[1][n + 4]) == 0.0                                                 # non-finite flag of the loss tail
        assert torch.equal(res[0], res[1])                                                 # gradient slab and loss tail
        # the difference part reaches the result (the comparison above is not vacuous): without the shared-centre backward the
        # same gradients come out of other sums, close but not the same bits
        eng.set_option("fast_bwd", 0)
        other = eng.gen_grad(ds, gs, dev(z), dev(cond), 41)
        assert not torch.equal(other[:n], res[1][:n])
        np.testing.assert_allclose(other[:n].cpu().numpy(), res[1][:n].cpu().numpy(), rtol=0, atol=1e-4 * float(res[1][:n].abs().max()))
    finally:
        eng.close()
