"""-m gpu: the fp32 one-pass input gradient of critic layer 1 (k_d1_dgrad_sample32, option "d1_dgrad_fused", ndomain 16) and the
gradient-penalty norm it takes over in the critic step, against the column GEMM + k_d1_col2im (+ k_gp_norm_r0) of the same
engine and against the fp64 definition (oracle/rdgan_np.py: conv3d_input_grad).

Tolerance.  The new kernel multiplies with the same instruction (v_mfma_f32_32x32x2f32) over the same k pairs in the same order as
the streaming GEMM, gathers the taps through the helpers that follow k_d1_col2im's order, and folds the norm in k_gp_norm_r0's
order: the two paths are required to be EQUAL BIT FOR BIT (torch.equal), g0, norm outputs and whole steps alike.  Both paths'
errors against the fp64 definition are printed and the fused one may be no worse than twice the old one (equal when the bits are).
Observed on MI355X: bit-identical everywhere; the figures against fp64 are in the docstrings below."""
import numpy as np
import pytest
import torch

from oracle import rdgan_np as onp
from oracle import rdgan_torch as ot
from pr_disagg_radar_gan_amd import Engine
from tests.hip_util import dev, rel_err, critic_step_on_engine_branch, gen_step_on_engine_branch
from tests.test_hip_step import _params, _grad_errors, TIGHT

pytestmark = pytest.mark.gpu

# one-hot probes: (row of the 11 x 7 x 7 layer-1 grid, channel) -- the eight corners and one interior position, channels 0 and 63
_CORNERS = [(od, oh, ow) for od in (0, 10) for oh in (0, 6) for ow in (0, 6)] + [(5, 3, 2)]
_PROBES = [((od * 7 + oh) * 7 + ow, c) for (od, oh, ow) in _CORNERS for c in (0, 63)]


def _u1(B, nd, seed):
    O = nd // 2 - 1
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, 11 * O * O, 64)).astype(np.float32)


def _g0_fp64(u1, w1, nd):
    O = nd // 2 - 1
    gy = u1.astype(np.float64).reshape(u1.shape[0], 11, O, O, 64)
    return onp.conv3d_input_grad(gy, w1.astype(np.float64), (24, nd, nd), 2, (0, 0, 0))[..., 0]


def _both_paths(eng, ds, u1, **kw):
    res = {}
    for on in (0, 1):
        eng.set_option("d1_dgrad_fused", on)
        res[on] = eng.debug_d1_input_grad(ds, dev(u1), **kw)
    return res


@pytest.fixture(scope="module")
def eng16():
    e = Engine(ndomain=16, max_batch=8)
    yield e
    e.close()


@pytest.mark.parametrize("B", [1, 3, 5])
def test_d1_dgrad_sample32_equals_the_column_gemm_and_the_fp64_definition(eng16, B):
    """Random u1: fused g0 == column GEMM + col2im bit for bit; both against the fp64 definition (observed on MI355X: bit-identical,
    so both paths the same error: 2.40e-7 / 2.56e-7 / 1.53e-7 of the largest entry at B = 1 / 3 / 5).  Then one-hot u1 (corners and an interior row of the
    11 x 7 x 7 grid, channels 0 and 63, one probe per sample in turn): g0 must be the 27 sample-channel taps of that channel at 2 o + tap, exactly (one
    product per output, no rounding) and zero elsewhere."""
    _, d = _params(16, 71)
    ds = eng16.to_slab(d)
    u1 = _u1(B, 16, 700 + B)
    res = _both_paths(eng16, ds, u1)
    ref = _g0_fp64(u1, d[0], 16)
    e_old, e_new = rel_err(res[0].cpu().numpy(), ref), rel_err(res[1].cpu().numpy(), ref)
    print(f"B {B}: g0 against fp64: column GEMM + col2im {e_old:.2e}, k_d1_dgrad_sample32 {e_new:.2e}; "
          f"bit-identical: {torch.equal(res[0], res[1])}")
    assert e_new <= 2 * e_old and e_new < 2e-6, (e_old, e_new)     # 64-term fp32 dot products, <= 8 of them added: ~ 1e-7 .. 1e-6
    assert torch.equal(res[0], res[1])
    for k in range(0, len(_PROBES), B):
        hot = np.zeros((B, 539, 64), np.float32)
        for b, (row, c) in enumerate(_PROBES[k:k + B]):
            hot[b, row, c] = 1.0
        r = _both_paths(eng16, ds, hot)
        assert torch.equal(r[0], r[1])
        assert np.array_equal(r[1].cpu().numpy(), _g0_fp64(hot, d[0], 16).astype(np.float32)), _PROBES[k:k + B]


def test_other_ndomains_keep_the_column_gemm():
    """ndomain 24 (fp32): the option routes nothing there -- the launch table names the column GEMM either way, and g0 is the
    same bits with the option on and off and matches the fp64 definition (observed 1.48e-7)."""
    eng = Engine(ndomain=24, max_batch=2)
    try:
        _, d = _params(24, 72)
        ds = eng.to_slab(d)
        u1 = _u1(2, 24, 711)
        eng.profile_launches(True)
        res = _both_paths(eng, ds, u1)
        torch.cuda.synchronize()
        kernels = {r["kernel"] for r in eng.launch_table()}
        eng.profile_launches(False)
        assert not any("k_d1_dgrad_sample32" in k for k in kernels), kernels
        assert torch.equal(res[0], res[1])
        e = rel_err(res[1].cpu().numpy(), _g0_fp64(u1, d[0], 24))
        print(f"nd 24 g0 against fp64: {e:.2e}")
        assert e < 2e-6
    finally:
        eng.close()


def test_launch_table_names_the_fused_kernel_and_counts_its_flops(eng16):
    """the per-launch table and rdgan_flop_count stay truthful: one launch named k_d1_dgrad_sample32 with 2 * B * 539 * 27 * 64
    FLOPs (the 27 sample-channel taps, as the bf16 branch counts them)"""
    _, d = _params(16, 71)
    ds = eng16.to_slab(d)
    eng16.set_option("d1_dgrad_fused", 1)
    eng16.profile_launches(True)
    eng16.flop_count(reset=True)
    eng16.debug_d1_input_grad(ds, dev(_u1(3, 16, 5)))
    torch.cuda.synchronize()
    rows = [r for r in eng16.launch_table() if "k_d1_dgrad_sample32" in r["kernel"]]
    eng16.profile_launches(False)
    assert len(rows) == 1 and rows[0]["launches"] == 1, rows
    want = 2.0 * 3 * 539 * 27 * 64
    assert abs(rows[0]["gflop"] * 1e9 - want) < 1e-3 * want
    assert abs(eng16.flop_count() - want) < 1e-3 * want


@pytest.mark.parametrize("B", [2, 3])
def test_gp_norm_in_the_same_pass_equals_k_gp_norm_r0(eng16, B):
    """Gradient-penalty sweep from a given u1 whose LAST sample is all zero: g0, gp = ||g0|| - 1 and the second sweep's input
    (coef * g0, 0) of the fused pass equal k_gp_norm_r0's bit for bit.  The zero sample: k_gp_norm_r0 has no epsilon -- n = 0
    gives gp = -1 and coef = -inf, so its second-sweep input is 0 * -inf = NaN in the sample channel and 0 in the condition
    channel; the fused pass must do exactly the same.  gp against fp64, observed on MI355X: 1.23e-8 at B = 2, 9.77e-8 at B = 3, the same for both paths (bit-identical)."""
    _, d = _params(16, 73)
    ds = eng16.to_slab(d)
    u1 = _u1(B, 16, 720 + B)
    u1[B - 1] = 0.0
    res = _both_paths(eng16, ds, u1, with_norm=True)
    (g0a, cha, gpa), (g0b, chb, gpb) = res[0], res[1]
    assert torch.equal(g0a, g0b)
    n64 = np.sqrt((_g0_fp64(u1, d[0], 16).reshape(B, -1) ** 2).sum(axis=1))
    ea, eb = rel_err(gpa.cpu().numpy(), n64 - 1.0), rel_err(gpb.cpu().numpy(), n64 - 1.0)
    print(f"B {B}: gp against fp64: k_gp_norm_r0 {ea:.2e}, fused {eb:.2e}; bit-identical: {torch.equal(gpa, gpb)}")
    assert eb <= 2 * ea and eb < 2e-6
    assert torch.equal(gpa, gpb)
    assert torch.equal(cha.view(torch.int32), chb.view(torch.int32))          # bitwise: NaNs included
    z = chb[B - 1].cpu().numpy()
    assert float(gpb[B - 1]) == -1.0 and np.isnan(z[:, 0]).all() and (z[:, 1] == 0).all()
    live = chb[:B - 1].cpu().numpy()
    assert np.isfinite(live).all() and (live[..., 1] == 0).all() and np.abs(live[..., 0]).max() > 0
    coef = (10.0 / B) * 2.0 * (n64[:B - 1] - 1.0) / n64[:B - 1]
    want = coef[:, None] * _g0_fp64(u1, d[0], 16).reshape(B, -1)[:B - 1]
    assert rel_err(live[..., 0], want) < 1e-5


@pytest.mark.parametrize("B", [2, 3])
def test_critic_and_generator_steps_are_unchanged_by_the_option(eng16, B):
    """Whole steps with "d1_dgrad_fused" 1 against 0: the critic step's gradient slab and loss tail [total, valid, fake, gp,
    nonfinite] (the penalty runs through the fused norm) and the generator step's (dL/dfake) equal bit for bit; the fused critic
    step against the fp64 oracle on its own LeakyReLU branch stays inside GATE_TOL / TIGHT as in tests/test_hip_step.py."""
    g, d = _params(16, 74)
    x, cond, z = ot.synthetic_batch(B, 16, 730 + B)
    gs, ds = eng16.to_slab(g), eng16.to_slab(d)
    res = {}
    for on in (0, 1):
        eng16.set_option("d1_dgrad_fused", on)
        res[on] = (eng16.critic_grad(ds, gs, dev(x), dev(cond), dev(z), 31).clone(), eng16.gen_grad(ds, gs, dev(z), dev(cond), 32).clone())
    assert bool(torch.isfinite(res[1][0]).all()) and float(res[1][0][eng16.n_critic + 3]) > 0      # the penalty term is live
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    slab, losses, grads = critic_step_on_engine_branch(eng16, ds, gs, d, g, x, cond, z, 31)
    n = eng16.n_critic
    np.testing.assert_allclose(slab[n:n + 4], losses.numpy(), rtol=2e-4, atol=1e-6)
    errs = _grad_errors(slab[:n], grads, eng16.critic_shapes)
    assert max(errs.values()) < TIGHT, errs
    slab, loss, grads = gen_step_on_engine_branch(eng16, ds, gs, d, g, z, cond, 32)
    errs = _grad_errors(slab[:eng16.n_gen], grads, eng16.gen_shapes)
    assert max(errs.values()) < TIGHT, errs
