"""-m gpu: the kernel variants and configurations that only occur at BASELINE sizes.

* B = 96 at ndomain 16 with DEFAULT options is the smallest batch at which the launcher picks what the bs = 256 step
  runs -- the 256-row weight-gradient tile ``k_wgrad_gemm_ws<256, 64>`` (``B * L >= 65536``, rdgan_api.hip
  ``wgrad_tiling``), the unforced 256x64 conv tile and the automatic K splits -- and is still small enough for the fp64
  torch oracle on the host, so both step gradients are compared with it directly.
* The BASELINE sizes themselves -- configs[1] (bs = 256, fp32: the metric), configs[2] (bs = 2048, n_critic = 5),
  configs[3]'s per-rank shard (bs = 1024) and configs[4]'s per-rank shard (ndomain 64, bs = 64), built as bench.py builds
  them (default options, ``Engine(nd, max_batch=B)``) -- are compared with the same fp64 oracle run ON THE GPU over sample
  ranges (oracle/rdgan_torch.py ``*_step_grads_chunked``, tests/hip_util.py), on the branch the engine took: the tile,
  K-split, partial-slab and row-slice choices the dispatcher makes only above B = 96 are covered by a gradient comparison,
  not only by properties.  Each comparison carries a sensitivity control: the same error against a reference that leaves
  out the last sample range (1/32 of the batch, the tail tiles) must be at least 3x the limit, so a dropped tile, partial
  slab or sample range could not pass.  The size-independent properties stay as well (mass conservation, batch
  independence against a small-batch run, run-to-run determinism, finite losses through a whole iteration).
* ndomain 64: the generator-step gradients (206 M-parameter Dense weight gradient included) against the oracle at B = 1.
"""
import numpy as np
import pytest
import torch

from oracle import rdgan_torch as ot
from pr_disagg_radar_gan_amd import Engine
from pr_disagg_radar_gan_amd import weights as W
from pr_disagg_radar_gan_amd.trainer import WGANGPTrainer
from tests.hip_util import (GATE_TOL, dev, rel_err, gen_step_on_engine_branch, critic_step_on_engine_branch,
                             gen_step_on_engine_branch_chunked, critic_step_on_engine_branch_chunked)
from tests.test_hip_step import _params, _t64, _grad_errors, TIGHT

pytestmark = pytest.mark.gpu


def test_device_oracle_matches_host_oracle():
    """The device fp64 oracle the production-size comparisons rely on (torch's fp64 GPU convolutions, dropout masks generated
    on the device, sample ranges) against the host fp64 oracle (numpy masks, one whole-batch call): nd 16, B = 2, forward and
    both steps, dropout on, an alpha offset, one range per sample."""
    g, d = _params(16, 17)
    x, cond, z = ot.synthetic_batch(2, 16, 19)
    xs, cs, zs = torch.from_numpy(x).double(), torch.from_numpy(cond).double(), torch.from_numpy(z).double()

    def close(a, b):
        a, b = a.detach().cpu().double(), b.detach().cpu().double()
        err = float((a - b).abs().max()) / float(b.abs().max())
        assert err < 1e-12, err

    close(ot.generator_forward([t.cuda() for t in _t64(g)], zs.cuda(), cs.cuda()), ot.generator_forward(_t64(g), zs, cs))
    losses, grads = ot.critic_step_grads(_t64(d), _t64(g), xs, cs, zs, 555, alpha_offset=2048 + 5)
    dl, dg, parts, _ = ot.critic_step_grads_chunked(d, g, xs.cuda(), cs.cuda(), zs.cuda(), 555, [1, 1], alpha_offset=2048 + 5,
                                                    device="cuda")
    assert dg[0].is_cuda and len(parts) == 2
    close(dl, losses)
    for a, b in zip(dg, grads):
        if float(b.abs().max()) > 1e-12:      # d/d(last critic bias) is analytically 0 in the critic step
            close(a, b)
    loss, grads = ot.gen_step_grads(_t64(d), _t64(g), zs, cs, 556)
    gl, gg, _, _ = ot.gen_step_grads_chunked(d, g, zs.cuda(), cs.cuda(), 556, 1, device="cuda")
    close(gl, loss)
    for a, b in zip(gg, grads):
        if float(b.abs().max()) > 1e-12:      # d/d(last generator bias) likewise (softmax shift invariance)
            close(a, b)


def test_b96_default_options_step_gradients_vs_oracle():
    B = 96
    eng = Engine(ndomain=16, max_batch=B)
    try:
        g, d = _params(16, 91)
        gs, ds = eng.to_slab(g), eng.to_slab(d)
        x, cond, z = ot.synthetic_batch(B, 16, 191)
        ref = ot.generator_forward(_t64(g), torch.from_numpy(z).double(), torch.from_numpy(cond).double()).numpy()
        out = eng.gen_forward(gs, dev(z), dev(cond)).cpu().numpy()
        np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-7)          # north_star tolerance
        assert rel_err(out, ref) < 2e-5
        # critic step: compared directly (observed 1e-7...8e-7).  Generator step: at this batch some of the ~2e8 LeakyReLU
        # inputs always sit within fp32 rounding of zero and take the other slope in fp64, which moves gradients by ~1e-3
        # whatever the batch (the number of flips and the gradient norm both scale as sqrt(B)); the oracle therefore
        # differentiates the branch the fp32 run took (its slope pattern, read back from the workspace) -- the same smooth
        # function on both sides, so the comparison is tight at any size.
        x, cond, z = ot.synthetic_batch(B, 16, 300)
        slab, losses, grads = critic_step_on_engine_branch(eng, ds, gs, d, g, x, cond, z, 4711)
        n = eng.n_critic
        np.testing.assert_allclose(slab[n:n + 4], losses.numpy(), rtol=2e-4, atol=1e-6)
        assert slab[n + 4] == 0.0
        errs = _grad_errors(slab[:n], grads, eng.critic_shapes)
        print("critic grad rel errors:", {k: float(f"{v:.2e}") for k, v in errs.items()})
        assert max(errs.values()) < TIGHT, errs
        slab, loss, grads = gen_step_on_engine_branch(eng, ds, gs, d, g, z, cond, 4712)
        n = eng.n_gen
        np.testing.assert_allclose(slab[n], loss.item(), rtol=2e-4, atol=1e-6)
        errs = _grad_errors(slab[:n], grads, eng.gen_shapes)
        print("gen grad rel errors:", {k: float(f"{v:.2e}") for k, v in errs.items()})
        assert max(errs.values()) < TIGHT, errs
    finally:
        eng.close()


def test_nd64_gen_step_gradients_vs_oracle():
    """largedomain variant (L:59,325,335), B = 1: generator-step gradients incl. the Dense kernel (4196 x 49152) and the
    shared-centre backward at ndomain 64, against the fp64 oracle differentiating the fp32 run's LeakyReLU branch (see the
    B = 96 test)."""
    eng = Engine(ndomain=64, max_batch=1)
    try:
        g, d = _params(64, 15)
        gs, ds = eng.to_slab(g), eng.to_slab(d)
        x, cond, z = ot.synthetic_batch(1, 64, 8)
        slab, loss, grads = gen_step_on_engine_branch(eng, ds, gs, d, g, z, cond, 6)
        n = eng.n_gen
        np.testing.assert_allclose(slab[n], loss.item(), rtol=2e-4, atol=1e-6)
        assert slab[n + 4] == 0.0
        errs = _grad_errors(slab[:n], grads, eng.gen_shapes)
        print("nd64 gen-step grad rel errors:", {k: float(f"{v:.2e}") for k, v in errs.items()})
        assert max(errs.values()) < TIGHT, errs
    finally:
        eng.close()


def _oracle_ranges(nd, B):
    """sample ranges of the device oracle: at most 128 ndomain-16 samples' worth each (~9 GB of fp64 autograd state for the
    generator step), the LAST one 1/32 of the batch -- the range the sensitivity control leaves out, holding the tail tiles"""
    last = max(1, B // 32)
    cap = max(1, 128 * 256 // (nd * nd))
    rest = B - last
    return [cap] * (rest // cap) + ([rest % cap] if rest % cap else []) + [last]


def _oracle_compare(eng, g, d, gs, ds, x, cond, z, out, limit, bf16, offset):
    """The engine's forward pass and both step gradients at this size against the fp64 oracle on the GPU (on the branch the
    engine took; in the bf16 mode fed the generator output `out` the engine fed its critic), plus the drop-the-last-range
    sensitivity control.  Forward: the north-star tolerance (fp32) / FWD_TOL_BF16; step gradients: `limit`."""
    nd, B = eng.ndomain, x.shape[0]
    chunks = _oracle_ranges(nd, B)
    mode = "bf16" if bf16 else "f32"
    tag = f"nd {nd} B {B} {mode} sample_offset {offset}"
    put = lambda a: torch.from_numpy(a).cuda().double()
    gp = [put(a) for a in g]
    with torch.no_grad():
        ref = torch.cat([ot.generator_forward(gp, put(z[lo:hi]), put(cond[lo:hi])) for lo, hi in ot.sample_ranges(B, chunks)])
    o = out.double()
    fwd = float((o - ref).abs().max() / ref.abs().max())
    print(f"{tag}: forward rel error {fwd:.2e}")
    if bf16:
        assert fwd < FWD_TOL_BF16, fwd
    else:
        assert bool(((o - ref).abs() <= 1e-7 + 1e-4 * ref.abs()).all()), fwd        # north-star tolerance
        assert fwd < 2e-5, fwd
    del gp, ref, o
    lrtol, latol = (5e-2, 5e-3) if bf16 else (2e-4, 1e-6)
    steps = []
    gtol = None if bf16 else F32_GATE_TOL_FULLSIZE
    slab, losses, grads, last = critic_step_on_engine_branch_chunked(eng, ds, gs, d, g, x, cond, z, 4711, chunks, mode=mode,
                                                                     fake=out if bf16 else None, alpha_offset=offset,
                                                                     gate_tol=gtol)
    n = eng.n_critic
    assert slab[n + 4] == 0.0
    np.testing.assert_allclose(slab[n:n + 4], losses.numpy(), rtol=lrtol, atol=latol)
    steps.append(("critic", slab[:n], grads, last, eng.critic_shapes))
    slab, loss, grads, last = gen_step_on_engine_branch_chunked(eng, ds, gs, d, g, z, cond, 4712, chunks, mode=mode, gate_tol=gtol)
    n = eng.n_gen
    assert slab[n + 4] == 0.0
    np.testing.assert_allclose(slab[n], loss.item(), rtol=lrtol, atol=latol)
    steps.append(("gen", slab[:n], grads, last, eng.gen_shapes))
    for name, got, ref, last, shapes in steps:
        errs = _grad_errors(got, ref, shapes)
        drop = _grad_errors(got, [r - l for r, l in zip(ref, last)], shapes)
        print(f"{tag}: {name}-step grad rel errors:", {k: float(f"{v:.2e}") for k, v in errs.items()})
        print(f"{tag}: {name}-step drop-last-range ({chunks[-1]} of {B} samples) errors:",
              {k: float(f"{v:.2e}") for k, v in drop.items()})
        # sensitivity: fp32 -- EVERY tensor's comparison would see the lost range (its error would be >= 3x the limit);
        # bf16 -- the step's comparison as a whole would (the largest tensor error): a kernel tensor loses ~3e-2 of its
        # largest entry with 1/32 of the batch, short of 3x the bf16 limit, so per tensor the fp32 twin carries the control
        sens = min(drop.values()) if not bf16 else max(drop.values())
        print(f"{tag}: {name}-step worst {max(errs.values()):.2e} (limit {limit:.1e}), drop-last-range "
              f"{'smallest' if not bf16 else 'largest'} {sens:.2e} (must be >= {3 * limit:.1e})")
        assert max(errs.values()) < limit, errs
        assert sens >= 3 * limit, drop          # the comparison would see a lost tile / partial slab / sample range


def _fullsize_properties(nd, B, n_critic, probe, small, bf16=0, limit=None, offset=0):
    """bf16 = 1: the bf16 storage mode, the mode BASELINE configs[2..4] are quoted in (bench.py --config 3|4|5).
    Properties that hold at any size: softmax mass conservation, batch independence of sample `probe` against a run of
    `small` samples around it, bit-identical repeats (no atomics anywhere on the path), finite gradient slabs with a clear
    non-finite flag, and one whole training iteration (n_critic critic updates + 1 generator update) with finite losses
    that really moved both weight slabs.  limit: first compare the forward pass and both step gradients of the same engine
    with the fp64 oracle on the GPU (_oracle_compare), gradients within `limit`.  offset: the engine's "sample_offset" (the
    global index of a shard's first sample, which keys RandomWeightedAverage's alpha)."""
    eng = Engine(ndomain=nd, max_batch=B)
    try:
        if bf16:
            eng.set_option("bf16", 1)
        if offset:
            eng.set_option("sample_offset", offset)
        g, d = _params(nd, 16)
        gs, ds = eng.to_slab(g), eng.to_slab(d)
        x, cond, z = ot.synthetic_batch(B, nd, 9)
        xd, cd, zd = dev(x), dev(cond), dev(z)
        out = eng.gen_forward(gs, zd, cd)
        if limit is not None:
            _oracle_compare(eng, g, d, gs, ds, x, cond, z, out, limit, bf16, offset)
        o = out.cpu().numpy()
        assert o.shape == (B, 24, nd, nd, 1) and np.all(np.isfinite(o)) and o.min() >= 0
        np.testing.assert_allclose(o.sum(axis=1), 1.0, atol=3e-6)
        lo = max(0, probe - small // 2); hi = lo + small
        part = eng.gen_forward(gs, dev(z[lo:hi]), dev(cond[lo:hi])).cpu().numpy()
        # tile / split-K choices depend on the batch size: fp32 sums round differently (2e-5); in the bf16 storage mode such a
        # difference can move a stored activation by one bf16 ulp (2^-8 relative), which the later layers carry along
        if bf16:
            assert rel_err(part, o[lo:hi]) < 2e-2
        else:
            np.testing.assert_allclose(part, o[lo:hi], rtol=2e-5, atol=1e-8)
        again = eng.gen_forward(gs, zd, cd)
        assert torch.equal(out, again)
        c1 = eng.critic_grad(ds, gs, xd, cd, zd, 31337).clone()
        c2 = eng.critic_grad(ds, gs, xd, cd, zd, 31337)
        assert torch.equal(c1, c2)
        g1 = eng.gen_grad(ds, gs, zd, cd, 31338).clone()
        g2 = eng.gen_grad(ds, gs, zd, cd, 31338)
        assert torch.equal(g1, g2)
        for slab, n in ((c1, eng.n_critic), (g1, eng.n_gen)):
            s = slab.cpu().numpy()
            assert np.all(np.isfinite(s)) and s[n + 4] == 0
            assert np.abs(s[:n]).max() > 0
        # critic loss parts as Keras reports them: valid = mean(-D(real)), fake = mean(D(fake)), total = sum with 10 gp
        t = c1[eng.n_critic:eng.n_critic + 4].cpu().numpy()
        np.testing.assert_allclose(t[0], t[1] + t[2] + 10.0 * t[3], rtol=1e-5, atol=1e-6)
        if bf16 and B >= 171:
            # from 171 samples on the column GEMM of the critic's input gradient takes the resident-tile kernel
            # (conv16_resident_ok accepts its plan): same products in the same order as the streaming kernel
            eng.set_option("resident", 0)
            c3 = eng.critic_grad(ds, gs, xd, cd, zd, 31337)
            eng.set_option("resident", 1)
            assert torch.equal(c1, c3)
        tr = WGANGPTrainer(eng, g, d, n_disc=n_critic)
        g_before, d_before = tr.gparams.clone(), tr.dparams.clone()
        d_loss, g_loss, bad = tr.iteration([(xd, cd, zd)] * n_critic, (zd, cd))
        assert float(bad) == 0 and np.isfinite(float(d_loss)) and np.isfinite(float(g_loss))
        assert tr.t == n_critic + 1
        assert not torch.equal(tr.gparams, g_before) and not torch.equal(tr.dparams, d_before)
        assert bool(torch.isfinite(tr.gparams).all()) and bool(torch.isfinite(tr.dparams).all())
    finally:
        eng.close()


# Step-gradient limits of the production-size oracle comparisons.  fp32: TIGHT, as at every other size.  bf16: 3x the largest
# error observed at these sizes (per tensor, relative to the tensor's largest entry), never above test_hip_bf16.GRAD_TOL.
# Observed (largest per step): fp32 critic / generator 8.4e-7 / 1.3e-6 (B 256), 2.2e-6 / 2.0e-6 (B 2048), 1.4e-6 / 1.6e-6
# (B 1024), 2.3e-6 / 2.9e-6 (ndomain 64); bf16 4.8e-3 / 7.0e-3 (B 2048), 5.1e-3 / 6.8e-3 (B 1024), 4.9e-3 / 7.8e-3 (ndomain 64).
# Forward: fp32 1.1e-6 ... 1.6e-6, bf16 5.2e-3 ... 7.8e-3 of the largest fraction.
FWD_TOL_BF16 = 2e-2                       # test_hip_bf16.FWD_TOL
BF16_LIMIT = 2.4e-2
# The fp32 gate guard at these sizes.  GATE_TOL["f32"] (tests/hip_util.py) keeps holding every other test; its margin limit
# (2.5e-6 RMS, 3x the largest margin the small-batch tests meet) is below what fp32 rounding alone reaches over 10-30x more
# LeakyReLU inputs: at B = 256 generator h3 (PixelNorm'ed, RMS 1) has 17 disagreements in 1.0e8 inputs, the farthest 2.64e-6
# from the kink; 2.72e-6 (critic layer 4, B = 2048), 3.04e-6 (B = 1024), 4.76e-6 (ndomain 64).  The fraction limit is kept
# (observed 5.5e-7 of 6e-5); the margin limit here is 3x the largest margin these sizes meet.
F32_GATE_TOL_FULLSIZE = dict(GATE_TOL["f32"], max_margin=1.5e-5)


def test_config1_bs256_fp32_vs_oracle():
    """BASELINE configs[1], the metric: ndomain 16, bs = 256, fp32, n_critic = 1 -- forward at the north-star tolerance and
    both step gradients at TIGHT against the fp64 oracle."""
    _fullsize_properties(16, 256, 1, probe=201, small=3, limit=TIGHT)


@pytest.mark.parametrize("bf16", [0, 1])
def test_config2_bs2048_ncritic5_properties(bf16):
    """BASELINE configs[2]: ndomain 16, bs = 2048, n_critic = 5 (30 GiB workspace, > 2 GiB tensors); quoted in bf16."""
    _fullsize_properties(16, 2048, 5, probe=1777, small=4, bf16=bf16, limit=BF16_LIMIT if bf16 else TIGHT)


@pytest.mark.parametrize("bf16", [0, 1])
def test_config3_shard_bs1024_properties(bf16):
    """BASELINE configs[3]: global bs 8192 over 8 GPUs = 1024 per rank (here rank 7: sample_offset 7 x 1024); quoted in bf16."""
    _fullsize_properties(16, 1024, 5, probe=1000, small=3, bf16=bf16, limit=BF16_LIMIT if bf16 else TIGHT, offset=7 * 1024)


@pytest.mark.parametrize("bf16", [0, 1])
def test_config4_shard_nd64_bs64_properties(bf16):
    """BASELINE configs[4]: ndomain 64, global bs 512 over 8 GPUs = 64 per rank (here rank 3: sample_offset 3 x 64); quoted
    in bf16."""
    _fullsize_properties(64, 64, 5, probe=41, small=2, bf16=bf16, limit=BF16_LIMIT if bf16 else TIGHT, offset=3 * 64)
