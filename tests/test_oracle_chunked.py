"""The chunked fp64 oracle (oracle/rdgan_torch.py: critic_step_grads_chunked, gen_step_grads_chunked) that the production-size
GPU comparisons (tests/test_hip_fullsize.py) run on the device: evaluating a batch over sample ranges must give what ONE
whole-batch call gives, and the pieces it is built from -- offset dropout masks, the torch port of the counter RNG, pooled
gate-guard counts -- must match their whole-tensor / numpy originals."""
import numpy as np
import pytest
import torch

from oracle import rdgan_np as onp
from oracle import rdgan_torch as ot
from oracle import rng as orng


def _setup(nd, B, seed):
    rng = np.random.default_rng(seed)
    g = [p.astype(np.float64) for p in onp.init_generator(rng, nd)]
    d = [p.astype(np.float64) for p in onp.init_critic(rng, nd)]
    g = [p if p.ndim > 1 else 0.05 * rng.standard_normal(p.shape) for p in g]
    d = [p if p.ndim > 1 else 0.05 * rng.standard_normal(p.shape) for p in d]
    x, cond, z = ot.synthetic_batch(B, nd, seed + 1, np.float64)
    t = lambda arrs: [torch.from_numpy(a) for a in arrs]
    return t(g), t(d), torch.from_numpy(x), torch.from_numpy(cond), torch.from_numpy(z)


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= tol * scale, float(np.abs(a - b).max()) / scale


@pytest.mark.parametrize("nd,B,chunk,alpha_offset", [(16, 5, [2, 2, 1], 7 * 1024 + 3), (8, 4, 3, 192)])
def test_critic_step_chunked_equals_whole_batch(nd, B, chunk, alpha_offset):
    g, d, x, cond, z = _setup(nd, B, 31)
    seed = 9001
    losses, grads = ot.critic_step_grads(d, g, x, cond, z, seed, alpha_offset=alpha_offset)
    cl, cg, parts, stats = ot.critic_step_grads_chunked(d, g, x, cond, z, seed, chunk, alpha_offset=alpha_offset)
    assert stats is None and len(parts) == len(ot.sample_ranges(B, chunk))
    _close(cl.numpy(), losses.numpy())
    for a, b in zip(cg, grads):
        if float(b.abs().max()) > 1e-12:      # d/d(last bias) of the critic step is analytically 0
            _close(a.numpy(), b.numpy())
    for a, ps in zip(cg, zip(*parts)):
        _close(sum(p.numpy() for p in ps), a.numpy(), 1e-14)
    # every range contributes: leaving one out changes the kernel gradients visibly
    for i in range(len(parts)):
        assert float((cg[2] - parts[i][2]).sub(grads[2]).abs().max()) > 1e-3 * float(grads[2].abs().max())


@pytest.mark.parametrize("nd,B,chunk", [(16, 5, [2, 2, 1]), (8, 4, 3)])
def test_gen_step_chunked_equals_whole_batch(nd, B, chunk):
    g, d, x, cond, z = _setup(nd, B, 41)
    seed = 9002
    loss, grads = ot.gen_step_grads(d, g, z, cond, seed)
    cl, cg, parts, stats = ot.gen_step_grads_chunked(d, g, z, cond, seed, chunk)
    assert stats is None
    _close(cl.numpy(), loss.numpy())
    for a, b in zip(cg, grads):
        if float(b.abs().max()) > 1e-12:      # d/d(last bias before the softmax) is analytically 0
            _close(a.numpy(), b.numpy())
    for a, ps in zip(cg, zip(*parts)):
        _close(sum(p.numpy() for p in ps), a.numpy(), 1e-14)


def _flip_near_kink(acts, n):
    """slope patterns of `acts` (post-activation, so sign = the oracle's own decision) with the n entries nearest the kink
    of every layer flipped -- an external run that rounded those inputs to the other side (dropped entries, which read 0,
    are left alone: the guard ignores them)"""
    out = []
    for a in acts:
        gt = (a > 0).contiguous()
        flat = gt.view(-1)
        key = a.abs().reshape(-1)
        flat[torch.where(key > 0, key, torch.full_like(key, np.inf)).argsort()[:n]] ^= True
        out.append(gt)
    return out


def test_gate_guard_pools_over_ranges():
    """The guard's disagreement fraction and kink margin of a chunked run equal those of check_gates on the whole batch
    (the fraction is pooled before max_fraction applies; the margin is relative to the RMS of the WHOLE layer)."""
    nd, B, seed, chunk = 16, 5, 4711, [2, 2, 1]
    g, d, x, cond, z = _setup(nd, B, 51)
    _, _, dh = ot.critic_step_grads(d, g, x, cond, z, seed, return_intermediates=True)
    gates = _flip_near_kink(dh, 3)
    _, _, dh2 = ot.critic_step_grads(d, g, x, cond, z, seed, gates=gates, return_intermediates=True)
    whole = ot.check_gates(gates, dh2, ot.critic_masks(seed, 3 * B, nd, torch.float64), max_margin=1, max_fraction=1)
    _, _, _, stats = ot.critic_step_grads_chunked(d, g, x, cond, z, seed, chunk, gates=gates)
    pooled = ot.check_gate_stats(stats, max_margin=1, max_fraction=1)
    assert whole[0] > 0 and whole[1] > 0
    np.testing.assert_allclose(pooled, whole, rtol=1e-12)
    # ... and it is the pooled fraction that max_fraction limits
    with pytest.raises(AssertionError, match="slope disagreements"):
        ot.check_gate_stats(stats, max_margin=1, max_fraction=0.99 * whole[1])

    _, _, (gh, gdh) = ot.gen_step_grads(d, g, z, cond, seed, return_intermediates=True)
    gg, dg = _flip_near_kink(gh, 2), _flip_near_kink(gdh, 2)
    _, _, (gh2, gdh2) = ot.gen_step_grads(d, g, z, cond, seed, gates=(gg, dg), return_intermediates=True)
    wg = ot.check_gates(gg, gh2, None, max_margin=1, max_fraction=1)
    wd = ot.check_gates(dg, gdh2, ot.critic_masks(seed, B, nd, torch.float64), max_margin=1, max_fraction=1)
    _, _, _, (sg, sd) = ot.gen_step_grads_chunked(d, g, z, cond, seed, chunk, gates=(gg, dg))
    np.testing.assert_allclose(ot.check_gate_stats(sg, 1, 1), wg, rtol=1e-12)
    np.testing.assert_allclose(ot.check_gate_stats(sd, 1, 1), wd, rtol=1e-12)


def test_sample_ranges():
    assert ot.sample_ranges(5, [2, 2, 1]) == [(0, 2), (2, 4), (4, 5)]
    assert ot.sample_ranges(2048, 64)[-1] == (1984, 2048) and len(ot.sample_ranges(2048, 64)) == 32
    assert ot.sample_ranges(7, 3) == [(0, 3), (3, 6), (6, 7)]
    with pytest.raises(AssertionError):
        ot.sample_ranges(5, [2, 2])


@pytest.mark.parametrize("start", [0, 4, 12, 37, 49152 * 3])
def test_dropout_mask_offset_is_a_slice_of_the_full_mask(start):
    shp = (7, 12, 8, 8, 64)
    full = orng.dropout_scale_mask(77, orng.STREAM_D1, shp).ravel()
    n = 3 * 12 * 8 * 8 * 64 - 5
    part = orng.dropout_scale_mask(77, orng.STREAM_D1, (n,), start=start)
    assert np.array_equal(part, full[start:start + n])
    dev = orng.dropout_scale_mask_t(77, orng.STREAM_D1, (n,), start=start).numpy()
    assert np.array_equal(dev, part)
    assert np.array_equal(orng.dropout_scale_mask_t(0, 1, (n,)).numpy(), np.ones(n, np.float32))


def test_torch_rng_port_is_bit_equal():
    x = np.random.default_rng(0).integers(0, 2 ** 32, 200000, dtype=np.uint64)
    x[:4] = [0, 1, 0xFFFFFFFF, 0x80000000]
    want = orng.mix32(x.astype(np.uint32))
    got = orng.mix32_t(torch.from_numpy(x.astype(np.int64))).numpy()
    assert np.array_equal(got.astype(np.uint32), want) and got.max() < 2 ** 32 and got.min() >= 0
    for seed, stream, start in ((0x123456789ABC, 3, 0), (5, orng.STREAM_ALPHA, 2 ** 32 - 10), (4242, 1, 10 ** 9)):
        assert np.array_equal(orng.bits_t(seed, stream, 5000, start=start).numpy().astype(np.uint32),
                              orng.bits(seed, stream, 5000, start=start))
