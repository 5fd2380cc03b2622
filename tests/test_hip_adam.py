"""-m gpu: the optimizer update itself -- k_adam (csrc/rdgan_elem.hip.h) launched by rdgan_adam (csrc/rdgan_api.hip) and driven
by WGANGPTrainer._update -- against fp64 Adam (tests/adam_np.py: adam_f64) of the very gradient slab the kernel consumed.  No
LeakyReLU kink and no generator or critic kernel enters any comparison here, so the bounds are those of fp32 arithmetic.

Every comparison goes through adam_np.check_update (tests/test_adam_host.py shows on the CPU that it accepts an honest fp32
evaluation at every grid point and refuses a misplaced eps, an unscaled v, t - 1 and a skipped tail):

    |p' - (p0 - delta64)| <= ulp(p0) + tol |delta64|,   tol = 4 x 2.4e-7 + 2^-24 beta2^t / (1 - beta2^t)
    |v' - v64|            <= 4 x 1.24e-7 v64 + 2^-126

2.4e-7 / 1.24e-7: what the float32 restatement deviates from fp64 (measured on the CPU, tests/test_adam_host.py); the factor 4
is margin for FMA contraction and the GPU's division and square root; the second term of tol is the cancellation in the fp32
`1 - powf(beta2, t)` of rdgan_adam (derived in adam_np.tol_delta, not measured).

Limits and what an MI355X showed on the first run (worst relative deviation of the step with p0 = 0; each test prints its own):
    grid, n = 4099, worst over grad_scale and eps       beta2 = 0.9               beta2 = 0.999
        t = 1                                  limit 1.496e-6  observed 2.31e-7   limit 6.051e-5  observed 2.22e-7
        t = 2                                  limit 1.214e-6  observed 2.51e-7   limit 3.072e-5  observed 3.48e-6
        t = 7                                  limit 1.015e-6  observed 1.98e-7   limit 9.441e-6  observed 1.39e-6
        t = 1000                               limit 9.600e-7  observed 1.70e-7   limit 9.947e-7  observed 2.36e-7
        t = 10^6                               limit 9.600e-7  observed 1.70e-7   limit 9.600e-7  observed 1.76e-7
      (beta2 = 0.999 at t = 2, 7: the cancellation term at work, an eighth of what it allows; never above 0.24 of a limit)
    v', every test                             limit 4.960e-7  observed 1.22e-7 (n = 8388613; grid 1.13e-7)
    sizes 1 ... 8388613 (beta2 0.9, t 7)       limit 1.015e-6  observed 2.36e-7 (n = 8388613; 3.0e-8 ... 1.7e-7 below 1026)
    trainer steps t = 1 ... 6, zero biases     limit 1.496e-6 ... 1.028e-6       observed 2.36e-7 (fp32), 2.34e-7 (bf16 storage)
"""
import numpy as np
import pytest
import torch

from oracle import rdgan_torch as ot
from pr_disagg_radar_gan_amd import Engine
from pr_disagg_radar_gan_amd import weights as W
from pr_disagg_radar_gan_amd.trainer import LOSS_SLOTS, WGANGPTrainer
from tests import adam_np as A
from tests.hip_util import dev, lib, ptr, stream

pytestmark = pytest.mark.gpu

N = 4099
PAD = 16                                     # canary floats on each side of p and v
CANARY = np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]      # a NaN with a payload: reading it would show, too
SECOND_SWEEP = 8192 * 256 * 4 + 5            # ew_blocks caps the grid at 8192 blocks of 256 threads x 4 floats


@pytest.fixture(scope="module")
def eng8():
    e = Engine(ndomain=8, max_batch=1)
    yield e
    e.close()


def _bits(t):
    return t.view(torch.int32)


def _update_on_gpu(eng, p0, g, v0, t, lr=1e-4, beta2=0.9, eps=1e-7, grad_scale=1.0, left=PAD, right=PAD, shard_extra=None):
    """One Engine.adam call on interior views p[left:left+n], v[left:left+n] of longer buffers whose other elements hold the
    canary, with the gradient slab of n + 8 floats (loss slots = canary) as the all-reduce exchange passes it -- or, with
    shard_extra, the view g[:n] of a shard buffer that much longer, as the sharded exchange does.  Asserts that every element
    outside the views, and the whole gradient buffer, is bit-identical afterwards; returns (p', v') of the views as numpy."""
    n = p0.size
    host = {}
    for name, a in (("p", p0), ("v", v0)):
        buf = np.full(left + n + right, CANARY, np.float32)
        buf[left:left + n] = a
        host[name] = buf
    gbuf = np.full(n + (LOSS_SLOTS if shard_extra is None else shard_extra), CANARY, np.float32)
    gbuf[:n] = g
    pd, vd, gd = dev(host["p"]), dev(host["v"]), dev(gbuf)
    g_before = gd.clone()
    eng.adam(pd[left:left + n], gd if shard_extra is None else gd[:n], vd[left:left + n], t, lr, beta2, eps, grad_scale)
    torch.cuda.synchronize()
    assert torch.equal(_bits(gd), _bits(g_before)), "the gradient slab changed"
    for name, d in (("p", pd), ("v", vd)):
        want = torch.from_numpy(host[name]).cuda()
        assert torch.equal(_bits(d[:left]), _bits(want[:left])), f"{name}: elements in front of the view changed"
        assert torch.equal(_bits(d[left + n:]), _bits(want[left + n:])), f"{name}: elements behind the view changed"
    return pd[left:left + n].cpu().numpy(), vd[left:left + n].cpu().numpy()


@pytest.mark.parametrize("eps", [1e-7, 1e-3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("beta2", [0.9, 0.999])
@pytest.mark.parametrize("t", A.T_CASES)
def test_step_at_full_precision_over_the_parameter_grid(eng8, t, beta2, grad_scale, eps):
    """p0 = 0: the kernel's p' is exactly the negated fp32 step, compared with fp64 at tol (module docstring)"""
    g, v0, _ = A.family(N)
    p0 = np.zeros(N, np.float32)
    p1, v1 = _update_on_gpu(eng8, p0, g, v0, t, 1e-4, beta2, eps, grad_scale)
    dd, dv = A.check_update(p1, v1, p0, g, v0, t, 1e-4, beta2, eps, grad_scale, what="k_adam")
    print(f"t {t} beta2 {beta2} grad_scale {grad_scale} eps {eps}: step deviates by {dd:.3e} (limit {A.tol_delta(beta2, t):.3e}), "
          f"v' by {dv:.3e} (limit {A.TOL_V:.3e})")


@pytest.mark.parametrize("beta2", [0.9, 0.999])
@pytest.mark.parametrize("t", [1, 7, 10 ** 6])
def test_zero_gradients_give_a_step_of_exactly_zero(eng8, t, beta2):
    """g = 0 with v0 = 0 (0 / (0 + eps)): the parameter keeps its bits and v' is 0; g = 0 with v0 > 0: the parameter keeps its
    bits and v' is the float32 product beta2 v0 (whatever the contraction: (1 - beta2) 0 0 adds an exact zero); nothing is
    non-finite -- for p0 = 0 and for p0 ~ N(0, 1)"""
    g, v0, bl = A.family(N)
    for p0 in (np.zeros(N, np.float32), np.random.default_rng(2).standard_normal(N).astype(np.float32)):
        p1, v1 = _update_on_gpu(eng8, p0, g, v0, t, beta2=beta2)
        assert np.isfinite(p1).all() and np.isfinite(v1).all()
        for name in ("zero_zero", "zero_v"):
            assert np.array_equal(p1[bl[name]].view(np.int32), p0[bl[name]].view(np.int32)), name
        assert not v1[bl["zero_zero"]].any()
        assert np.array_equal(v1[bl["zero_v"]], np.float32(beta2) * v0[bl["zero_v"]])
        A.check_update(p1, v1, p0, g, v0, t, beta2=beta2, what="k_adam")


@pytest.mark.parametrize("t,beta2,grad_scale,eps", [(1, 0.9, 1.0, 1e-7), (7, 0.9, 0.5, 1e-7), (2, 0.999, 0.125, 1e-3), (10 ** 6, 0.999, 1.0, 1e-7)])
def test_step_composed_with_a_real_parameter(eng8, t, beta2, grad_scale, eps):
    g, v0, _ = A.family(N)
    p0 = np.random.default_rng(3).standard_normal(N).astype(np.float32)
    p1, v1 = _update_on_gpu(eng8, p0, g, v0, t, 1e-4, beta2, eps, grad_scale)
    A.check_update(p1, v1, p0, g, v0, t, 1e-4, beta2, eps, grad_scale, what="k_adam")
    assert (p1 != p0).mean() > 0.3            # (a step below half an ulp of p0 leaves it: |g| << 1e-7)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1025, SECOND_SWEEP])
def test_sizes_tails_and_canaries(eng8, n):
    """n < 4: only the n % 4 tail of block 0 runs; 4, 5, 7: one float4 and a tail; 1023 / 1025: around a whole block;
    8192 x 256 x 4 + 5: the first size at which the grid-stride loop takes a second sweep.  16 canary floats on each side of p
    and v, and the gradient slab with its 8 loss slots, keep their bits (_update_on_gpu)."""
    g, v0, _ = A.family(n)
    p0 = np.zeros(n, np.float32)
    p1, v1 = _update_on_gpu(eng8, p0, g, v0, 7, grad_scale=0.5)
    dd, dv = A.check_update(p1, v1, p0, g, v0, 7, grad_scale=0.5, what=f"k_adam n {n}")
    print(f"n {n}: step deviates by {dd:.3e} (limit {A.tol_delta(0.9, 7):.3e}), v' by {dv:.3e} (limit {A.TOL_V:.3e})")
    assert p1[-(n % 4):].all() and v1[-(n % 4):].all()               # the tail moved: every g of the family's free part is != 0
    if n < 2048:                                                     # and composed with a parameter of ordinary size
        p0 = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        p1, v1 = _update_on_gpu(eng8, p0, g, v0, 7, grad_scale=0.5)
        A.check_update(p1, v1, p0, g, v0, 7, grad_scale=0.5, what=f"k_adam n {n}")


@pytest.mark.parametrize("length", [1, 1026, 4099])          # (hi - lo) % 4 = 1, 2, 3
@pytest.mark.parametrize("lo", [4, 4096])
def test_the_call_shape_of_the_sharded_exchange(eng8, lo, length):
    """WGANGPTrainer._update (sharded): eng.adam(pbuf[lo:hi], gsh[:hi - lo], vbuf[lo:hi], ...) -- interior views that start at a
    multiple of 4 floats and whose length is none, with the gradient at the head of a longer shard buffer.  Elements outside
    the views keep their bits; inside, the composed bound holds."""
    assert lo % 4 == 0 and length % 4 in (1, 2, 3)
    g, v0, _ = A.family(length, seed=lo)
    p0 = np.random.default_rng(lo + length).standard_normal(length).astype(np.float32)
    for t, s in ((1, 0.5), (2, 0.125)):
        p1, v1 = _update_on_gpu(eng8, p0, g, v0, t, grad_scale=s, left=lo, right=37, shard_extra=43)
        A.check_update(p1, v1, p0, g, v0, t, grad_scale=s, what=f"k_adam on [{lo}:{lo + length}]")


def test_refusals_leave_every_buffer_alone(eng8):
    """rdgan_adam returns -2 for t = 0, n = 0 or a null pointer and launches nothing; Engine.adam raises ValueError for a
    gradient slab shorter than the parameters"""
    g, v0, _ = A.family(64)
    p0 = np.random.default_rng(4).standard_normal(64).astype(np.float32)
    pd, gd, vd = dev(p0), dev(g), dev(v0)
    before = [x.clone() for x in (pd, gd, vd)]
    L = lib()
    hyper = (1e-4, 0.9, 1e-7, 1.0)
    assert L.rdgan_adam(ptr(pd), ptr(gd), ptr(vd), 64, 0, *hyper, stream()) == -2
    assert L.rdgan_adam(ptr(pd), ptr(gd), ptr(vd), 64, -1, *hyper, stream()) == -2
    assert L.rdgan_adam(ptr(pd), ptr(gd), ptr(vd), 0, 1, *hyper, stream()) == -2
    assert L.rdgan_adam(ptr(None), ptr(gd), ptr(vd), 64, 1, *hyper, stream()) == -2
    assert L.rdgan_adam(ptr(pd), ptr(None), ptr(vd), 64, 1, *hyper, stream()) == -2
    assert L.rdgan_adam(ptr(pd), ptr(gd), ptr(None), 64, 1, *hyper, stream()) == -2
    with pytest.raises(ValueError):
        eng8.adam(pd, gd[:63], vd, 1)
    torch.cuda.synchronize()
    for x, b in zip((pd, gd, vd), before):
        assert torch.equal(_bits(x), _bits(b))
    assert L.rdgan_adam(ptr(pd), ptr(gd), ptr(vd), 64, 1, *hyper, stream()) == 0       # and the same call with t = 1 is taken
    torch.cuda.synchronize()
    A.check_update(pd.cpu().numpy(), vd.cpu().numpy(), p0, g, v0, 1, what="rdgan_adam")


# ---- the trainer, one update at a time

@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("overlap", [False, True])
def test_every_trainer_update_is_adam_of_the_slab_the_engine_left(overlap, bf16):
    """World 1, n_disc = 2, two iterations (t = 1 ... 6: critic, critic, generator, twice), fp32 and bf16 storage, with and
    without the communication stream.  After each step: the shared counter grew by one; the updated network's parameters and
    v are fp64 Adam of (parameters before, the gradient slab the step left, v before, t) within the composed bound; the other
    network's parameters and v kept their bits; the loss tail behind the gradients holds the finite losses the step returned."""
    nd, B = 8, 2
    eng = Engine(ndomain=nd, max_batch=B)
    try:
        if bf16:
            eng.set_option("bf16", 1)
        rng = np.random.default_rng(5)
        tr = WGANGPTrainer(eng, W.init_generator(rng, nd), W.init_critic(rng, nd), n_disc=2, overlap=overlap, base_seed=7)
        assert tr.overlap == overlap and tr.world == 1 and tr.exchange == {"g": "allreduce", "d": "allreduce"}
        worst = 0.0
        for it in range(2):
            steps = [("d", 100 + 10 * it), ("d", 101 + 10 * it), ("g", 102 + 10 * it)]
            for which, seed in steps:
                x, c, z = (dev(a) for a in ot.synthetic_batch(B, nd, seed))
                other = "g" if which == "d" else "d"
                before = {k: getattr(tr, k).clone() for k in ("gparams", "dparams", "gv", "dv")}
                t0 = tr.t
                losses = tr.critic_step(x, c, z) if which == "d" else tr.gen_step(z, c)
                tr.join()
                torch.cuda.synchronize()
                assert tr.t == t0 + 1
                n = before[which + "params"].numel()
                grad = tr.reduced_grad(which)[:n].cpu().numpy()
                dd, _ = A.check_update(getattr(tr, which + "params").cpu().numpy(), getattr(tr, which + "v").cpu().numpy(),
                                       before[which + "params"].cpu().numpy(), grad, before[which + "v"].cpu().numpy(),
                                       tr.t, tr.lr, tr.beta2, tr.eps, 1.0, what=f"{which} update at t = {tr.t}")
                worst = max(worst, dd)
                assert np.abs(grad).max() > 0
                for k in (other + "params", other + "v"):
                    assert torch.equal(_bits(getattr(tr, k)), _bits(before[k])), f"{k} changed in a '{which}' step (t = {tr.t})"
                tail = tr._slab(which)[n:n + LOSS_SLOTS].cpu()
                assert tail.numel() == LOSS_SLOTS and bool(torch.isfinite(tail).all())
                assert torch.equal(tail[:5], losses.cpu()) and float(tail[4]) == 0.0 and float(tail[0]) != 0.0
        assert tr.t == 6
        print(f"overlap {overlap} bf16 {bf16}: worst step deviation where p0 = 0 (the biases' first updates): {worst:.3e}")
    finally:
        eng.close()
