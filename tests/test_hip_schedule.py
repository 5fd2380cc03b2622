"""The generator forward ahead ("gen_fwd_ahead", default on with fp32 storage; rdgan_critic_grad_ahead): the last critic step of an iteration
issues the generator step's forward on a stream of the handle's own, beside its tail; the generator step skips its forward.
Everything here compares against the option off, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pr_disagg_radar_gan_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(nd, seed):
    rng = np.random.default_rng(seed)
    return W.init_generator(rng, nd), W.init_critic(rng, nd)


def test_trainer_hands_the_generator_batch_to_the_last_critic_step_only():
    """CPU: iteration() passes (z, cond) of the generator step to the last of the n_disc critic steps, and only to an engine
    that declares it can use it (Engine.forward_ahead); the oracle-backed stand-in never sees the argument."""
    from pr_disagg_radar_gan_amd.trainer import WGANGPTrainer
    from tests.fake_engine import FakeEngine
    from oracle import rdgan_torch as ot

    class Recording(FakeEngine):
        forward_ahead = True

        def __init__(self, nd):
            super().__init__(nd)
            self.seen = []

        def critic_grad(self, dparams, gparams, x_real, cond, z, seed, grad_out=None, gen_batch=None):
            self.seen.append(gen_batch)
            return super().critic_grad(dparams, gparams, x_real, cond, z, seed, grad_out=grad_out)

    g, d = _weights(8, 3)
    x, c, z = (torch.from_numpy(a) for a in ot.synthetic_batch(2, 8, 4))
    _, c2, z2 = (torch.from_numpy(a) for a in ot.synthetic_batch(2, 8, 5))
    eng = Recording(8)
    tr = WGANGPTrainer(eng, g, d, n_disc=3)
    tr.iteration([(x, c, z)] * 3, (z2, c2))
    assert eng.seen[:2] == [None, None]
    assert eng.seen[2][0] is z2 and eng.seen[2][1] is c2
    tr.iteration_raw([(x, c, z)] * 3, (z2, c2))
    assert eng.seen[3:5] == [None, None] and eng.seen[5][0] is z2
    plain = WGANGPTrainer(FakeEngine(8), g, d, n_disc=1)          # no forward_ahead: called exactly as before
    plain.iteration([(x, c, z)], (z2, c2))


def _train(eng, g, d, batches, n_disc, iters, ahead, overlap=None):
    from pr_disagg_radar_gan_amd.trainer import WGANGPTrainer
    eng.set_option("gen_fwd_ahead", ahead)
    tr = WGANGPTrainer(eng, g, d, n_disc=n_disc, base_seed=5, overlap=overlap)
    tails = []
    for it in range(iters):
        crit = [batches[(it + j) % len(batches)] for j in range(n_disc)]
        _, c, z = batches[(it + n_disc) % len(batches)]
        dl, gl = tr.iteration_raw(crit, (z, c))
        tails.append(torch.cat([dl[:5].clone(), gl[:5].clone()]))
    tr.join()
    torch.cuda.synchronize()
    return tr.gparams.clone(), tr.dparams.clone(), tr.gv.clone(), tr.dv.clone(), torch.stack(tails)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("n_disc", [1, 5])
@pytest.mark.parametrize("B", [1, 7, 256])
def test_training_run_is_bit_identical_with_the_forward_ahead(bf16, n_disc, B):
    """Whole iterations with the option on and off from the same weights, batches and seeds: loss tails, both weight slabs and
    both Adam slabs are torch.equal -- a missing wait between the two streams, or a buffer both of them write, would show."""
    from pr_disagg_radar_gan_amd import Engine
    from pr_disagg_radar_gan_amd.trainer import synthetic_batch_device
    eng = Engine(ndomain=16, max_batch=B)
    try:
        if bf16:
            eng.set_option("bf16", 1)
        g, d = _weights(16, 40 + B)
        batches = [synthetic_batch_device(B, 16, 300 + i, eng.device) for i in range(3)]
        iters = 3 if n_disc == 5 else 6
        on = _train(eng, g, d, batches, n_disc, iters, 1)
        off = _train(eng, g, d, batches, n_disc, iters, 0)
        for a, b in zip(on, off):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(on[4]).all()) and float(on[4][:, 4].abs().max()) == 0 and float(on[4][:, 9].abs().max()) == 0
        assert not torch.equal(on[0], eng.to_slab(g))
    finally:
        eng.close()


@pytest.mark.gpu
def test_overlapped_trainer_is_bit_identical_with_the_forward_ahead():
    """overlap=True (the data-parallel schedule: exchange + Adam on a communication stream, g_ready / d_ready events) at
    world 1: the forward ahead forks behind the compute stream's wait for the generator update."""
    from pr_disagg_radar_gan_amd import Engine
    from pr_disagg_radar_gan_amd.trainer import synthetic_batch_device
    B = 24
    eng = Engine(ndomain=16, max_batch=B)
    try:
        g, d = _weights(16, 7)
        batches = [synthetic_batch_device(B, 16, 500 + i, eng.device) for i in range(3)]
        on = _train(eng, g, d, batches, 2, 6, 1, overlap=True)
        off = _train(eng, g, d, batches, 2, 6, 0, overlap=True)
        for a, b in zip(on, off):
            assert torch.equal(a, b)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [0, 1])
def test_generator_step_uses_the_batch_it_is_given(bf16):
    """Engine level.  The critic step is told one generator batch (z1, c1); then
    (a) the generator step on exactly that batch equals the option off,
    (b) a generator step on another batch in other buffers (z2, c2) -- the early forward is dropped -- equals the option off
        on (z2, c2), not the forward of (z1, c1),
    (c) the caller rewrites its critic-step inputs right after issuing the critic step (on the same stream): the early
        forward read only the generator batch,
    (d) a new generator content version in between also drops it,
    and the early forward really ran on (z1, c1): the Dense layer's output left in the workspace is that of z1, not of the
    critic step's own latent."""
    from pr_disagg_radar_gan_amd import Engine
    from pr_disagg_radar_gan_amd.trainer import synthetic_batch_device
    B = 5
    eng = Engine(ndomain=16, max_batch=B)
    try:
        if bf16:
            eng.set_option("bf16", 1)
        g, d = _weights(16, 11)
        gs, ds = eng.to_slab(g), eng.to_slab(d)
        x, c, z = synthetic_batch_device(B, 16, 1, eng.device)
        _, c1, z1 = synthetic_batch_device(B, 16, 2, eng.device)
        _, c2, z2 = synthetic_batch_device(B, 16, 3, eng.device)
        ver = dict(gen_version=77, critic_version=78)

        def step(ahead, gz, gc, rewrite=False, gen_version=77):
            eng.set_option("gen_fwd_ahead", ahead)
            xx, cc, zz = x.clone(), c.clone(), z.clone()
            dg = eng.critic_grad(ds, gs, xx, cc, zz, 9, gen_batch=(z1, c1), **ver).clone()
            if rewrite:
                xx.fill_(0.5); cc.fill_(2.0); zz.fill_(-1.0)
            gg = eng.gen_grad(ds, gs, gz, gc, 10, gen_version=gen_version, critic_version=78).clone()
            torch.cuda.synchronize()
            return dg, gg

        ref1 = step(0, z1, c1)
        ref2 = step(0, z2, c2)
        assert not torch.equal(ref1[1], ref2[1])
        for got, want in ((step(1, z1, c1), ref1), (step(1, z2, c2), ref2), (step(1, z1, c1, rewrite=True), ref1)):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        got = step(1, z1, c1, gen_version=79)                       # (the forms are rebuilt from the same weights)
        assert torch.equal(got[0], ref1[0]) and torch.equal(got[1], ref1[1])
        # the workspace after a critic step told (z1, c1): h0 = Dense(z1, c1), which the generator forward of z1 also leaves
        eng.set_option("gen_fwd_ahead", 1)
        eng.critic_grad(ds, gs, x, c, z, 9, gen_batch=(z1, c1), **ver)
        shape = (B, 3 * 2 * 2 * 256)                               # Dense output [B, 3 x 2 x 2 x 256] at ndomain 16
        h0_ahead = eng.debug_activation(0, shape).clone()
        eng.gen_forward(gs, z1, c1, gen_version=77)
        h0_z1 = eng.debug_activation(0, shape).clone()
        eng.gen_forward(gs, z, c, gen_version=77)
        h0_z = eng.debug_activation(0, shape).clone()
        assert torch.equal(h0_ahead, h0_z1) and not torch.equal(h0_ahead, h0_z)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gloo_rehearsal_with_the_forward_ahead(tmp_path):
    """Two ranks on cuda:0 over gloo (bench.py --single-device): the data-parallel schedule with the option on and off writes
    byte-identical outputs."""
    outs = []
    for opt in ([], ["--opt", "gen_fwd_ahead=0"]):
        out = tmp_path / ("on" if not opt else "off")
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--single-device", "--backend", "gloo", "--steps", "2",
               "--warmup", "1", "--batch", "8", "--n-critic", "2", "--dump-outputs", str(out)] + opt
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(out)
    names = sorted(os.listdir(outs[0]))
    assert names and names == sorted(os.listdir(outs[1]))
    for n in names:
        assert (outs[0] / n).read_bytes() == (outs[1] / n).read_bytes(), n
