"""CPU: the conditions the GPU tests of the optimizer update (tests/test_hip_adam.py) rely on -- tests/adam_np.py only.

Measured here (family(4099, 0), lr 1e-4, eps 1e-7, grad_scale 1, beta2 0.9, worst over t in 1, 2, 7, 1000, 10^6):
  adam_f32 against adam_f64, relative:   step 2.400e-7    v' 1.237e-7     (adam_np.F32_DEV_DELTA / F32_DEV_V = 2.4e-7 / 1.24e-7)
  the GPU tolerances built on them:      step 9.6e-7 + 2^-24 beta2^t / (1 - beta2^t)  (1.50e-6 at t = 1 ... 9.6e-7)    v' 4.96e-7
  eps inside the square root (fp64):     the step differs by up to 41.4 % (sqrt 2 - 1, where sqrt(v') = eps), 24.4 % in "below_eps"
"""
import numpy as np
import pytest

from tests import adam_np as A

N = 4099
GRID = [(t, b2, s, eps) for t in A.T_CASES for b2 in (0.9, 0.999) for s in (1.0, 0.5, 0.125) for eps in (1e-7, 1e-3)]


def test_family_has_the_regimes_the_gpu_tests_need():
    g, v0, bl = A.family(N)
    assert g.dtype == v0.dtype == np.float32 and g.shape == v0.shape == (N,)
    free = np.ones(N, bool)
    for s in bl.values():
        free[s] = False
    a = np.abs(g[free])
    assert a.min() >= 1e-12 * (1 - 1e-6) and a.max() <= 1e2 * (1 + 1e-6) and a.min() < 1e-11 and a.max() > 1e1
    assert (g[free] > 0).any() and (g[free] < 0).any()
    assert 0.25 < (v0[free] == 0).mean() < 0.35
    nz = free & (v0 != 0)
    ratio = v0[nz].astype(np.float64) / g[nz].astype(np.float64) ** 2
    assert ratio.min() >= 1e-2 * (1 - 1e-5) and ratio.max() <= 1e2 * (1 + 1e-5)
    assert not g[bl["zero_zero"]].any() and not v0[bl["zero_zero"]].any()
    assert not g[bl["zero_v"]].any() and (v0[bl["zero_v"]] > 0).all()
    _, v1 = A.adam_f64(np.zeros(N), g, v0, 1)
    assert (np.sqrt(v1[bl["below_eps"]]) < 1e-7).all() and (g[bl["below_eps"]] != 0).all()
    assert N % 4 == 3 and free[-3:].all() and (g[-3:] != 0).all()
    for n in (1, 2, 3, 4, 5, 7):
        gs, vs, bs = A.family(n)
        assert gs.shape == (n,) and not bs and (gs != 0).all()


def test_restatement_in_float32_stays_inside_the_gpu_tolerance():
    g, v0, _ = A.family(N)
    worst_d = worst_v = 0.0
    for t in A.T_CASES:
        d32, v32 = A.adam_f32(np.zeros(N, np.float32), g, v0, t)
        dd, dv, i, j = A.deviations(d32, v32, g, v0, t)
        print(f"adam_f32 against adam_f64 at t = {t}: step {dd:.3e} (element {i}), v' {dv:.3e} (element {j}); "
              f"GPU tolerance {A.tol_delta(0.9, t):.3e} / {A.TOL_V:.3e}")
        assert dd < A.tol_delta(0.9, t) and dv < A.TOL_V
        worst_d, worst_v = max(worst_d, dd), max(worst_v, dv)
    print(f"worst over t: step {worst_d:.4e} (recorded {A.F32_DEV_DELTA:.2e}), v' {worst_v:.4e} (recorded {A.F32_DEV_V:.2e})")
    # the GPU tolerances are 4 x the recorded figures: those must be what this machine measures, not less
    assert worst_d <= A.F32_DEV_DELTA and worst_v <= A.F32_DEV_V
    assert worst_d > 0.5 * A.F32_DEV_DELTA and worst_v > 0.5 * A.F32_DEV_V


@pytest.mark.parametrize("t,beta2,s,eps", GRID)
def test_restatement_passes_the_gpu_comparison_on_the_whole_grid(t, beta2, s, eps):
    """check_update -- the comparison every GPU test goes through -- accepts the honest float32 evaluation at every grid
    point, alone and composed with a parameter of ordinary size"""
    g, v0, _ = A.family(N)
    step, v32 = A.adam_f32(np.zeros(N, np.float32), g, v0, t, 1e-4, beta2, eps, s)      # from p0 = 0: the fp32 step itself
    for p0 in (np.zeros(N, np.float32), np.random.default_rng(1).standard_normal(N).astype(np.float32)):
        p1 = p0 - step                                                                   # one more fp32 rounding
        assert p1.dtype == np.float32
        A.check_update(p1, v32, p0, g, v0, t, 1e-4, beta2, eps, s, what="adam_f32")


def test_family_can_tell_where_eps_stands():
    """the power of the family, not of a kernel: eps inside the square root moves the fp64 step by more than 10 % somewhere"""
    g, v0, bl = A.family(N)
    for t in A.T_CASES:
        d, _ = A.adam_f64(np.zeros(N), g, v0, t)
        dm, _ = A.adam_f64(np.zeros(N), g, v0, t, eps_inside_sqrt=True)
        with np.errstate(invalid="ignore"):
            rel = np.where(d != 0, np.abs(dm - d) / np.abs(d), 0.0)
        i = int(np.argmax(rel))
        print(f"t = {t}: eps inside the square root moves the step by up to {rel[i]:.3%} (element {i}, g {g[i]!r}, v0 {v0[i]!r}); "
              f"in the below_eps block by up to {rel[bl['below_eps']].max():.3%}")
        assert rel[i] > 0.10 and rel[bl["below_eps"]].max() > 0.10


@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_each_mutation_of_the_restatement_fails_the_gpu_comparison(mutation):
    """A wrong update must not pass: each mutation of adam_f32 is refused by check_update at one grid point at least (and the
    unmutated restatement passes everywhere: the test above)."""
    g, v0, _ = A.family(N)
    p0 = np.zeros(N, np.float32)
    refused = []
    for t, beta2, s, eps in GRID:
        d32, v32 = A.adam_f32(p0, g, v0, t, 1e-4, beta2, eps, s, mutation=mutation)
        try:
            A.check_update(p0 - d32, v32, p0, g, v0, t, 1e-4, beta2, eps, s, what=mutation)
        except AssertionError as e:
            refused.append(((t, beta2, s, eps), str(e)))
    print(f"{mutation}: refused at {len(refused)} of {len(GRID)} grid points; first: {refused[0][1] if refused else None}")
    assert refused
    if mutation in ("eps_inside_sqrt", "skip_tail"):
        assert len(refused) == len(GRID)            # these are wrong at every t, beta2, grad_scale and eps
    if mutation == "skip_tail":                     # ... and at the small sizes, where the tail is all or most of the slab
        for n in (1, 2, 3, 5, 7, 1023, 1025):
            gs, vs, _ = A.family(n)
            z = np.zeros(n, np.float32)
            d32, v32 = A.adam_f32(z, gs, vs, 7, mutation=mutation)
            with pytest.raises(AssertionError):
                A.check_update(z - d32, v32, z, gs, vs, 7)


def test_shards_start_on_16_bytes_and_cover_the_slab():
    """WGANGPTrainer's sharded exchange: per = ceil((n + LOSS_SLOTS) / (4 world)) 4 -- every shard starts at a multiple of 4
    floats (k_adam reads 16 bytes at a time from the view's first element) and the shards cover parameters and loss slots"""
    from pr_disagg_radar_gan_amd import trainer as T
    from pr_disagg_radar_gan_amd import weights as W
    from tests.fake_engine import FakeEngine
    slabs = {nd: (W.param_count(W.gen_param_shapes(nd)), W.param_count(W.critic_param_shapes(nd))) for nd in (8, 16)}
    for world in (1, 2, 3, 8):
        for n in (1, 5) + slabs[8] + slabs[16]:
            per = A.shard_len(n, world, T.LOSS_SLOTS)
            assert per % 4 == 0 and per * world >= n + T.LOSS_SLOTS > (per - 4) * world
            for r in range(world):
                assert (r * per) % 4 == 0            # _update hands the kernel pbuf[lo:hi], gsh[:hi - lo], vbuf[lo:hi], lo = r per
            assert sum(max(min((r + 1) * per, n) - r * per, 0) for r in range(world)) == n
    # the restated formula is the trainer's (nd 8: the constructor only lays out buffers)
    rng = np.random.default_rng(0)
    g, d = W.init_generator(rng, 8), W.init_critic(rng, 8)
    for world in (2, 3, 8):
        tr = T.WGANGPTrainer(FakeEngine(8), g, d, world_size=world, rank=world - 1, exchange="sharded")
        for which, n in (("g", slabs[8][0]), ("d", slabs[8][1])):
            assert tr._pad[which] == (n, A.shard_len(n, world, T.LOSS_SLOTS), A.shard_len(n, world, T.LOSS_SLOTS) * world)
