"""Plain numpy restatement of the optimizer update (k_adam / rdgan_adam): Keras optimizer_v2 Adam with beta_1 = 0,

    lr_t = lr sqrt(1 - beta2^t)        v' = beta2 v + (1 - beta2) (s g)^2        p' = p - lr_t s g / (sqrt(v') + eps)

in fp64 (adam_f64, what the GPU tests compare with) and in float32 with one rounding per operation (adam_f32, which says how
far an honest fp32 evaluation is from the fp64 one), the input family both test files draw from, the tolerances of the GPU
tests and the comparison they all go through (check_update).  Test infrastructure; numpy only.

lr, beta2, eps and grad_scale are rounded to float32 first in both functions: those are the values the C ABI receives.
"""
import numpy as np

# Worst relative deviation of adam_f32 from adam_f64 over family(4099, 0), t in T_CASES, beta2 = 0.9 (lr 1e-4, eps 1e-7,
# grad_scale 1): measured 2.39999e-7 for the step and 1.23720e-7 for v'.  tests/test_adam_host.py re-measures both and fails if
# either constant is exceeded.  (Roundings counted by hand: at most ~4 ulp on the step, ~2.5 ulp on v', i.e. 5e-7 and 3e-7.)
F32_DEV_DELTA = 2.4e-7
F32_DEV_V = 1.24e-7

T_CASES = (1, 2, 7, 1000, 10 ** 6)
MUTATIONS = ("eps_inside_sqrt", "unscaled_v", "t_minus_1", "skip_tail")


def _f32_args(lr, beta2, eps, grad_scale):
    return tuple(np.float32(x) for x in (lr, beta2, eps, grad_scale))


def adam_f64(p, g, v, t, lr=1e-4, beta2=0.9, eps=1e-7, grad_scale=1.0, eps_inside_sqrt=False):
    """(delta, v') in fp64 with delta = p - p'.  eps_inside_sqrt: the misplaced form sqrt(v' + eps^2), for the power check of
    the input family only."""
    lr, beta2, eps, s = (float(x) for x in _f32_args(lr, beta2, eps, grad_scale))
    p, g, v = (np.asarray(a, np.float64) for a in (p, g, v))
    lr_t = lr * np.sqrt(1.0 - beta2 ** float(t))
    sg = s * g
    v1 = beta2 * v + (1.0 - beta2) * (sg * sg)
    den = np.sqrt(v1 + eps * eps) if eps_inside_sqrt else np.sqrt(v1) + eps
    p1 = p - lr_t * sg / den
    return p - p1, v1


def adam_f32(p, g, v, t, lr=1e-4, beta2=0.9, eps=1e-7, grad_scale=1.0, mutation=None):
    """The same statement in float32, every operation rounded once.  Returns (delta, v') as float32, delta = p - p'.
    mutation: one of MUTATIONS -- a deliberately wrong variant, for the check that the comparison has the power to see it."""
    assert mutation is None or mutation in MUTATIONS, mutation
    f = np.float32
    lr, beta2, eps, s = _f32_args(lr, beta2, eps, grad_scale)
    p, g, v = (np.asarray(a, f) for a in (p, g, v))
    tt = t - 1 if mutation == "t_minus_1" else t
    with np.errstate(under="ignore"):
        lr_t = f(lr * np.sqrt(f(f(1) - np.power(beta2, f(tt)))))
        sg = s * g
        sgv = g if mutation == "unscaled_v" else sg
        v1 = beta2 * v + (f(1) - beta2) * (sgv * sgv)
        den = np.sqrt(v1 + eps * eps) if mutation == "eps_inside_sqrt" else np.sqrt(v1) + eps
        p1 = p - lr_t * sg / den
    assert p1.dtype == f and v1.dtype == f
    if mutation == "skip_tail" and p.size % 4:
        k = p.size - p.size % 4
        p1[k:] = p[k:]
        v1[k:] = v[k:]
    return p - p1, v1


def family(n, seed=0):
    """(g, v0, blocks): float32 inputs of n elements.  |g| log-uniform over 1e-12 ... 1e+2 with random signs; v0 exactly 0 for
    about 30 % of the elements and g^2 10^U(-2,2) otherwise.  From n = 1024 on, three blocks are laid over that (slices in
    `blocks`): "zero_zero" g = 0 and v0 = 0; "zero_v" g = 0 and v0 > 0; "below_eps" |g| in 1e-12 ... 1e-7 with v0 = 0, so that
    sqrt(v') <= sqrt(0.1) 1e-7 < eps = 1e-7 (a misplaced eps shows most where sqrt(v') approaches eps, and not at all at 0).  The last n % 4 elements are never inside a block (they have g != 0)."""
    r = np.random.default_rng([int(seed), int(n)])
    g = (10.0 ** r.uniform(-12, 2, n)) * r.choice([-1.0, 1.0], n)
    v0 = np.where(r.random(n) < 0.3, 0.0, g * g * 10.0 ** r.uniform(-2, 2, n))
    blocks = {}
    if n >= 1024:
        blocks = {"zero_zero": slice(128, 192), "zero_v": slice(320, 384), "below_eps": slice(512, 768)}
        g[blocks["zero_zero"]] = 0.0
        v0[blocks["zero_zero"]] = 0.0
        g[blocks["zero_v"]] = 0.0
        v0[blocks["zero_v"]] = 10.0 ** r.uniform(-24, 4, 64)
        k = blocks["below_eps"]
        g[k] = (10.0 ** r.uniform(-12, -7, 256)) * r.choice([-1.0, 1.0], 256)
        v0[k] = 0.0
    return g.astype(np.float32), v0.astype(np.float32), blocks


def tol_delta(beta2, t):
    """Relative tolerance of a GPU step against adam_f64: 4 x what adam_f32 itself deviates (margin for FMA contraction and
    the GPU's division and square root, a few ulp) + the cancellation in rdgan_adam's fp32 `1 - powf(beta2, t)`: beta2^t
    carries a rounding error of up to 2^-25 beta2^t .. 2^-24 beta2^t, which the subtraction leaves as a relative
    2^-24 beta2^t / (1 - beta2^t) (the square root behind it halves that; kept as margin for powf's own last bit)."""
    b = float(np.float32(beta2)) ** float(t)
    return 4.0 * F32_DEV_DELTA + 2.0 ** -24 * b / (1.0 - b)


TOL_V = 4.0 * F32_DEV_V          # relative, for v'
ATOL_V = 2.0 ** -126             # absolute, for squares that are subnormal in fp32


def deviations(delta, v1, g, v0, t, lr=1e-4, beta2=0.9, eps=1e-7, grad_scale=1.0):
    """Worst relative deviation of (delta, v1) from adam_f64 as (dev_delta, dev_v, i_delta, i_v) with the elements where they
    occur.  An element whose exact value is 0 counts as 0 when matched exactly and as inf otherwise; v' below ATOL_V apart is
    no deviation."""
    d64, v64 = adam_f64(np.zeros(np.shape(g)), g, v0, t, lr, beta2, eps, grad_scale)
    out = []
    for got, want, atol in ((delta, d64, 0.0), (v1, v64, ATOL_V)):
        got = np.asarray(got, np.float64)
        err = np.abs(got - want)
        err = np.where(err <= atol, 0.0, err)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(err == 0, 0.0, err / np.abs(want))
        rel = np.where(np.isfinite(got), rel, np.inf)
        i = int(np.argmax(rel)) if rel.size else 0
        out.append((float(rel[i]) if rel.size else 0.0, i))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def check_update(p1, v1, p0, g, v0, t, lr=1e-4, beta2=0.9, eps=1e-7, grad_scale=1.0, what=""):
    """THE comparison of the GPU tests: parameters p1 and second moments v1 after one update of (p0, g, v0), elementwise
    against adam_f64:

        |p1 - (p0 - delta64)| <= ulp(p0) + tol_delta |delta64|          (ulp(0) = 0: with p0 = 0, p1 is the negated step)
        |v1 - v64|            <= TOL_V v64 + 2^-126

    and everything finite.  Returns (worst |step error| / |delta64| where p0 = 0, worst relative v' deviation) and raises
    AssertionError naming the worst element otherwise."""
    p1, v1, p0, g, v0 = (np.asarray(a) for a in (p1, v1, p0, g, v0))
    assert p1.shape == v1.shape == p0.shape == g.shape == v0.shape, (p1.shape, v1.shape, p0.shape, g.shape, v0.shape)
    d64, v64 = adam_f64(p0, g, v0, t, lr, beta2, eps, grad_scale)
    hyper = f"t {t} lr {lr} beta2 {beta2} eps {eps} grad_scale {grad_scale}"
    assert np.isfinite(p1).all() and np.isfinite(v1).all(), f"{what}: non-finite output ({hyper})"
    tol = tol_delta(beta2, t)
    ulp = np.where(p0 == 0, 0.0, np.spacing(np.abs(p0.astype(np.float32))).astype(np.float64))
    errp = np.abs(p1.astype(np.float64) - (p0.astype(np.float64) - d64))
    bad = errp - (ulp + tol * np.abs(d64))
    i = int(np.argmax(bad))
    assert bad[i] <= 0, (f"{what}: parameter {i} of {p1.size} is {p1[i]!r}, fp64 Adam gives {p0[i] - d64[i]!r} (p0 {p0[i]!r}, g {g[i]!r}, "
                         f"v0 {v0[i]!r}, step {d64[i]!r}; {hyper}): off by {errp[i]:.3e}, allowed {ulp[i] + tol * abs(d64[i]):.3e}")
    errv = np.abs(v1.astype(np.float64) - v64)
    bad = errv - (TOL_V * v64 + ATOL_V)
    i = int(np.argmax(bad))
    assert bad[i] <= 0, (f"{what}: v[{i}] of {v1.size} is {v1[i]!r}, fp64 Adam gives {v64[i]!r} (g {g[i]!r}, v0 {v0[i]!r}; {hyper}): "
                         f"off by {errv[i]:.3e}, allowed {TOL_V * v64[i] + ATOL_V:.3e}")
    exact = p0 == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = np.where(exact & (d64 != 0), errp / np.abs(d64), 0.0)
        rv = np.where(errv <= ATOL_V, 0.0, errv / v64)
    return float(rd.max()) if rd.size else 0.0, float(rv.max()) if rv.size else 0.0


def shard_len(n, world, loss_slots=8):
    """`per` of WGANGPTrainer's sharded exchange, restated: `world` equal shards of a multiple of 4 floats that together
    cover the n parameters and the loss slots behind them"""
    return -(-(n + loss_slots) // (4 * world)) * 4
