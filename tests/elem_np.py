"""Plain numpy restatements of the step's elementwise / reduction kernels (csrc/rdgan_elem.hip.h), one per op entry
(rdgan_op_softmax_tail ... rdgan_op_diff_combine), written from the formula in the kernel's header comment and the Keras line it
cites (T = gan_train_cwgangp_pixelnorm.py):

    each in fp64 (what the GPU tests compare with) and in float32 (`dtype=np.float32`: every operation rounded once, sums taken
    as a 256-thread workgroup would take them -- see sum32 -- which says how far an honest fp32 evaluation is from the fp64 one),
    the seeded input families of both test files, the limits of the GPU tests and the one comparison they all go through
    (compare).  Test infrastructure; numpy only.

LIMITS[family] = 4 x the deviation of the float32 restatement from the fp64 one as measured on the CPU by
tests/test_elem_host.py (the measured value stands beside each constant; that file re-measures and fails when a constant leaves
[2 x, 8 x] of it).  The margin covers a different but equally valid fp32 order of the same sums and the GPU's expf / division /
square root.  Exact quantities -- zeros, flags, padded channels -- are compared exactly and have no limit.
"""
import numpy as np

NH = 24                     # hours (RDGAN_NHOURS)
GP_WEIGHT = 10.0            # T:392
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------------------------------------
def deviation(got, want, scale):
    """max |got - want| / scale, elementwise with `scale` broadcast; a non-finite `got` where `want` is finite counts as inf, and
    where scale == 0 the values must be equal (0 when they are, inf otherwise)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    scale = np.broadcast_to(np.asarray(scale, F64), want.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / scale)
    r = np.where(np.isfinite(got) | ~np.isfinite(want), r, np.inf)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def compare(got, want, scale, limit, what=""):
    """THE comparison of the GPU tests: deviation(got, want, scale) <= limit.  Returns the deviation."""
    d = deviation(got, want, scale)
    assert d <= limit, f"{what}: deviation {d:.3e} exceeds the limit {limit:.3e} ({d / limit:.2f} x)"
    return d


def sum32(a, axis=-1, chains=256):
    """float32 sum along `axis` as a workgroup of `chains` threads takes it: element i goes to chain i % chains, every chain adds
    its elements in order, the chains are folded in order.  (One of the valid fp32 orders; numpy's own sum is another.)"""
    a = np.moveaxis(np.asarray(a, F32), axis, 0)
    n = a.shape[0]
    pad = (-n) % chains
    if pad:
        a = np.concatenate([a, np.zeros((pad,) + a.shape[1:], F32)], 0)
    a = a.reshape((-1, chains) + a.shape[1:])
    acc = np.zeros(a.shape[1:], F32)
    for k in range(a.shape[0]):
        acc = acc + a[k]
    out = np.zeros(a.shape[2:], F32)
    for c in range(min(chains, n)):
        out = out + acc[c]
    return out


def _sum(a, axis, dtype, chains=256):
    return np.sum(np.asarray(a, F64), axis=axis) if dtype is F64 else sum32(a, axis, chains)


def bf16_round(a):
    """float32 values rounded to nearest-even bfloat16, returned as float32"""
    u = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(a))


# ------------------------------------------------------------------------------------------------------------------------------
# softmax tails (T:345-350): logits = bias + the remaining tap sums, Softmax(axis = hours)
# ------------------------------------------------------------------------------------------------------------------------------
TAIL_FORMS = (0, 3, 9, 12)
TAIL_FAMILIES = ("flat", "rain", "ties", "offset", "border")
TAIL_MUTATIONS = ("no_max", "den_23_hours", "upper_hour_tap_dropped")


def tail_shape(form, B, H, W):
    return {0: (B, NH, H, W, 32), 3: (B, NH, 3, H, W), 9: (B, NH, 9, H, W), 12: (B, NH // 4, 6, 4, 4, 64)}[form]


def _shift(a, axis, s):
    """b[i] = a[i + s] along `axis`, zero outside"""
    out = np.zeros_like(a)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if s >= 0:
        src[axis], dst[axis] = slice(s, n), slice(0, n - s)
    else:
        src[axis], dst[axis] = slice(0, n + s), slice(-s, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _class_index(H=16, W=16):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return 2 * (y & 1) + (x & 1), (y >> 1) * 8 + (x >> 1)


def tail_logits(form, taps, bias, dtype=F64, mutation=None):
    """logits [B,24,H,W] from the tap-product buffer of `form` (layouts: include/rdgan.h, rdgan_op_softmax_tail); the terms are
    added one after the other in `dtype`, the bias first.  mutation "upper_hour_tap_dropped": the products of the hour above
    (kd = 2) are left out."""
    t = np.asarray(taps, dtype)
    up = mutation != "upper_hour_tap_dropped"
    terms = []
    if form == 0:
        for td in range(3):
            for th in range(3):
                for tw in range(3):
                    if td == 2 and not up:
                        continue
                    a = t[..., (td * 3 + th) * 3 + tw]
                    terms.append(_shift(_shift(_shift(a, 1, td - 1), 2, th - 1), 3, tw - 1))
    elif form == 3:
        for td in range(3 if up else 2):
            terms.append(_shift(t[:, :, td], 1, td - 1))
    elif form == 9:
        for td in range(3 if up else 2):
            for th in range(3):
                terms.append(_shift(_shift(t[:, :, td * 3 + th], 1, td - 1), 2, th - 1))
    elif form == 12:
        q, pos = _class_index()
        B = t.shape[0]
        tt = t[:, :, :, :, q, pos]                                # [B, item, tp, p, y, x]
        zero = np.zeros((B, 16, 16), dtype)
        for grp in ("below", "own", "above"):
            for p in range(4):
                planes = []
                for d in range(NH):
                    it, k = d >> 2, d & 3
                    if grp == "own":
                        planes.append(tt[:, it, k + 1, p])
                    elif grp == "below":
                        planes.append(tt[:, it - 1, 5, p] if k == 0 and it > 0 else zero)
                    else:
                        planes.append(tt[:, it + 1, 0, p] if k == 3 and it < NH // 4 - 1 and up else zero)
                terms.append(np.stack(planes, 1))
    else:
        raise ValueError(form)
    s = np.full(terms[0].shape, dtype(np.asarray(bias).ravel()[0]), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in terms:
            s = s + a
    return s


def softmax_hours(logits, dtype=F64, mutation=None):
    """Softmax(axis=1) (T:347): exp(l - max) / sum exp(l - max)"""
    l = np.asarray(logits, dtype)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        e = np.exp(l if mutation == "no_max" else l - l.max(1, keepdims=True))
        parts = e[:, :NH - 1] if mutation == "den_23_hours" else e
        den = np.zeros(e[:, 0].shape, dtype)
        for d in range(parts.shape[1]):
            den = den + parts[:, d]
        return (e / den[:, None]).astype(dtype)


def softmax_tail(form, taps, bias, dtype=F64, mutation=None):
    return softmax_hours(tail_logits(form, taps, bias, dtype, mutation), dtype, mutation)


def target_logits(family, B, H, W, rng):
    """the logits a family asks for, [B,24,H,W] fp64"""
    shp = (B, NH, H, W)
    col = (B, 1, H, W)
    if family == "flat":
        return 1e-3 * rng.uniform(-1, 1, shp)
    if family in ("rain", "border"):
        t = rng.uniform(-1, 1, shp)
        hours = rng.integers(0, NH, col) if family == "rain" else rng.choice([0, NH - 1], col)
        second = np.where(rng.random(col) < 0.5, rng.integers(0, NH, col), hours)        # one or two hours carry the day
        d = np.arange(NH).reshape(1, NH, 1, 1)
        return t + np.where((d == hours) | (d == second), rng.uniform(20, 80, shp), 0.0)
    if family == "ties":
        t = np.round(rng.uniform(-1, 1, shp) * 16) / 16
        k = rng.integers(2, 6, col)
        rank = np.argsort(np.argsort(rng.random(shp), 1), 1)
        return np.where(rank < k, 3.0, t)
    if family == "offset":
        return np.where(rng.random(col) < 0.5, 1e4, -1e4) + rng.uniform(-2, 2, shp)
    raise ValueError(family)


def tail_family(form, family, B, H, W, seed=0):
    """(taps, bias) float32 whose logits are the family's: every entry of the buffer random (so that a tap taken from the wrong
    place, or past a border, shows), the centre entry of each grid point then set so that the sum comes out at the target.
    "ties": all values multiples of 1/16, so the sums are exact and the maxima tie exactly.  "border": neighbours of size 5, the
    sharp hour is the first or the last."""
    rng = np.random.default_rng([int(seed), form, TAIL_FAMILIES.index(family), B, H, W])
    target = target_logits(family, B, H, W, rng)
    shp = tail_shape(form, B, H, W)
    mag = {"ties": 1.0, "border": 5.0}.get(family, 0.5)
    taps = rng.uniform(-mag, mag, shp)
    bias = np.array([0.25])
    if family == "ties":
        taps = np.round(taps * 16) / 16
    if form == 0:
        taps[..., 27:] = rng.uniform(-100, 100, shp[:-1] + (5,))       # columns 27..31 of P: never read
        centre = (Ellipsis, 13)
    elif form == 3:
        centre = (slice(None), slice(None), 1)
    elif form == 9:
        centre = (slice(None), slice(None), 4)
    else:
        centre = None
    taps = taps.astype(F32).astype(F64)
    if centre is not None:
        taps[centre] = 0.0
        taps[centre] = target - tail_logits(form, taps, bias)
    else:
        q, pos = _class_index()
        for d in range(NH):
            taps[:, d >> 2, (d & 3) + 1, 0, q, pos] = 0.0
        rest = tail_logits(form, taps, bias)
        for d in range(NH):
            taps[:, d >> 2, (d & 3) + 1, 0, q, pos] = target[:, d] - rest[:, d]
    return taps.astype(F32), bias.astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------
# softmax backward: dl = p * (g - sum_d p g)
# ------------------------------------------------------------------------------------------------------------------------------
BWD_MUTATIONS = ("dot_23_hours", "dot_unweighted")


def softmax_bwd(p, g, dtype=F64, mutation=None):
    p, g = np.asarray(p, dtype), np.asarray(g, dtype)
    w = np.full_like(p, dtype(1.0 / NH)) if mutation == "dot_unweighted" else p
    dot = np.zeros(p[:, 0].shape, dtype)
    for d in range(NH - 1 if mutation == "dot_23_hours" else NH):
        dot = dot + w[:, d] * g[:, d]
    return p * (g - dot[:, None])


def bwd_family(family, B, H, W, seed=0):
    """(p, g): p = the fp64 softmax of the family's logits rounded to float32; g of mixed sign, |g| log-uniform in 1e-6 .. 1e2"""
    rng = np.random.default_rng([int(seed), 77, TAIL_FAMILIES.index(family), B, H, W])
    p = softmax_hours(target_logits(family, B, H, W, rng)).astype(F32)
    g = (10.0 ** rng.uniform(-6, 2, p.shape) * rng.choice([-1.0, 1.0], p.shape)).astype(F32)
    return p, g


def bwd_scale(p, g):
    """per column: max_d |p_d| max_d |g_d| -- a flat column must not hide a sharp one"""
    return (np.abs(np.asarray(p, F64)).max(1, keepdims=True) * np.abs(np.asarray(g, F64)).max(1, keepdims=True))


# ------------------------------------------------------------------------------------------------------------------------------
# gradient-penalty norm (T:238-241): n = ||g0||, gp = n - 1, cin_hat[..., 0] = (10 / B) 2 (n - 1) / n g0, other channels 0
# ------------------------------------------------------------------------------------------------------------------------------
GP_NORMS = {"1e-3": 1e-3, "1-2^-20": 1 - 2.0 ** -20, "1": 1.0, "1+1e-6": 1 + 1e-6, "7": 7.0, "1e3": 1e3}
GP_MUTATIONS = ("coef_without_division", "short_last_slice_skipped", "weight_not_over_batch")


def gp_norm(g0, dtype=F64, mutation=None, S=1):
    """(gp [B], r0 [B, per], coef [B], n [B]) from g0 [B, per].  S: slices per sample of the sum of squares (the mutation
    "short_last_slice_skipped" leaves the last, short one out)."""
    g = np.asarray(g0, dtype)
    B, per = g.shape
    sq = g * g
    if mutation == "short_last_slice_skipped" and S > 1:
        sq = sq[:, :min(per, (S - 1) * -(-per // S))]
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.sqrt(_sum(sq, 1, dtype))
        one = dtype(1)
        coef = (dtype(GP_WEIGHT) / dtype(1 if mutation == "weight_not_over_batch" else B)) * dtype(2) * (n - one)
        if mutation != "coef_without_division":
            coef = coef / n
        return n - one, coef[:, None] * g, coef, n


def gp_family(B, per, norm, seed=0, zero_sample=None):
    """g0 [B, per] float32 with ||g0[b]|| = GP_NORMS[norm] up to the rounding of the elements; zero_sample: that sample all zero"""
    rng = np.random.default_rng([int(seed), 31, B, per, list(GP_NORMS).index(norm)])
    g = rng.standard_normal((B, per)) * 10.0 ** rng.uniform(-2, 0, (B, per))
    g *= GP_NORMS[norm] / np.sqrt((g * g).sum(1, keepdims=True))
    if zero_sample is not None:
        g[zero_sample] = 0.0
    return g.astype(F32)


def gp_scales(g0):
    """(scale of gp [B], scale of cin_hat[..., 0] [B, 1]).  gp = n - 1 is a float32 of magnitude up to max(n, 1), so it is
    compared against that.  r0 is compared against max |g0| |coef|, with a floor for coef of what ONE ulp of n does to it:
    coef = (20 / B) (n - 1) / n and ulp(n) / n <= 2^-23, hence (20 / B) 2^-23."""
    g = np.asarray(g0, F64)
    B = g.shape[0]
    _, _, coef, n = gp_norm(g)
    coef = np.where(np.isfinite(coef), coef, 0.0)
    return np.maximum(n, 1.0), (np.abs(g).max(1) * (np.abs(coef) + 2 * GP_WEIGHT / B * 2.0 ** -23))[:, None]


# ------------------------------------------------------------------------------------------------------------------------------
# loss tails (T:215-216, T:388-392, T:408)
# ------------------------------------------------------------------------------------------------------------------------------
LOSS_MUTATIONS = ("real_third_plus", "penalty_unweighted", "mean_over_B_minus_1")


def loss_tail(mode, v, gp, B, dtype=F64, mutation=None):
    """out[0:4].  mode 0: (total, mean(-v_real), mean(v_fake), mean(gp^2)), total = the three with weight 1, 1, 10;
    mode 1: (mean(-v), 0, 0, 0)"""
    v = np.asarray(v, dtype)
    nb = dtype(B - 1 if mutation == "mean_over_B_minus_1" and B > 1 else B)
    if mode == 1:
        return np.array([_sum(-v[:B], 0, dtype) / nb, 0, 0, 0], dtype)
    gp = np.asarray(gp, dtype)
    a = _sum(v[:B] if mutation == "real_third_plus" else -v[:B], 0, dtype) / nb
    f = _sum(v[B:2 * B], 0, dtype) / nb
    g = _sum(gp[:B] * gp[:B], 0, dtype) / nb
    w = dtype(1.0 if mutation == "penalty_unweighted" else GP_WEIGHT)
    return np.array([a + f + w * g, a, f, g], dtype)


def loss_family(B, seed=0):
    """(v [2B], gp [B]) float32: critic values of mixed sign, |v| log-uniform in 1e-2 .. 1e4; gp = n - 1 with n in 1e-2 .. 30"""
    rng = np.random.default_rng([int(seed), 53, B])
    v = 10.0 ** rng.uniform(-2, 4, 2 * B) * rng.choice([-1.0, 1.0], 2 * B)
    gp = 10.0 ** rng.uniform(-2, 1.5, B) - 1.0
    return v.astype(F32), gp.astype(F32)


def loss_scale(mode, v, gp, B):
    """what each mean can be wrong by is a fraction of the mean of the MAGNITUDES it adds (the values cancel, the errors do not)"""
    v = np.abs(np.asarray(v, F64))
    if mode == 1:
        return np.array([v[:B].mean(), 0, 0, 0])
    a, f, g = v[:B].mean(), v[B:2 * B].mean(), (np.asarray(gp, F64)[:B] ** 2).mean()
    return np.array([a + f + GP_WEIGHT * g, a, f, g])


# ------------------------------------------------------------------------------------------------------------------------------
# column sums behind every bias gradient: out[c] = sum_r src[r][c]
# ------------------------------------------------------------------------------------------------------------------------------
COLSUM_MUTATIONS = ("last_row_skipped", "rows_to_multiple_of_32")


def colsum(src, dtype=F64, mutation=None):
    a = np.asarray(src, dtype)
    if mutation == "last_row_skipped" and a.shape[0] > 1:
        a = a[:-1]
    if mutation == "rows_to_multiple_of_32" and a.shape[0] > 32:
        a = a[:a.shape[0] // 32 * 32]
    return _sum(a, 0, dtype, chains=64)


def colsum_family(rows, C, seed=0, bf16=False):
    """[rows][C] float32 with mean 1 and spread 1e-3: where an fp32 running sum drifts.  bf16: spread 0.05 and the values rounded
    to bf16 (a spread of 1e-3 is below bf16's step of 2^-7 at 1: every value would be exactly 1).  The values lie in 0.5 .. 2 and
    are multiples of 2^-8, so any partial sum of up to 40 000 of them is a multiple of 2^-8 below 2^17: 25 bits at the most, and
    24 as long as the sum stays below 2^16 = 65 536 (it is about 40 000) -- every fp32 addition is exact and the limit is 0.
    colsum_family asserts that bound."""
    rng = np.random.default_rng([int(seed), 11, rows, C])
    a = (1.0 + (0.05 if bf16 else 1e-3) * rng.standard_normal((rows, C))).astype(F32)
    if bf16:
        a = bf16_round(a)
        assert a.min() >= 0.5 and a.max() < 2.0 and np.abs(a.astype(F64)).sum(0).max() < 2.0 ** 16, "bf16 sums no longer exact in fp32"
    return a


def colsum_scale(src):
    return np.abs(np.asarray(src, F64)).sum(0)


# ------------------------------------------------------------------------------------------------------------------------------
# hour differences of the shared-centre form and their adjoint
# ------------------------------------------------------------------------------------------------------------------------------
DIFF_MUTATIONS = ("last_plane_dropped", "sign_flipped")


def _store(a, dtype, bf16):
    a = np.asarray(a, dtype)
    return bf16_round(a) if (bf16 and dtype is F32) else a


def diff_d(x, dtype=F64, mutation=None, bf16=False):
    """E[b][j] = x[b][j] - x[b][j-1], j = 0..D, x zero outside [0, D); x [B, D, P]"""
    x = np.asarray(x, dtype)
    z = np.zeros_like(x[:, :1])
    hi, lo = np.concatenate([x, z], 1), np.concatenate([z, x], 1)
    if mutation == "last_plane_dropped":
        hi = hi.copy(); lo = lo.copy(); lo[:, -1] = 0
    return _store(lo - hi if mutation == "sign_flipped" else hi - lo, dtype, bf16)


def combine_dx(dx, dE, dtype=F64, mutation=None, bf16=False):
    """dx[b][d] + (dE[b][d] - dE[b][d+1]): the adjoint of diff_d added to dx; dE [B, D + 1, P]"""
    dx, dE = np.asarray(dx, dtype), np.asarray(dE, dtype)
    e1 = dE[:, 1:]
    if mutation == "last_plane_dropped":
        e1 = e1.copy(); e1[:, -1] = 0
    t = e1 - dE[:, :-1] if mutation == "sign_flipped" else dE[:, :-1] - e1
    return _store(dx + t, dtype, bf16)


def diff_family(B, D, P, seed=0, bf16=False):
    """(x [B,D,P], dx [B,D,P], dE [B,D+1,P]) float32 of mixed sign and magnitudes 1e-3 .. 1e1"""
    rng = np.random.default_rng([int(seed), 91, B, D, P])
    mk = lambda shp: (10.0 ** rng.uniform(-3, 1, shp) * rng.choice([-1.0, 1.0], shp)).astype(F32)
    out = mk((B, D, P)), mk((B, D, P)), mk((B, D + 1, P))
    return tuple(bf16_round(a) for a in out) if bf16 else out


def diff_scale(x):
    """largest operand of each difference"""
    x = np.abs(np.asarray(x, F64))
    z = np.zeros_like(x[:, :1])
    return np.maximum(np.concatenate([x, z], 1), np.concatenate([z, x], 1))


def combine_scale(dx, dE):
    dx, dE = np.abs(np.asarray(dx, F64)), np.abs(np.asarray(dE, F64))
    return np.maximum(dx, np.maximum(dE[:, :-1], dE[:, 1:]))


# ------------------------------------------------------------------------------------------------------------------------------
# limits of the GPU tests: 4 x the measured deviation of the float32 restatement (tests/test_elem_host.py prints and checks them)
# ------------------------------------------------------------------------------------------------------------------------------
# ------------------------------------------------------------------------------------------------------------------------------
# the critic's Dense layer (T:303-304), the top of its input-gradient chain and its weight gradient (T:388-392, T:452-454)
# ------------------------------------------------------------------------------------------------------------------------------
DENSE_MUTATIONS = ("bias_dropped", "real_third_plus", "gate_without_keep_scale", "last_slice_skipped")
LRELU_ALPHA = 0.2
# (NB, B, mode): the 3B batch real | fake | interpolated of a critic step, or B samples of a generator step
DENSE_CASES = [(1, 1, 1), (3, 1, 0), (15, 5, 0), (33, 11, 0), (33, 33, 1)]
DENSE_F = (256, 4096, 257 * 4)
DENSE_SLICES = (1, 2, 16)


def dense_dv(NB, B, mode, dtype=F64, mutation=None):
    """d loss / d v per sample: real -1/B, fake +1/B, interpolated 1 (critic step); -1/B (generator step)"""
    b = np.arange(NB)
    inv = dtype(1) / dtype(B)
    if mode == 1:
        return np.full(NB, -inv, dtype)
    real = inv if mutation == "real_third_plus" else -inv
    return np.where(b < B, real, np.where(b < 2 * B, inv, dtype(1))).astype(dtype)


def dense_gate(h4, mask, dtype=F64, mutation=None):
    """LeakyReLU' from the stored output x the dropout keep-scale mask (0 or 1/0.75; None: dropout off)"""
    h = np.asarray(h4, dtype)
    g = np.where(h > 0, dtype(1), dtype(LRELU_ALPHA))
    if mask is not None:
        keep = np.asarray(mask) != 0
        g = np.where(keep, g if mutation == "gate_without_keep_scale" else g * (dtype(1) / dtype(0.75)), dtype(0))
    return g.astype(dtype)


def dense_fwd(h4, w, bias, dtype=F64, mutation=None):
    h, w = np.asarray(h4, dtype), np.asarray(w, dtype)
    s = _sum(h * w[None, :], 1, dtype)
    return s if mutation == "bias_dropped" else s + dtype(np.asarray(bias).ravel()[0])


def dense_top_bwd(h4, w, mask, B, mode, dtype=F64, mutation=None, bf16=False):
    g = dense_gate(h4, mask, dtype, mutation)
    dv = dense_dv(g.shape[0], B, mode, dtype, mutation)
    return _store(g * np.asarray(w, dtype)[None, :] * dv[:, None], dtype, bf16)


def dense_wgrad(buf, B, dtype=F64, mutation=None, slices=1):
    a = np.asarray(buf, dtype)
    NB = a.shape[0]
    a = a * dense_dv(NB, B, 0, dtype, mutation)[:, None]
    if mutation == "last_slice_skipped" and slices > 1:
        a = a[:min(NB, (slices - 1) * -(-NB // slices))]
    return _sum(a, 0, dtype, chains=32)


def dense_family(NB, F, mask=None, seed=0, bf16=False):
    """(h4 [NB, F], w [F], bias [1]) float32: h4 = LeakyReLU of a normal pre-activation (so negative entries), times `mask`
    (0 or 1/0.75) when given, stored as the step stores it: a DROPPED element as +0.0, a kept exact zero as -0.0.  Without a mask
    every 7th element is an exact +0.0 all the same (dropout off: it then reads as LeakyReLU' = 0.2)."""
    rng = np.random.default_rng([int(seed), 23, NB, F])
    pre = rng.standard_normal((NB, F)) * 10.0 ** rng.uniform(-2, 1, (NB, F))
    h = np.where(pre > 0, pre, LRELU_ALPHA * pre).astype(F32)
    if mask is not None:
        m = np.asarray(mask, F32).reshape(NB, F)
        y = h * m
        h = np.where(m != 0, np.where(y == 0, F32(-0.0), y), F32(0.0)).astype(F32)
    else:
        h.reshape(-1)[::7] = 0.0
    w = (rng.standard_normal(F) / np.sqrt(F)).astype(F32)
    return (bf16_round(h) if bf16 else h), w, np.array([0.37], F32)


def dense_fwd_scale(h4, w, bias):
    return (np.abs(np.asarray(h4, F64)) * np.abs(np.asarray(w, F64))[None, :]).sum(1) + abs(float(np.asarray(bias).ravel()[0]))


def dense_wgrad_scale(buf, B):
    return (np.abs(np.asarray(buf, F64)) * np.abs(dense_dv(np.shape(buf)[0], B, 0))[:, None]).sum(0)


# ------------------------------------------------------------------------------------------------------------------------------
# weight forms of a generator block as matrices M [forms][27] of -1 / 0 / 1: forms = M W, adjoint = M^T
# ------------------------------------------------------------------------------------------------------------------------------
FORMS_CC = (64 * 64, 256 * 128)
FORMS_MUTATIONS = ("centre_tap_twice", "first_group_sign")
_AXIS = {(0, 0): (1, 0, 0), (0, 1): (0, 1, 1), (1, 0): (1, 1, 0), (1, 1): (0, 0, 1)}     # (parity p, tap a) -> taps summed on an axis


def forms_matrix(which, mutation=None):
    """which = 0, collapsed: row phase(pd,ph,pw) * 8 + tap(ad,ah,aw); per axis p = 0: (W0 | W1 + W2), p = 1: (W0 + W1 | W2).
    which = 1, shared centre: row g * 16 + (ph * 2 + th) * 4 + (pw * 2 + tw); along d the groups -W0, W0 + W1 + W2, W2."""
    ax = dict(_AXIS)
    if mutation == "centre_tap_twice":
        ax[(0, 0)] = (1, 1, 0)
    dgrp = [(1 if mutation == "first_group_sign" else -1, 0, 0), (1, 1, 1), (0, 0, 1)]
    rows = []
    if which == 0:
        for ph in range(8):
            for tp in range(8):
                c = [ax[((ph >> s) & 1, (tp >> s) & 1)] for s in (2, 1, 0)]
                rows.append([c[0][k // 9] * c[1][(k // 3) % 3] * c[2][k % 3] for k in range(27)])
    else:
        for g in range(3):
            for a in range(4):
                for b in range(4):
                    ca, cb = ax[(a >> 1, a & 1)], ax[(b >> 1, b & 1)]
                    rows.append([dgrp[g][k // 9] * ca[(k // 3) % 3] * cb[k % 3] for k in range(27)])
    return np.array(rows, np.int8)


def forms_apply(M, W, dtype=F64):
    """out[u] = sum_k M[u][k] W[k], the terms added in the order of k in `dtype`"""
    W = np.asarray(W, dtype)
    out = np.zeros((M.shape[0],) + W.shape[1:], dtype)
    for k in range(M.shape[1]):
        out = out + M[:, k].astype(dtype)[:, None] * W[k][None, :]
    return out


def forms_scale(M, W):
    return np.abs(M).astype(F64) @ np.abs(np.asarray(W, F64))


def forms_family(rows, CC, seed=0):
    """[rows][CC] float32 of mixed sign, magnitudes 1e-3 .. 1"""
    rng = np.random.default_rng([int(seed), 67, rows, CC])
    return (10.0 ** rng.uniform(-3, 0, (rows, CC)) * rng.choice([-1.0, 1.0], (rows, CC))).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------------
# critic input (T:275-282, T:221-224): (sample | nc condition channels | zeros) per voxel; x_hat = alpha real + (1 - alpha) fake
# ------------------------------------------------------------------------------------------------------------------------------
CIN_MUTATIONS = ("alpha_swapped", "alpha_of_sample_0")
CIN_CASES = [(B, HW, nc) for B in (1, 5) for HW in (64, 400) for nc in (1, 2, 3)]
CIN_D = 24


def critic_input(real, fake, cond, alpha, CP, mode, dtype=F64, mutation=None):
    """real, fake [B, D, HW], cond [B, HW, nc], alpha [B] -> [B or 3B, D, HW, CP]"""
    cond = np.asarray(cond, dtype)
    B, HW, nc = cond.shape

    def put(x):
        x = np.asarray(x, dtype)
        out = np.zeros(x.shape + (CP,), dtype)
        out[..., 0] = x
        out[..., 1:1 + nc] = cond[:, None, :, :]
        return out
    if mode == 1:
        return put(fake)
    if mode == 2:
        return put(real)
    a = np.asarray(alpha, dtype)
    if mutation == "alpha_of_sample_0":
        a = np.full_like(a, a[0])
    a = a[:, None, None]
    r, f = np.asarray(real, dtype), np.asarray(fake, dtype)
    if mutation == "alpha_swapped":
        r, f = f, r
    return np.concatenate([put(real), put(fake), put(a * r + (dtype(1) - a) * f)], 0)


def cin_family(B, HW, nc, seed=0):
    rng = np.random.default_rng([int(seed), 41, B, HW, nc])
    mk = lambda shp: (10.0 ** rng.uniform(-3, 1, shp) * rng.choice([-1.0, 1.0], shp)).astype(F32)
    return mk((B, CIN_D, HW)), mk((B, CIN_D, HW)), mk((B, HW, nc))


def cin_scale(real, fake, cond, CP, mode):
    """the interpolated sample against max(|real|, |fake|); everything else is a copy: exact (scale 0)"""
    r, f = np.abs(np.asarray(real, F64)), np.abs(np.asarray(fake, F64))
    z = np.zeros(r.shape + (CP,))
    if mode != 0:
        return z
    hat = z.copy()
    hat[..., 0] = np.maximum(r, f)
    return np.concatenate([z, z, hat], 0)


# ------------------------------------------------------------------------------------------------------------------------------
# gradient wrt the generator's Dense pre-activation (T:326-328): (sum of the 8 children of the upsampled grid) x LeakyReLU'(h0)
# ------------------------------------------------------------------------------------------------------------------------------
LRELU_MUTATIONS = ("slope_from_gradient", "seven_children")
POOL_CASES = [(1, 3, 2, 2, 256), (3, 3, 1, 1, 256), (2, 2, 3, 5, 12)]
LRELU_CASES = [4, 3 * 2 * 2 * 256 * 3, 4 * 1000 + 4]


def lrelu_slope(h, dtype=F64):
    return np.where(np.asarray(h, dtype) > 0, dtype(1), dtype(LRELU_ALPHA)).astype(dtype)


def lrelu_bwd(g, h, dtype=F64, mutation=None):
    g = np.asarray(g, dtype)
    return g * lrelu_slope(g if mutation == "slope_from_gradient" else h, dtype)


def pool_lrelu_bwd(gup, h0, dtype=F64, mutation=None):
    """gup [B, 2D, 2H, 2W, C], h0 [B, D, H, W, C]"""
    g = np.asarray(gup, dtype)
    s = np.zeros(np.shape(h0), dtype)
    for e in range(7 if mutation == "seven_children" else 8):
        s = s + g[:, (e >> 2)::2, ((e >> 1) & 1)::2, (e & 1)::2]
    return lrelu_bwd(s, h0, dtype, "slope_from_gradient" if mutation == "slope_from_gradient" else None)


def lrelu_family(shape_g, shape_h, seed=0, bf16=False):
    rng = np.random.default_rng([int(seed), 83] + list(shape_g))
    g = (10.0 ** rng.uniform(-4, 1, shape_g) * rng.choice([-1.0, 1.0], shape_g)).astype(F32)
    h = rng.standard_normal(shape_h).astype(F32)
    h.reshape(-1)[::5] = 0.0                    # exact zeros take the slope 0.2
    return (bf16_round(g), bf16_round(h)) if bf16 else (g, h)


def pool_scale(gup, h0):
    return pool_lrelu_bwd(np.abs(np.asarray(gup, F64)), h0)


# the cases of both test files.  Pictures of 8 x 8 and 16 x 16 always give a multiple of 64 columns, so forms 0 / 3 / 9 also run a
# 7 x 9 picture (189 columns at B = 3): the `live` mask and a last partial wave.  Form 12 is 16 x 16 by construction.
TAIL_CASES = [(f, B, H, W) for f in (0, 3, 9) for B, H, W in ((1, 8, 8), (3, 16, 16), (3, 7, 9))] + [(12, 1, 16, 16), (12, 3, 16, 16)]
BWD_CASES = [(1, 8, 8), (3, 16, 16), (3, 7, 9)]
# (B, per, CP, force_S).  force_S = 0: the step's choice (1 slice, or 24 at per = 98304).  Every `per` of the project is a multiple of
# 3, so 3 slices never leave a short one; 7 always do (per % 7 != 0), and per = 6143 (prime) is ragged for every S and every vector width.
GP_CASES = [(1, 6144, 2, 0), (5, 6144, 4, 7), (1, 6144, 4, 3), (5, 24 * 20 * 20, 2, 3), (1, 24 * 20 * 20, 4, 7), (1, 24 * 20 * 20, 2, 1),
            (1, 24 * 64 * 64, 4, 0), (5, 24 * 64 * 64, 2, 7), (1, 24 * 64 * 64, 4, 3), (1, 6143, 2, 3), (5, 6143, 4, 7), (1, 6143, 2, 1)]
LOSS_BATCHES = (1, 2, 255, 256, 257, 2048)
COLSUM_CASES = [(1, 64), (31, 128), (32, 256), (33, 100), (8 * 1024 + 5, 64), (40000, 64), (40000, 128), (8 * 1024 + 5, 256),
                (8 * 1024 + 5, 100), (33, 3072), (40000, 100), (8 * 1024 + 5, 3072), (40000, 3072), (40000, 256), (1, 3072)]
COLSUM_BF16_CASES = [(33, 64), (8 * 1024 + 5, 128), (40000, 256)]
DIFF_CASES = [(1, 6, 4 * 4 * 256 + 4), (3, 12, 8 * 8 * 128), (3, 6, 1028), (1, 12, 20)]

# measured deviation of the float32 restatement per family (worst over the family's cases)
MEASURED = {
    "tail/flat": 2.490e-08, "tail/rain": 2.378e-06, "tail/ties": 9.301e-08, "tail/offset": 5.247e-04, "tail/border": 3.773e-06,
    "bwd/flat": 8.925e-08, "bwd/rain": 6.200e-08, "bwd/ties": 1.243e-07, "bwd/offset": 8.317e-08, "bwd/border": 7.928e-08,
    "gp/1e-3": 1.288e-08, "gp/1-2^-20": 2.381e-07, "gp/1": 2.392e-07, "gp/1+1e-6": 2.845e-07, "gp/7": 2.045e-07, "gp/1e3": 2.438e-07,
    # (r0 near n = 1 is measured in units of the floor, what one ulp of n does to coef: the float32 n is off by up to two)
    "r0/1e-3": 3.150e-07, "r0/1-2^-20": 2.219e-01, "r0/1": 1.999e+00, "r0/1+1e-6": 2.543e-01, "r0/7": 9.217e-08, "r0/1e3": 8.903e-08,
    "loss/0": 3.893e-07, "loss/1": 7.823e-08,
    # (bf16 values near 1 are multiples of 2^-8; 40 000 of them add up exactly in float32 in any order: the limit is 0)
    "colsum/f32": 4.599e-07, "colsum/bf16": 0.0,
    "diff/f32": 1.188e-07, "combine/f32": 2.473e-07, "diff/bf16": 7.752e-03, "combine/bf16": 1.026e-02,
    "dense_fwd/f32": 2.798e-07, "dense_top/f32": 1.873e-07, "dense_wgrad/f32": 3.305e-07,
    "dense_fwd/bf16": 2.965e-07, "dense_top/bf16": 3.889e-03, "dense_wgrad/bf16": 2.718e-07,
    "forms/0": 2.690e-07, "forms_adj/0": 2.567e-07, "forms/1": 2.823e-07, "forms_adj/1": 2.352e-07,
    "cin": 1.103e-07, "pool_lrelu": 1.976e-07, "lrelu": 1.430e-08,
}
LIMITS = {k: 4.0 * v for k, v in MEASURED.items()}
