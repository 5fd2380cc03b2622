"""CPU: how far the float32 restatements of tests/elem_np.py are from the fp64 ones over every input family, against the limits
the GPU tests use (LIMITS = 4 x MEASURED), and that named wrong variants of each formula are refused at those limits."""
import numpy as np
import pytest

from tests import elem_np as en

F32 = np.float32


def _check_limit(key, worst):
    print(f"{key}: float32 restatement deviates {worst:.4e}; limit {en.LIMITS[key]:.4e}")      # (0: the fp32 sums are exact)
    assert 2.0 * worst <= en.LIMITS[key] <= 8.0 * worst, (key, worst, en.LIMITS[key])


def measure_tail(family, mutation=None):
    worst = 0.0
    for form, B, H, W in en.TAIL_CASES:
        taps, bias = en.tail_family(form, family, B, H, W)
        worst = max(worst, en.deviation(en.softmax_tail(form, taps, bias, F32, mutation), en.softmax_tail(form, taps, bias), 1.0))
    return worst


def measure_bwd(family, mutation=None):
    worst = 0.0
    for B, H, W in en.BWD_CASES:
        p, g = en.bwd_family(family, B, H, W)
        worst = max(worst, en.deviation(en.softmax_bwd(p, g, F32, mutation), en.softmax_bwd(p, g), en.bwd_scale(p, g)))
    return worst


def measure_gp(norm, mutation=None):
    wg = wr = 0.0
    for B, per, CP, S in en.GP_CASES:
        g0 = en.gp_family(B, per, norm)
        gp, r0, _, _ = en.gp_norm(g0)
        gp32, r32, _, _ = en.gp_norm(g0, F32, mutation, S=S)
        sg, sr = en.gp_scales(g0)
        wg, wr = max(wg, en.deviation(gp32, gp, sg)), max(wr, en.deviation(r32, r0, sr))
    return wg, wr


def measure_loss(mode, mutation=None):
    worst = 0.0
    for B in en.LOSS_BATCHES:
        v, gp = en.loss_family(B)
        worst = max(worst, en.deviation(en.loss_tail(mode, v, gp, B, F32, mutation), en.loss_tail(mode, v, gp, B),
                                        en.loss_scale(mode, v, gp, B)))
    return worst


def measure_colsum(bf16, mutation=None):
    worst = 0.0
    for rows, C in (en.COLSUM_BF16_CASES if bf16 else en.COLSUM_CASES):
        a = en.colsum_family(rows, C, bf16=bf16)
        worst = max(worst, en.deviation(en.colsum(a, F32, mutation), en.colsum(a), en.colsum_scale(a)))
    return worst


def measure_diff(bf16, mutation=None):
    wd = wc = 0.0
    for B, D, P in en.DIFF_CASES:
        x, dx, dE = en.diff_family(B, D, P, bf16=bf16)
        wd = max(wd, en.deviation(en.diff_d(x, F32, mutation, bf16), en.diff_d(x), en.diff_scale(x)))
        wc = max(wc, en.deviation(en.combine_dx(dx, dE, F32, mutation, bf16), en.combine_dx(dx, dE), en.combine_scale(dx, dE)))
    return wd, wc


@pytest.mark.parametrize("family", en.TAIL_FAMILIES)
def test_softmax_tail_limits(family):
    _check_limit(f"tail/{family}", measure_tail(family))


@pytest.mark.parametrize("family", en.TAIL_FAMILIES)
def test_softmax_bwd_limits(family):
    _check_limit(f"bwd/{family}", measure_bwd(family))


@pytest.mark.parametrize("norm", list(en.GP_NORMS))
def test_gp_norm_limits(norm):
    wg, wr = measure_gp(norm)
    _check_limit(f"gp/{norm}", wg)
    _check_limit(f"r0/{norm}", wr)


@pytest.mark.parametrize("mode", (0, 1))
def test_loss_tail_limits(mode):
    _check_limit(f"loss/{mode}", measure_loss(mode))


@pytest.mark.parametrize("bf16", (False, True))
def test_colsum_limits(bf16):
    _check_limit("colsum/bf16" if bf16 else "colsum/f32", measure_colsum(bf16))


@pytest.mark.parametrize("bf16", (False, True))
def test_diff_combine_limits(bf16):
    wd, wc = measure_diff(bf16)
    sfx = "bf16" if bf16 else "f32"
    _check_limit(f"diff/{sfx}", wd)
    _check_limit(f"combine/{sfx}", wc)


def _dense_mask(NB, F, seed):
    from oracle import rng as orng
    return orng.dropout_scale_mask(seed, orng.STREAM_D4, (NB, F)) if seed else None


def measure_dense(bf16, mutation=None):
    wv = wu = ww = 0.0
    for NB, B, mode in en.DENSE_CASES:
        for F in en.DENSE_F:
            for seed in (0, 4242):
                mask = _dense_mask(NB, F, seed)
                h4, w, bias = en.dense_family(NB, F, mask, bf16=bf16)
                wv = max(wv, en.deviation(en.dense_fwd(h4, w, bias, F32, mutation), en.dense_fwd(h4, w, bias), en.dense_fwd_scale(h4, w, bias)))
                want = en.dense_top_bwd(h4, w, mask, B, mode)
                wu = max(wu, en.deviation(en.dense_top_bwd(h4, w, mask, B, mode, F32, mutation, bf16), want, np.abs(want)))
            if mode == 0:
                for sl in en.DENSE_SLICES:
                    ww = max(ww, en.deviation(en.dense_wgrad(h4, B, F32, mutation, sl), en.dense_wgrad(h4, B), en.dense_wgrad_scale(h4, B)))
    return wv, wu, ww


def measure_forms(which, mutation=None):
    wf = wa = 0.0
    M, Mm = en.forms_matrix(which), en.forms_matrix(which, mutation)
    for CC in en.FORMS_CC:
        W, dF = en.forms_family(27, CC), en.forms_family(M.shape[0], CC)
        wf = max(wf, en.deviation(en.forms_apply(Mm, W, F32), en.forms_apply(M, W), en.forms_scale(M, W)))
        wa = max(wa, en.deviation(en.forms_apply(Mm.T, dF, F32), en.forms_apply(M.T, dF), en.forms_scale(M.T, dF)))
    return wf, wa


def _alpha(B, seed, base):
    from oracle import rng as orng
    return orng.uniform(seed, orng.STREAM_ALPHA, B, start=base)


def measure_cin(mutation=None):
    worst = 0.0
    for B, HW, nc in en.CIN_CASES:
        real, fake, cond = en.cin_family(B, HW, nc)
        CP = 2 if nc == 1 else 4
        for base in (0, 7):
            a = _alpha(B, 99, base)
            for mode in (0, 1, 2):
                worst = max(worst, en.deviation(en.critic_input(real, fake, cond, a, CP, mode, F32, mutation),
                                                en.critic_input(real, fake, cond, a, CP, mode), en.cin_scale(real, fake, cond, CP, mode)))
    return worst


def measure_lrelu(mutation=None):
    wp = wl = 0.0
    for B, D, H, W, C in en.POOL_CASES:
        g, h = en.lrelu_family((B, 2 * D, 2 * H, 2 * W, C), (B, D, H, W, C))
        wp = max(wp, en.deviation(en.pool_lrelu_bwd(g, h, F32, mutation), en.pool_lrelu_bwd(g, h), en.pool_scale(g, h)))
    for n in en.LRELU_CASES:
        for bf16 in (False, True):
            g, h = en.lrelu_family((n,), (n,), bf16=bf16)
            wl = max(wl, en.deviation(en.lrelu_bwd(g, h, F32, mutation), en.lrelu_bwd(g, h), np.abs(g)))
    return wp, wl


@pytest.mark.parametrize("bf16", (False, True))
def test_dense_limits(bf16):
    wv, wu, ww = measure_dense(bf16)
    sfx = "bf16" if bf16 else "f32"
    _check_limit(f"dense_fwd/{sfx}", wv)
    _check_limit(f"dense_top/{sfx}", wu)
    _check_limit(f"dense_wgrad/{sfx}", ww)


@pytest.mark.parametrize("which", (0, 1))
def test_weight_forms_limits(which):
    wf, wa = measure_forms(which)
    _check_limit(f"forms/{which}", wf)
    _check_limit(f"forms_adj/{which}", wa)


def test_critic_input_limits():
    _check_limit("cin", measure_cin())


def test_lrelu_bwd_limits():
    wp, wl = measure_lrelu()
    _check_limit("pool_lrelu", wp)
    _check_limit("lrelu", wl)


@pytest.mark.parametrize("mutation", en.DENSE_MUTATIONS)
def test_dense_mutations_refused(mutation):
    wv, wu, ww = measure_dense(False, mutation)
    got = {"bias_dropped": (wv, "dense_fwd/f32"), "real_third_plus": (min(wu, ww), "dense_top/f32"),
           "gate_without_keep_scale": (wu, "dense_top/f32"), "last_slice_skipped": (ww, "dense_wgrad/f32")}[mutation]
    assert got[0] > en.LIMITS[got[1]], (mutation, wv, wu, ww)
    if mutation in ("real_third_plus", "last_slice_skipped"):
        assert ww > en.LIMITS["dense_wgrad/f32"]


@pytest.mark.parametrize("mutation", en.FORMS_MUTATIONS)
def test_weight_forms_mutations_refused(mutation):
    for which in ((0, 1) if mutation == "centre_tap_twice" else (1,)):
        wf, wa = measure_forms(which, mutation)
        assert wf > en.LIMITS[f"forms/{which}"] and wa > en.LIMITS[f"forms_adj/{which}"], (which, wf, wa)


def test_weight_form_adjoints():
    """<M W, dF> = <W, M^T dF> in fp64, to 1e-12"""
    for which in (0, 1):
        M = en.forms_matrix(which)
        W, dF = en.forms_family(27, 64 * 64).astype(np.float64), en.forms_family(M.shape[0], 64 * 64).astype(np.float64)
        lhs, rhs = (en.forms_apply(M, W) * dF).sum(), (W * en.forms_apply(M.T, dF)).sum()
        assert abs(lhs - rhs) <= 1e-12 * (en.forms_scale(M, W) * np.abs(dF)).sum()
    # the collapsed forms of a phase add up to the whole kernel, tap by tap: every tap lies in exactly one of the 8 entries
    assert (en.forms_matrix(0).reshape(8, 8, 27).sum(1) == 1).all()


@pytest.mark.parametrize("mutation", en.CIN_MUTATIONS)
def test_critic_input_mutations_refused(mutation):
    assert measure_cin(mutation) > en.LIMITS["cin"]


@pytest.mark.parametrize("mutation", en.LRELU_MUTATIONS)
def test_lrelu_mutations_refused(mutation):
    wp, wl = measure_lrelu(mutation)
    assert wp > en.LIMITS["pool_lrelu"]
    if mutation == "slope_from_gradient":
        assert wl > en.LIMITS["lrelu"]


# ---- the comparison has the power to see a wrong formula: each named variant exceeds the limit of a sharp family ----
@pytest.mark.parametrize("mutation,family", [("no_max", "offset"), ("den_23_hours", "rain"), ("den_23_hours", "border"),
                                             ("upper_hour_tap_dropped", "border"), ("upper_hour_tap_dropped", "rain")])
def test_softmax_tail_mutations_refused(mutation, family):
    d = measure_tail(family, mutation)
    print(f"tail/{family} with {mutation}: {d:.3e} against the limit {en.LIMITS['tail/' + family]:.3e}")
    assert d > en.LIMITS[f"tail/{family}"]


@pytest.mark.parametrize("mutation", en.BWD_MUTATIONS)
@pytest.mark.parametrize("family", ("rain", "border"))
def test_softmax_bwd_mutations_refused(mutation, family):
    d = measure_bwd(family, mutation)
    print(f"bwd/{family} with {mutation}: {d:.3e} against the limit {en.LIMITS['bwd/' + family]:.3e}")
    assert d > en.LIMITS[f"bwd/{family}"]


def test_softmax_bwd_scale_is_per_column():
    """one wrong sharp column among flat ones: against the global maximum of |g| it would pass"""
    p, g = en.bwd_family("flat", 1, 8, 8)
    ps, _ = en.bwd_family("rain", 1, 8, 8)
    p[:, :, 3, 3] = ps[:, :, 3, 3]
    g[:, :, 3, 3] *= F32(1e-9)
    want = en.softmax_bwd(p, g)
    got = want.copy()
    got[:, :, 3, 3] = en.softmax_bwd(p, g, F32, "dot_unweighted")[:, :, 3, 3]
    assert en.deviation(got, want, en.bwd_scale(p, g)) > en.LIMITS["bwd/rain"]
    assert en.deviation(got, want, np.abs(p).max() * np.abs(g).max()) < en.LIMITS["bwd/rain"]


@pytest.mark.parametrize("mutation,norm", [("coef_without_division", "7"), ("coef_without_division", "1e-3"),
                                           ("short_last_slice_skipped", "7"), ("short_last_slice_skipped", "1+1e-6"),
                                           ("weight_not_over_batch", "1e3")])
def test_gp_norm_mutations_refused(mutation, norm):
    wg, wr = measure_gp(norm, mutation)
    print(f"gp/{norm} with {mutation}: gp {wg:.3e} (limit {en.LIMITS['gp/' + norm]:.3e}), r0 {wr:.3e} (limit {en.LIMITS['r0/' + norm]:.3e})")
    assert wr > en.LIMITS[f"r0/{norm}"]
    if mutation == "short_last_slice_skipped":
        assert wg > en.LIMITS[f"gp/{norm}"]


@pytest.mark.parametrize("mutation", en.LOSS_MUTATIONS)
def test_loss_tail_mutations_refused(mutation):
    d = measure_loss(0, mutation)
    print(f"loss/0 with {mutation}: {d:.3e} against the limit {en.LIMITS['loss/0']:.3e}")
    assert d > en.LIMITS["loss/0"]
    if mutation == "mean_over_B_minus_1":
        assert measure_loss(1, mutation) > en.LIMITS["loss/1"]


@pytest.mark.parametrize("mutation", en.COLSUM_MUTATIONS)
def test_colsum_mutations_refused(mutation):
    d = measure_colsum(False, mutation)
    print(f"colsum with {mutation}: {d:.3e} against the limit {en.LIMITS['colsum/f32']:.3e}")
    assert d > en.LIMITS["colsum/f32"]
    assert measure_colsum(True, mutation) > en.LIMITS["colsum/bf16"]


@pytest.mark.parametrize("mutation", en.DIFF_MUTATIONS)
@pytest.mark.parametrize("bf16", (False, True))
def test_diff_combine_mutations_refused(mutation, bf16):
    wd, wc = measure_diff(bf16, mutation)
    sfx = "bf16" if bf16 else "f32"
    assert wd > en.LIMITS[f"diff/{sfx}"] and wc > en.LIMITS[f"combine/{sfx}"]


def test_combine_is_the_adjoint_of_diff():
    """<E(x), dE> = <x, fold(dE)> in fp64, to 1e-12"""
    for B, D, P in en.DIFF_CASES:
        x, _, dE = en.diff_family(B, D, P)
        lhs = float((en.diff_d(x) * dE.astype(np.float64)).sum())
        rhs = float((x.astype(np.float64) * en.combine_dx(np.zeros_like(x), dE)).sum())
        scale = float((np.abs(en.diff_d(x)) * np.abs(dE)).sum())
        assert abs(lhs - rhs) <= 1e-12 * scale, (B, D, P, lhs, rhs)


def test_families_are_what_they_say():
    for form, B, H, W in en.TAIL_CASES:
        for fam in en.TAIL_FAMILIES:
            taps, bias = en.tail_family(form, fam, B, H, W)
            assert taps.shape == en.tail_shape(form, B, H, W) and taps.dtype == F32
            lg = en.tail_logits(form, taps, bias)
            top = np.sort(lg, 1)
            if fam == "flat":
                assert (top[:, -1] - top[:, 0]).max() < 3e-3
            elif fam in ("rain", "border"):
                assert (top[:, -1] - top[:, 0]).min() > 15          # the rest underflow against the sharp hour
            elif fam == "ties":
                assert (top[:, -1] == top[:, -2]).all() and (top[:, -1] == 3.0).all()
            else:
                assert np.abs(lg).min() > 9.9e3
    for norm, n in en.GP_NORMS.items():
        g0 = en.gp_family(5, 6144, norm)
        assert np.allclose(np.sqrt((g0.astype(np.float64) ** 2).sum(1)), n, rtol=1e-6)
    assert (en.bf16_round(np.array([1.0, 1.00390625, 1.01171875], F32)) == np.array([1.0, 1.0, 1.015625], F32)).all()
