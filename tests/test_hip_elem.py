"""-m gpu: the step's elementwise / reduction kernels one by one (rdgan_op_softmax_tail ... rdgan_op_diff_combine: the production
kernel through the launcher the step uses) against the fp64 restatements of tests/elem_np.py, on input families away from the
regime of a freshly initialised step -- sharp softmax columns, ||grad|| at 1, large critic values of mixed sign, mean-1 column
sums -- with the shared comparison and the committed limits (4 x what a float32 restatement deviates).  Every output buffer
stands between canary-filled margins that must come back untouched."""
import json

import numpy as np
import pytest
import torch

from tests import elem_np as en
from tests.hip_util import dev, lib, ptr, stream

pytestmark = pytest.mark.gpu

MARGIN = 64
CANARY = -8192.0          # (exact in bf16 and int32 too)
OBSERVED = {}           # family -> worst deviation as a fraction of its limit


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rep = {k: round(v, 4) for k, v in sorted(OBSERVED.items())}
    print("\nelementwise kernels, worst deviation / limit: " + json.dumps(rep))


def guarded(shape, dtype=torch.float32, fill=float("nan")):
    """(whole buffer, view of `shape` inside it): the view filled with `fill`, MARGIN canaries on either side"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * MARGIN,), CANARY, dtype=dtype, device="cuda")
    view = buf[MARGIN:MARGIN + n]
    view.fill_(fill)
    return buf, view.view(*shape)


def margins_ok(*bufs):
    for b in bufs:
        assert bool((b[:MARGIN] == CANARY).all()) and bool((b[-MARGIN:] == CANARY).all()), "a kernel wrote outside its output"


def check(key, got, want, scale, what):
    lim = en.LIMITS[key]
    d = en.deviation(got, want, scale)
    print(f"{what}: deviation {d:.3e}, limit {lim:.3e}")
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), d / lim if lim else d)
    en.compare(got, want, scale, lim, what)


def np_(t):
    return t.float().cpu().numpy()


# ---- softmax tails ----
def _run_tail(form, taps, bias, B, H, W, flag0=0):
    obuf, out = guarded((B, en.NH, H, W))
    fbuf, flag = guarded((1,), torch.int32, flag0)
    td, bd = dev(taps), dev(bias)
    assert lib().rdgan_op_softmax_tail(form, ptr(td), ptr(bd), ptr(out), ptr(flag), B, H, W, stream()) == 0
    margins_ok(obuf, fbuf)
    return np_(out), int(flag.item())


@pytest.mark.parametrize("family", en.TAIL_FAMILIES)
@pytest.mark.parametrize("case", en.TAIL_CASES, ids=lambda c: "form%d-B%d-%dx%d" % c)
def test_softmax_tail(case, family):
    form, B, H, W = case
    taps, bias = en.tail_family(form, family, B, H, W)
    out, flag = _run_tail(form, taps, bias, B, H, W)
    check(f"tail/{family}", out, en.softmax_tail(form, taps, bias), 1.0, f"softmax tail form {form} {family} B {B} {H}x{W}")
    assert flag == 0


_CENTRE = {0: (0, 5, 2, 2, 13), 3: (0, 5, 1, 2, 2), 9: (0, 5, 4, 2, 2), 12: (0, 1, 2, 0, 1, 5)}


@pytest.mark.parametrize("form", en.TAIL_FORMS)
def test_softmax_tail_flag(form):
    """the flag word gets bit 0 exactly when a logit is +-Inf or NaN, and the kernel never clears it"""
    B, H, W = (1, 16, 16) if form == 12 else (3, 7, 9)
    taps, bias = en.tail_family(form, "rain", B, H, W)
    assert _run_tail(form, taps, bias, B, H, W, flag0=0)[1] == 0
    assert _run_tail(form, taps, bias, B, H, W, flag0=2)[1] == 2
    for bad in (np.inf, -np.inf, np.nan):
        t = taps.copy()
        t[_CENTRE[form]] = bad
        assert not np.isfinite(en.tail_logits(form, t, bias)).all()
        assert _run_tail(form, t, bias, B, H, W, flag0=0)[1] == 1, bad
        assert _run_tail(form, t, bias, B, H, W, flag0=2)[1] == 3, bad
    if form == 0:                     # columns 27 .. 31 of P are never read
        t = taps.copy()
        t[..., 27:] = np.nan
        out, flag = _run_tail(form, t, bias, B, H, W)
        assert flag == 0 and np.isfinite(out).all()


# ---- softmax backward ----
@pytest.mark.parametrize("family", en.TAIL_FAMILIES)
@pytest.mark.parametrize("case", en.BWD_CASES, ids=lambda c: "B%d-%dx%d" % c)
def test_softmax_bwd(case, family):
    B, H, W = case
    p, g = en.bwd_family(family, B, H, W)
    obuf, dl = guarded(p.shape)
    pd, gd = dev(p), dev(g)
    assert lib().rdgan_op_softmax_bwd(ptr(pd), ptr(gd), ptr(dl), B, H, W, stream()) == 0
    margins_ok(obuf)
    check(f"bwd/{family}", np_(dl), en.softmax_bwd(p, g), en.bwd_scale(p, g), f"softmax backward {family} B {B} {H}x{W}")


# ---- gradient-penalty norm ----
def _run_gp(g0, CP, S):
    B, per = g0.shape
    cbuf, cin = guarded((B, per, CP))
    gbuf, gp = guarded((B,))
    gd = dev(g0)
    assert lib().rdgan_op_gp_norm(ptr(gd), B, per, CP, S, ptr(cin), ptr(gp), stream()) == 0
    margins_ok(cbuf, gbuf)
    return np_(cin), np_(gp)


@pytest.mark.parametrize("norm", list(en.GP_NORMS))
@pytest.mark.parametrize("case", en.GP_CASES, ids=lambda c: "B%d-per%d-CP%d-S%d" % c)
def test_gp_norm(case, norm):
    B, per, CP, S = case
    g0 = en.gp_family(B, per, norm)
    cin, gp = _run_gp(g0, CP, S)
    want_gp, want_r0, _, _ = en.gp_norm(g0)
    sg, sr = en.gp_scales(g0)
    check(f"gp/{norm}", gp, want_gp, sg, f"gp norm n = {norm} {case}")
    check(f"r0/{norm}", cin[..., 0], want_r0, sr, f"gp r0 n = {norm} {case}")
    assert (cin[..., 1:] == 0).all()


@pytest.mark.parametrize("S", (0, 7))
def test_gp_norm_of_a_zero_sample(S):
    """pinned: a sample of norm 0 gets gp = -1 and NaN r0 (0 * inf, the gradient of Keras's sqrt at 0); its neighbours are untouched"""
    B, per, CP = 5, 6144, 2
    g0 = en.gp_family(B, per, "7", zero_sample=2)
    cin, gp = _run_gp(g0, CP, S)
    assert gp[2] == -1.0 and np.isnan(cin[2, :, 0]).all() and (cin[..., 1:] == 0).all()
    keep = [0, 1, 3, 4]
    want_gp, want_r0, _, _ = en.gp_norm(g0)
    sg, sr = en.gp_scales(g0)
    check("gp/7", gp[keep], want_gp[keep], sg[keep], "gp norm beside a zero sample")
    check("r0/7", cin[keep, :, 0], want_r0[keep], sr[keep], "gp r0 beside a zero sample")


# ---- loss tails ----
def _run_loss(mode, v, gp, B, gflag):
    obuf, out = guarded((8,))
    vd, gd = dev(v), dev(gp)
    assert lib().rdgan_op_loss_tail(mode, ptr(vd), ptr(gd), B, gflag, ptr(out), stream()) == 0
    margins_ok(obuf)
    return np_(out)


@pytest.mark.parametrize("gflag", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("B", en.LOSS_BATCHES)
def test_loss_tail(B, mode, gflag):
    v, gp = en.loss_family(B)
    out = _run_loss(mode, v, gp, B, gflag)
    check(f"loss/{mode}", out[:4], en.loss_tail(mode, v, gp, B), en.loss_scale(mode, v, gp, B), f"loss tail mode {mode} B {B}")
    assert out[4] == float(gflag) and (out[5:] == 0).all()
    if gflag == 0:
        for bad in (np.inf, np.nan):
            vb = v.copy()
            vb[B // 2] = bad
            outb = _run_loss(mode, vb, gp, B, 0)
            assert outb[4] == 1.0 and (outb[5:] == 0).all(), bad


# ---- column sums ----
@pytest.fixture(scope="module")
def engine():
    from pr_disagg_radar_gan_amd import Engine
    eng = Engine(ndomain=16, max_batch=2)
    yield eng
    eng.close()


def _run_colsum(engine, a, bf16):
    rows, C = a.shape
    obuf, out = guarded((C,))
    src = dev(a, torch.bfloat16 if bf16 else torch.float32)
    assert lib().rdgan_op_colsum(engine._h, ptr(src), rows, C, ptr(out), int(bf16), stream()) == 0
    margins_ok(obuf)
    return np_(out)


@pytest.mark.parametrize("case", en.COLSUM_CASES, ids=lambda c: "%dx%d" % c)
def test_colsum(engine, case):
    a = en.colsum_family(*case)
    check("colsum/f32", _run_colsum(engine, a, False), en.colsum(a), en.colsum_scale(a), f"colsum {case}")


@pytest.mark.parametrize("case", en.COLSUM_BF16_CASES, ids=lambda c: "%dx%d" % c)
def test_colsum_bf16(engine, case):
    """bf16 values near 1 add up exactly in fp32, in any order"""
    a = en.colsum_family(*case, bf16=True)
    check("colsum/bf16", _run_colsum(engine, a, True), en.colsum(a), en.colsum_scale(a), f"colsum bf16 {case}")


def test_colsum_refuses_bf16_for_other_widths(engine):
    a = dev(np.ones((8, 100), np.float32), torch.bfloat16)
    obuf, out = guarded((100,))
    assert lib().rdgan_op_colsum(engine._h, ptr(a), 8, 100, ptr(out), 1, stream()) == -2
    margins_ok(obuf)


# ---- hour differences and their adjoint ----
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("case", en.DIFF_CASES, ids=lambda c: "B%d-D%d-P%d" % c)
def test_diff_combine(case, bf16):
    B, D, P = case
    sfx, dt = ("bf16", torch.bfloat16) if bf16 else ("f32", torch.float32)
    x, dx, dE = en.diff_family(B, D, P, bf16=bf16)
    ebuf, E = guarded((B, D + 1, P), dt)
    dbuf, dxd = guarded((B, D, P), dt)
    dxd.copy_(dev(dx, dt))
    xd, dEd = dev(x, dt), dev(dE, dt)
    assert lib().rdgan_op_diff_combine(ptr(xd), ptr(E), ptr(dxd), ptr(dEd), B, D, P, int(bf16), stream()) == 0
    margins_ok(ebuf, dbuf)
    check(f"diff/{sfx}", np_(E), en.diff_d(x), en.diff_scale(x), f"diff_d {sfx} {case}")
    check(f"combine/{sfx}", np_(dxd), en.combine_dx(dx, dE), en.combine_scale(dx, dE), f"combine_dx {sfx} {case}")
    # combine_dx is the adjoint of diff_d: <E(x), dE> = <x, fold(dE)> with both maps taken by the GPU, each of whose elements
    # is off by at most its limit times its scale
    zbuf, fold = guarded((B, D, P), dt, 0.0)
    assert lib().rdgan_op_diff_combine(None, None, ptr(fold), ptr(dEd), B, D, P, int(bf16), stream()) == 0
    margins_ok(zbuf)
    x64, dE64 = x.astype(np.float64), dE.astype(np.float64)
    lhs, rhs = (np_(E).astype(np.float64) * dE64).sum(), (x64 * np_(fold).astype(np.float64)).sum()
    bound = (en.LIMITS[f"diff/{sfx}"] * (en.diff_scale(x) * np.abs(dE64)).sum()
             + en.LIMITS[f"combine/{sfx}"] * (np.abs(x64) * en.combine_scale(np.zeros_like(x), dE)).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


def test_bad_arguments_are_refused():
    L = lib()
    z = ptr(None)
    t = dev(np.zeros(64, np.float32))
    assert L.rdgan_op_softmax_tail(5, ptr(t), ptr(t), ptr(t), ptr(t), 1, 8, 8, stream()) == -2
    assert L.rdgan_op_softmax_tail(12, ptr(t), ptr(t), ptr(t), ptr(t), 1, 8, 8, stream()) == -2
    assert L.rdgan_op_softmax_tail(0, z, ptr(t), ptr(t), ptr(t), 1, 8, 8, stream()) == -2
    assert L.rdgan_op_softmax_bwd(ptr(t), ptr(t), z, 1, 8, 8, stream()) == -2
    assert L.rdgan_op_gp_norm(ptr(t), 1, 64, 2, 65, ptr(t), ptr(t), stream()) == -2
    assert L.rdgan_op_gp_norm(ptr(t), 0, 64, 2, 0, ptr(t), ptr(t), stream()) == -2
    assert L.rdgan_op_loss_tail(2, ptr(t), ptr(t), 1, 0, ptr(t), stream()) == -2
    assert L.rdgan_op_loss_tail(0, ptr(t), z, 1, 0, ptr(t), stream()) == -2
    assert L.rdgan_op_colsum(None, ptr(t), 1, 64, ptr(t), 0, stream()) == -2
    assert L.rdgan_op_diff_combine(ptr(t), ptr(t), z, z, 1, 6, 6, 0, stream()) == -2
    assert L.rdgan_op_diff_combine(ptr(t), z, z, z, 1, 6, 8, 0, stream()) == -2


# ---- the critic's Dense layer, the top of its backward, its weight gradient ----
def _gpu_mask(NB, F, seed):
    """the dropped pattern of critic layer 4 from the library's own RNG, pinned to the oracle's"""
    if not seed:
        return None
    from oracle import rng as orng
    m = torch.empty(NB * F, device="cuda")
    assert lib().rdgan_op_rng(seed, orng.STREAM_D4, ptr(m), ptr(None), NB * F, stream()) == 0
    m = np_(m).reshape(NB, F)
    assert (m == orng.dropout_scale_mask(seed, orng.STREAM_D4, (NB, F))).all()
    return m


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("seed", (0, 4242))
@pytest.mark.parametrize("F", en.DENSE_F)
@pytest.mark.parametrize("case", en.DENSE_CASES, ids=lambda c: "NB%d-B%d-mode%d" % c)
def test_critic_dense(case, F, seed, bf16):
    NB, B, mode = case
    sfx, dt = ("bf16", torch.bfloat16) if bf16 else ("f32", torch.float32)
    mask = _gpu_mask(NB, F, seed)
    h4, w, bias = en.dense_family(NB, F, mask, bf16=bf16)
    assert (h4 < 0).any() and ((h4 == 0) & ~np.signbit(h4)).any()
    vbuf, v = guarded((NB,))
    ubuf, u4 = guarded((NB, F), dt)
    hd, wd, bd = dev(h4, dt), dev(w), dev(bias)
    assert lib().rdgan_op_critic_dense(ptr(hd), ptr(wd), ptr(bd), ptr(v), ptr(u4), NB, F, B, mode, seed, int(bf16), stream()) == 0
    margins_ok(vbuf, ubuf)
    check(f"dense_fwd/{sfx}", np_(v), en.dense_fwd(h4, w, bias), en.dense_fwd_scale(h4, w, bias), f"dense forward {sfx} {case} F {F} seed {seed}")
    want = en.dense_top_bwd(h4, w, mask, B, mode)
    check(f"dense_top/{sfx}", np_(u4), want, np.abs(want), f"dense top backward {sfx} {case} F {F} seed {seed}")
    if mode == 0:
        for sl in en.DENSE_SLICES:
            obuf, out = guarded((F,))
            assert lib().rdgan_op_critic_dense_wgrad(ptr(hd), ptr(out), NB, F, B, sl, int(bf16), stream()) == 0
            margins_ok(obuf)
            check(f"dense_wgrad/{sfx}", np_(out), en.dense_wgrad(h4, B), en.dense_wgrad_scale(h4, B),
                  f"dense wgrad {sfx} {case} F {F} slices {sl}")


# ---- weight forms ----
@pytest.mark.parametrize("CC", en.FORMS_CC)
@pytest.mark.parametrize("which", (0, 1), ids=("collapsed", "shared-centre"))
def test_weight_forms(which, CC):
    M = en.forms_matrix(which)
    nf = M.shape[0]
    W, dF = en.forms_family(27, CC), en.forms_family(nf, CC)
    fbuf, forms = guarded((nf, CC))
    abuf, dW = guarded((27, CC))
    Wd, dFd = dev(W), dev(dF)
    assert lib().rdgan_op_weight_forms(which, ptr(Wd), ptr(forms), CC, stream()) == 0
    assert lib().rdgan_op_weight_forms_adj(which, ptr(dFd), ptr(dW), CC, stream()) == 0
    margins_ok(fbuf, abuf)
    check(f"forms/{which}", np_(forms), en.forms_apply(M, W), en.forms_scale(M, W), f"weight forms {which} CC {CC}")
    check(f"forms_adj/{which}", np_(dW), en.forms_apply(M.T, dF), en.forms_scale(M.T, dF), f"weight forms adjoint {which} CC {CC}")
    W64, dF64 = W.astype(np.float64), dF.astype(np.float64)
    lhs, rhs = (np_(forms).astype(np.float64) * dF64).sum(), (W64 * np_(dW).astype(np.float64)).sum()
    bound = (en.LIMITS[f"forms/{which}"] * (en.forms_scale(M, W) * np.abs(dF64)).sum()
             + en.LIMITS[f"forms_adj/{which}"] * (np.abs(W64) * en.forms_scale(M.T, dF)).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ---- critic input ----
@pytest.mark.parametrize("base", (0, 7))
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("case", en.CIN_CASES, ids=lambda c: "B%d-HW%d-nc%d" % c)
def test_critic_input(case, mode, base):
    from oracle import rng as orng
    B, HW, nc = case
    D, CP, seed = en.CIN_D, (2 if nc == 1 else 4), 99
    real, fake, cond = en.cin_family(B, HW, nc)
    alpha = orng.uniform(seed, orng.STREAM_ALPHA, B, start=base)
    rd, fd, cd = dev(real), dev(fake), dev(cond)
    nb = 3 * B if mode == 0 else B
    outs = []
    for scalar in (0, 1):
        obuf, out = guarded((nb, D, HW, CP))
        assert lib().rdgan_op_critic_input(ptr(rd) if mode != 1 else ptr(None), ptr(fd) if mode != 2 else ptr(None), ptr(cd), ptr(out),
                                           B, D, HW, nc, CP, mode, seed, base, scalar, stream()) == 0
        margins_ok(obuf)
        outs.append(np_(out))
    assert (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all(), "the four-voxel and the scalar route differ"
    check("cin", outs[0], en.critic_input(real, fake, cond, alpha, CP, mode), en.cin_scale(real, fake, cond, CP, mode),
          f"critic input {case} mode {mode} alpha_base {base}")


# ---- LeakyReLU backward, with and without the pooling ----
@pytest.mark.parametrize("case", en.POOL_CASES, ids=lambda c: "B%d-%dx%dx%d-C%d" % c)
def test_pool_lrelu_bwd(case):
    B, D, H, W, C = case
    g, h = en.lrelu_family((B, 2 * D, 2 * H, 2 * W, C), (B, D, H, W, C))
    obuf, out = guarded(h.shape)
    gd, hd = dev(g), dev(h)
    assert lib().rdgan_op_pool_lrelu_bwd(ptr(gd), ptr(hd), ptr(out), B, D, H, W, C, stream()) == 0
    margins_ok(obuf)
    check("pool_lrelu", np_(out), en.pool_lrelu_bwd(g, h), en.pool_scale(g, h), f"pool + lrelu backward {case}")


@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("n", en.LRELU_CASES)
def test_lrelu_bwd(n, bf16):
    dt = torch.bfloat16 if bf16 else torch.float32
    g, h = en.lrelu_family((n,), (n,), bf16=bf16)
    obuf, out = guarded((n,))
    gd, hd = dev(g, dt), dev(h, dt)
    assert lib().rdgan_op_lrelu_bwd(ptr(gd), ptr(hd), ptr(out), n, int(bf16), stream()) == 0
    margins_ok(obuf)
    check("lrelu", np_(out), en.lrelu_bwd(g, h), np.abs(g), f"lrelu backward n {n} bf16 {bf16}")


def test_bad_arguments_of_the_remaining_entries_are_refused():
    L = lib()
    z = ptr(None)
    t = dev(np.zeros(64, np.float32))
    assert L.rdgan_op_critic_dense(ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), 1, 64, 1, 2, 0, 0, stream()) == -2
    assert L.rdgan_op_critic_dense(z, ptr(t), ptr(t), ptr(t), ptr(t), 1, 64, 1, 0, 0, 0, stream()) == -2
    assert L.rdgan_op_critic_dense_wgrad(ptr(t), z, 1, 64, 1, 1, 0, stream()) == -2
    assert L.rdgan_op_weight_forms(2, ptr(t), ptr(t), 64, stream()) == -2
    assert L.rdgan_op_weight_forms_adj(0, ptr(t), ptr(t), 6, stream()) == -2
    assert L.rdgan_op_critic_input(ptr(t), ptr(t), ptr(t), ptr(t), 1, 24, 64, 2, 2, 0, 0, 0, 0, stream()) == -2
    assert L.rdgan_op_critic_input(z, ptr(t), ptr(t), ptr(t), 1, 24, 64, 1, 2, 0, 0, 0, 0, stream()) == -2
    assert L.rdgan_op_pool_lrelu_bwd(ptr(t), ptr(t), ptr(t), 1, 1, 1, 1, 6, stream()) == -2
    assert L.rdgan_op_lrelu_bwd(ptr(t), ptr(t), ptr(t), 6, 0, stream()) == -2
