"""The bars of tests/test_regimes_gpu.py, checked on the CPU: every stored fp32 error is measured again, and every wrong variant of
tests/regimes_ref.py (an eps in the wrong place, a one-pass variance, a softmax without its maximum) misses the bar of some regime by
10 x -- while on the `plain` data of the older tests the eps variants pass, which is the blindness the regimes remove."""
import math

import pytest
import torch

import regimes_ref as R

NORM_BAR = 5e-6            # test_groupnorm_mish, test_chan_layernorm
ATTN_BAR = 1e-5            # test_linattn


def _check(name, stored, measured):
    print(f"{name}: stored {stored:.2e} measured {measured:.2e}")
    if stored == 0.0:
        assert measured == 0.0, f"{name}: expected to be exact, measured {measured:.2e}"
        return
    assert math.isfinite(measured) and measured <= stored, f"{name}: stored e32 {stored:.2e} is below the measured {measured:.2e}"
    assert stored <= 2.0 * measured + 1e-9, f"{name}: stored e32 {stored:.2e} is more than twice the measured {measured:.2e}"


@pytest.mark.parametrize("regime", [r for r in R.GN_REGIMES if r != "const"])
def test_groupnorm_e32(regime):
    _check(f"gn {regime}", R.E32_GN[regime], max(R.gn_e32(regime, s) for s in R.GN_SHAPES + R.GN_SHAPES_BIG))
    _check(f"gn tail {regime}", R.E32_GN_TAIL[regime], R.gn_tail_e32(regime))


@pytest.mark.parametrize("regime", R.GN_BWD_REGIMES)
def test_groupnorm_backward_e32(regime):
    vals = [R.gn_bwd_e32(regime, s) for s in R.GN_BWD_SHAPES]
    for i, what in enumerate(("dx", "dgamma", "dbeta")):
        _check(f"gn bwd {regime} {what}", R.E32_GN_BWD[regime][i], max(v[i] for v in vals))


def test_groupnorm_const_is_exact():
    """a constant group: mean == the constant and var == 0 exactly, so the output is mish(beta) -- in fp32 as in fp64"""
    for shape in R.GN_SHAPES:
        x = R.gn_input("const", *shape)
        g, b, _ = R.gn_params(shape[1])
        want = R.U.mish(b.double()).view(1, -1, 1, 1).expand(shape)
        assert R.abs_err(R.gn_mish(x, g, b), want) <= R.MISH_ABS_BAR
        assert R.abs_err(R.gn_mish(*R.d(x, g, b)), want) == 0.0
        dx, dg, db = R.gn_grads(*R.d(x, g, b, R.gn_dy(*shape)))
        assert bool(torch.isfinite(dx).all()) and float(dg.abs().max()) == 0.0


@pytest.mark.parametrize("regime", R.LN_REGIMES)
def test_layernorm_e32(regime):
    if regime != "const":      # (const is exact: the test below)
        _check(f"ln {regime}", R.E32_LN[regime], max(R.ln_e32(regime, s) for s in R.LN_SHAPES))
    vals = [R.ln_bwd_e32(regime, s) for s in R.LN_SHAPES]
    for i, what in enumerate(("dx", "dg", "db")):
        _check(f"ln bwd {regime} {what}", R.E32_LN_BWD[regime][i], max(v[i] for v in vals))
    _check(f"ln folded {regime}", R.E32_LN_FOLDED[regime], R.ln_folded_e32(regime))


def test_layernorm_const_is_exact_and_closed_form_gradients_are_autograd():
    for M, C in R.LN_SHAPES:
        x = R.ln_input("const", M, C)
        g, b = R.ln_params(C)
        assert torch.equal(R.chan_layernorm(x, g, b), b.expand(M, C))
        dx, dg, db = R.ln_grads(*R.d(x, g, b, R.ln_dy(M, C)))
        assert bool(torch.isfinite(dx).all()) and float(dg.abs().max()) == 0.0
    for regime in ("plain", "tinystd", "std~eps", "offset"):
        x = R.ln_input(regime, 90, 24)
        g, b = R.ln_params(24)
        args = R.d(x, g, b, R.ln_dy(90, 24))
        for got, want in zip(R.ln_grads(*args), R.ln_grads_autograd(*args)):
            assert R.err(got, want) < 1e-9, regime


def test_attention_e32():
    """torch's fp32 softmax subtracts the maximum: every k regime costs what `plain` costs, forward and backward"""
    worst, worst_g = 0.0, 0.0
    for regime in R.K_REGIMES:
        for B, H, W in R.QKV_SHAPES + [(2, 48, 40)]:
            q = R.qkv_input(regime, B, H, W)
            (o32, c32), (o64, c64) = R.linattn(q), R.linattn(q.double())
            assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(c32).all())
            worst = max(worst, R.err(o32, o64), R.err(c32, c64))
            dy = R.rnd(B, R.HC, H, W, seed=9)
            worst_g = max(worst_g, R.err(R.linattn_grad(q, dy), R.linattn_grad(q.double(), dy.double())))
    _check("linattn", R.E32_ATTN, worst)
    _check("linattn grad", R.E32_ATTN_BWD, worst_g)
    assert R.bar(ATTN_BAR, R.E32_ATTN) == ATTN_BAR and R.bar(3e-5, R.E32_ATTN_BWD) == 3e-5      # the existing bars apply unchanged


@pytest.mark.parametrize("kreg,xreg", R.FROM_X_CASES)
def test_attention_from_x_e32(kreg, xreg):
    vals = [R.from_x_e32(kreg, xreg, s) for s in R.FROM_X_SHAPES]
    for i, what in enumerate(("out", "ctx")):
        _check(f"from x {kreg} {xreg} {what}", R.E32_FROM_X[(kreg, xreg)][i], max(v[i] for v in vals))


@pytest.mark.parametrize("kreg,xreg", R.FROM_X_CASES)
def test_attention_block_e32(kreg, xreg):
    _check(f"attention block {kreg} {xreg}", R.E32_ATTN_BLOCK[(kreg, xreg)], R.attn_block_e32(kreg, xreg))


def test_attention_weights_carry_the_k_regime():
    for C in (64, 256):
        w0, g, b = R.attn_weights("plain", C)
        for regime, want in (("k+85", 85.0), ("k-110", -110.0)):
            w, _, _ = R.attn_weights(regime, C)
            assert torch.allclose(w[R.HC:2 * R.HC] @ b, torch.full((R.HC,), want), rtol=1e-5)
            assert torch.equal(w[:R.HC], w0[:R.HC]) and torch.equal(w[2 * R.HC:], w0[2 * R.HC:])
        assert float(R.attn_weights("k-equal", C)[0][R.HC:2 * R.HC].abs().max()) == 0.0


def test_adam_e32():
    for regime in R.ADAM_REGIMES[1:]:
        _check(f"adam {regime}", R.E32_ADAM[regime], max(R.adam_e32(regime, s) for s in R.ADAM_STEPS))
    p, g, m, v = R.adam_state("g0")
    for step in R.ADAM_STEPS:
        p2, m2, v2 = R.adam_step(p, g, m, v, step)
        assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)


def test_activation_gradient_e32():
    x = R.act_grid().requires_grad_(True)
    gm, = torch.autograd.grad(torch.nn.functional.mish(x).sum(), x)
    gt, = torch.autograd.grad(torch.tanh(x).sum(), x)
    rm, rt = R.act_grads()
    assert bool(torch.isfinite(rm).all()) and bool(torch.isfinite(rt).all())
    _check("mish'", R.E32_ACT_ABS[0], R.abs_err(gm, rm))
    _check("tanh'", R.E32_ACT_ABS[1], R.abs_err(gt, rt))


# ------------------------------------------------------------------ the condition: a wrong variant misses the bar by 10 x
GN_WRONG = [("eps_outside", "tinyvar"), ("eps_outside", "var~eps"), ("no_eps", "tinyvar"), ("no_eps", "var~eps"), ("no_eps", "const"),
            ("no_eps", "mixed"), ("onepass", "offset"), ("onepass", "tinyvar"), ("onepass", "mixed")]
LN_WRONG = [("eps_inside", "tinystd"), ("eps_inside", "std~eps"), ("eps_inside", "mixed"), ("onepass", "offset"), ("onepass", "tinystd"),
            ("onepass", "std~eps")]


@pytest.mark.parametrize("variant,regime", GN_WRONG)
def test_wrong_groupnorm_misses_the_bar(variant, regime):
    shape = (2, 64, 8, 8)
    x = R.gn_input(regime, *shape)
    g, b, _ = R.gn_params(64)
    ref = R.gn_mish(*R.d(x, g, b))
    e = R.err(R.gn_mish(x, g, b, variant=variant), ref)
    limit = R.MISH_ABS_BAR / float(ref.abs().max()) if regime == "const" else R.bar(NORM_BAR, R.E32_GN[regime])
    print(f"gn {variant} on {regime}: {e:.2e} against {limit:.2e}")
    assert e >= 10 * limit
    assert R.err(R.gn_mish(x, g, b), ref) <= limit                     # ... which the right form in fp32 meets


def test_mean_by_reciprocal_misses_the_constant_group():
    """x - sum * fl(1 / n), contracted to one fused multiply-add, at n = 5 * 7 * 8 = 280: a constant group keeps the rounding of 1 / n
    times rstd ~ 316 instead of 0 and misses the 2e-6 bar (what ddk_groupnorm_mish did before it divided); at n = 512 the reciprocal
    is exact"""
    for shape, misses in (((3, 64, 5, 7), True), ((2, 64, 8, 8), False)):
        x = R.gn_input("const", *shape)
        g, b, _ = R.gn_params(64)
        e = R.abs_err(R.gn_mish(x, g, b, variant="mean_recip"), R.gn_mish(*R.d(x, g, b)))
        print(f"gn mean by reciprocal on const {shape}: {e:.2e} against {R.MISH_ABS_BAR:.2e}")
        assert (e > R.MISH_ABS_BAR) == misses


@pytest.mark.parametrize("variant,regime", LN_WRONG)
def test_wrong_layernorm_misses_the_bar(variant, regime):
    x = R.ln_input(regime, 90, 32)
    g, b = R.ln_params(32)
    ref = R.chan_layernorm(*R.d(x, g, b))
    e = R.err(R.chan_layernorm(x, g, b, variant=variant), ref)
    limit = R.bar(NORM_BAR, R.E32_LN[regime])
    print(f"ln {variant} on {regime}: {e:.2e} against {limit:.2e}")
    assert e >= 10 * limit
    assert R.err(R.chan_layernorm(x, g, b), ref) <= limit


@pytest.mark.parametrize("regime", ["k+85", "k-110", "kx20"])
def test_softmax_without_the_max_is_not_finite(regime):
    for B, H, W in R.QKV_SHAPES:
        q = R.qkv_input(regime, B, H, W)
        out, ctx = R.linattn(q, "nomax")
        assert R.err(out, R.linattn(q.double())[0]) == math.inf and R.err(ctx, R.linattn(q.double())[1]) == math.inf
    if regime == "k+85":       # through the weights too (there the shifted rows also spread the logits: only +85 must overflow)
        x = R.attn_x("plain", 3, 128, 8, 8)
        w, g, b = R.attn_weights(regime, 128)
        ref = R.attn_from_x(*R.d(x, w, g, b))
        assert R.err(R.attn_from_x(x, w, g, b, folded=True, variant="nomax")[1], ref[1]) == math.inf


@pytest.mark.parametrize("regime", ["g1e-9", "g1e-8"])
def test_wrong_adam_misses_the_bar(regime):
    p, g, m, v = R.adam_state(regime)
    limit = R.bar(R.ADAM_BAR, R.E32_ADAM[regime])
    for step in R.ADAM_STEPS:
        ref = R.adam_step(*R.d(p, g, m, v), step)[0]
        e = R.adam_update_err(R.adam_step(p, g, m, v, step, variant="eps_inside")[0], p, ref)
        print(f"adam eps inside the root on {regime}, step {step}: {e:.2e} against {limit:.2e}")
        assert e >= 10 * limit
        assert R.adam_update_err(R.adam_step(p, g, m, v, step)[0], p, ref) <= limit


def test_plain_data_does_not_see_the_eps_variants():
    """on the data of the older tests an eps in the wrong place, or none, passes the bars those tests use: 5e-6 for the norms, and the
    optimiser's at the steps test_optimizer_kernels_match_oracle takes; a softmax without its maximum is within 1e-5 too"""
    x = R.gn_input("plain", 2, 64, 8, 8)
    g, b, _ = R.gn_params(64)
    ref = R.gn_mish(*R.d(x, g, b))
    for variant in ("eps_outside", "no_eps", "onepass"):
        e = R.err(R.gn_mish(x, g, b, variant=variant), ref)
        print(f"gn {variant} on plain: {e:.2e}")
        assert e < NORM_BAR
    x = R.ln_input("plain", 90, 32)
    g, b = R.ln_params(32)
    ref = R.chan_layernorm(*R.d(x, g, b))
    for variant in ("eps_inside", "onepass"):
        e = R.err(R.chan_layernorm(x, g, b, variant=variant), ref)
        print(f"ln {variant} on plain: {e:.2e}")
        assert e < NORM_BAR
    q = R.qkv_input("plain", 1, 10, 13)
    assert R.err(R.linattn(q, "nomax")[1], R.linattn(q.double())[1]) < ATTN_BAR
    p, gr, m, v = R.adam_state("plain")
    for step in (1, 2):
        ref = R.adam_step(*R.d(p, gr, m, v), step)[0]
        assert R.adam_update_err(R.adam_step(p, gr, m, v, step, variant="eps_inside")[0], p, ref) < R.ADAM_BAR


def test_restatements_are_the_operators():
    """the fp64 references against torch's own operators and the oracle on every regime: a slip of an eps or of the maximum in a
    restatement itself (which the e32 measurements, fp32 against fp64 of the same text, would not see) fails here"""
    import torch.nn.functional as F
    for regime in R.GN_REGIMES:
        x = R.gn_input(regime, 2, 64, 8, 8)
        g, b, _ = R.gn_params(64)
        want = F.mish(F.group_norm(x.double(), R.GROUPS, g.double(), b.double(), R.GN_EPS))
        assert R.err(R.gn_mish(*R.d(x, g, b)), want) < 1e-10, regime
    for regime in R.LN_REGIMES:
        x = R.ln_input(regime, 90, 32)
        g, b = R.ln_params(32)
        nchw = x.double().t().reshape(1, 32, 90, 1)
        want = R.U.chan_layernorm(nchw, g.double().view(1, 32, 1, 1), b.double().view(1, 32, 1, 1)).reshape(32, 90).t()
        assert R.err(R.chan_layernorm(*R.d(x, g, b)), want) < 1e-10, regime
        w = R.ln_weight(384, 32)
        if regime not in ("const", "mixed", "std~eps"):      # in fp64 the folded form is the plain one (where it keeps its digits)
            assert R.err(R.ln_linear_folded(*R.d(x, g, b, w)), R.ln_linear(*R.d(x, g, b, w))) < 1e-9, regime
    for regime in R.K_REGIMES:
        q = R.qkv_input(regime, 1, 10, 13).double()
        k = q[:, R.HC:2 * R.HC].reshape(1, R.HEADS, R.DH, -1)
        ks = (k - torch.logsumexp(k, dim=-1, keepdim=True)).exp()
        want = torch.einsum("bhdn,bhen->bhde", ks, q[:, 2 * R.HC:].reshape(1, R.HEADS, R.DH, -1))
        assert R.err(R.linattn(q)[1], want) < 1e-10, regime


def test_regimes_are_what_they_say():
    """var below / about eps, |mean| / std of 1000, every group of `mixed` in its own regime, inputs finite and reproducible"""
    shape = (2, 64, 8, 8)
    var = lambda r: R.gn_input(r, *shape).double().reshape(2, R.GROUPS, -1).var(dim=-1, unbiased=False)
    assert float(var("tinyvar").max()) < 0.2 * R.GN_EPS and 0.5 * R.GN_EPS < float(var("var~eps").min()) < float(var("var~eps").max()) < 2 * R.GN_EPS
    assert float(var("const").max()) == 0.0 and float(R.gn_input("offset", *shape).mean()) > 990
    vm = var("mixed")
    for j, r in enumerate(R.GN_MIXED):
        assert 0.5 * float(var(r).mean()) <= float(vm[:, j].mean()) <= 2.0 * float(var(r).mean()) or r == "const" and float(vm[:, j].max()) == 0.0
    std = lambda r: R.ln_input(r, 90, 32).double().std(dim=-1, unbiased=False)
    assert float(std("std~eps").max()) < 4 * R.LN_EPS and float(std("tinystd").max()) < 2e-3 and float(std("const").max()) == 0.0
    for r in R.GN_REGIMES:
        assert bool(torch.isfinite(R.gn_input(r, *shape)).all()) and R.gn_input(r, *shape).dtype == torch.float32
    R.gn_input.cache_clear()
    a = R.gn_input("mixed", *shape).clone()
    R.gn_input.cache_clear()
    assert torch.equal(a, R.gn_input("mixed", *shape))
