"""The kernels of csrc/resample.hip, each op and each gradient, against tests/resample_ref.py (float64).

Tolerance, derived: every op here is linear, out = sum of N terms w x.  In fp32, whatever the summation order and with or without
FMA, |out - exact| <= (N + 8) 2^-24 sum |w| |x| elementwise (the 8 covers the bias add and the two weight roundings of a bicubic
tap product).  sum |w| |x| is the float64 reference op run on the absolute values; N is the op's own term count.  A wrong tap, a
wrong clamp or a missed border is off by orders of magnitude more."""
import pytest
import torch

import resample_ref as RR
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    return o


def within(got, want, mag, n, what):
    """|got - want| <= (n + 8) 2^-24 mag, elementwise; `want` and `mag` float64"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    excess = ((got - want).abs() - (n + 8) * U * mag).max()
    assert float(excess) <= 0.0, (what, float((got - want).abs().max()), float(((n + 8) * U * mag).min()))


def same_bits(fn):
    a, b = fn(), fn()
    if not isinstance(a, tuple):
        a, b = (a,), (b,)
    for p, q in zip(a, b):
        assert (p is None and q is None) or torch.equal(p, q)
    return a if len(a) > 1 else a[0]


# ---------------------------------------------------------------- bicubic
SIZES = [(8, 4), (32, 4), (16, 8), (24, 12), (24, 6), (4, 8), (4, 32), (12, 24), (2, 1), (1, 2)]
BICUBIC = [(b, c, i, o) for i, o in SIZES for b, c in ((1, 1), (2, 3), (5, 3))] + [(2, 3, 256, 32), (2, 3, 32, 256)]


@pytest.mark.parametrize("B,C,n_in,n_out", BICUBIC)
def test_bicubic_resize_and_its_gradient(ops, B, C, n_in, n_out):
    x = syn.synthetic_normal((B, C, n_in, n_in), f"bic.x.{n_in}.{n_out}")
    dy = syn.synthetic_normal((B, C, n_out, n_out), f"bic.dy.{n_in}.{n_out}")
    xd, dyd = x.to(DEV), dy.to(DEV)
    y = same_bits(lambda: ops.bicubic_resize(xd, (n_out, n_out)))
    within(y, RR.bicubic(x.double(), (n_out, n_out)), RR.bicubic(x.double().abs(), (n_out, n_out), absolute=True), 16, "forward")
    dx = same_bits(lambda: ops.bicubic_resize_grad(dyd, (n_in, n_in)))
    start, _, _ = ops.bicubic_taps_transposed(n_in, n_out)
    longest = int((start[1:] - start[:-1]).max())             # outputs that tap one input index, per dimension
    within(dx, RR.bicubic_grad(dy.double(), (n_in, n_in)), RR.bicubic_grad(dy.double().abs(), (n_in, n_in), absolute=True), longest * longest,
           "input gradient")


def test_bicubic_through_autograd_and_rectangular(ops):
    """BicubicResizeFn: the backward is the gradient kernel; H != W goes through the same tables per dimension"""
    from ddk import autograd as AG
    x = syn.synthetic_normal((2, 3, 12, 20), "bic.rect.x")
    wgt = syn.synthetic_normal((2, 3, 6, 30), "bic.rect.w")
    xd = x.to(DEV).requires_grad_(True)
    y = AG.BicubicResizeFn.apply(xd, (6, 30))
    (y * wgt.to(DEV)).sum().backward()
    within(y, RR.bicubic(x.double(), (6, 30)), RR.bicubic(x.double().abs(), (6, 30), absolute=True), 16, "forward")
    sh, sw = ops.bicubic_taps_transposed(12, 6)[0], ops.bicubic_taps_transposed(20, 30)[0]
    n = int((sh[1:] - sh[:-1]).max()) * int((sw[1:] - sw[:-1]).max())
    within(xd.grad, RR.bicubic_grad(wgt.double(), (12, 20)), RR.bicubic_grad(wgt.double().abs(), (12, 20), absolute=True), n, "input gradient")


# ---------------------------------------------------------------- the two convs
PAIRS = [(1, 1), (1, 3), (3, 3), (3, 8), (8, 8), (5, 32)]


def _ref_all(fn, x, w, b, dy):
    """float64: y, dx, dw, db of the linear op fn(x, w, b) for the upstream gradient dy"""
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = fn(x, w, b)
    gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy)
    return y.detach(), gx, gw, gb


def _check_conv(ops, name, fwd, dgrad, wgrad, ref, x, w, b, dy, n_fwd, n_dgrad):
    x64, w64, b64, dy64 = (t.double() for t in (x, w, b, dy))
    y_r, dx_r, dw_r, db_r = _ref_all(ref, x64, w64, b64, dy64)
    y_m, dx_m, dw_m, db_m = _ref_all(ref, x64.abs(), w64.abs(), b64.abs(), dy64.abs())
    xd, wd, bd, dyd = (t.to(DEV) for t in (x, w, b, dy))
    within(same_bits(lambda: fwd(xd, wd, bd)), y_r, y_m, n_fwd, f"{name} forward")
    within(same_bits(lambda: dgrad(dyd, wd)), dx_r, dx_m, n_dgrad, f"{name} input gradient")
    dw, db = same_bits(lambda: wgrad(xd, dyd))
    n_w = dy.shape[0] * dy.shape[2] * dy.shape[3]           # B Hout Wout
    within(dw, dw_r, dw_m, n_w, f"{name} weight gradient")
    within(db, db_r, db_m, n_w, f"{name} bias gradient")
    assert wgrad(xd, dyd, want_bias=False)[1] is None and torch.equal(wgrad(xd, dyd, want_bias=False)[0], dw)


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (7, 5), (16, 16)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv_small_s2_and_its_gradients(ops, cin, cout, H, W, B):
    tag = f"cs.{cin}.{cout}.{H}.{W}.{B}"
    x = syn.synthetic_normal((B, cin, H, W), tag + ".x")
    w = syn.synthetic_normal((cout, cin, 3, 3), tag + ".w") * (9 * cin) ** -0.5
    b = syn.synthetic_normal((cout,), tag + ".b") * 0.1
    dy = syn.synthetic_normal((B, cout, (H + 1) // 2, (W + 1) // 2), tag + ".dy")
    _check_conv(ops, "conv_small_s2", ops.conv_small_s2, lambda g, wt: ops.conv_small_s2_dgrad(g, wt, (H, W)), ops.conv_small_s2_wgrad,
                RR.conv_down, x, w, b, dy, 9 * cin + 1, 4 * cout)          # an input pixel lies under at most 2 x 2 taps per output channel


@pytest.mark.parametrize("cout,cin", PAIRS)
@pytest.mark.parametrize("H,W", [(1, 1), (3, 2), (8, 8)])
@pytest.mark.parametrize("B", [1, 3])
def test_convt_small_s2_and_its_gradients(ops, cin, cout, H, W, B):
    tag = f"ct.{cin}.{cout}.{H}.{W}.{B}"
    x = syn.synthetic_normal((B, cin, H, W), tag + ".x")
    w = syn.synthetic_normal((cin, cout, 4, 4), tag + ".w") * (4 * cin) ** -0.5
    b = syn.synthetic_normal((cout,), tag + ".b") * 0.1
    dy = syn.synthetic_normal((B, cout, 2 * H, 2 * W), tag + ".dy")
    _check_conv(ops, "convt_small_s2", ops.convt_small_s2, ops.convt_small_s2_dgrad, ops.convt_small_s2_wgrad, RR.conv_up, x, w, b, dy,
                4 * cin + 1, 16 * cout)


def test_widest_filters_fit(ops):
    """32 -> 32 channels: the 4x4 filter fills the 64 KiB of LDS a launch may ask for, to the byte"""
    x = syn.synthetic_normal((1, 32, 3, 2), "wide.x")
    w = syn.synthetic_normal((32, 32, 4, 4), "wide.w") * 128 ** -0.5
    b = syn.synthetic_normal((32,), "wide.b") * 0.1
    dy = syn.synthetic_normal((1, 32, 6, 4), "wide.dy")
    _check_conv(ops, "convt_small_s2", ops.convt_small_s2, ops.convt_small_s2_dgrad, ops.convt_small_s2_wgrad, RR.conv_up, x, w, b, dy,
                4 * 32 + 1, 16 * 32)
    w3 = syn.synthetic_normal((32, 32, 3, 3), "wide.w3") * 288 ** -0.5
    dy3 = syn.synthetic_normal((1, 32, 2, 1), "wide.dy3")
    _check_conv(ops, "conv_small_s2", ops.conv_small_s2, lambda g, wt: ops.conv_small_s2_dgrad(g, wt, (3, 2)), ops.conv_small_s2_wgrad,
                RR.conv_down, x, w3, b, dy3, 9 * 32 + 1, 4 * 32)


def test_convs_through_autograd(ops):
    """ConvSmallS2Fn / ConvTSmallS2Fn hand autograd the kernels' gradients, and skip what is not asked for"""
    from ddk import autograd as AG
    x = syn.synthetic_normal((2, 3, 7, 6), "ag.x")
    w1, b1 = syn.synthetic_normal((5, 3, 3, 3), "ag.w1") * 0.2, syn.synthetic_normal((5,), "ag.b1") * 0.1
    w2, b2 = syn.synthetic_normal((5, 2, 4, 4), "ag.w2") * 0.2, syn.synthetic_normal((2,), "ag.b2") * 0.1
    wgt = syn.synthetic_normal((2, 2, 8, 6), "ag.wgt")
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = AG.ConvTSmallS2Fn.apply(AG.ConvSmallS2Fn.apply(*leaves[:3]), *leaves[3:])
    (y * wgt.to(DEV)).sum().backward()
    ref = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y_r = RR.conv_up(RR.conv_down(*ref[:3]), *ref[3:])
    (y_r * wgt.double()).sum().backward()
    for got, want in zip([y] + [t.grad for t in leaves], [y_r.detach()] + [t.grad for t in ref]):
        assert float((got.detach().cpu().double() - want).abs().max() / want.abs().max()) < 1e-5
    frozen = x.to(DEV).requires_grad_(True)
    AG.ConvSmallS2Fn.apply(frozen, leaves[1].detach(), leaves[2].detach()).sum().backward()
    assert frozen.grad is not None


# ---------------------------------------------------------------- what every entry refuses
def test_every_op_refuses_cpu_and_non_contiguous_tensors(ops):
    from ddk.lib import DDKError
    w3, w4, b = torch.zeros(3, 3, 3, 3), torch.zeros(3, 3, 4, 4), torch.zeros(3)
    calls = {
        "bicubic_resize": lambda t: ops.bicubic_resize(t, (4, 4)),
        "bicubic_resize_grad": lambda t: ops.bicubic_resize_grad(t, (16, 16)),
        "conv_small_s2": lambda t: ops.conv_small_s2(t, w3.to(t.device), b.to(t.device)),
        "conv_small_s2_dgrad": lambda t: ops.conv_small_s2_dgrad(t, w3.to(t.device), (16, 16)),
        "conv_small_s2_wgrad": lambda t: ops.conv_small_s2_wgrad(t, torch.zeros(2, 3, 4, 4, device=t.device)),
        "convt_small_s2": lambda t: ops.convt_small_s2(t, w4.to(t.device), b.to(t.device)),
        "convt_small_s2_dgrad": lambda t: ops.convt_small_s2_dgrad(t, w4.to(t.device)),
        "convt_small_s2_wgrad": lambda t: ops.convt_small_s2_wgrad(t, torch.zeros(2, 3, 16, 16, device=t.device)),
    }
    for name, call in calls.items():
        with pytest.raises(DDKError, match="CPU tensor"):
            call(torch.zeros(2, 3, 8, 8))
        strided = torch.zeros(2, 3, 8, 16, device=DEV)[..., ::2]
        assert not strided.is_contiguous()
        with pytest.raises(DDKError, match="contiguous"):
            call(strided)
        call(strided.contiguous())               # the same call on the packed tensor goes through
    with pytest.raises(DDKError, match="channels"):
        ops.conv_small_s2(torch.zeros(1, 33, 4, 4, device=DEV), torch.zeros(3, 33, 3, 3, device=DEV), b.to(DEV))
    with pytest.raises(DDKError, match="float32"):
        ops.bicubic_resize(torch.zeros(1, 1, 4, 4, device=DEV, dtype=torch.float64), (2, 2))
