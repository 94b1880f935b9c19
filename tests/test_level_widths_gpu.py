"""Level widths that are multiples of 32 but no powers of two -- 96, 160, 192, 224, 320, 384 -- and 512: `Unet` takes any unet_chan % 8 == 0
up to 512 with any unet_dims (the reference's train.py names (1, 2, 3, 4) for 64x64 images), so such levels are ordinary.  They run the
tuned kernels on instantiations and branches that no power-of-two width reaches, and in training the forms of the padded widths with
pitch == C wherever the tuned normalisation backward has no instantiation.

Kernel level: each op against the same expression in float64 on the CPU, at the bar of the existing test of that op (named in each
docstring).  Model level: forward, three ancestral steps and every gradient against oracle.unet_ref on the CPU.
Reference: models/unet/blocks.py:57-60 (LayerNorm), :75-84,105-115 (Block, ResnetBlock), :123-134 (LinearAttention), models/unet/unet.py:74-104."""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, to_nchw, to_nhwc
from test_backward_gpu import rnd
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    from ddk import lib
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


@pytest.fixture(scope="module")
def AG():
    from ddk import autograd as ag
    return ag


def mish64(x):
    return F.mish(x.double())


def grads64(fn, *tensors):
    """grads_cpu of test_backward_gpu.py -- the same cotangent rnd(seed=999), torch autograd on the CPU -- evaluated in float64"""
    leaves = [t.double().clone().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    g = rnd(*out.shape, seed=999)
    gs = torch.autograd.grad(out, leaves, g.double(), allow_unused=True)
    return out.detach(), g, gs


# ---------------------------------------------------------------- 1. channel LayerNorm
@pytest.mark.parametrize("M", [90, 1])
@pytest.mark.parametrize("C", [96, 192, 384, 768, 1024])
def test_chan_layernorm_three_and_four_quads_per_lane(ops, C, M):
    """chan_layernorm_kernel<LPP, VPL> with VPL > 1: <8,3> at C = 96, <16,3> at 192, <32,3> at 384, <64,3> at 768, <64,4> at 1024 (8, 4,
    2, 1, 1 pixels per wave).  M = 3*6*5 = 90 pixels leave a ragged last wave for every one of them (90 = 11*8 + 2 = 22*4 + 2 = 45*2:
    the last workgroup has idle waves), M = 1 a wave with one live lane group.  Bar of test_kernels_gpu.py::test_chan_layernorm (5e-6
    of the output's max), reference in float64."""
    x = (3.0 * rnd(3, C, 6, 5, seed=40) + 1.0) if M == 90 else (3.0 * rnd(1, C, 1, 1, seed=40) + 1.0)
    g, b = 1 + 0.1 * rnd(1, C, 1, 1, seed=41), 0.1 * rnd(1, C, 1, 1, seed=42)
    xd = x.double()
    std = xd.var(dim=1, unbiased=False, keepdim=True).sqrt()
    ref = (xd - xd.mean(dim=1, keepdim=True)) / (std + 1e-5) * g.double() + b.double()
    out = ops.chan_layernorm(to_nhwc(x).to(DEV), g.to(DEV), b.to(DEV))
    e = rel_err(to_nchw(out.cpu()), ref)
    print(f"chan_layernorm C={C} M={M}: {e:.3e}")
    assert e < 5e-6


@pytest.mark.parametrize("C", [160, 224, 320])
def test_chan_layernorm_widths_without_an_instantiation(ops, C):
    """the plan admits every multiple of 32 up to 512; 160, 224, 320, ... have no chan_layernorm_kernel instantiation and run the
    one-wave-per-pixel kernel of the padded widths with pitch == C (an attention block of a unet_chan = 160 model meets it wherever
    the LayerNorm is not folded into to_qkv).  Same bar, same input."""
    x = 3.0 * rnd(3, C, 6, 5, seed=40) + 1.0
    g, b = 1 + 0.1 * rnd(1, C, 1, 1, seed=41), 0.1 * rnd(1, C, 1, 1, seed=42)
    xd = x.double()
    std = xd.var(dim=1, unbiased=False, keepdim=True).sqrt()
    ref = (xd - xd.mean(dim=1, keepdim=True)) / (std + 1e-5) * g.double() + b.double()
    out = ops.chan_layernorm(to_nhwc(x).to(DEV), g.to(DEV), b.to(DEV))
    e = rel_err(to_nchw(out.cpu()), ref)
    print(f"chan_layernorm C={C}: {e:.3e}")
    assert e < 5e-6


# ---------------------------------------------------------------- 2. GroupNorm + Mish (inference kernels)
def gn_nsplit(hw, cpg):
    """norm_act.hip gn_nsplit: statistics splits of the large-slab path, 0 on the register-resident one"""
    n = hw * cpg
    return 0 if n <= 16384 else min(64, max(2, n // 16384))


def gn_apply_fixed(batch, hw, c):
    """groupnorm_mish_ex's choice between gn_apply_kernel<true> (a thread keeps one channel quad) and <false>"""
    per_image4 = hw * (c // 4)
    bpi = max(1, min(-(-4096 // batch), -(-per_image4 // 2048)))
    return (bpi * 256) % (c // 4) == 0


GN_CASES = [  # B, H, W, C, large slab?, gn_apply_kernel<FIXED>
    (2, 4, 4, 96, False, None), (3, 5, 7, 96, False, None), (2, 48, 40, 96, True, False),
    (2, 4, 4, 160, False, None), (3, 5, 7, 160, False, None), (2, 32, 28, 160, True, False),
    (2, 4, 4, 192, False, None), (3, 5, 7, 192, False, None), (2, 32, 24, 192, True, True),
    (2, 4, 4, 384, False, None), (3, 5, 7, 384, False, None), (2, 24, 16, 384, True, True),
]


@pytest.mark.parametrize("B,H,W,C,large,fixed", GN_CASES)
def test_groupnorm_mish_group_rows_of_3_5_6_12_quads(ops, B, H, W, C, large, fixed):
    """ops.groupnorm_mish with 12, 20, 24, 48 channels per group (8 groups): a group's pixel row is 3, 5, 6, 12 float4 units, so
    div_upr divides instead of shifting.
    4x4 and 5x7 maps: gn_mish_resident_kernel<1,256> (48 ... 420 units per slab).
    Large slabs (H*W*C/8 > 16384, two statistics splits each): 256 % (C/4) != 0 at all four widths, so launch_gn_partials takes
    gn_partial_kernel instead of gn_partial_rows_kernel; the apply pass has 23, 18, 18, 18 workgroups per image and
    (workgroups * 256) % (C/4) decides: 48x40 at C = 96 (5888 % 24 = 8) and 32x28 at C = 160 (4608 % 40 = 8) run
    gn_apply_kernel<false>, 32x24 at C = 192 (4608 % 48 = 0) and 24x16 at C = 384 (4608 % 96 = 0) gn_apply_kernel<true>.
    Strided time-shift view and addend as in test_kernels_gpu.py::test_groupnorm_mish, its bar (5e-6), reference in float64."""
    assert (gn_nsplit(H * W, C // 8) >= 2) == large and (gn_nsplit(H * W, C // 8) == 0) == (not large)
    if large:
        assert 256 % (C // 4) != 0 and gn_apply_fixed(B, H * W, C) == fixed
    x = rnd(B, C, H, W, seed=30, scale=2.0) + 0.5
    g, b = 1 + 0.1 * rnd(C, seed=31), 0.1 * rnd(C, seed=32)
    tb = rnd(B, C + 8, seed=33)
    temb = tb[:, 4:4 + C]                               # strided view, like a slice of the time-shift table
    add = rnd(B, C, H, W, seed=34)
    ref0 = mish64(F.group_norm(x.double(), 8, g.double(), b.double(), 1e-5))
    xh = to_nhwc(x).to(DEV)
    out0 = ops.groupnorm_mish(xh, g.to(DEV), b.to(DEV))
    out1 = ops.groupnorm_mish(xh, g.to(DEV), b.to(DEV), temb=tb.to(DEV)[:, 4:4 + C], addend=to_nhwc(add).to(DEV))
    e0 = rel_err(to_nchw(out0.cpu()), ref0)
    e1 = rel_err(to_nchw(out1.cpu()), ref0 + temb.double()[:, :, None, None] + add.double())
    print(f"groupnorm_mish {B}x{H}x{W}x{C}: plain {e0:.3e} shift+addend {e1:.3e}")
    assert e0 < 5e-6 and e1 < 5e-6
    assert torch.equal(out0, ops.groupnorm_mish(xh, g.to(DEV), b.to(DEV)))


# ---------------------------------------------------------------- 3. first conv with partials, GroupNorm from partials
def test_conv_first_and_partials_28_channels_per_group(ops):
    """ops.conv_first at N = 224 (seven 32-channel blocks: the waves of odd parity take three, those of even parity four; 28 channels
    = 7 quads per group) and ops.groupnorm_mish_from_partials on its partials: C/4 = 56 does not divide 256, so a thread of
    gn_apply_parts_kernel<false> changes its channel quad from unit to unit (same_c0 == false).  N = 96 and 160 are cases of
    test_step_edges_gpu.py::test_conv_first_and_partials already; its shape and bars (2e-5 conv, partial means 2e-5 of the output's
    max, M2 1e-4, activation 2e-5), reference in float64, plus a tensor addend."""
    B, H, W, cin, N = 2, 16, 16, 3, 224
    x = rnd(B, cin, H, W, seed=1 + cin) + 0.3
    w = rnd(N, cin, 3, 3, seed=2 + cin, scale=(cin * 9) ** -0.5)
    b = rnd(N, seed=3)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    raw, part, tiles = ops.conv_first(to_nhwc(x).to(DEV), ops.pack_conv_weight_first(w.to(DEV)), b.to(DEV), N)
    assert tiles == H * W // 128
    assert rel_err(to_nchw(raw.cpu()), ref) < 2e-5
    raw2, part2, _ = ops.conv_first(to_nhwc(x).to(DEV), ops.pack_conv_weight_first(w.to(DEV)), b.to(DEV), N)
    assert torch.equal(raw, raw2) and torch.equal(part, part2)
    cpg = N // 8
    t = to_nhwc(ref).reshape(B * tiles, 128, 8, cpg).permute(0, 2, 1, 3).reshape(B * tiles, 8, 128 * cpg)
    mean = t.mean(-1)
    m2 = ((t - mean[..., None]) ** 2).sum(-1)
    assert (part[..., 0].cpu().double() - mean).abs().max() < 2e-5 * ref.abs().max()
    assert rel_err(part[..., 1].cpu(), m2) < 1e-4
    gamma, beta, temb = 1 + 0.1 * rnd(N, seed=5), 0.1 * rnd(N, seed=6), rnd(B, N, seed=7)
    add = rnd(B, N, H, W, seed=8)
    want = mish64(F.group_norm(ref, 8, gamma.double(), beta.double(), 1e-5)) + temb.double()[:, :, None, None]
    out = ops.groupnorm_mish_from_partials(raw, part, tiles, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV))
    assert rel_err(to_nchw(out.cpu()), want) < 2e-5
    out = ops.groupnorm_mish_from_partials(raw, part, tiles, gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV), addend=to_nhwc(add).to(DEV))
    assert rel_err(to_nchw(out.cpu()), want + add.double()) < 2e-5


@pytest.mark.parametrize("N", [96, 160, 224])
def test_groupnorm_res1x1_addend_refuses_widths_it_cannot_index(ops, N):
    """gn_apply_parts_kernel<true> keeps the 1x1 weights of ONE channel quad per thread, which needs 256 % (C/4) == 0:
    groupnorm_mish_parts refuses 96, 160 and 224 (C/4 = 24, 40, 56) before any launch, and the plan does not choose the form
    there (unet_plan.hip first_fast: `upr > 256 || 256 % upr`).  Inputs of test_step_edges_gpu.py::test_groupnorm_res1x1_addend."""
    B, H, W, cin = 2, 16, 16, 3
    x = rnd(B, cin, H, W, seed=21)
    h_in = rnd(B, 4, H, W, seed=22)
    w3 = rnd(N, 4, 3, 3, seed=23, scale=(4 * 9) ** -0.5)
    b3 = rnd(N, seed=24)
    wr, br = rnd(N, cin, 1, 1, seed=25, scale=cin ** -0.5), rnd(N, seed=26)
    gamma, beta = 1 + 0.1 * rnd(N, seed=27), 0.1 * rnd(N, seed=28)
    raw, part, tiles = ops.conv_first(to_nhwc(h_in).to(DEV), ops.pack_conv_weight_first(w3.to(DEV)), b3.to(DEV), N)
    with pytest.raises(ops.L.DDKError, match="C/4 to divide 256"):
        ops.groupnorm_mish_from_partials_res1x1(raw, part, tiles, gamma.to(DEV), beta.to(DEV), to_nhwc(x).to(DEV), wr.to(DEV), br.to(DEV))
    # the two launches the plan runs there instead: res_conv as a tensor addend
    conv = F.conv2d(h_in.double(), w3.double(), b3.double(), padding=1)
    want = mish64(F.group_norm(conv, 8, gamma.double(), beta.double(), 1e-5)) + F.conv2d(x.double(), wr.double(), br.double())
    res = ops.conv(ops.CONV1X1, ops.nchw_to_nhwc(x.to(DEV), 32), ops.pack_conv_weight(wr.to(DEV)), br.to(DEV))
    out = ops.groupnorm_mish_from_partials(raw, part, tiles, gamma.to(DEV), beta.to(DEV), addend=res)
    assert rel_err(to_nchw(out.cpu()), want) < 2e-5


@pytest.mark.parametrize("B", [1, 14])
def test_conv_winograd_groupnorm_partials_64_channels_per_group(ops, B):
    """a 512-wide level on a map of >= 128 pixels: the one-pass Winograd conv leaves per-tile {mean, M2} for groups of 64 channels = 16
    quads -- a whole 64-channel tile is ONE group (B = 1: four m tiles x eight n tiles; the group sum runs over the whole wave), a
    128-channel tile two (B = 14: 56 x 4 = 224 workgroups, the wide tile).  test_kernels_gpu.py::
    test_conv_winograd_groupnorm_partials stops at 32 channels per group; its inputs and bars (2e-5 against torch, 2e-6 against the
    GroupNorm that computes its own statistics), reference in float64."""
    H, W, cin, N = 32, 16, 32, 512
    assert ops.L.load().ddk_conv_gn_partials(B, H, W, cin, N, 8) == H * W // 128
    x = rnd(B, cin, H, W, seed=81)
    w = rnd(N, cin, 3, 3, seed=82, scale=(cin * 9) ** -0.5)
    bias = rnd(N, seed=83, scale=0.3)
    gamma, beta = 1 + rnd(N, seed=84, scale=0.2), rnd(N, seed=85, scale=0.2)
    temb = rnd(B, N, seed=86)
    resid = rnd(B, N, H, W, seed=87)
    h = F.group_norm(F.conv2d(x.double(), w.double(), bias.double(), padding=1), 8, gamma.double(), beta.double(), eps=1e-5)
    want = mish64(h) + temb.double()[:, :, None, None] + resid.double()
    xh = to_nhwc(x).to(DEV)
    wp, wu = ops.pack_conv_weight(w.to(DEV)), ops.pack_conv_weight_wino(w.to(DEV))
    args = (xh, wp, bias.to(DEV), gamma.to(DEV), beta.to(DEV))
    out = ops.conv3x3_groupnorm_mish(*args, temb=temb.to(DEV), addend=to_nhwc(resid).to(DEV), w_wino=wu)
    two = ops.groupnorm_mish(ops.conv(ops.CONV3X3_S1, xh, wp, bias.to(DEV), w_wino=wu), gamma.to(DEV), beta.to(DEV), temb=temb.to(DEV),
                             addend=to_nhwc(resid).to(DEV))
    e, e2 = rel_err(to_nchw(out.cpu()), want), rel_err(out.cpu(), two.cpu())
    print(f"conv + GroupNorm from partials, 64 channels per group, batch {B}: {e:.3e}, against the two launches {e2:.3e}")
    assert e < 2e-5 and e2 < 2e-6
    assert torch.equal(out, ops.conv3x3_groupnorm_mish(*args, temb=temb.to(DEV), addend=to_nhwc(resid).to(DEV), w_wino=wu))


# ---------------------------------------------------------------- 4. attention, pixel-split launch
@pytest.mark.parametrize("H", [8, 16])
@pytest.mark.parametrize("C", [96, 160, 192])
def test_attention_split_three_five_six_chunks(ops, C, H):
    """ops.attention_split_from_x (attn_split_kernel<32> on 8x8, <128> on 16x16 maps) with 3, 5 and 6 K chunks of 32 channels: fewer
    chunks than the four ring slots at C = 96, an odd count and a wrap of the ring at 160, and LayerNorm rows of 6, 10, 12 float4 per
    thread.  Against the expression of test_kernels_gpu.py::test_linattn_small_maps_projection_inside in float64, at the bar of
    test_attention_split_gpu.py (2e-5 for out and ctx); run-to-run bit equal; no wait gives up."""
    B, W = 2, H
    x = rnd(B, C, H, W, seed=62, scale=1.3) + 0.4
    g, b = 1 + rnd(C, seed=63, scale=0.2), rnd(C, seed=64, scale=0.2)
    wq = rnd(384, C, seed=65, scale=C ** -0.5)
    xd = x.double()
    mean = xd.mean(dim=1, keepdim=True)
    std = xd.var(dim=1, unbiased=False, keepdim=True).sqrt()
    xn = (xd - mean) / (std + 1e-5) * g.double()[None, :, None, None] + b.double()[None, :, None, None]
    qkv = F.conv2d(xn, wq.double()[:, :, None, None])
    q, k, v = qkv.reshape(B, 3, 4, 32, H * W).unbind(1)
    ctx_ref = torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v)
    out_ref = torch.einsum("bhde,bhdn->bhen", ctx_ref, q).reshape(B, 128, H, W)
    before = ops.cluster_timeouts()
    out, ctx = ops.attention_split_from_x(to_nhwc(x).to(DEV), wq.to(DEV), g.to(DEV), b.to(DEV))
    out2, ctx2 = ops.attention_split_from_x(to_nhwc(x).to(DEV), wq.to(DEV), g.to(DEV), b.to(DEV))
    e_out, e_ctx = rel_err(to_nchw(out.cpu()), out_ref), rel_err(ctx.cpu(), ctx_ref)
    print(f"split attention {B}x{H}x{W}x{C}: out {e_out:.3e} ctx {e_ctx:.3e}")
    assert ops.cluster_timeouts() == before
    assert e_out <= 2e-5 and e_ctx <= 2e-5
    assert torch.equal(out, out2) and torch.equal(ctx, ctx2)


# ---------------------------------------------------------------- 5. training ops
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (3, 5, 7)])
@pytest.mark.parametrize("C", [96, 192, 384, 512])
def test_groupnorm_mish_backward_other_group_sizes(AG, C, B, H, W):
    """AG.groupnorm_mish, the call of test_backward_gpu.py::test_groupnorm_mish_backward, at 12, 24, 48 and 64 channels per group.
    gn_train_launch takes 4, 8, 16 or 32: these widths run gn_generic_train_kernel<false / true> with pitch == C (thread columns of
    16, 32, 64, 64 channels, of which 4, 8, 16, 0 idle).  That test's bars: forward 5e-6, gradients 3e-5, addend
    gradient 1e-6; its inputs; torch autograd in float64."""
    x = rnd(B, C, H, W, seed=10, scale=2.0) + 0.3
    g, b = 1 + 0.1 * rnd(C, seed=11), 0.1 * rnd(C, seed=12)
    temb, add = rnd(B, C, seed=13), rnd(B, C, H, W, seed=14)
    f = lambda xx, gg, bb, tt, aa: F.mish(F.group_norm(xx, 8, gg, bb, 1e-5)) + tt[:, :, None, None] + aa
    out_ref, go, (gx, gg, gb, gt, ga) = grads64(f, x, g, b, temb, add)
    xd = to_nhwc(x).to(DEV).requires_grad_(True)
    gd, bd = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    td, ad = temb.to(DEV).requires_grad_(True), to_nhwc(add).to(DEV).requires_grad_(True)
    out = AG.groupnorm_mish(xd, gd, bd, temb=td, addend=ad)
    e_fwd = rel_err(to_nchw(out.detach().cpu()), out_ref)
    out.backward(to_nhwc(go).to(DEV))
    errs = dict(x=rel_err(xd.grad.cpu(), to_nhwc(gx)), gamma=rel_err(gd.grad.cpu(), gg), beta=rel_err(bd.grad.cpu(), gb),
                temb=rel_err(td.grad.cpu(), gt), addend=rel_err(ad.grad.cpu(), to_nhwc(ga)))
    print(f"groupnorm_mish backward {B}x{H}x{W}x{C}: forward {e_fwd:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert e_fwd < 5e-6
    assert errs["x"] < 3e-5 and errs["gamma"] < 3e-5 and errs["beta"] < 3e-5 and errs["temb"] < 3e-5 and errs["addend"] < 1e-6


@pytest.mark.parametrize("C", [96, 192, 384])
def test_chan_layernorm_backward_other_widths(AG, C):
    """AG.ChanLayerNormFn, the call of test_backward_gpu.py::test_chan_layernorm_backward: the forward runs chan_layernorm_kernel
    <8,3>, <16,3>, <32,3>; ddk_chan_layernorm_bwd has 32, 64, 128, 256 and 512 only, so the backward runs
    chan_layernorm_generic_bwd_kernel with pitch == C (a lane owns up to 2, 3, 6 channels).  That test's bar (3e-5), its inputs, torch
    autograd in float64; and the Residual's gradient added by the same launch == a separate add, bit for bit, as there."""
    from ddk import ops
    x = rnd(3, C, 6, 5, seed=30, scale=2.0) + 0.5
    g, b = 1 + 0.1 * rnd(1, C, 1, 1, seed=31), 0.1 * rnd(1, C, 1, 1, seed=32)

    def f(a, gg_, bb_):
        std = a.var(dim=1, unbiased=False, keepdim=True).sqrt()
        return (a - a.mean(dim=1, keepdim=True)) / (std + 1e-5) * gg_ + bb_
    out_ref, go, (gx, gg, gb) = grads64(f, x, g, b)
    xd = to_nhwc(x).to(DEV).requires_grad_(True)
    gd, bd = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = AG.ChanLayerNormFn.apply(xd, gd, bd, 1e-5)
    out.backward(to_nhwc(go).to(DEV))
    errs = (rel_err(xd.grad.cpu(), to_nhwc(gx)), rel_err(gd.grad.cpu(), gg), rel_err(bd.grad.cpu(), gb))
    print(f"chan_layernorm backward C={C}: x {errs[0]:.3e} g {errs[1]:.3e} b {errs[2]:.3e}")
    assert max(errs) < 3e-5
    dy, extra = to_nhwc(go).to(DEV), to_nhwc(rnd(3, C, 6, 5, seed=33)).to(DEV)
    dx0, _, _ = ops.chan_layernorm_generic_bwd(xd.detach(), gd.detach(), dy)
    dx1, _, _ = ops.chan_layernorm_generic_bwd(xd.detach(), gd.detach(), dy, addend=extra)
    assert torch.equal(dx0, xd.grad) and torch.equal(dx1, dx0 + extra)


@pytest.mark.parametrize("B,H,W,c0,c1,N", [(3, 5, 7, 64, 0, 96), (2, 8, 8, 128, 64, 192)])
def test_block_backward_other_group_sizes(AG, B, H, W, c0, c1, N):
    """AG.conv_groupnorm_mish -- one `Block` with its time shift -- at 64 -> 96 (odd map: direct conv kernels) and cat(128, 64) -> 192
    (Winograd forward and input gradients): the conv family, then GNMishGenericFn with pitch == C; the conv's bias gradient comes
    from its weight-gradient launches, not from the GroupNorm backward.  Against torch autograd in float64 with the bars of
    test_groupnorm_mish_backward: forward 5e-6, gradients 3e-5."""
    cin = c0 + c1
    x = rnd(B, cin, H, W, seed=1)
    w, bias = rnd(N, cin, 3, 3, seed=2, scale=(cin * 9) ** -0.5), rnd(N, seed=3, scale=0.1)
    g, b, temb = 1 + 0.1 * rnd(N, seed=11), 0.1 * rnd(N, seed=12), rnd(B, N, seed=13)
    f = lambda xx, ww, cb, gg, bb, tt: F.mish(F.group_norm(F.conv2d(xx, ww, cb, padding=1), 8, gg, bb, 1e-5)) + tt[:, :, None, None]
    out_ref, go, (gx, gw, gcb, gg, gb, gt) = grads64(f, x, w, bias, g, b, temb)
    xh = to_nhwc(x).to(DEV)
    x0 = xh[..., :c0].contiguous().requires_grad_(True)
    x1 = xh[..., c0:].contiguous().requires_grad_(True) if c1 else None
    wd, cbd = w.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    gd, bd, td = g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), temb.to(DEV).requires_grad_(True)
    out = AG.conv_groupnorm_mish(x0, wd, cbd, gd, bd, x2=x1, temb=td)
    e_fwd = rel_err(to_nchw(out.detach().cpu()), out_ref)
    out.backward(to_nhwc(go).to(DEV))
    gxh = to_nhwc(gx)
    errs = dict(x=rel_err(x0.grad.cpu(), gxh[..., :c0]), w=rel_err(wd.grad.cpu(), gw), bias=rel_err(cbd.grad.cpu(), gcb),
                gamma=rel_err(gd.grad.cpu(), gg), beta=rel_err(bd.grad.cpu(), gb), temb=rel_err(td.grad.cpu(), gt))
    if c1:
        errs["x2"] = rel_err(x1.grad.cpu(), gxh[..., c0:])
    print(f"Block backward {cin} -> {N}: forward {e_fwd:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert e_fwd < 5e-6
    assert max(errs.values()) < 3e-5
    with pytest.raises(RuntimeError, match="hand-off"):
        AG.conv_groupnorm_mish(x0, wd, cbd, gd, bd, x2=x1, temb=td, give2=AG.GradHandoff())


# ---------------------------------------------------------------- 6 / 7. whole model
MODEL_CASES = [  # chan, dims, cin, B, H, W
    (32, (1, 2, 3, 4), 3, 2, 16, 16),       # levels 32, 64, 96, 128: the reference's 64x64 setting; tuned and generic modules alternate
    (96, (1, 2), 3, 3, 8, 12),              # 96, 192 on a map that is not square; the first and the final Block are 96 wide
    (64, (1, 3, 6), 8, 2, 16, 16),          # 64, 192, 384
    (128, (1, 4), 3, 1, 8, 8),              # 128, 512: LayerNorm tuned, GroupNorm not (64 channels per group)
    (160, (1, 2), 1, 2, 8, 8),              # 160, 320: neither has a chan_layernorm_kernel instantiation
]


def model_cfg(chan, dims, cin, H, dropout=0.0):
    return dict(unet_chan=chan, unet_in=cin, unet_dims=dims, unet_dropout=dropout, image_size=H, T=100, loss_type="simple",
                beta_schedule="linear", loss_flat="sum")


@functools.lru_cache(maxsize=None)
def oracle_case(chan, dims, cin, B, H, W):
    """weights, input, and the CPU oracle's output and gradients (input and EVERY parameter) for one configuration: computed once,
    shared by the forward and the training test, never modified"""
    from models import Unet
    from oracle import unet_ref as U
    cfg = model_cfg(chan, dims, cin, H)
    sd = syn.fill_state_dict(Unet(cfg).state_dict(), 91)
    x = syn.synthetic_normal((B, cin, H, W), "lvl.x")
    t = torch.tensor([5, 40, 99, 0, 77][:B])
    wgt = syn.synthetic_normal((B, cin, H, W), "lvl.w")
    ref_sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    out_ref = U.unet_forward(ref_sd, cfg, xr, t)
    (out_ref * wgt).sum().backward()
    grads = {k: v.grad for k, v in ref_sd.items()}
    return cfg, sd, x, t, wgt, out_ref.detach(), xr.grad, grads


def make_model(cfg, sd):
    from models import Unet
    model = Unet(cfg)
    model.load_state_dict(sd)
    return model.to(DEV)


@pytest.mark.parametrize("chan,dims,cin,B,H,W", MODEL_CASES)
def test_unet_forward_and_sampler_vs_oracle(chan, dims, cin, B, H, W):
    """the plan at level widths of 96, 160, 192, 320, 384 and 512: no Winograd where N % 64 != 0 (96, 160 -> direct conv kernels),
    no one-launch Block where a group has 12, 20, 24, 40, 48 or 64 channels (-> conv, then the register-resident GroupNorm with 3, 5, 6,
    10, 12, 16 units per row, summing the conv's split-K slabs where it left them), chan_layernorm_kernel<.,3> or the generic
    LayerNorm where the projection does not fold it.  Against oracle.unet_ref at the bars of
    test_unet_gpu.py::test_unet_widths_that_are_not_multiples_of_32_vs_oracle: forward 5e-5 of the output's max, run-to-run bit equal,
    three ancestral steps (square maps) within 1e-4.  (From x_T ~ N(0, 1) at T = 100 the clip of x_0 to [-1, 1] saturates for part of the
    pixels, in the one-image 8x8 case for all of them: there the steps check the update's arithmetic and the forward check the model.)"""
    from models import DDPM
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    cfg, sd, x, t, _, ref, _, _ = oracle_case(chan, dims, cin, B, H, W)
    u = make_model(cfg, sd).eval()
    with torch.no_grad():
        y = u(x.to(DEV), t.to(DEV))
        assert torch.equal(y, u(x.to(DEV), t.to(DEV)))
    e = rel_err(y.cpu(), ref)
    print(f"unet forward chan {chan} dims {dims}: {e:.3e}")
    assert e < 5e-5
    if H == W:
        m = DDPM(cfg, u, DEV, cin).to(DEV).eval()
        noise = torch.stack([syn.synthetic_normal((B, cin, H, W), f"lvl.n{k}") for k in range(3)])
        got = m.p_sample_loop((B, cin, H, W), early_stop=97, x_T=x, noise=noise).cpu()
        buf = D.schedule_buffers("linear", 100)
        with torch.no_grad():
            want, _ = D.p_sample_loop(buf, lambda a, b: U.unet_forward(sd, cfg, a, b), x, list(noise), 100, 97)
        e3 = float((got - want).abs().max())
        print(f"three ancestral steps chan {chan} dims {dims}: {e3:.3e}")
        assert e3 < 1e-4


@pytest.mark.parametrize("chan,dims,cin,B,H,W", MODEL_CASES)
def test_unet_training_at_other_level_widths(chan, dims, cin, B, H, W):
    """loss.backward() through unet_forward_autograd where ResnetBlocks and attention blocks of tuned widths (hand-offs, slab links)
    and of the others (generic forms, pitch == C, autograd adds) alternate: the output, the input gradient and the gradient of EVERY
    parameter against torch-CPU autograd of oracle.unet_ref, at the bars of
    test_generic_width_train_gpu.py::test_unet_training_at_widths_that_are_not_multiples_of_32 (forward 5e-5, gradients 2e-4 of each
    tensor's max); and the eval-mode plan agrees with the training forward (5e-5)."""
    cfg, sd, x, t, wgt, out_ref, gx, grads = oracle_case(chan, dims, cin, B, H, W)
    model = make_model(cfg, sd).train()
    xd = x.to(DEV).requires_grad_(True)
    out = model(xd, t.to(DEV))
    e = rel_err(out.detach().cpu(), out_ref)
    (out * wgt.to(DEV)).sum().backward()
    ex = rel_err(xd.grad.cpu(), gx)
    errs = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        errs[k] = rel_err(p.grad.cpu(), grads[k])
    worst = max(errs, key=errs.get)
    print(f"unet training chan {chan} dims {dims}: forward {e:.3e} input gradient {ex:.3e} worst parameter {worst} {errs[worst]:.3e}")
    assert e < 5e-5 and ex < 2e-4
    assert len(errs) == len(grads)
    for k, v in errs.items():
        assert v < 2e-4, (k, v)
    model.eval()
    with torch.no_grad():
        y_plan = model(x.to(DEV), t.to(DEV))
    assert rel_err(y_plan.cpu(), out.detach().cpu()) < 5e-5


def test_unet_dropout_trains_at_other_level_widths():
    """unet_dropout = 0.1 at levels of 32, 64, 96, 128: the tuned and the generic GroupNorm draw their masks from the same per-forward
    seed and regenerate them in the backward.  No torch counterpart for the mask: everything finite, the same bits under the same
    seed, other bits under another seed and without Dropout."""
    chan, dims, cin, B, H, W = MODEL_CASES[0]
    cfg, sd, x, t, wgt, _, _, _ = oracle_case(chan, dims, cin, B, H, W)
    model = make_model(model_cfg(chan, dims, cin, H, dropout=0.1), sd).train()

    def run(seed):
        torch.manual_seed(seed)
        model.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        out = model(xd, t.to(DEV))
        (out * wgt.to(DEV)).sum().backward()
        return [out.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in model.parameters()]
    a, b, c = run(7), run(7), run(8)
    assert all(bool(torch.isfinite(v).all()) for v in a)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    model.eval()
    with torch.no_grad():
        assert not torch.equal(a[0], model(x.to(DEV), t.to(DEV)))
