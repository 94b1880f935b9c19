"""Every statistics path of the norm, attention and optimiser kernels on the input regimes of tests/regimes_ref.py: variance below and
about eps, |mean| >> std, constant groups, groups of different regimes side by side, k logits that overflow or underflow exp without
the maximum, gradients below Adam's eps.  References are the plain restatements of regimes_ref.py in fp64; the bar of a path is
max(the bar its older test uses, 8 x the fp32 restatement's error), tests/test_regimes_cpu.py shows what those bars catch.

The conv-fused paths get weights that copy channels (centre tap, 0 / 1, no bias), so the regime reaches the normalisation unchanged."""
import functools

import pytest
import torch
import torch.nn.functional as F

import regimes_ref as R
from oracle import diffusion_ref as D
from oracle import train_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NORM, FUSED, BWD = 5e-6, 2e-5, 3e-5          # the bars of the older tests: norms, conv-fused norms and contractions, backward


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


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def dev(*ts):
    out = tuple(None if t is None else t.to(DEV) for t in ts)
    return out if len(out) > 1 else out[0]


def hold(name, e, limit):
    print(f"{name}: {e:.3e} (bar {limit:.3e})")
    assert e <= limit, f"{name}: {e:.3e} > {limit:.3e}"


# ------------------------------------------------------------------ GroupNorm forward
@functools.lru_cache(maxsize=None)
def gn_case(regime, B, C, H, W, src_c=None):
    """the tensor GroupNorm sees (NCHW; with src_c: src_c channels of the regime, each copied C / src_c times -- group j of the source
    is group j of the copy), parameters, extras and the fp64 references without and with the extras"""
    src = R.gn_input(regime, B, src_c or C, H, W)
    y = src.repeat_interleave(C // (src_c or C), dim=1)
    g, b, temb = R.gn_params(C, B)
    add = R.rnd(B, C, H, W, seed=2030)
    ref0 = R.gn_mish(*R.d(y, g, b))
    return dict(src=src, y=y, g=g, b=b, temb=temb, add=add, ref0=ref0, ref1=ref0 + temb.double()[:, :, None, None] + add.double())


def check_gn(name, regime, case, out0, out1=None, existing=FUSED):
    """out0 / out1: NCHW results on the CPU without / with (shift, residual).  const: mish(beta) (+ extras) to 2e-6 absolute."""
    for tag, out, ref in (("", out0, case["ref0"]), (" +shift +res", out1, case["ref1"])):
        if out is None:
            continue
        assert bool(torch.isfinite(out).all()), f"{name} {regime}{tag}: not finite"
        if regime == "const":
            hold(f"{name} const{tag} (abs)", R.abs_err(out, ref), R.MISH_ABS_BAR)
        else:
            hold(f"{name} {regime}{tag}", R.err(out, ref), R.bar(existing, R.E32_GN[regime]))


def copy_weight(N, cin):
    """OIHW 3x3: output channel n copies input channel n // (N / cin)"""
    w = torch.zeros(N, cin, 3, 3)
    w[torch.arange(N), torch.arange(N) // (N // cin), 1, 1] = 1.0
    return w


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("B,H,W,C", [(2, 8, 8, 32), (3, 5, 7, 64), (2, 65, 64, 32)])
def test_groupnorm_mish(ops, regime, B, H, W, C):
    """ddk_groupnorm_mish: register-resident, ragged, and the Welford large-slab path (65 * 64 * 4 > 16384 elements per group)"""
    assert (ops.L.load().ddk_groupnorm_workspace_bytes(B, H * W, C, 8) != 0) == (H * W * C // 8 > 16384)
    c = gn_case(regime, B, C, H, W)
    x, g, b, temb, add = dev(nhwc(c["y"]), c["g"], c["b"], c["temb"], nhwc(c["add"]))
    out0 = ops.groupnorm_mish(x, g, b)
    out1 = ops.groupnorm_mish(x, g, b, temb=temb, addend=add)
    check_gn(f"groupnorm_mish {B}x{H}x{W}x{C}", regime, c, nchw(out0.cpu()), nchw(out1.cpu()), existing=NORM)


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("B,H,W,cin,N,wino", [(1, 32, 16, 32, 64, True), (2, 8, 8, 64, 64, False)])
def test_conv3x3_groupnorm_mish(ops, regime, B, H, W, cin, N, wino):
    """two launches: the Winograd conv's {mean, M2} tile partials merged by the GroupNorm kernel; and (no Winograd filter) the split-K
    slabs summed by the GroupNorm kernel's load"""
    lib = ops.L.load()
    if wino:
        assert lib.ddk_conv_wino_splits(B, H, W, cin, N) > 0 and lib.ddk_conv_gn_partials(B, H, W, cin, N, 8) == H * W // 128
    else:
        assert lib.ddk_conv_splits(ops.CONV3X3_S1, B, H, W, cin, N) > 1 and lib.ddk_groupnorm_workspace_bytes(B, H * W, N, 8) == 0
    c = gn_case(regime, B, N, H, W, src_c=cin)
    w = copy_weight(N, cin).to(DEV)
    x, g, b, temb, add = dev(nhwc(c["src"]), c["g"], c["b"], c["temb"], nhwc(c["add"]))
    args = (x, ops.pack_conv_weight(w), torch.zeros(N, device=DEV), g, b)
    wu = ops.pack_conv_weight_wino(w) if wino else None
    out0 = ops.conv3x3_groupnorm_mish(*args, w_wino=wu)
    out1 = ops.conv3x3_groupnorm_mish(*args, temb=temb, addend=add, w_wino=wu)
    check_gn(f"conv3x3_groupnorm_mish {'partials' if wino else 'slabs'}", regime, c, nchw(out0.cpu()), nchw(out1.cpu()))


@pytest.mark.parametrize("regime", R.GN_REGIMES)
def test_conv_first_partials_res1x1_and_final_tail(ops, regime):
    """the first conv's {mean, M2} partials through ddk_groupnorm_mish_partials, ..._res1x1 and ddk_final_tail (eps_hat and the ancestral
    update in the same launch)"""
    B, H, W, cin, N = 2, 16, 16, 8, 32
    c = gn_case(regime, B, N, H, W, src_c=cin)
    g, b, temb = dev(c["g"], c["b"], c["temb"])
    raw, part, tiles = ops.conv_first(nhwc(c["src"]).to(DEV), ops.pack_conv_weight_first(copy_weight(N, cin).to(DEV)),
                                      torch.zeros(N, device=DEV), N)
    assert tiles == 2 and torch.equal(nchw(raw.cpu()), c["y"]), "the copying conv is exact"
    out0 = ops.groupnorm_mish_from_partials(raw, part, tiles, g, b)
    out1 = ops.groupnorm_mish_from_partials(raw, part, tiles, g, b, temb=temb, addend=nhwc(c["add"]).to(DEV))
    check_gn("conv_first + groupnorm_mish_from_partials", regime, c, nchw(out0.cpu()), nchw(out1.cpu()))
    # the residual 1x1 conv of a 3-channel tensor formed inside the GroupNorm launch
    rx, rw, rb = R.rnd(B, 3, H, W, seed=2040), R.rnd(N, 3, 1, 1, seed=2041, scale=3 ** -0.5), R.rnd(N, seed=2042)
    out2 = ops.groupnorm_mish_from_partials_res1x1(raw, part, tiles, g, b, nhwc(rx).to(DEV), rw.to(DEV), rb.to(DEV), temb=temb)
    ref2 = c["ref0"] + c["temb"].double()[:, :, None, None] + F.conv2d(*R.d(rx, rw, rb))
    assert bool(torch.isfinite(out2).all())
    if regime == "const":
        hold("res1x1 const (abs)", R.abs_err(nchw(out2.cpu()), ref2), R.MISH_ABS_BAR + 2e-5 * float(ref2.abs().max()))   # + the 1x1 conv's bar
    else:
        hold(f"res1x1 {regime}", R.err(nchw(out2.cpu()), ref2), R.bar(FUSED, R.E32_GN[regime]))
    # final tail: GroupNorm + Mish + projection to 3 channels
    w, bw = R.tail_proj(N)
    ref3 = R.gn_tail(*R.d(c["y"], c["g"], c["b"], w, bw))
    eps = ops.final_tail(raw, part, tiles, g, b, w.to(DEV), bw.to(DEV))
    assert bool(torch.isfinite(eps).all())
    hold(f"final_tail eps {regime}", R.err(nchw(eps.cpu()), ref3), R.bar(FUSED, R.E32_GN_TAIL.get(regime, 0.0)))
    buf = D.schedule_buffers("linear", 1000)
    tb = {k: buf[v].to(DEV) for k, v in (("c_recip", "sqrt_recip_alphas_cumprod"), ("c_recipm1", "sqrt_recipm1_alphas_cumprod"),
                                         ("c1", "posterior_mean_coef1"), ("c2", "posterior_mean_coef2"))}
    tb["sigma"] = torch.exp(0.5 * buf["posterior_log_variance_clipped"]).to(DEV)
    x0, z, t = R.rnd(B, H, W, 3, seed=2043, scale=1.5), R.rnd(B, H, W, 3, seed=2044), torch.tensor([0, 999])
    xa = x0.to(DEV).clone()
    eps2 = ops.final_tail(raw, part, tiles, g, b, w.to(DEV), bw.to(DEV), x=xa, t=t.to(DEV), tables=tb, noise=z.to(DEV))
    # the update is p_sample_update_ (bit-exact against the oracle in test_kernels_gpu.py) on the eps_hat of the same launch
    assert torch.equal(eps2, eps) and bool(torch.isfinite(xa).all())
    assert torch.equal(xa, ops.p_sample_update_(x0.to(DEV).clone(), eps, t.to(DEV), noise=z.to(DEV), **tb))


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("B,H,W,cin,N", [(2, 4, 4, 32, 64), (8, 2, 2, 32, 64), (2, 8, 8, 32, 64)])
def test_conv3x3_gn_mish_one_launch(ops, regime, B, H, W, cin, N):
    """the image-local one-launch Blocks: 4x4 direct, 2x2 (four images share a 16-row block), 8x8 Winograd"""
    lib = ops.L.load()
    wl = H * W == 64
    assert (lib.ddk_conv3x3_gn_mish_wino_ok if wl else lib.ddk_conv3x3_gn_mish_ok)(H, W, cin, cin, N, 8)
    c = gn_case(regime, B, N, H, W, src_c=cin)
    w = copy_weight(N, cin).to(DEV)
    fn, wp = (ops.conv3x3_gn_mish_wino, ops.pack_conv_weight_wino_local(w)) if wl else (ops.conv3x3_gn_mish, ops.pack_conv_weight_local(w))
    x, g, b, temb, add = dev(nhwc(c["src"]), c["g"], c["b"], c["temb"], nhwc(c["add"]))
    out0 = fn(x, wp, torch.zeros(N, device=DEV), g, b)
    out1 = fn(x, wp, torch.zeros(N, device=DEV), g, b, temb=temb, addend=add)
    check_gn(f"conv3x3_gn_mish{'_wino' if wl else ''} {B}x{H}x{W}", regime, c, nchw(out0.cpu()), nchw(out1.cpu()))


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("H", [4, 8])
def test_conv3x3_gn_mish_slabs(ops, regime, H):
    """the one-launch Blocks on an input still in split-K form: two slabs whose fp32 sum is the regime exactly (its high and low bits)"""
    B, C = 2, 256
    c = gn_case(regime, B, C, H, H)
    x = nhwc(c["y"])
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    lo = x - hi
    assert torch.equal(hi + lo, x)
    w = copy_weight(C, C).to(DEV)
    wp = ops.pack_conv_weight_local(w) if H == 4 else ops.pack_conv_weight_wino_local(w)
    g, b, temb = dev(c["g"], c["b"], c["temb"])
    zero = torch.zeros(C, device=DEV)
    slabs = torch.stack([hi, lo]).to(DEV).contiguous()
    a_sl = torch.stack([nhwc(c["add"]), torch.zeros_like(x)]).to(DEV).contiguous()
    out0 = ops.conv3x3_gn_mish_slabs(slabs, zero, wp, zero, g, b)
    out1 = ops.conv3x3_gn_mish_slabs(slabs, zero, wp, zero, g, b, temb=temb, addend_slabs=a_sl, addend_bias=zero)
    check_gn(f"conv3x3_gn_mish_slabs {H}x{H}", regime, c, nchw(out0.cpu()), nchw(out1.cpu()))


@pytest.mark.parametrize("regime", R.GN_REGIMES)
def test_conv3x3_gn_mish_cluster(ops, regime):
    """GroupNorm finished inside the Winograd conv launch, tile statistics exchanged between the workgroups of an image"""
    B, N, H, W = R.CLUSTER_SHAPE
    if ops.L.load().ddk_conv3x3_gn_mish_cluster_ok(B, H, W, N, N, 8) <= 0:
        pytest.skip("shape not eligible on this device")
    c = gn_case(regime, B, N, H, W)
    wu = ops.pack_conv_weight_wino(copy_weight(N, N).to(DEV))
    x, g, b, temb, add = dev(nhwc(c["y"]), c["g"], c["b"], c["temb"], nhwc(c["add"]))
    before = ops.cluster_timeouts()
    out0 = ops.conv3x3_gn_mish_cluster(x, wu, torch.zeros(N, device=DEV), g, b)
    out1 = ops.conv3x3_gn_mish_cluster(x, wu, torch.zeros(N, device=DEV), g, b, temb=temb, addend=add)
    torch.cuda.synchronize()
    assert ops.cluster_timeouts() == before
    check_gn("conv3x3_gn_mish_cluster", regime, c, nchw(out0.cpu()), nchw(out1.cpu()))


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("hw", [16, 64])
def test_level_chain_conv3(regime, hw):
    """the level chain's CONV3 op (conv3x3 + GroupNorm + Mish + time shift), alone, B = 2"""
    from ddk import ops
    from test_level_chain_gpu import CONV3, ChainOp, _p, pack3, run_chain
    B, C, S = 2, 256, (4 if hw == 16 else 8)
    c = gn_case(regime, B, C, S, S)
    wp = pack3(copy_weight(C, C).to(DEV), hw)
    x, g, b, temb = dev(nhwc(c["y"]), c["g"], c["b"], c["temb"])
    zero = torch.zeros(C, device=DEV)
    out0, out1 = torch.empty((B, S, S, C), device=DEV), torch.empty((B, S, S, C), device=DEV)
    run_chain([ChainOp(_p(x), None, _p(wp), _p(zero), _p(g), _p(b), _p(out0), C, 0, CONV3, 0, -1, C)], hw, B, temb)
    run_chain([ChainOp(_p(x), None, _p(wp), _p(zero), _p(g), _p(b), _p(out1), C, 0, CONV3, 0, 0, C)], hw, B, temb)
    assert bool(torch.isfinite(out1).all())
    check_gn(f"level chain CONV3 hw {hw}", regime, c, nchw(out0.cpu()))
    ref = c["ref0"] + c["temb"].double()[:, :, None, None]
    if regime == "const":
        hold(f"level chain CONV3 hw {hw} const +shift (abs)", R.abs_err(nchw(out1.cpu()), ref), R.MISH_ABS_BAR)
    else:
        hold(f"level chain CONV3 hw {hw} {regime} +shift", R.err(nchw(out1.cpu()), ref), R.bar(FUSED, R.E32_GN[regime]))


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("B,H,W,C", [(2, 8, 8, 32), (3, 5, 7, 64), (2, 65, 64, 32)])
def test_groupnorm_mish_train(ops, regime, B, H, W, C):
    """the training forward: register-resident, ragged (a group size that is no power of two), and the large-slab form"""
    assert ops.gn_train_resident(B, H * W, C) == (H * W * C // 8 <= 16384)
    c = gn_case(regime, B, C, H, W)
    x, g, b, temb, add = dev(nhwc(c["y"]), c["g"], c["b"], c["temb"], nhwc(c["add"]))
    out0 = ops.groupnorm_mish_train(x, g, b)
    out1 = ops.groupnorm_mish_train(x, g, b, temb=temb, addend=add)
    check_gn(f"groupnorm_mish_train {B}x{H}x{W}x{C}", regime, c, nchw(out0.cpu()), nchw(out1.cpu()), existing=NORM)


def pad_c(t, cp):
    out = torch.zeros((*t.shape[:-1], cp))
    out[..., :t.shape[-1]] = t
    return out


@pytest.mark.parametrize("regime", R.GN_REGIMES)
def test_groupnorm_mish_generic_train(ops, regime):
    """C = 24: three channels per group in 32-pitched rows"""
    B, H, W, C = 2, 8, 8, 24
    c = gn_case(regime, B, C, H, W)
    x, add = pad_c(nhwc(c["y"]), 32).to(DEV), pad_c(nhwc(c["add"]), 32).to(DEV)
    g, b, temb = dev(c["g"], c["b"], c["temb"])
    out0 = ops.groupnorm_mish_generic_train(x, g, b)
    out1 = ops.groupnorm_mish_generic_train(x, g, b, temb=temb, addend=add)
    assert float(out0[..., C:].abs().max()) == 0.0 and float(out1[..., C:].abs().max()) == 0.0
    check_gn("groupnorm_mish_generic_train", regime, c, nchw(out0[..., :C].cpu()), nchw(out1[..., :C].cpu()), existing=NORM)


# ------------------------------------------------------------------ GroupNorm backward
@functools.lru_cache(maxsize=None)
def gn_bwd_case(regime, B, C, H, W, src_c=None):
    c = gn_case(regime, B, C, H, W, src_c)
    dy = R.gn_dy(B, C, H, W)
    return c, dy, R.gn_grads(*R.d(c["y"], c["g"], c["b"], dy))


def check_gn_bwd(name, regime, got, want, existing=BWD):
    for i, what in enumerate(("dx", "dgamma", "dbeta")):
        assert bool(torch.isfinite(got[i]).all()), f"{name} {regime} {what}: not finite"
        if regime == "const" and what == "dgamma":        # xn == 0 exactly
            hold(f"{name} const dgamma (abs)", R.abs_err(got[i], want[i]), 0.0)
        else:
            hold(f"{name} {regime} {what}", R.err(got[i], want[i]), R.bar(existing, R.E32_GN_BWD[regime][i]))


@pytest.mark.parametrize("regime", R.GN_BWD_REGIMES)
@pytest.mark.parametrize("B,H,W,C", [(2, 8, 8, 32), (3, 5, 7, 64), (2, 48, 48, 128)])
def test_groupnorm_mish_backward(AG, regime, B, H, W, C):
    """AG.groupnorm_mish: register-resident, ragged, and the streamed form (36864 elements per group, 2 splits)"""
    c, dy, want = gn_bwd_case(regime, B, C, H, W)
    x, g, b = (t.requires_grad_(True) for t in dev(nhwc(c["y"]), c["g"], c["b"]))
    out = AG.groupnorm_mish(x, g, b)
    out.backward(nhwc(dy).to(DEV))
    check_gn(f"AG.groupnorm_mish {B}x{H}x{W}x{C}", regime, c, nchw(out.detach().cpu()), existing=NORM)
    check_gn_bwd(f"AG.groupnorm_mish {B}x{H}x{W}x{C}", regime, (nchw(x.grad.cpu()), g.grad.cpu(), b.grad.cpu()), want)


@pytest.mark.parametrize("regime", R.GN_BWD_REGIMES)
def test_conv_groupnorm_mish_backward(AG, regime):
    """AG.conv_groupnorm_mish with the copying conv: dgamma, dbeta as above; dx is the sum of the copies' gradients"""
    B, H, W, cin, N = 2, 8, 8, 32, 64
    c, dy, want = gn_bwd_case(regime, B, N, H, W, src_c=cin)
    x, g, b = (t.requires_grad_(True) for t in dev(nhwc(c["src"]), c["g"], c["b"]))
    out = AG.conv_groupnorm_mish(x, copy_weight(N, cin).to(DEV), torch.zeros(N, device=DEV), g, b)
    out.backward(nhwc(dy).to(DEV))
    check_gn("AG.conv_groupnorm_mish", regime, c, nchw(out.detach().cpu()))
    dx = want[0].reshape(B, cin, N // cin, H, W).sum(dim=2)
    check_gn_bwd("AG.conv_groupnorm_mish", regime, (nchw(x.grad.cpu()), g.grad.cpu(), b.grad.cpu()), (dx, want[1], want[2]))


@pytest.mark.parametrize("regime", R.GN_BWD_REGIMES)
def test_groupnorm_generic_backward(ops, regime):
    B, H, W, C = 2, 8, 8, 24
    c, dy, want = gn_bwd_case(regime, B, C, H, W)
    x, dyp = pad_c(nhwc(c["y"]), 32).to(DEV), pad_c(nhwc(dy), 32).to(DEV)
    dx, _, sums = ops.groupnorm_mish_generic_bwd(x, c["g"].to(DEV), c["b"].to(DEV), dyp)
    assert float(dx[..., C:].abs().max()) == 0.0
    check_gn_bwd("groupnorm_mish_generic_bwd", regime, (nchw(dx[..., :C].cpu()), sums[0].cpu(), sums[1].cpu()), want, existing=2e-5)


# ------------------------------------------------------------------ channel LayerNorm
def ln_rows(regime, C):
    """90 pixels as a (3, 6, 5, C) map"""
    return R.ln_input(regime, 90, C)


def check_ln(name, regime, out, x, g, b):
    assert bool(torch.isfinite(out).all()), f"{name} {regime}: not finite"
    if regime == "const":
        assert torch.equal(out, b.expand_as(out)), f"{name} const: {float((out - b).abs().max()):.3e} off b"
        print(f"{name} const: == b")
    else:
        hold(f"{name} {regime}", R.err(out, R.chan_layernorm(*R.d(x, g, b))), R.bar(NORM, R.E32_LN[regime]))


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("C", [32, 256])
def test_chan_layernorm(ops, regime, C):
    x = ln_rows(regime, C)
    g, b = R.ln_params(C)
    out = ops.chan_layernorm(x.reshape(3, 6, 5, C).to(DEV), g.to(DEV), b.to(DEV))
    check_ln(f"chan_layernorm C {C}", regime, out.cpu().reshape(90, C), x, g, b)


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("C", [24, 200])
def test_chan_layernorm_generic(ops, regime, C):
    x = ln_rows(regime, C)
    g, b = R.ln_params(C)
    cp = ops.pad32(C)
    out = ops.chan_layernorm_generic(pad_c(x, cp).reshape(3, 6, 5, cp).to(DEV), g.to(DEV), b.to(DEV)).cpu().reshape(90, cp)
    assert float(out[:, C:].abs().max()) == 0.0
    check_ln(f"chan_layernorm_generic C {C}", regime, out[:, :C], x, g, b)


@pytest.mark.parametrize("regime", R.LN_REGIMES)
def test_conv1x1_ws_with_layernorm(ops, regime):
    """to_qkv behind the LayerNorm in the folded form r (W o g) x - r mean (W g) + W b: held to that form's own fp32 error"""
    M, C, N = 2048, 128, 384
    x = R.ln_input(regime, M, C)
    g, b = R.ln_params(C)
    w = R.ln_weight(N, C)
    assert ops.L.load().ddk_conv1x1_ws_ok(M, C, N)
    out = ops.conv1x1_ws(x.reshape(2, 32, 32, C).to(DEV), (w * g).contiguous().to(DEV), None, None,
                         ((w @ g).contiguous().to(DEV), (w @ b).contiguous().to(DEV)))
    assert bool(torch.isfinite(out).all())
    hold(f"conv1x1_ws(ln) {regime}", R.err(out.cpu().reshape(M, N), R.ln_linear(*R.d(x, g, b, w))), R.bar(FUSED, R.E32_LN_FOLDED[regime]))


def check_ln_bwd(name, regime, got, want, existing):
    for i, what in enumerate(("dx", "dg", "db")):
        assert bool(torch.isfinite(got[i]).all()), f"{name} {regime} {what}: not finite"
        if regime == "const" and what == "dg":
            hold(f"{name} const dg (abs)", R.abs_err(got[i], want[i]), 0.0)
        else:
            hold(f"{name} {regime} {what}", R.err(got[i], want[i]), R.bar(existing, R.E32_LN_BWD[regime][i]))


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("C", [32, 256])
def test_chan_layernorm_backward(ops, regime, C):
    x, dy = ln_rows(regime, C), R.ln_dy(90, C)
    g, b = R.ln_params(C)
    want = R.ln_grads(*R.d(x, g, b, dy))
    xd, gd, dyd = x.reshape(3, 6, 5, C).to(DEV), g.to(DEV), dy.reshape(3, 6, 5, C).to(DEV)
    dx, dg, db = ops.chan_layernorm_bwd(xd, gd, dyd)
    check_ln_bwd(f"chan_layernorm_bwd C {C}", regime, (dx.cpu().reshape(90, C), dg.cpu(), db.cpu()), want, BWD)
    extra = R.rnd(3, 6, 5, C, seed=3400).to(DEV)
    dx1, dg1, db1 = ops.chan_layernorm_bwd(xd, gd, dyd, addend=extra)
    assert torch.equal(dx1, dx + extra) and torch.equal(dg1, dg) and torch.equal(db1, db)


@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("C", [24, 200])
def test_chan_layernorm_generic_backward(ops, regime, C):
    x, dy = ln_rows(regime, C), R.ln_dy(90, C)
    g, b = R.ln_params(C)
    want = R.ln_grads(*R.d(x, g, b, dy))
    cp = ops.pad32(C)
    dx, dg, db = ops.chan_layernorm_generic_bwd(pad_c(x, cp).reshape(3, 6, 5, cp).to(DEV), g.to(DEV), pad_c(dy, cp).reshape(3, 6, 5, cp).to(DEV))
    dx = dx.cpu().reshape(90, cp)
    assert float(dx[:, C:].abs().max()) == 0.0
    check_ln_bwd(f"chan_layernorm_generic_bwd C {C}", regime, (dx[:, :C], dg.cpu(), db.cpu()), want, 2e-5)


# ------------------------------------------------------------------ linear attention
@functools.lru_cache(maxsize=None)
def qkv_ref(regime, B, H, W):
    q = R.qkv_input(regime, B, H, W)
    return q, R.linattn(q.double())


@pytest.mark.parametrize("regime", R.K_REGIMES)
@pytest.mark.parametrize("B,H,W", R.QKV_SHAPES)
def test_linattn(ops, regime, B, H, W):
    q, (out_ref, ctx_ref) = qkv_ref(regime, B, H, W)
    runs = [("", {})] + ([("fused_up_to=64 ", dict(fused_up_to=64))] if 64 < H * W <= 256 else [])
    for tag, kw in runs:
        out, ctx = ops.linattn(nhwc(q).to(DEV), 4, **kw)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ctx).all())
        hold(f"linattn {tag}{B}x{H}x{W} {regime} ctx", R.err(ctx.cpu(), ctx_ref), R.bar(1e-5, R.E32_ATTN))
        hold(f"linattn {tag}{B}x{H}x{W} {regime} out", R.err(nchw(out.cpu()), out_ref), R.bar(1e-5, R.E32_ATTN))


@pytest.mark.parametrize("regime", R.K_REGIMES)
@pytest.mark.parametrize("B,H,W", [(2, 4, 4), (1, 10, 13), (2, 48, 40)])
def test_linattn_backward(AG, regime, B, H, W):
    """AG.LinAttnFn: one-launch statistics, ragged, and the pixel-split form"""
    q, (out_ref, _) = qkv_ref(regime, B, H, W)
    dy = R.rnd(B, R.HC, H, W, seed=4300)
    want = R.linattn_grad(q.double(), dy.double())
    qd = nhwc(q).to(DEV).requires_grad_(True)
    out = AG.LinAttnFn.apply(qd, 4)
    out.backward(nhwc(dy).to(DEV))
    assert bool(torch.isfinite(qd.grad).all())
    hold(f"LinAttnFn {B}x{H}x{W} {regime} out", R.err(nchw(out.detach().cpu()), out_ref), R.bar(1e-5, R.E32_ATTN))
    hold(f"LinAttnFn {B}x{H}x{W} {regime} dqkv", R.err(nchw(qd.grad.cpu()), want), R.bar(BWD, R.E32_ATTN_BWD))


@functools.lru_cache(maxsize=None)
def from_x_case(kreg, xreg, B, C, H, W):
    x = R.attn_x(xreg, B, C, H, W)
    w, g, b = R.attn_weights(kreg, C)
    return x, w, g, b, R.attn_from_x(*R.d(x, w, g, b))


def check_from_x(name, kreg, xreg, out, ctx, ref):
    e_out, e_ctx = R.E32_FROM_X[(kreg, xreg)]
    if out is not None:
        assert bool(torch.isfinite(out).all())
        hold(f"{name} k {kreg} x {xreg} out", R.err(out, ref[0]), R.bar(FUSED, e_out))
    if ctx is not None:
        assert bool(torch.isfinite(ctx).all())
        hold(f"{name} k {kreg} x {xreg} ctx", R.err(ctx, ref[1]), R.bar(FUSED, e_ctx))


@pytest.mark.parametrize("kreg,xreg", R.FROM_X_CASES)
@pytest.mark.parametrize("B,H,W,C", [(2, 2, 2, 64), (3, 8, 8, 128)])
def test_linattn_small_from_x(ops, kreg, xreg, B, H, W, C):
    x, w, g, b, ref = from_x_case(kreg, xreg, B, C, H, W)
    out, ctx = ops.linattn_small_from_x(nhwc(x).to(DEV), w.to(DEV), g.to(DEV), b.to(DEV))
    check_from_x(f"linattn_small_from_x {B}x{H}x{W}x{C}", kreg, xreg, nchw(out.cpu()), ctx.cpu(), ref)


@pytest.mark.parametrize("kreg,xreg", R.FROM_X_CASES)
@pytest.mark.parametrize("B,H,W,C", [(2, 8, 8, 32), (2, 16, 16, 128)])
def test_attention_split_from_x(ops, kreg, xreg, B, H, W, C):
    assert ops.L.load().ddk_attention_split_ok(B, H * W, C, 4)
    x, w, g, b, ref = from_x_case(kreg, xreg, B, C, H, W)
    before = ops.cluster_timeouts()
    out, ctx = ops.attention_split_from_x(nhwc(x).to(DEV), w.to(DEV), g.to(DEV), b.to(DEV))
    torch.cuda.synchronize()
    assert ops.cluster_timeouts() == before
    check_from_x(f"attention_split_from_x {B}x{H}x{W}x{C}", kreg, xreg, nchw(out.cpu()), ctx.cpu(), ref)


@pytest.mark.parametrize("kreg,xreg", R.FROM_X_CASES)
def test_attention_kv_context_and_folded(ops, kreg, xreg):
    """ddk_attention_kv_context at 16x16 (ctx) and the folded attention block at 32x32 (to_out and the residual included)"""
    B, C, H, W = 2, 128, 16, 16
    assert ops.L.load().ddk_attention_kv_context_ok(B, H * W, C, 4)
    x, w, g, b, ref = from_x_case(kreg, xreg, B, C, H, W)
    ctx = ops.attention_kv_context(nhwc(x).to(DEV), w.to(DEV), g.to(DEV), b.to(DEV))
    check_from_x("attention_kv_context", kreg, xreg, None, ctx.cpu(), ref)
    B, C, H, W = R.BLOCK_SHAPE
    x = R.attn_x(xreg, B, C, H, W)
    wo, bo = R.attn_out_proj(C)
    out = ops.attention_folded(nhwc(x).to(DEV), w.to(DEV), g.to(DEV), b.to(DEV), wo.to(DEV), bo.to(DEV))
    assert bool(torch.isfinite(out).all())
    hold(f"attention_folded k {kreg} x {xreg}", R.err(nchw(out.cpu()), R.attn_block(*R.d(x, w, g, b, wo, bo))),
         R.bar(FUSED, R.E32_ATTN_BLOCK[(kreg, xreg)]))


@pytest.mark.parametrize("kreg,xreg", R.FROM_X_CASES)
@pytest.mark.parametrize("hw", [16, 64])
def test_level_chain_attention(kreg, xreg, hw):
    """the level chain's ATTN op, alone, B = 3, 256 channels"""
    from ddk import lib as L
    from test_level_chain_gpu import ATTN, ChainOp, _p, run_chain
    B, C, S = 3, 256, (4 if hw == 16 else 8)
    x, w, g, b, ref = from_x_case(kreg, xreg, B, C, S, S)
    lnw = (w * g[None, :]).contiguous().to(DEV)
    c1, c2 = lnw.sum(dim=1).contiguous(), (w * b[None, :]).sum(dim=1).contiguous().to(DEV)
    wop = torch.empty_like(lnw)
    L.check(L.load().ddk_pack_qkv_operand(L.ptr(lnw), L.ptr(wop), 4, C, L.stream()), "pack_qkv_operand")
    xin = nhwc(x).to(DEV)
    heads = torch.empty((B, S, S, R.HC), device=DEV)
    run_chain([ChainOp(_p(xin), None, _p(wop), None, _p(c1), _p(c2), _p(heads), C, 0, ATTN, 0, -1, R.HC)], hw, B)
    check_from_x(f"level chain ATTN hw {hw}", kreg, xreg, nchw(heads.cpu()), None, ref)


# ------------------------------------------------------------------ optimiser and activation gradients
@pytest.mark.parametrize("regime", R.ADAM_REGIMES)
@pytest.mark.parametrize("clip", [False, True])
def test_adam_step(ops, regime, clip):
    """one step at each of the step numbers 1, 2 and 1000 from the same state, against oracle.train_ref.adam_step in fp64: the
    relative error of the update p_new - p_old (an eps in the wrong place changes nothing else), m and v to the older bar"""
    p, g, m, v = R.adam_state(regime)
    coef, nc = 1.0, None
    if clip:
        nc = ops.grad_norm_clip(g.to(DEV), TR.CLIP_NORM)
        _, total = TR.clip_grads({"g": g.double()})
        coef = float(torch.clamp(TR.CLIP_NORM / (total + 1e-6), max=1.0))
        print(f"adam {regime}: norm {float(nc[0]):.6e} coef {float(nc[1]):.6e} (reference {float(total):.6e}, {coef:.6e})")
        assert abs(float(nc[1]) - coef) <= 1e-6 * coef and abs(float(nc[0]) - float(total)) <= 1e-5 * float(total) + 1e-30
    for step in R.ADAM_STEPS:
        pd, gd, md, vd = (t.to(DEV).clone() for t in (p, g, m, v))
        ops.adam_step_(pd, gd, md, vd, R.ADAM_LR, step, clip=nc)
        p_ref, m_ref, v_ref = TR.adam_step(p.double(), g.double() * coef, m.double(), v.double(), step, R.ADAM_LR)
        got = (pd.cpu(), md.cpu(), vd.cpu())
        assert all(bool(torch.isfinite(t).all()) for t in got)
        if regime == "g0":
            assert torch.equal(got[0], p) and torch.equal(got[1], m) and torch.equal(got[2], v), "a zero gradient moved the state"
            continue
        hold(f"adam {regime} clip {clip} step {step} update", R.adam_update_err(got[0], p, p_ref), R.bar(R.ADAM_BAR, R.E32_ADAM[regime]))
        hold(f"adam {regime} clip {clip} step {step} m", R.err(got[1], m_ref), R.ADAM_BAR)
        hold(f"adam {regime} clip {clip} step {step} v", R.err(got[2], v_ref), R.ADAM_BAR)


def test_grad_norm_clip_edges(ops):
    n = R.ADAM_N
    zero = ops.grad_norm_clip(torch.zeros(n, device=DEV), 1.0).cpu()
    print(f"grad_norm_clip of zeros: norm {float(zero[0])} coef {float(zero[1])}")
    assert float(zero[0]) == 0.0 and float(zero[1]) == 1.0
    g = torch.zeros(n)
    g[7], g[n - 1] = 3.0, 4.0                # norm == 5 exactly
    nc = ops.grad_norm_clip(g.to(DEV), 5.0).cpu()
    want = 5.0 / (5.0 + 1e-6)                # clip_grad_norm_: max_norm / (norm + 1e-6), not above 1
    print(f"grad_norm_clip at norm == max_norm: norm {float(nc[0]):.9f} coef {float(nc[1]):.9f} (reference {want:.9f})")
    assert abs(float(nc[0]) - 5.0) <= 5e-7 and abs(float(nc[1]) - want) <= 1.2e-7 and float(nc[1]) <= 1.0


def test_activation_gradients_on_the_grid(ops):
    """mish' and tanh' against fp64 autograd where exp, softplus and tanh change regime: finite everywhere"""
    x = R.act_grid()
    gm_ref, gt_ref = R.act_grads()
    one = torch.ones_like(x).to(DEV)
    gm = ops.mish_bwd(x.to(DEV), one).cpu()
    gt = ops.tanh_bwd(ops.tanh(x.to(DEV)), one).cpu()
    assert bool(torch.isfinite(gm).all()) and bool(torch.isfinite(gt).all())
    hold("mish_bwd (abs)", R.abs_err(gm, gm_ref), R.bar(R.MISH_ABS_BAR, R.E32_ACT_ABS[0]))
    hold("tanh_bwd (abs)", R.abs_err(gt, gt_ref), R.bar(R.MISH_ABS_BAR, R.E32_ACT_ABS[1]))
