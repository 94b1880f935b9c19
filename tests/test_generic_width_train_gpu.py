"""Training at the widths the reference accepts beyond multiples of 32 (VERDICT round 4 "missing 3"):
`GroupNorm(8, C)` takes any unet_chan % 8 == 0 (reference models/unet/blocks.py:75-79) and `ConvResNet(dim, ...)` any d_chans
(models/downsampled/convblocks.py:133-159; here any multiple of 32).  The HIP training path runs those on a zero-padded channel
pitch: conv family unchanged on padded parameter copies, GroupNorm / channel LayerNorm on kernels that see the real channel count.

Checked against torch-CPU autograd through oracle/ (the functional restatement pinned by tests/golden): outputs, the input
gradient and parameter gradients of every kind of layer; Dropout by the property its mask is regenerated identically in the backward."""
import pytest
import torch

from helpers import rel_err
from oracle import resampler_ref as R
from oracle import unet_ref as U
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    return o


@pytest.mark.parametrize("B,H,W,C,with_drop", [(2, 8, 8, 24, False), (3, 4, 4, 40, False), (2, 16, 16, 72, False), (2, 8, 8, 24, True)])
def test_groupnorm_generic_train_fwd_bwd(ops, B, H, W, C, with_drop):
    """ddk_groupnorm_mish_generic_train_fwd / _bwd vs torch autograd of mish(group_norm(x)) + temb, + addend (blocks.py:79-80,106-111)"""
    import torch.nn.functional as F
    from ddk import autograd as AG
    CP = ops.pad32(C)
    x = syn.synthetic_normal((B, H, W, C), "ggn.x") * 1.3 + 0.2
    gamma, beta = 1 + 0.2 * syn.synthetic_normal((C,), "ggn.g"), 0.2 * syn.synthetic_normal((C,), "ggn.b")
    temb, add = syn.synthetic_normal((B, C), "ggn.t"), syn.synthetic_normal((B, H, W, C), "ggn.a")
    wgt = syn.synthetic_normal((B, H, W, C), "ggn.w")

    def pad(t):
        out = torch.zeros((*t.shape[:-1], CP))
        out[..., :C] = t
        return out.to(DEV)
    xd = pad(x).requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    td, ad = temb.to(DEV).requires_grad_(True), pad(add).requires_grad_(True)
    p = 0.25 if with_drop else 0.0
    y = AG.GNMishGenericFn.apply(xd, gd, bd, td, ad, p, 1234, 7, 8, 1e-5)
    assert float(y[..., C:].abs().max()) == 0.0                         # padding stays exactly zero
    (y * pad(wgt)).sum().backward()
    assert float(xd.grad[..., C:].abs().max()) == 0.0
    if with_drop:
        # no torch counterpart for the mask: the forward's kept set is what the backward regenerates -- d y / d temb is the mask itself
        y0 = AG.GNMishGenericFn.apply(xd.detach(), gd.detach(), bd.detach(), td.detach(), None, 0.0, 0, 0, 8, 1e-5)
        scale = (y.detach() - ad.detach())[..., :C] / y0[..., :C]
        kept = scale.abs() > 0.5
        assert torch.allclose(scale[kept], torch.full_like(scale[kept], 1 / (1 - p)), rtol=1e-4)
        assert 0.6 < float(kept.float().mean()) < 0.9
        want_dtemb = (pad(wgt)[..., :C] * kept / (1 - p)).sum(dim=(1, 2))
        assert rel_err(td.grad.cpu(), want_dtemb.cpu()) < 2e-5
        return
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    tr, ar = temb.clone().requires_grad_(True), add.clone().requires_grad_(True)
    yr = F.mish(F.group_norm(xr.permute(0, 3, 1, 2), 8, gr, br, eps=1e-5)).permute(0, 2, 3, 1) + tr[:, None, None, :] + ar
    (yr * wgt).sum().backward()
    assert rel_err(y[..., :C].detach().cpu(), yr.detach()) < 5e-6
    for got, want in ((xd.grad[..., :C], xr.grad), (gd.grad, gr.grad), (bd.grad, br.grad), (td.grad, tr.grad), (ad.grad[..., :C], ar.grad)):
        assert rel_err(got.cpu(), want) < 2e-5


@pytest.mark.parametrize("M,C", [(70, 24), (33, 40), (260, 72), (5, 200)])
def test_chan_layernorm_generic_fwd_bwd(ops, M, C):
    """ddk_chan_layernorm_generic / _bwd vs torch autograd of the reference's LayerNorm (blocks.py:57-60: eps on the std)"""
    from ddk import autograd as AG
    CP = ops.pad32(C)
    x = syn.synthetic_normal((1, M, 1, C), "gln.x") * 0.9 + 0.5
    g, b = 1 + 0.2 * syn.synthetic_normal((1, C, 1, 1), "gln.g"), 0.2 * syn.synthetic_normal((1, C, 1, 1), "gln.b")
    wgt = syn.synthetic_normal((1, M, 1, C), "gln.w")
    xp = torch.zeros((1, M, 1, CP))
    xp[..., :C] = x
    xd, gd, bd = xp.to(DEV).requires_grad_(True), g.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = AG.ChanLayerNormGenericFn.apply(xd, gd, bd, 1e-5)
    wp = torch.zeros((1, M, 1, CP))
    wp[..., :C] = wgt
    (y * wp.to(DEV)).sum().backward()
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    mean = xr.mean(dim=-1, keepdim=True)
    std = xr.var(dim=-1, unbiased=False, keepdim=True).sqrt()
    yr = (xr - mean) / (std + 1e-5) * gr.reshape(1, 1, 1, C) + br.reshape(1, 1, 1, C)
    (yr * wgt).sum().backward()
    assert float(y[..., C:].abs().max()) == 0.0 and float(xd.grad[..., C:].abs().max()) == 0.0
    assert rel_err(y[..., :C].detach().cpu(), yr.detach()) < 5e-6
    assert rel_err(xd.grad[..., :C].cpu(), xr.grad) < 2e-5
    assert rel_err(gd.grad.cpu(), gr.grad) < 2e-5 and rel_err(bd.grad.cpu(), br.grad) < 2e-5


@pytest.mark.parametrize("C", [32, 96, 224, 288, 352, 416, 448, 480, 512])
@pytest.mark.parametrize("n_out", [3, 8])
def test_small_n_conv1x1_backward_at_every_padded_width(ops, C, n_out):
    """final_conv.1's backward (da, dw, db) at every multiple of 32 a padded generic width can give -- 224 (unet_chan 200..224),
    288, 352, ... take the 32-channels-per-trip form of the kernel; against the plain products in float64"""
    g = torch.Generator().manual_seed(C * 10 + n_out)
    M = 2 * 13 * 11
    a = torch.randn(M, C, generator=g)
    w = torch.randn(n_out, C, generator=g) * C ** -0.5
    dy = torch.randn(M, n_out, generator=g)
    da, dw, db = ops.conv1x1_small_n_bwd(a.to(DEV), w.to(DEV), dy.to(DEV))
    assert rel_err(da.cpu(), (dy.double() @ w.double()).float()) < 1e-5
    assert rel_err(dw.cpu(), (dy.double().t() @ a.double()).float()) < 1e-5
    assert rel_err(db.cpu(), dy.double().sum(0).float()) < 1e-5


@pytest.mark.parametrize("chan,cin,size,dims", [(24, 3, 16, (1, 2, 2, 2)), (40, 8, 16, (1, 2, 2, 2)), (200, 3, 8, (1, 2))])
def test_unet_training_at_widths_that_are_not_multiples_of_32(chan, cin, size, dims):
    """forward, input gradient and parameter gradients of every layer kind of the full UNet (attention at every level) at
    unet_chan = 24 / 40 (4 levels) and 200 (levels of 200 and 400 channels: pitches 224 and 416) against torch-CPU autograd through
    oracle.unet_ref (reference models/unet/unet.py:74-104)"""
    from models import Unet
    cfg = dict(unet_chan=chan, unet_in=cin, unet_dims=dims, unet_dropout=0.0)
    model = Unet(cfg)
    sd = syn.fill_state_dict(model.state_dict(), 91)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    x = syn.synthetic_input((2, cin, size, size), "gw.x")
    t = torch.tensor([11, 640])
    wgt = syn.synthetic_normal((2, cin, size, size), "gw.w")
    probe = ["downs.0.0.block1.block.0.weight", "downs.0.0.block1.block.0.bias", "downs.0.0.block1.block.1.weight", "downs.0.0.res_conv.weight",
             "downs.1.2.fn.fn.to_qkv.weight", "downs.1.2.fn.fn.to_out.bias", "downs.1.2.fn.norm.g", "downs.0.3.conv.weight", "mid_block1.block2.block.1.bias",
             "ups.0.0.block1.block.0.weight", "ups.0.0.res_conv.weight", "ups.1.3.conv.weight", "ups.2.1.block2.block.0.weight",
             "final_conv.0.block.0.weight", "final_conv.1.weight", "time_mlp.1.weight", "downs.2.1.mlp.1.bias", "ups.1.0.mlp.1.weight"]
    probe = [k for k in probe if k in sd]            # the two-level case has no downs.2 / ups.1 / ups.2
    assert len(probe) >= 10
    ref_sd = {k: v.clone() for k, v in sd.items()}
    for k in probe:
        ref_sd[k].requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    out_ref = U.unet_forward(ref_sd, cfg, xr, t)
    (out_ref * wgt).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = model(xd, t.to(DEV))
    assert rel_err(out.detach().cpu(), out_ref.detach()) < 5e-5
    (out * wgt.to(DEV)).sum().backward()
    params = dict(model.named_parameters())
    assert rel_err(xd.grad.cpu(), xr.grad) < 2e-4
    for k in probe:
        assert params[k].grad is not None, k
        assert rel_err(params[k].grad.cpu(), ref_sd[k].grad) < 2e-4, k
    # ... and the eval-mode plan of the same module (the padded inference path) agrees with the training forward
    model.eval()
    with torch.no_grad():
        y_plan = model(x.to(DEV), t.to(DEV))
    assert rel_err(y_plan.cpu(), out.detach().cpu()) < 5e-5


def test_unet_training_generic_width_with_tuned_eligible_levels():
    """unet_chan = 16, dims (1, 2, 4): levels of 16, 32 and 64 channels -- the smallest model in which a network on the padded pitch
    holds widths (32, 64) that the tuned GroupNorm / LayerNorm backward would take.  Every module runs the generic forms there and no
    gradient is handed over (ddk.autograd.resnet_tuned / attention_tuned / pitch_tuned); a walk that mixed the two forms would show
    here.  The output, the input gradient and the gradient of EVERY parameter against torch-CPU autograd of oracle.unet_ref at the
    bars of test_unet_training_at_widths_that_are_not_multiples_of_32 (forward 5e-5, gradients 2e-4 of each tensor's max; two channels
    per group at the first level), and the eval-mode plan against the training forward (5e-5)."""
    from models import Unet
    cfg = dict(unet_chan=16, unet_in=3, unet_dims=(1, 2, 4), unet_dropout=0.0)
    model = Unet(cfg)
    sd = syn.fill_state_dict(model.state_dict(), 91)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    x = syn.synthetic_input((2, 3, 8, 8), "gw16.x")
    t = torch.tensor([11, 640])
    wgt = syn.synthetic_normal((2, 3, 8, 8), "gw16.w")
    ref_sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr = x.clone().requires_grad_(True)
    out_ref = U.unet_forward(ref_sd, cfg, xr, t)
    (out_ref * wgt).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = model(xd, t.to(DEV))
    e = rel_err(out.detach().cpu(), out_ref.detach())
    (out * wgt.to(DEV)).sum().backward()
    ex = rel_err(xd.grad.cpu(), xr.grad)
    errs = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        errs[k] = rel_err(p.grad.cpu(), ref_sd[k].grad)
    worst = max(errs, key=errs.get)
    print(f"unet training chan 16 dims (1, 2, 4): forward {e:.3e} input gradient {ex:.3e} worst parameter {worst} {errs[worst]:.3e}")
    assert e < 5e-5 and ex < 2e-4
    assert len(errs) == len(ref_sd)
    for k, v in errs.items():
        assert v < 2e-4, (k, v)
    model.eval()
    with torch.no_grad():
        y_plan = model(x.to(DEV), t.to(DEV))
    assert rel_err(y_plan.cpu(), out.detach().cpu()) < 5e-5


def test_unet_generic_width_dropout_trains(tmp_path):
    """unet_dropout > 0 at width 24: two optimiser steps through the product trainer (device-graph capture included) stay finite and
    move the weights -- the Dropout mask of the generic GroupNorm kernel is drawn in the forward and regenerated in the backward"""
    import trainers.trainer as T
    import trainers.trainer_ddpm as TD
    from trainers import setup_trainer
    T.LOGGING_DIR = TD.LOGGING_DIR = str(tmp_path) + "/"
    config = dict(model="ddpm", dataset="cifar10", n_steps=2, batch_size=4, image_size=16, n_downsamples=0, lr=2e-4, unet_chan=24,
                  unet_dims=(1, 2, 2, 2), unet_dropout=0.1, T=100, loss_type="simple", beta_schedule="linear", ema_decay=0.995,
                  loss_flat="sum", val_split=0, n_samples=4)
    trainer, _ = setup_trainer(config, True, str(tmp_path), "unit", seed=0)
    p0 = trainer.opt.fp.flat.clone()
    losses = trainer.train()
    assert len(losses) == 2 and all(l == l and abs(l) < 1e9 for l in losses)
    assert not torch.equal(p0, trainer.opt.fp.flat) and bool(torch.isfinite(trainer.opt.fp.flat).all())


@pytest.mark.parametrize("d_chans,d_dropout", [(32, 0.0), (96, 0.0), (48, 0.0), (16, 0.0), (224, 0.0), (48, 0.1), (64, 0.25)])
def test_resampler_training_at_d_chans_not_a_multiple_of_64(d_chans, d_dropout):
    """the dDDPM encoder / decoder (ConvResNet, convblocks.py:92-159) in training at d_chans = 32 / 96 -- inner widths 16 / 48 on a
    zero-padded pitch --, at d_chans = 48 / 16 -- the trunk itself on a padded pitch (any even d_chans, convblocks.py:133-159) --
    and with d_dropout > 0 (nn.Dropout2d on c4's output, convblocks.py:106,121-124; the draws injected on both sides): outputs and
    gradients (input, first / inner / last conv parameters) vs torch-CPU autograd through oracle.resampler_ref"""
    from helpers import dddpm_cfg
    from models import DownsampleDDPMAutoencoder, Unet
    cfg = dddpm_cfg(32, 32, 2)
    cfg["d_chans"] = d_chans
    cfg["d_dropout"] = d_dropout
    model = DownsampleDDPMAutoencoder(cfg, Unet(cfg), DEV, 3)
    sd = syn.fill_state_dict(model.state_dict(), 17, skip=syn.SCHEDULE_KEYS)
    model.load_state_dict(sd)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = syn.synthetic_input((2, 3, 32, 32), "gres.x")
    wz, wx = syn.synthetic_normal((2, 8, 8, 8), "gres.wz"), syn.synthetic_normal((2, 3, 32, 32), "gres.wx")
    probe = ["downsample.conv.0.weight", "downsample.conv.1.c1.weight", "downsample.conv.1.c2.weight", "downsample.conv.2.c3.bias",
             "downsample.conv.4.c4.weight", "upsample.conv.1.c1.bias", "upsample.conv.3.c2.weight", "upsample.conv.6.c4.weight"]
    probe = [k for k in probe if k in sd]
    assert len(probe) >= 6
    ref = {k: v.clone() for k, v in sd.items()}
    for k in probe:
        ref[k].requires_grad_(True)
    masks = None
    if d_dropout > 0:
        # one Dropout2d draw per ConvResBlock, the same on both sides: [B, d_chans] of {0, 1 / (1 - p)}
        masks = {}
        g = torch.Generator().manual_seed(5)
        for name, net in (("downsample.", model.downsample), ("upsample.", model.upsample)):
            for i, blk in enumerate(list(net.conv)[1:-1], start=1):
                m = (torch.rand((2, d_chans), generator=g) >= d_dropout).float() / (1.0 - d_dropout)
                masks[f"{name}conv.{i}."] = m
                blk._mask_hook = (lambda mm: (lambda b, c, dev: mm))(m)
        assert any(float((m == 0).float().mean()) > 0 for m in masks.values())
    xr = x.clone().requires_grad_(True)
    zr = R.rescaled_downsample(ref, cfg, xr, masks)
    xo_r = R.rescaled_upsample(ref, cfg, zr, masks)
    ((zr * wz).sum() + (xo_r * wx).sum()).backward()
    xd = x.to(DEV).requires_grad_(True)
    z = model.rescaled_downsample(xd)
    xo = model.rescaled_upsample(z)
    assert rel_err(z.detach().cpu(), zr.detach()) < 2e-5 and rel_err(xo.detach().cpu(), xo_r.detach()) < 2e-5
    ((z * wz.to(DEV)).sum() + (xo * wx.to(DEV)).sum()).backward()
    params = dict(model.named_parameters())
    assert rel_err(xd.grad.cpu(), xr.grad) < 2e-4
    for k in probe:
        assert rel_err(params[k].grad.cpu(), ref[k].grad) < 2e-4, k
    # eval mode: Dropout2d is the identity, the sampler's decode path (forward_nhwc) == the oracle without masks
    model.eval()
    with torch.no_grad():
        z_e = model.rescaled_downsample(x.to(DEV))
        x_e = model.rescaled_upsample(z_e)
        z_ref = R.rescaled_downsample(sd, cfg, x)
        assert rel_err(z_e.cpu(), z_ref) < 2e-5 and rel_err(x_e.cpu(), R.rescaled_upsample(sd, cfg, z_ref)) < 2e-5


def test_resampler_dropout_draws_whole_channels(monkeypatch):
    """d_dropout > 0 without injected draws: in training a ConvResBlock zeroes whole (sample, channel) planes of c4's output with
    probability p and scales the rest by 1 / (1 - p) (nn.Dropout2d, convblocks.py:106,121-124); two forwards draw different masks"""
    from models.downsampled.convblocks import ConvResBlock
    blk = ConvResBlock(32, 64, 64, dropout=0.5, residual=False).to(DEV).train()
    x = torch.randn(16, 64, 8, 8, device=DEV)
    with torch.no_grad():
        y1, y2 = blk(x), blk(x)
        blk.eval()
        y0 = blk(x)
    dead1 = (y1.abs().amax(dim=(2, 3)) == 0)
    frac = float(dead1.float().mean())
    assert 0.3 < frac < 0.7
    keep = ~dead1
    assert torch.allclose(y1.permute(0, 2, 3, 1)[keep[:, None, None, :].expand(16, 8, 8, 64)],
                          2.0 * y0.permute(0, 2, 3, 1)[keep[:, None, None, :].expand(16, 8, 8, 64)], rtol=1e-5, atol=1e-6)
    assert not torch.equal(dead1, (y2.abs().amax(dim=(2, 3)) == 0))
