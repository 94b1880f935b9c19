"""to_qkv + attention core in one launch on the 16x16 and 8x8 maps, an (image, head) split over two workgroups that exchange their
softmax partials inside the launch (csrc/attention.hip attn_split_kernel, ddk_attention_split_from_x, DDK_OPT_ATTENTION_SPLIT).
Reference: models/unet/blocks.py:57-60 (PreNorm LayerNorm), :123 (to_qkv), :126-131 (softmax over the pixels of k, the two einsums)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS, HC = 4, 128

# B, H, W, C, shift -- shift != 0: a per-pixel ramp along one channel direction (and weights x 3) moves the column maxima of k by
# 5-11 between the two halves of an image, so the merge's rescale does real work; (2, 8, 8, 32): one K chunk; (32, 8, 8, 256): 256
# workgroups, one per CU -- the occupancy of the timed step
CASES = [(3, 8, 8, 256, 0.0), (3, 8, 8, 256, 30.0), (2, 16, 16, 128, 0.0), (2, 16, 16, 128, 30.0), (2, 16, 16, 256, 30.0),
         (2, 8, 8, 32, 30.0), (2, 16, 16, 32, 0.0), (32, 8, 8, 256, 0.0)]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    from ddk import lib
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


@functools.lru_cache(maxsize=None)
def case(B, H, W, C, shift):
    """inputs of tests/test_step_edges_gpu.py::test_attention_kv_projection_and_context_in_one_launch at width C, and the block in
    torch fp64: (x NHWC, wq, g, be, ref out NCHW, ref ctx); computed once per shape, never modified"""
    x = rnd(B, C, H, W, seed=181) * 1.3 + 0.2
    if shift:
        ramp = torch.linspace(0, 1, H * W).reshape(1, 1, H, W)
        x = x + shift * ramp * rnd(1, C, 1, 1, seed=187)
    wq = rnd(3 * HC, C, 1, 1, seed=182, scale=C ** -0.5 * (3.0 if shift else 1.0))
    g, be = 1 + 0.2 * rnd(C, seed=185), 0.1 * rnd(C, seed=186)
    xd = x.double()
    std = xd.var(dim=1, unbiased=False, keepdim=True).sqrt()
    xn = (xd - xd.mean(dim=1, keepdim=True)) / (std + 1e-5) * g.double().view(1, C, 1, 1) + be.double().view(1, C, 1, 1)
    q, k, v = F.conv2d(xn, wq.double()).reshape(B, 3, HEADS, 32, H * W).unbind(1)
    ctx = torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, HC, H, W)
    return to_nhwc(x), wq, g, be, out, ctx


def run(ops, B, H, W, C, shift, workspace=None):
    x, wq, g, be, _, _ = case(B, H, W, C, shift)
    return ops.attention_split_from_x(x.to(DEV), wq.to(DEV), g.to(DEV), be.to(DEV), workspace=workspace)


@pytest.mark.parametrize("B,H,W,C,shift", CASES)
def test_split_attention_vs_torch_fp64(ops, B, H, W, C, shift):
    """out and ctx against torch in fp64: max|diff| / max|ref| <= 2e-5, the library's bar for contractions (the same split-and-merge
    arithmetic in fp32 on the CPU stays within 2.1e-6 for ctx and 6.2e-7 for out on these inputs)"""
    _, _, _, _, ref_out, ref_ctx = case(B, H, W, C, shift)
    before = ops.cluster_timeouts()
    out, ctx = run(ops, B, H, W, C, shift)
    e_out, e_ctx = rel_err(to_nchw(out.cpu()), ref_out), rel_err(ctx.cpu(), ref_ctx)
    print(f"split attention {B}x{H}x{W}x{C} shift {shift}: out {e_out:.3e} ctx {e_ctx:.3e}")
    assert ops.cluster_timeouts() == before
    assert e_out <= 2e-5 and e_ctx <= 2e-5


@pytest.mark.parametrize("B,H,W,C,shift", CASES)
def test_split_attention_vs_the_two_launches_it_replaces(ops, B, H, W, C, shift):
    """against the LayerNorm-folded 1x1 conv + ddk_linattn_fused_small: <= 2e-5, not bit-equal (another summation order), and two
    runs of the new entry bit-equal.  (The C ABI's folded 1x1 conv takes 128-channel inputs of >= 2048 pixels only, so the conv of
    W o g runs through ddk_conv_forward and the fold r acc - r mean (W g) + W b is applied to its output here, in fp32.)"""
    x, wq, g, be, _, _ = case(B, H, W, C, shift)
    xh = x.to(DEV)
    wf = wq.reshape(3 * HC, C)
    wg = (wf * g.view(1, C)).to(DEV)
    acc = ops.conv(ops.CONV1X1, xh, ops.pack_conv_weight(wg.reshape(3 * HC, C, 1, 1)), n_out=3 * HC)
    mean = xh.mean(dim=-1, keepdim=True)
    r = 1.0 / ((xh - mean).square().mean(dim=-1, keepdim=True).sqrt() + 1e-5)
    qkv = (r * acc - (r * mean) * wg.sum(dim=1) + (wf @ be).to(DEV)).contiguous()
    old_out, old_ctx = ops.linattn(qkv, HEADS)
    out, ctx = run(ops, B, H, W, C, shift)
    out2, ctx2 = run(ops, B, H, W, C, shift)
    assert torch.equal(out, out2) and torch.equal(ctx, ctx2)
    assert not torch.equal(out, old_out) and not torch.equal(ctx, old_ctx)
    e_out, e_ctx = rel_err(out.cpu(), old_out.cpu()), rel_err(ctx.cpu(), old_ctx.cpu())
    print(f"split attention vs two launches {B}x{H}x{W}x{C} shift {shift}: out {e_out:.3e} ctx {e_ctx:.3e}")
    assert e_out <= 2e-5 and e_ctx <= 2e-5


@pytest.mark.parametrize("H,C", [(8, 256), (16, 128)])
def test_split_attention_hand_off_is_never_stale(ops, H, C):
    """one workspace throughout: input A, another input B, A again, out and ctx poisoned in between -- the third result equals the
    first bit for bit and equals A on a fresh workspace; the counters re-arm and no wait gives up"""
    B = 3
    xa, wq, g, be, _, _ = case(B, H, H, C, 30.0)
    xb = to_nhwc(rnd(B, C, H, H, seed=191) * 0.7 - 0.4)
    ws = ops.attention_split_workspace(B, DEV)
    before = ops.cluster_timeouts()
    args = (wq.to(DEV), g.to(DEV), be.to(DEV))
    outs = []
    for x in (xa, xb, xa):
        out, ctx = ops.attention_split_from_x(x.to(DEV), *args, workspace=ws)
        outs.append((out.clone(), ctx.clone()))
        out.fill_(float("nan"))
        ctx.fill_(float("nan"))
    fresh = ops.attention_split_from_x(xa.to(DEV), *args)
    assert ops.cluster_timeouts() == before
    assert all(torch.isfinite(t).all() for pair in outs for t in pair)
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    assert not torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][0], fresh[0]) and torch.equal(outs[0][1], fresh[1])
    nwords = 32 + B * 4 * 32                                   # the give-up line and the pair counters: all back to zero
    assert int(ws[:nwords].view(torch.int32).abs().sum()) == 0


def test_split_attention_eligibility(ops):
    """ddk_attention_split_ok refuses H*W of 16 and 1024, C of 288 and 24, 3 heads, and a batch whose 8 B workgroups exceed the CUs;
    the entry returns an error for a refused shape instead of launching"""
    lib = ops.L.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.ddk_attention_split_ok(32, 64, 256, 4) == 1 and lib.ddk_attention_split_ok(2, 256, 128, 4) == 1
    for B, HW, C, heads in [(2, 16, 256, 4), (2, 1024, 128, 4), (2, 64, 288, 4), (2, 64, 24, 4), (2, 64, 256, 3), (cus // 8 + 1, 64, 256, 4)]:
        assert lib.ddk_attention_split_ok(B, HW, C, heads) == 0, (B, HW, C, heads)
    x = torch.zeros((2, 4, 4, 256), device=DEV)
    w = torch.zeros((3 * HC, 256), device=DEV)
    c = torch.zeros(3 * HC, device=DEV)
    ctx = torch.full((2, HEADS, 32, 32), 7.0, device=DEV)
    out = torch.full((2, 4, 4, HC), 7.0, device=DEV)
    ws = ops.attention_split_workspace(2, DEV)
    rc = lib.ddk_attention_split_from_x(ops.L.ptr(x), ops.L.ptr(w), ops.L.ptr(c), ops.L.ptr(c), 1e-5, ops.L.ptr(ctx), ops.L.ptr(out), 2, 16, 256,
                                        HEADS, ops.L.ptr(ws), ws.numel() * 4, ops.L.stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((ctx == 7.0).all()) and bool((out == 7.0).all())
    with pytest.raises(ops.L.DDKError):
        ops.attention_split_from_x(x, w, c + 1, c)


def _net(in_ch=8):
    from helpers import det_state, unet_cfg
    from models import Unet
    net = Unet(unet_cfg(128, in_ch))
    net.load_state_dict(det_state({k: v.shape for k, v in net.state_dict().items()}))
    return net.to(DEV).eval()


@pytest.mark.parametrize("batch", [32, 5, 40])
def test_attention_split_option_gives_the_same_unet(batch):
    """plan option DDK_OPT_ATTENTION_SPLIT in the cfg4-shaped UNet with the in-launch paths allowed in single forwards: on vs off
    <= 2e-5 of the output's max and not the same bits, on == on bit for bit with a forward on other data in between, no wait gives
    up.  Batch 40 (320 workgroups would not be one dispatch round) keeps the two launches: on and off bit-equal."""
    from ddk import ops
    from utils import synthetic as syn
    net = _net()
    x = syn.synthetic_normal((batch, 8, 32, 32), f"attnsplit.x{batch}").to(DEV)
    x2 = syn.synthetic_normal((batch, 8, 32, 32), f"attnsplit.y{batch}").to(DEV)
    t = (torch.arange(batch, device=DEV) * 23) % 1000
    with torch.no_grad():
        plan = net.plan()
        plan.set_option(plan.OPT_CLUSTER_GROUPNORM, 2)
        before = ops.cluster_timeouts()
        y_on = net(x, t)
        y_other = net(x2, t)
        y_on2 = net(x, t)
        plan.set_option(plan.OPT_ATTENTION_SPLIT, 0)
        y_off = net(x, t)
        plan.set_option(plan.OPT_ATTENTION_SPLIT, 1)
        y_on3 = net(x, t)
    assert plan._cluster == 2, "the in-launch paths were switched off by a failed check"
    assert ops.cluster_timeouts() == before
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_on2) and torch.equal(y_on, y_on3)
    assert not torch.equal(y_on, y_other)
    if batch > 32:
        assert torch.equal(y_on, y_off)
        return
    assert not torch.equal(y_on, y_off)
    e = rel_err(y_on.cpu(), y_off.cpu())
    print(f"attention split option, batch {batch}: on vs off {e:.3e}")
    assert e <= 2e-5


def test_attention_split_in_the_sampler_matches_the_two_launches():
    """ddk_sampler_run (hipGraph replay) with the option on (the default) vs off: 40 reverse steps of batch 8 from the same x_T with
    the same Philox stream end within 1e-4 of the output's max of each other, and the pair counters re-arm across replays"""
    from ddk import ops
    from helpers import ddpm_cfg
    from models import DDPM, Unet
    from utils import synthetic as syn
    cfg = ddpm_cfg(128, 3, 32, T=1000)
    model = DDPM(cfg, Unet(cfg), "cuda", 3)
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    model = model.to(DEV).eval()
    plan = model.latent_model.plan()
    tables = model._tables()
    outs = {}
    before = ops.cluster_timeouts()
    for on in (1, 0):
        plan.set_option(plan.OPT_ATTENTION_SPLIT, on)
        x = ops.randn((8, 32, 32, 3), DEV, seed=77, step=1000, stream_id=0)
        with torch.no_grad():
            plan.sample_nhwc(x, tables, 999, 960, seed=77, stream_id=0, use_graph=True)
        outs[on] = x.clone()
    plan.set_option(plan.OPT_ATTENTION_SPLIT, 1)
    assert plan._cluster >= 1 and ops.cluster_timeouts() == before
    assert torch.isfinite(outs[1]).all()
    assert not torch.equal(outs[0], outs[1])
    e = float((outs[0] - outs[1]).abs().max()) / float(outs[0].abs().max())
    print(f"attention split in the sampler: on vs off {e:.3e}")
    assert e < 1e-4
