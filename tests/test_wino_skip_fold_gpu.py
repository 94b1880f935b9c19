"""The skip fold of the Winograd conv (conv3x3_wino2_kernel<4, 0, CL, SK = true>): a ResnetBlock's 1x1 res_conv computed
inside the launch of the 3x3 conv that reads the same input, from the four inner positions of the input transform.

Every case is held, for BOTH outputs, to a torch-CPU fp64 reference at test_wlocal_loop_gpu.py's bar, max|diff| / max|ref| < 2e-5; the
conv output must be bit-identical with the fold on and off (the extra MFMAs go to other accumulators); the launches go A / B / A through
the same NaN-filled device buffers and must be bit-stable; with every allocation poisoned with NaN, and with every tensor between guard
bands, the results keep their bits and no band is touched; no in-launch wait gives up.  No case provokes a timeout."""
import pytest
import torch
import torch.nn.functional as F

import poison
from guard import format_violation, guard_bands
from helpers import rel_err, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-5

# id, B, H, W, c0, c1, N, channel-chunk splits the library must report for it
CONV_CASES = [
    ("one-chunk", 2, 8, 8, 32, 0, 64, 1),                  # a single m tile of 32 tiles, one chunk: no steady state, written directly
    ("odd-chunks-two-sources", 2, 8, 8, 64, 32, 128, 2),   # 3 chunks over 2 splits (2 + 1), the second source, two n tiles: slab form
    ("ragged-m-tile", 3, 4, 4, 64, 0, 64, 2),              # 12 of the m tile's 32 tiles exist
    ("slabs-2", 2, 8, 8, 64, 0, 64, 2),
    ("slabs-4", 2, 8, 8, 128, 0, 64, 4),
]
# in-launch GroupNorm: the smallest shapes ddk_conv3x3_gn_mish_cluster_ok admits (two m tiles per image; unsplit needs m tiles % 8 == 0)
CLUSTER_CASES = [
    ("cluster-unsplit", 8, 16, 16, 32, 0, 64, 1),
    ("cluster-hand-off", 8, 16, 16, 64, 0, 64, 2),
    ("cluster-hand-off-odd-two-sources", 8, 16, 16, 64, 32, 64, 2),
]
GROUPS = 8


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    from ddk import lib
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


def mish64(v):
    return v * torch.tanh(F.softplus(v))


def params(cin, N):
    return dict(w3=rnd(N, cin, 3, 3, seed=1, scale=(cin * 9) ** -0.5), b3=rnd(N, seed=2, scale=0.1), w1=rnd(N, cin, seed=3, scale=cin ** -0.5),
                b1=rnd(N, seed=4, scale=0.1), gamma=1 + rnd(N, seed=5, scale=0.2), beta=rnd(N, seed=6, scale=0.2))


def inputs(B, H, W, cin, N, seed):
    return dict(x=rnd(B, cin, H, W, seed=seed), temb=rnd(B, N, seed=seed + 1), add=rnd(B, N, H, W, seed=seed + 2))


def reference(inp, par, cluster):
    """fp64 on the CPU (NCHW): the conv (or the whole Block of the in-launch GroupNorm form) and the 1x1 skip conv"""
    x = inp["x"].double()
    y = F.conv2d(x, par["w3"].double(), par["b3"].double(), padding=1)
    if cluster:
        y = mish64(F.group_norm(y, GROUPS, par["gamma"].double(), par["beta"].double(), eps=1e-5)) + inp["temb"].double()[:, :, None, None] \
            + inp["add"].double()
    return y, F.conv2d(x, par["w1"].double()[:, :, None, None], par["b1"].double())


class Site:
    """the device side of one case: packed weights, the buffers every launch goes through, and the launch itself"""

    def __init__(self, ops, B, H, W, c0, c1, N, cluster):
        self.ops, self.cluster, self.c0, self.c1 = ops, cluster, c0, c1
        par = params(c0 + c1, N)
        self.par = par
        self.w = ops.pack_conv_weight(par["w3"].to(DEV)) if not cluster else None
        self.wu = ops.pack_conv_weight_wino(par["w3"].to(DEV))
        self.wsk = ops.pack_conv_skip_weight_wino(par["w1"].to(DEV))
        self.b3, self.b1, self.gamma, self.beta = (par[k].to(DEV) for k in ("b3", "b1", "gamma", "beta"))
        self.x0 = torch.empty(B, H, W, c0, device=DEV)
        self.x1 = torch.empty(B, H, W, c1, device=DEV) if c1 else None
        self.temb = torch.empty(B, N, device=DEV)
        self.add = torch.empty(B, H, W, N, device=DEV)
        self.out = torch.empty(B, H, W, N, device=DEV)
        self.skip = torch.empty(B, H, W, N, device=DEV)

    def launch(self, inp, fold=True):
        ops, x = self.ops, to_nhwc(inp["x"])
        self.x0.copy_(x[..., :self.c0])
        if self.c1:
            self.x1.copy_(x[..., self.c0:])
        self.temb.copy_(inp["temb"])
        self.add.copy_(to_nhwc(inp["add"]))
        self.out.fill_(float("nan"))
        self.skip.fill_(float("nan"))
        sk = dict(skip_w=self.wsk, skip_bias=self.b1, skip_out=self.skip) if fold else {}
        if self.cluster:
            ops.conv3x3_gn_mish_cluster(self.x0, self.wu, self.b3, self.gamma, self.beta, x2=self.x1, temb=self.temb, addend=self.add,
                                        groups=GROUPS, out=self.out, **sk)
        else:
            ops.conv(ops.CONV3X3_S1, self.x0, self.w, self.b3, x2=self.x1, w_wino=self.wu, out=self.out, **sk)
        return self.out.cpu(), (self.skip.cpu() if fold else None)


def check_case(ops, name, B, H, W, c0, c1, N, splits, cluster):
    lib = ops.L.load()
    cin = c0 + c1
    assert lib.ddk_conv_wino_splits(B, H, W, cin, N) == splits and lib.ddk_conv_wino_skip_ok(B, H, W, cin, N) == 1
    if cluster and lib.ddk_conv3x3_gn_mish_cluster_ok(B, H, W, cin, N, GROUPS) <= 0:
        pytest.skip("the in-launch GroupNorm needs a whole MI355X (256 CUs in 8 XCDs, no CU mask)")
    before = ops.cluster_timeouts()
    site = Site(ops, B, H, W, c0, c1, N, cluster)
    in_a, in_b = inputs(B, H, W, cin, N, 100), inputs(B, H, W, cin, N, 200)
    (out_a, sk_a), (out_b, sk_b), (out_a2, sk_a2) = site.launch(in_a), site.launch(in_b), site.launch(in_a)
    for tag, out, sk, inp in (("A", out_a, sk_a, in_a), ("B", out_b, sk_b, in_b)):
        ref_out, ref_sk = reference(inp, site.par, cluster)
        e_out, e_sk = rel_err(to_nchw(out).double(), ref_out), rel_err(to_nchw(sk).double(), ref_sk)
        print(f"{name} {tag}: max|diff| / max|ref|: conv {e_out:.3e}, skip {e_sk:.3e}")
        assert e_out < BAR and e_sk < BAR
    assert not torch.equal(out_a, out_b) and not torch.equal(sk_a, sk_b)
    assert torch.equal(out_a, out_a2) and torch.equal(sk_a, sk_a2)                 # A / B / A
    out_off, _ = site.launch(in_a, fold=False)
    assert torch.equal(out_off, out_a), "the conv output changes with the fold"
    # every allocation of the wrappers (output defaults, split-K workspace) and the cached scratch (cluster records) poisoned with NaN
    with poison.poisoned_allocations(poison.NAN):
        poison.repoison(poison.NAN)
        psite = Site(ops, B, H, W, c0, c1, N, cluster)
        out_p, sk_p = psite.launch(in_a)
    assert torch.equal(out_p, out_a) and torch.equal(sk_p, sk_a), "a result depends on the contents of a buffer it should only write"
    # every tensor between guard bands of NaN: nothing outside a tensor is written, nothing beside one is read
    with guard_bands(poison.NAN) as g:
        gsite = Site(ops, B, H, W, c0, c1, N, cluster)
        out_g, sk_g = gsite.launch(in_a)
        found = g.check()
    assert g.count > 0
    assert not found, "bytes outside a tensor were written\n" + "\n".join(map(format_violation, found))
    assert torch.equal(out_g, out_a) and torch.equal(sk_g, sk_a)
    assert ops.cluster_timeouts() == before


@pytest.mark.parametrize("name,B,H,W,c0,c1,N,splits", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_skip_fold_conv(ops, name, B, H, W, c0, c1, N, splits):
    check_case(ops, name, B, H, W, c0, c1, N, splits, cluster=False)


@pytest.mark.parametrize("name,B,H,W,c0,c1,N,splits", CLUSTER_CASES, ids=[c[0] for c in CLUSTER_CASES])
def test_skip_fold_in_launch_groupnorm(ops, name, B, H, W, c0, c1, N, splits):
    check_case(ops, name, B, H, W, c0, c1, N, splits, cluster=True)


def test_skip_fold_is_refused_where_it_cannot_run(ops):
    """no quiet second conv: the 128-channel tile (variant F) and the im2col path refuse skip_out"""
    lib = ops.L.load()
    B, H, W, cin, N = 32, 32, 32, 32, 128
    assert lib.ddk_conv_wino_skip_ok(B, H, W, cin, N) == 0
    par = params(cin, N)
    x = torch.zeros(B, H, W, cin, device=DEV)
    wu, wsk = ops.pack_conv_weight_wino(par["w3"].to(DEV)), ops.pack_conv_skip_weight_wino(par["w1"].to(DEV))
    with pytest.raises(ops.L.DDKError):
        ops.conv(ops.CONV3X3_S1, x, ops.pack_conv_weight(par["w3"].to(DEV)), None, w_wino=wu, skip_w=wsk)
    x = torch.zeros(2, 8, 8, cin, device=DEV)
    with pytest.raises(ops.L.DDKError):
        ops.conv(ops.CONV3X3_S1, x, ops.pack_conv_weight(par["w3"].to(DEV)), None, skip_w=wsk)


def _net(in_ch=8):
    from helpers import det_state, unet_cfg
    from models import Unet
    net = Unet(unet_cfg(128, in_ch))
    net.load_state_dict(det_state({k: v.shape for k, v in net.state_dict().items()}))
    return net.to(DEV).eval()


@pytest.mark.parametrize("batch", [5, 40])
def test_skip_fold_option_gives_the_same_unet(batch):
    """plan option DDK_OPT_SKIP_FOLD in the cfg4-shaped UNet through ddk_unet_forward: on vs off <= 2e-5 of the output's max (the bar of
    test_attention_split_gpu.py's option-in-UNet test) and not the same bits (both batches have eligible sites: the 16x16 and 8x8 ones,
    at batch 5 also the 32x32 up block, whose conv runs on the 64-channel tile there), on == on bit for bit with other data in between"""
    from utils import synthetic as syn
    net = _net()
    x = syn.synthetic_normal((batch, 8, 32, 32), f"skipfold.x{batch}").to(DEV)
    x2 = syn.synthetic_normal((batch, 8, 32, 32), f"skipfold.y{batch}").to(DEV)
    t = (torch.arange(batch, device=DEV) * 23) % 1000
    with torch.no_grad():
        plan = net.plan()
        y_on = net(x, t)
        y_other = net(x2, t)
        y_on2 = net(x, t)
        plan.set_option(plan.OPT_SKIP_FOLD, 0)
        y_off = net(x, t)
        plan.set_option(plan.OPT_SKIP_FOLD, 1)
        y_on3 = net(x, t)
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_on2) and torch.equal(y_on, y_on3)
    assert not torch.equal(y_on, y_other)
    assert not torch.equal(y_on, y_off)
    e = rel_err(y_on.cpu(), y_off.cpu())
    print(f"skip fold option, batch {batch}: on vs off {e:.3e}")
    assert e <= 2e-5


def test_skip_fold_in_the_sampler_matches_the_separate_launches():
    """ddk_sampler_run (hipGraph replay, the in-launch forms) at batch 32 with the option on (the default) vs off: 4 reverse steps from the
    same x_T with the same Philox stream end within 1e-4 of the output's max of each other (the bar of test_attention_split_gpu.py's
    sampler test), bit-stable across two runs, and no in-launch wait gives up"""
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
    for tag, on in (("on", 1), ("off", 0), ("on2", 1)):
        plan.set_option(plan.OPT_SKIP_FOLD, on)
        x = ops.randn((32, 32, 32, 3), DEV, seed=78, step=1000, stream_id=0)
        with torch.no_grad():
            plan.sample_nhwc(x, tables, 999, 996, seed=78, stream_id=0, use_graph=True)
        outs[tag] = x.clone()
    assert plan._cluster >= 1 and ops.cluster_timeouts() == before
    assert torch.isfinite(outs["on"]).all()
    assert torch.equal(outs["on"], outs["on2"])
    assert not torch.equal(outs["on"], outs["off"])
    e = float((outs["on"] - outs["off"]).abs().max()) / float(outs["on"].abs().max())
    print(f"skip fold in the sampler: on vs off {e:.3e}")
    assert e < 1e-4
