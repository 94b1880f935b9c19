"""ddk_attention_fold_partials (attn_fold_parts_kernel): the folded attention block's per-image matrix A and fold vectors
a1, a2 straight from the context's split records {max[32], den[32], ctx[32][32]}, in one launch instead of the merge launch +
ddk_attention_fold.

Every case is held, for all three outputs, to a torch-CPU fp64 reference (the merge formula, then A = W_out (ctx^T Wqg), a1, a2) at the
attention tests' bar, max|diff| / max|ref| < 2e-5, and at the same bar to the two-launch path on the same records; launches go A / B / A
through the same NaN-filled device buffers and must be bit-stable; with every tensor between guard bands no band is touched; a split
count outside the predicate is refused; a NaN or +Inf maximum in one image's records spoils exactly that image.  The kernel waits on
nothing, so no case can time out."""
import pytest
import torch

import poison
from guard import format_violation, guard_bands
from helpers import rel_err, to_nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-5
C, HEADS, DH, PART = 128, 4, 32, 2 * 32 + 32 * 32


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    from ddk import lib
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


def weights(bias, seed=0):
    """wqg, c1q, c2q, wout, bout on the CPU (fp32)"""
    return dict(wqg=rnd(C, C, seed=seed + 1, scale=C ** -0.5), c1q=rnd(C, seed=seed + 2), c2q=rnd(C, seed=seed + 3, scale=0.3),
                wout=rnd(C, C, seed=seed + 4, scale=C ** -0.5), bout=rnd(C, seed=seed + 5, scale=0.1) if bias else None)


def records(B, S, seed, kind="plain"):
    """[B][4][S][PART]: maxima of a few units, positive denominators, random unnormalised contexts.  kind "spread": the maxima differ by
    tens between the splits (the weights exp(m_s - M) matter); "underflow": split 0 of every (image, head) lies 120 below the others
    (its weight is exactly zero in fp32)"""
    m = rnd(B, HEADS, S, DH, seed=seed, scale=2.0)
    if kind == "spread":
        m = m + 25.0 * torch.arange(S).view(1, 1, S, 1) * (1 + 0.3 * rnd(B, HEADS, 1, DH, seed=seed + 3))
    if kind == "underflow":
        m[:, :, 0] -= 120.0
    den = 1.0 + 60.0 * torch.rand(B, HEADS, S, DH, generator=torch.Generator().manual_seed(seed + 1))
    ctx = rnd(B, HEADS, S, DH * DH, seed=seed + 2, scale=8.0)
    return torch.cat([m, den, ctx], dim=-1).contiguous()


def reference(part, w):
    """fp64 on the CPU: the merge formula, then A = W_out (ctx^T Wqg), a1 = W_out (ctx^T c1q), a2 = W_out (ctx^T c2q) + b_out"""
    p = part.double()
    B, _, S, _ = p.shape
    m, den, c = p[..., :DH], p[..., DH:2 * DH], p[..., 2 * DH:].reshape(B, HEADS, S, DH, DH)
    wt = torch.exp(m - m.max(dim=2, keepdim=True).values)
    ctx = (c * wt[..., None]).sum(2) / (den * wt).sum(2)[..., None]                                        # [B][h][d][e]
    wout = w["wout"].double()
    T = torch.einsum("bhde,hdc->bhec", ctx, w["wqg"].double().view(HEADS, DH, C)).reshape(B, C, C)         # [(h, e)][c]
    t1 = torch.einsum("bhde,hd->bhe", ctx, w["c1q"].double().view(HEADS, DH)).reshape(B, C)
    t2 = torch.einsum("bhde,hd->bhe", ctx, w["c2q"].double().view(HEADS, DH)).reshape(B, C)
    a2 = t2 @ wout.T
    return wout @ T, t1 @ wout.T, a2 + w["bout"].double() if w["bout"] is not None else a2


def on_device(w):
    return {k: (v.to(DEV) if v is not None else None) for k, v in w.items()}


def fold(ops, part, wd, out=None):
    return ops.attention_fold_partials(part, wd["wqg"], wd["c1q"], wd["c2q"], wd["wout"], wd["bout"], out=out)


def two_launch(ops, part, wd):
    """the path the entry replaces: ddk_linattn_merge, then ddk_attention_fold"""
    L = ops.L
    B = part.shape[0]
    ctx = ops.linattn_merge(part)
    A, a1, a2 = torch.empty(B, C, C, device=DEV), torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
    L.check(L.load().ddk_attention_fold(L.ptr(ctx), L.ptr(wd["wqg"]), L.ptr(wd["c1q"]), L.ptr(wd["c2q"]), L.ptr(wd["wout"]), L.ptr(wd["bout"]),
                                        L.ptr(A), L.ptr(a1), L.ptr(a2), B, C, HEADS, L.stream()), "attention_fold")
    return A, a1, a2


def held(tag, got, want):
    for name, g, r in zip(("A", "a1", "a2"), got, want):
        e = rel_err(g.cpu().double(), r.cpu().double())
        print(f"{tag} {name}: max|diff| / max|ref| {e:.3e}")
        assert e < BAR, (tag, name, e)


CASES = [(B, S, bias, "plain") for B in (1, 3) for S in (1, 2, 4, 8) for bias in (True, False)] + \
        [(3, 4, True, "spread"), (3, 8, False, "spread"), (3, 4, True, "underflow"), (1, 2, False, "underflow")]


@pytest.mark.parametrize("B,S,bias,kind", CASES, ids=[f"B{b}-S{s}-{'bias' if bi else 'nobias'}-{k}" for b, s, bi, k in CASES])
def test_fold_partials_matches_fp64_and_the_two_launches(ops, B, S, bias, kind):
    assert ops.L.load().ddk_attention_fold_partials_ok(C, HEADS, S) == 1
    part, w = records(B, S, 10 * S + B, kind), weights(bias, seed=100 * S)
    if kind == "underflow":
        p = part.double()
        assert float(torch.exp(p[:, :, 0, :DH] - p[:, :, 1:, :DH].max(dim=2).values).float().max()) == 0.0
    pd, wd = part.to(DEV), on_device(w)
    got = fold(ops, pd, wd)
    assert all(torch.isfinite(t).all() for t in got)
    held(f"{kind} B{B} S{S} vs fp64", got, reference(part, w))
    held(f"{kind} B{B} S{S} vs merge + fold", got, two_launch(ops, pd, wd))


def test_fold_partials_is_bit_stable_and_writes_only_its_outputs(ops):
    """A / B / A through the same NaN-filled device buffers: the two A runs are bit-identical; with every tensor between NaN guard bands
    the result keeps its bits and no band is touched"""
    B, S = 3, 4
    part_a, part_b, w = records(B, S, 1), records(B, S, 2, "spread"), weights(True)
    wd = on_device(w)
    bufs = (torch.empty(B, C, C, device=DEV), torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV))
    pbuf = torch.empty(B, HEADS, S, PART, device=DEV)
    runs = []
    for part in (part_a, part_b, part_a):
        pbuf.copy_(part)
        for t in bufs:
            t.fill_(float("nan"))
        fold(ops, pbuf, wd, out=bufs)
        runs.append([t.cpu() for t in bufs])
    assert all(torch.isfinite(t).all() for r in runs for t in r)
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[2]))
    assert not any(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
    with guard_bands(poison.NAN) as g:
        got = fold(ops, part_a.to(DEV), on_device(w))
        found = g.check()
        got = [t.cpu() for t in got]
    assert g.count >= 8                       # the records, five weights and three outputs
    assert not found, "bytes outside a tensor were written\n" + "\n".join(map(format_violation, found))
    assert all(torch.equal(x, y) for x, y in zip(got, runs[0]))


@pytest.mark.parametrize("S", [3, 5, 16])
def test_fold_partials_refuses_other_split_counts(ops, S):
    """no quiet second path inside the entry: _ok is 0, the wrapper raises and the entry itself returns an error without writing"""
    L = ops.L
    lib = L.load()
    assert lib.ddk_attention_fold_partials_ok(C, HEADS, S) == 0
    assert lib.ddk_attention_fold_partials_ok(C, 2, 4) == 0 and lib.ddk_attention_fold_partials_ok(64, 2, 4) == 0
    part, wd = records(1, S, 3).to(DEV), on_device(weights(True))
    with pytest.raises(L.DDKError):
        fold(ops, part, wd)
    A, a1, a2 = torch.zeros(1, C, C, device=DEV), torch.zeros(1, C, device=DEV), torch.zeros(1, C, device=DEV)
    rc = lib.ddk_attention_fold_partials(L.ptr(part), S, L.ptr(wd["wqg"]), L.ptr(wd["c1q"]), L.ptr(wd["c2q"]), L.ptr(wd["wout"]),
                                         L.ptr(wd["bout"]), L.ptr(A), L.ptr(a1), L.ptr(a2), 1, C, HEADS, L.stream())
    assert rc != 0
    torch.cuda.synchronize()
    assert not A.any() and not a1.any() and not a2.any()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_maximum_spoils_exactly_its_image(ops, bad):
    """a NaN / +Inf maximum in one record of image 1: that image's A, a1, a2 are non-finite with the isfinite mask of the two-launch
    path (NaN maximum: fmaxf skips it, exp(NaN - M) = NaN; +Inf: exp(Inf - Inf) = NaN -- the row of the context is NaN, and every
    entry of the image's matrix sums over it); images 0 and 2 keep the bits of the clean run"""
    B, S = 3, 4
    part, wd = records(B, S, 7), on_device(weights(True))
    clean = [t.cpu() for t in fold(ops, part.to(DEV), wd)]
    part[1, 2, 1, 5] = bad
    got = [t.cpu() for t in fold(ops, part.to(DEV), wd)]
    two = [t.cpu() for t in two_launch(ops, part.to(DEV), wd)]
    for g, t, c in zip(got, two, clean):
        assert not torch.isfinite(g[1]).any()
        assert torch.equal(torch.isfinite(g), torch.isfinite(t))
        assert torch.equal(g[0], c[0]) and torch.equal(g[2], c[2])


# batches 2 and 5 split the 32x32 map 16 ways (outside the predicate: the two launches stay), 9 splits it 8 ways, 17 4 ways
@pytest.mark.parametrize("B", [2, 5, 9, 17])
def test_from_x_matches_kv_context_then_fold(ops, B):
    """x -> ddk_attention_kv_partials -> ddk_attention_fold_partials against ddk_attention_kv_context -> ddk_attention_fold on a 32x32
    map; where the split count is outside the predicate the records are merged by ddk_linattn_merge instead, which must give
    ddk_attention_kv_context's bits"""
    L = ops.L
    lib = L.load()
    H = W = 32
    x = to_nhwc(rnd(B, C, H, W, seed=181) * 1.3 + 0.2).to(DEV)
    wq, g, be = rnd(3 * C, C, seed=182, scale=C ** -0.5).to(DEV), (1 + 0.2 * rnd(C, seed=185)).to(DEV), (0.1 * rnd(C, seed=186)).to(DEV)
    wg = wq * g.view(1, C)
    wd = dict(wqg=wg[:C].contiguous(), c1q=(wq @ g)[:C].contiguous(), c2q=(wq @ be)[:C].contiguous(), **on_device(
        {k: v for k, v in weights(True).items() if k in ("wout", "bout")}))
    ctx = ops.attention_kv_context(x, wq, g, be)
    part = ops.attention_kv_partials(x, wq, g, be)
    S = part.shape[2]
    assert S == lib.ddk_attention_kv_context_splits(B, H * W) == {2: 16, 5: 16, 9: 8, 17: 4}[B]
    assert torch.equal(ops.linattn_merge(part), ctx)
    want = torch.empty(B, C, C, device=DEV), torch.empty(B, C, device=DEV), torch.empty(B, C, device=DEV)
    L.check(lib.ddk_attention_fold(L.ptr(ctx), L.ptr(wd["wqg"]), L.ptr(wd["c1q"]), L.ptr(wd["c2q"]), L.ptr(wd["wout"]), L.ptr(wd["bout"]),
                                   L.ptr(want[0]), L.ptr(want[1]), L.ptr(want[2]), B, C, HEADS, L.stream()), "attention_fold")
    if not lib.ddk_attention_fold_partials_ok(C, HEADS, S):
        with pytest.raises(L.DDKError):
            fold(ops, part, wd)
        return
    held(f"from x, B{B} S{S}", fold(ops, part, wd), want)


def _net(in_ch=8):
    from helpers import det_state, unet_cfg
    from models import Unet
    net = Unet(unet_cfg(128, in_ch))
    net.load_state_dict(det_state({k: v.shape for k, v in net.state_dict().items()}))
    return net.to(DEV).eval()


@pytest.mark.parametrize("batch", [5, 40])
def test_fold_partials_option_gives_the_same_unet(ops, batch):
    """plan option DDK_OPT_ATTENTION_FOLD_PARTIALS in the cfg4-shaped UNet through ddk_unet_forward, on vs off, asserted at 2e-5 of the
    output's max.  Batch 40 (beyond the level chain's batch limit) splits the 32x32 attention sites 2 ways and takes the new launch:
    the outputs differ, measured 1.8e-6 of the output's max.  Batch 5 splits them 16 ways, outside the predicate: both settings run the two launches
    and the bits are the same.  on == on bit for bit with other data in between; no in-launch wait gives up."""
    from utils import synthetic as syn
    lib = ops.L.load()
    taken = lib.ddk_attention_fold_partials_ok(C, HEADS, lib.ddk_attention_kv_context_splits(batch, 32 * 32)) == 1
    assert taken == (batch == 40)
    net = _net()
    x = syn.synthetic_normal((batch, 8, 32, 32), f"foldparts.x{batch}").to(DEV)
    x2 = syn.synthetic_normal((batch, 8, 32, 32), f"foldparts.y{batch}").to(DEV)
    t = (torch.arange(batch, device=DEV) * 23) % 1000
    before = ops.cluster_timeouts()
    with torch.no_grad():
        plan = net.plan()
        y_on = net(x, t)
        y_other = net(x2, t)
        y_on2 = net(x, t)
        plan.set_option(plan.OPT_ATTENTION_FOLD_PARTIALS, 0)
        y_off = net(x, t)
        plan.set_option(plan.OPT_ATTENTION_FOLD_PARTIALS, 1)
        y_on3 = net(x, t)
    assert torch.isfinite(y_on).all()
    assert torch.equal(y_on, y_on2) and torch.equal(y_on, y_on3)
    assert not torch.equal(y_on, y_other)
    assert torch.equal(y_on, y_off) == (not taken)
    e = rel_err(y_on.cpu(), y_off.cpu())
    print(f"fold partials option, batch {batch}: on vs off {e:.3e}")
    assert e <= 2e-5
    assert ops.cluster_timeouts() == before


def test_fold_partials_in_the_sampler_matches_the_two_launches(ops):
    """ddk_sampler_run (hipGraph replay) at batch 32 (4 splits) with the option on (the default) vs off: 4 reverse steps from the same
    x_T with the same Philox stream, asserted at 2e-5 of the output's max (measured 5.1e-8), bit-stable across two runs, and no
    in-launch wait gives up"""
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
        plan.set_option(plan.OPT_ATTENTION_FOLD_PARTIALS, on)
        x = ops.randn((32, 32, 32, 3), DEV, seed=78, step=1000, stream_id=0)
        with torch.no_grad():
            plan.sample_nhwc(x, tables, 999, 996, seed=78, stream_id=0, use_graph=True)
        outs[tag] = x.clone()
    assert ops.cluster_timeouts() == before
    assert torch.isfinite(outs["on"]).all()
    assert torch.equal(outs["on"], outs["on2"])
    assert not torch.equal(outs["on"], outs["off"])
    e = float((outs["on"] - outs["off"]).abs().max()) / float(outs["on"].abs().max())
    print(f"fold partials in the sampler: on vs off {e:.3e}")
    assert e < 2e-5
