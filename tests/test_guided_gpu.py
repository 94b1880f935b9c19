"""Diffusion Posterior Sampling on the device: the measurement distance and its adjoint, the x0 op, the guided
update, one whole step, a 4-step chain and the dDDPM step against the float64 reference tests/guidance_ref.py, the edges of the loss, and
the autograd path when nothing is trained."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import guidance_ref as GR
from guard import guard_bands, rehouse
from helpers import dddpm_cfg, ddpm_cfg, det_load, rel_err, to_nchw, to_nhwc
from poison import WORDS, poisoned_allocations
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _G():
    from models.diffusion import guidance
    return guidance


def _AG():
    from ddk import autograd
    return autograd


def _ops():
    from ddk import ops
    return ops


# ---------------------------------------------------------------- 1. MeasureDistFn against the reference
def _dist_case(n, masked, response, gain, B, C, h, w, key):
    """(operator, img, y, gout) on the host, NCHW fp32: block means spread over [-1.5, 1.5] so that both branches of a saturating
    response occur at every n, and no gain u within 1e-5 of a saturation bound (an fp32 and a float64 evaluation would take different
    branches there; the bounds themselves are test_saturation_bounds_are_inclusive's)"""
    G = _G()
    H, W = h * n, w * n
    low = 0.6 * syn.synthetic_normal((B, C, h, w), key + ".low")
    img = low.repeat_interleave(n, 2).repeat_interleave(n, 3) + 0.3 * syn.synthetic_normal((B, C, H, W), key + ".img")
    mask = (syn.synthetic_input((B, h, w), key + ".mask") > -0.2).float() if masked else None
    op = G.Operator("mean", (C, H, W), n=n, mask=mask, response=response, gain=gain)
    if response == "saturate":          # a block that lands within 1e-5 of a bound is moved off it by 0.01
        near = ((gain * GR.linear(op, img.double())).abs() - 1).abs() < 1e-5
        img = img + 0.01 * near.float().repeat_interleave(n, 2).repeat_interleave(n, 3)
        assert not bool((((gain * GR.linear(op, img.double())).abs() - 1).abs() < 1e-5).any())
    y = syn.synthetic_input((B, C, h, w), key + ".y")
    gout = 1.0 + 0.5 * syn.synthetic_input((B,), key + ".gout")
    return op, img, y, gout


def _device_dist(op, img, y, gout):
    """(dist, v) of AG.MeasureDistFn on the device for host NCHW operands, back on the host (v as NCHW)"""
    AG = _AG()
    x = to_nhwc(img).to(DEV).requires_grad_(True)
    op.to(DEV)
    dist = AG.MeasureDistFn.apply(x, to_nhwc(y).to(DEV), op)
    (v,) = torch.autograd.grad((dist * gout.to(DEV)).sum(), x)
    return dist.detach().cpu(), to_nchw(v.cpu())


def _deviations(op, img, y, gout, got):
    """relative deviation of got = (dist, v) from the float64 reference: the largest per-image error of dist over dist, the largest
    error of v over max |v|"""
    d64, v64 = GR.dist_and_grad(op, img.double(), y.double(), gout.double())
    return float(((got[0].double() - d64).abs() / d64).max()), float((got[1].double() - v64).abs().max() / v64.abs().max())


# The reduction's launch shapes (csrc/guidance.hip): an image of m = h w C measured elements takes ONE launch up to m = 2048 and
# min(ceil(m / 2048), 64) workgroups plus a finishing launch above; the slice count stops growing at m = 64 * 2048 = 131072.
BOUNDARY_SHAPES = [(16, 16, 8), (19, 27, 4), (128, 128, 8), (128, 129, 8)]     # m = 2048 | 2052 and 131072 | 132096


def _group(n, masked):
    """the 36 cases of one (n, mask): both responses with gain 1 and 2.5, B in {1, 3}, C in {1, 3, 8}, maps of 16 x 16 and 16 x 32"""
    for response, gain in (("linear", 1.0), ("saturate", 1.0), ("saturate", 2.5)):
        for B in (1, 3):
            for C in (1, 3, 8):
                for h, w in ((16, 16), (16, 32)):
                    yield _dist_case(n, masked, response, gain, B, C, h, w, f"g1.{n}.{masked}.{response}.{gain}.{B}.{C}.{w}")


def _boundary_case(h, w, C):
    return _dist_case(1, True, "saturate", 2.5, 2, C, h, w, f"g1.edge.{h}.{w}.{C}")


_FP32 = []


def _torch_fp32_deviation():
    """(dist, v): the largest relative deviation, over EVERY case of this section, of the same formula evaluated by torch in fp32 on the
    CPU from its float64 evaluation.  Made once (three seconds of host time) and shared: one image's dist is a single fp32 number whose
    own rounding is anywhere between 0 and 2^-24, so a bound taken from a handful of them would be luck."""
    if not _FP32:
        worst = [0.0, 0.0]
        cases = [c for n in (1, 2, 4, 8) for masked in (False, True) for c in _group(n, masked)] + [_boundary_case(*s) for s in BOUNDARY_SHAPES]
        for op, img, y, gout in cases:
            worst = [max(a, b) for a, b in zip(worst, _deviations(op, img, y, gout, GR.dist_and_grad(op, img, y, gout)))]
        _FP32.append(tuple(worst))
    return _FP32[0]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_measure_dist_forward_and_backward_against_the_reference(n, masked):
    """dist and v = d(sum gout dist) / d img against the float64 reference, 36 cases per (n, mask) (_group).  The bound is measured, not
    fixed: 4 x the deviation of torch's own fp32 evaluation on the CPU (_torch_fp32_deviation; the kernel's double accumulation should do
    better than torch's fp32 sum).
    Measured, torch fp32 on the CPU: dist 1.01e-7 and v 2.69e-7 on one host, 1.15e-7 and 2.75e-7 on another (torch's vectorised sums
    differ between CPUs), so the kernel is held to about 4.3e-7 and 1.1e-6.  Measured on an MI355X, largest per (n, mask) group: dist
    4.3e-8 .. 6.0e-8 -- the rounding of the result to fp32 and nothing else -- and v 1.6e-7 .. 2.7e-7 (largest at n = 8, where a block
    mean is 64 fp32 additions); the boundary shapes: dist 1.6e-8 .. 3.6e-8, v 1.4e-7 .. 1.5e-7."""
    ref32 = _torch_fp32_deviation()
    worst = [0.0, 0.0]
    for op, img, y, gout in _group(n, masked):
        got = _device_dist(op, img, y, gout)
        assert got[0].shape == (img.shape[0],) and got[1].shape == img.shape
        worst = [max(a, b) for a, b in zip(worst, _deviations(op, img, y, gout, got))]
    print(f"\nn={n} mask={masked}: torch fp32 dist {ref32[0]:.2e} v {ref32[1]:.2e} | device dist {worst[0]:.2e} v {worst[1]:.2e}")
    assert ref32[0] > 0 and ref32[1] > 0
    assert worst[0] <= 4 * ref32[0] and worst[1] <= 4 * ref32[1]


@pytest.mark.parametrize("h,w,C", BOUNDARY_SHAPES)
def test_measure_dist_on_each_side_of_the_launch_shape_boundaries(h, w, C):
    """one shape on each side of both boundaries (n = 1, B = 2, masked, saturating), held to the same measured bound"""
    lib = _ops().L.load()
    assert (lib.ddk_measure_residual_workspace_bytes(2, h, w, C, 1) // 16) == {2048: 0, 2052: 2, 131072: 64, 132096: 64}[h * w * C]
    ref32 = _torch_fp32_deviation()
    op, img, y, gout = _boundary_case(h, w, C)
    dev = _deviations(op, img, y, gout, _device_dist(op, img, y, gout))
    print(f"\n{h}x{w}x{C}: torch fp32 dist {ref32[0]:.2e} v {ref32[1]:.2e} | device dist {dev[0]:.2e} v {dev[1]:.2e}")
    assert dev[0] <= 4 * ref32[0] and dev[1] <= 4 * ref32[1]


# ---------------------------------------------------------------- 2. edges of the loss
def test_saturation_bounds_are_inclusive():
    """gain u exactly on +-1 has slope gain (torch's clamp backward includes its bounds), one ulp outside it has slope 0 -- at n = 1 and
    for a block mean that is exact in fp32"""
    ops, G = _ops(), _G()
    gain = 2.0
    up, dn = float(np.nextafter(np.float32(0.5), np.float32(1))), float(np.nextafter(np.float32(0.5), np.float32(0)))
    vals = torch.tensor([0.5, -0.5, up, -up, dn, -dn, 0.0, 0.75], dtype=torch.float32)
    img = vals.reshape(1, 1, 8, 1).repeat(1, 2, 1, 3).contiguous()                           # [B=1, H=2, W=8, C=3]
    y = torch.full_like(img, 0.25)
    r, dist = ops.measure_residual(img.to(DEV), y.to(DEV), None, 1, "saturate", gain)
    want = torch.tensor([gain * 0.75, gain * -1.25, 0, 0, gain * (gain * dn - 0.25), gain * (-gain * dn - 0.25), gain * -0.25, 0], dtype=torch.float32)
    assert torch.equal(r.cpu(), want.reshape(1, 1, 8, 1).expand(1, 2, 8, 3))
    x = img.clone().requires_grad_(True)
    ref = ((torch.clamp(gain * x, -1, 1) - y) ** 2).flatten(1).sum(1).sqrt()
    ref.sum().backward()
    op = G.Operator("mean", (3, 2, 8), response="saturate", gain=gain)
    xd = img.to(DEV).requires_grad_(True)
    d = _AG().MeasureDistFn.apply(xd, y.to(DEV), op)
    (v,) = torch.autograd.grad(d.sum(), xd)
    assert abs(float(d.detach()) / float(ref.detach()) - 1) <= 4 * U
    assert bool((v.cpu()[0, 0, :, 0] != 0).eq(torch.tensor([1, 1, 0, 0, 1, 1, 1, 0], dtype=torch.bool)).all())
    assert (v.cpu() - x.grad).abs().max() <= 4 * U * x.grad.abs().max()
    # a 2 x 2 block whose mean is exactly 0.5 / just above it
    blk = torch.tensor([[0.25, 0.75], [0.5, 0.5]]).reshape(1, 2, 2, 1)
    r2, _ = ops.measure_residual(torch.cat([blk, blk + torch.tensor([[0.0, 2.0 ** -22], [0.0, 0.0]]).reshape(1, 2, 2, 1)]).to(DEV),
                                 torch.zeros(2, 1, 1, 1, device=DEV), None, 2, "saturate", gain)
    assert r2.flatten().tolist() == [gain * 1.0, 0.0]


@pytest.mark.parametrize("n,C,h,w", [(1, 3, 16, 16), (4, 3, 16, 16), (2, 8, 16, 32)])
def test_zero_distance_gives_a_zero_finite_gradient_and_the_unguided_step(n, C, h, w):
    """y = phi(A img) of an img on a 1/64 grid (block sums exact in fp32): dist == 0 exactly, v == 0 and finite -- no 0 / 0 -- and a guided
    update with that v and a large zeta is the unguided update bit for bit; the image beside it has dist > 0 and is guided"""
    ops, G, AG = _ops(), _G(), _AG()
    img = (syn.synthetic_input((2, h * n, w * n, C), f"g2.zero.{n}") * 64).round() / 64
    mask = (syn.synthetic_input((2, h, w), "g2.zero.mask") > 0).float()
    for response, gain in (("linear", 1.0), ("saturate", 2.5)):
        op = G.Operator("mean", (C, h * n, w * n), n=n, mask=mask, response=response, gain=gain).to(DEV)
        y = op.measure(img.to(DEV))
        y[1] += 0.125 * mask[1].to(DEV).unsqueeze(-1)
        x = img.to(DEV).requires_grad_(True)
        dist = AG.MeasureDistFn.apply(x, y, op)
        (v,) = torch.autograd.grad(dist.sum(), x)
        assert float(dist[0]) == 0.0 and float(dist[1]) > 0
        assert bool(torch.isfinite(v).all()) and bool((v[0] == 0).all()) and bool((v[1] != 0).any())
        m = _pixel_model()
        tables, _ = m._guided_tables("20", False, 0.0, G.zeta_table(50.0, 20))()
        rule = {k: tables[k] for k in m.GUIDED_RULE}
        t = torch.tensor([7, 7], device=DEV)
        eps, z = (syn.synthetic_normal(tuple(img.shape), f"g2.zero.{k}").to(DEV) for k in ("eps", "z"))
        plain = ops.p_sample_update_(img.to(DEV).clone(), eps, t, noise=z, **rule)
        guided = ops.p_sample_update_guided_(img.to(DEV).clone(), eps, v.contiguous(), t, **rule, zeta=tables["zeta"], noise=z)
        assert torch.equal(guided[0], plain[0]) and not torch.equal(guided[1], plain[1])


@pytest.mark.parametrize("h,w,C", [(16, 16, 3), (16, 32, 8)])
def test_a_nan_in_one_measurement_stays_in_its_image(h, w, C):
    """(one launch, and sliced with a finishing launch)"""
    op, img, y, gout = _dist_case(2, True, "saturate", 2.5, 3, C, h, w, f"g2.nan.{C}")
    clean = _device_dist(op, img, y, gout)
    pos = tuple(int(i) for i in torch.nonzero(op.mask.cpu()[1])[5])
    y2 = y.clone()
    y2[1, C - 1, pos[0], pos[1]] = float("nan")
    dist, v = _device_dist(op, img, y2, gout)
    assert bool(torch.isnan(dist[1])) and bool(torch.isnan(v[1]).all())
    for b in (0, 2):
        assert torch.equal(dist[b], clean[0][b]) and torch.equal(v[b], clean[1][b])


def _all_new_ops(dev_inputs):
    """every new entry once, on operands already on the device: (dist, v, x0, dx, deps, x_guided)"""
    ops, AG = _ops(), _AG()
    op, img, y, gout, eps, t, tables = dev_inputs
    x = img.clone().requires_grad_(True)
    e = eps.clone().requires_grad_(True)
    x0 = AG.PredictX0Fn.apply(x, e, t, tables["c_recip"], tables["c_recipm1"], True)
    dist = AG.MeasureDistFn.apply(x0, y, op)
    dx, deps = torch.autograd.grad((dist * gout).sum(), (x, e))
    r, _ = ops.measure_residual(x0.detach(), y, op.mask, op.n, op.response, op.gain)
    v = ops.measure_adjoint(r, dist.detach(), gout, op.n)
    xg = ops.p_sample_update_guided_(rehouse(img.clone()), eps, rehouse(dx.contiguous()), t, **{k: tables[k] for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")},
                                     zeta=tables["zeta"], seed=5, stream_id=1)
    return [a.detach().clone() for a in (dist, v, x0, dx, deps, xg)]


@pytest.mark.parametrize("h,w,C", [(16, 16, 3), (19, 27, 4)])
def test_outputs_are_fully_written_nothing_else_is_and_two_calls_agree(h, w, C):
    """guard bands around every tensor (tests/guard.py), poisoned allocations (tests/poison.py) and a second call: the same bits each
    time, on the one-launch and on the sliced shape of the reduction"""
    G = _G()
    m = _pixel_model()
    tables_dev, _ = m._guided_tables("20", True, 0.5, G.zeta_table(0.7, 20))()
    tables_host = {k: v.cpu() for k, v in tables_dev.items()}

    def inputs():
        op, img, y, gout = _dist_case(1, True, "saturate", 2.5, 2, C, h, w, f"g2.guard.{h}")
        op.mask = op.mask.cpu().to(DEV)
        tb = {k: v.to(DEV) for k, v in tables_host.items()}
        return (op, to_nhwc(img).to(DEV), to_nhwc(y).to(DEV), gout.to(DEV), to_nhwc(syn.synthetic_normal(tuple(img.shape), "g2.guard.eps")).to(DEV),
                torch.tensor([3, 0]).to(DEV), tb)
    plain = _all_new_ops(inputs())
    again = _all_new_ops(inputs())
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    for word in WORDS:
        for skew in (0, 16):
            with guard_bands(word, skew=skew) as g:
                got = _all_new_ops(inputs())
                assert g.check() == [] and g.count >= 8
            assert all(torch.equal(a, b) for a, b in zip(plain, got)), (hex(word), skew)
        with poisoned_allocations(word) as p:
            got = _all_new_ops(inputs())
            assert p.count >= 6
        assert all(torch.equal(a, b) for a, b in zip(plain, got)), hex(word)


# ---------------------------------------------------------------- 3. PredictX0Fn
@pytest.mark.parametrize("clip", [True, False])
def test_predict_x0_against_torch_including_the_bounds(clip):
    """forward and both gradients against the same expression in torch on the CPU, operation for operation (two products and a
    difference; one product per gradient), so bit for bit; elements exactly on +-1 keep their gradient"""
    AG = _AG()
    cr = torch.tensor([2.0, 1.25, 1.0078125, 3.5])
    crm1 = torch.tensor([1.0, 0.75, 0.125, 3.25])
    t = torch.tensor([0, 2, 3])
    x = syn.synthetic_input((3, 8, 8, 3), "g3.x")
    eps = syn.synthetic_normal((3, 8, 8, 3), "g3.eps")
    x[0, 0, :4, 0], eps[0, 0, :4, 0] = torch.tensor([0.75, -0.75, 1.0, 0.25]), torch.tensor([0.5, -0.5, 1.0, 1.5])       # 1, -1, 1, -1 exactly
    w = syn.synthetic_normal((3, 8, 8, 3), "g3.w")
    xr, er = x.clone().requires_grad_(True), eps.clone().requires_grad_(True)
    x0r = cr[t].view(3, 1, 1, 1) * xr - crm1[t].view(3, 1, 1, 1) * er
    if clip:
        x0r = x0r.clamp(-1, 1)
    (x0r * w).sum().backward()
    xd, ed = x.to(DEV).requires_grad_(True), eps.to(DEV).requires_grad_(True)
    x0 = AG.PredictX0Fn.apply(xd, ed, t.to(DEV), cr.to(DEV), crm1.to(DEV), clip)
    dx, de = torch.autograd.grad((x0 * w.to(DEV)).sum(), (xd, ed))
    assert x0r[0, 0, :4, 0].tolist() == [1.0, -1.0, 1.0, -1.0]
    assert torch.equal(x0.detach().cpu(), x0r.detach())
    assert torch.equal(dx.cpu(), xr.grad) and torch.equal(de.cpu(), er.grad)
    assert bool((dx.cpu()[0, 0, :4, 0] != 0).all())
    if clip:
        assert 0 < int((xr.grad == 0).sum()) < x.numel()


# ---------------------------------------------------------------- 4. the update kernel
def _pixel_model(chan=32, dims=(1, 2), size=16):
    from models import DDPM, Unet
    cfg = ddpm_cfg(chan, 3, size)
    cfg["unet_dims"] = dims
    key = ("pixel", chan, dims, size)
    if key not in _MODELS:
        _MODELS[key] = (det_load(DDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval(), cfg)
    return _MODELS[key][0]


_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the models this module shares live as long as the module: a model kept beyond it keeps its packed weights registered, which
    the refresh counters of tests/test_pack_jobs_gpu.py would see"""
    yield
    _MODELS.clear()
    import gc
    gc.collect()


@pytest.mark.parametrize("ddim", [False, True])
def test_guided_update_with_zero_zeta_is_the_plain_update(ddim):
    """bit for bit on ancestral and DDIM tables, rows 0 (no draw), 1 and the last, with injected noise and with Philox, whatever g holds"""
    ops, G = _ops(), _G()
    m = _pixel_model()
    tables, _ = m._guided_tables("20", ddim, 0.5 if ddim else 0.0, G.zeta_table(0.0, 20))()
    rule = {k: tables[k] for k in m.GUIDED_RULE}
    shape = (4, 16, 16, 3)
    x, eps, z, g = (syn.synthetic_normal(shape, f"g4.{k}").to(DEV) for k in ("x", "eps", "z", "g"))
    g[0, 0, 0, 0], g[1, 0, 0, 0] = float("nan"), float("inf")
    t = torch.tensor([0, 1, 19, 7], device=DEV)
    for noise, seed in ((z, 0), (None, 123456789)):
        plain = ops.p_sample_update_(x.clone(), eps, t, noise=noise, seed=seed, stream_id=3, **rule)
        guided = ops.p_sample_update_guided_(x.clone(), eps, g, t, **rule, zeta=tables["zeta"], noise=noise, seed=seed, stream_id=3)
        assert torch.equal(plain, guided) and bool(torch.isfinite(guided).all())


def test_guided_update_against_float64():
    """x = p_step(...) - zeta[t] g.  p_step's value o is held bit for bit by the zero-zeta case; what the guided kernel adds is the
    product zeta g and the difference, each rounded once to fp32 from the fp32 table entry: |got - (o - zeta g)| <= 2^-24 (|zeta g| +
    |o - zeta g|), evaluated in float64 (the third operation, the table's own rounding of zeta, is the same number on both sides)"""
    ops, G = _ops(), _G()
    m = _pixel_model()
    tables, _ = m._guided_tables("20", True, 0.5, G.zeta_table(np.linspace(0.0, 3.0, 20), 20))()
    rule = {k: tables[k] for k in m.GUIDED_RULE}
    shape = (4, 16, 16, 3)
    x, eps, z, g = (syn.synthetic_normal(shape, f"g4b.{k}").to(DEV) for k in ("x", "eps", "z", "g"))
    t = torch.tensor([0, 1, 19, 7], device=DEV)
    o = ops.p_sample_update_(x.clone(), eps, t, noise=z, **rule).double().cpu()
    got = ops.p_sample_update_guided_(x.clone(), eps, g, t, **rule, zeta=tables["zeta"], noise=z).double().cpu()
    zg = tables["zeta"].double().cpu()[t.cpu()].view(4, 1, 1, 1) * g.double().cpu()
    assert torch.equal(got[0], o[0])                                        # row 0 of this table has zeta = 0
    assert bool(((got - (o - zg)).abs() <= U * (zg.abs() + (o - zg).abs())).all())
    assert float((got - o).abs().max()) > 1.0


# ---------------------------------------------------------------- 5. one whole guided step on a tiny model
def _host_state(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def _step_operators(G, shape):
    C, H, W = shape
    mask = (syn.synthetic_input((2, H, W), "g5.mask") > 0).float()
    return {"mean4": G.make_operator(("mean", 4), shape), "pixels": G.make_operator(("mean", 1), shape, mask=mask),
            "blur": G.make_operator("gauss", shape), "psf": G.make_operator("disk", shape)}


def _per_image_rel(a, b):
    return max(rel_err(a[i], b[i]) for i in range(a.shape[0]))


@pytest.mark.parametrize("which", ["mean4", "pixels", "blur", "psf"])
def test_one_guided_step_on_a_tiny_model(which):
    """unet_chan 32, dims (1, 2), 3 x 16 x 16, B = 2, row 2 of a 20-step chain (t = 100, where about half of x0 is clipped): eps_hat, dist,
    g and x_{t-1} with an injected draw against the float64 reference.  Bounds: those tests/test_backward_gpu.py holds this network's
    forward and input gradient to, 5e-5 and 2e-4 relative; dist is a forward quantity, g is that input gradient up to a per-image scale
    (so it is held per image), and x_{t-1} contains zeta g.
    Measured on an MI355X: eps_hat 7.6e-7, dist 3.2e-9 .. 7.7e-8, g 1.0e-6 .. 1.3e-6, x_{t-1} 4.0e-7 .. 4.7e-7."""
    G = _G()
    m = _pixel_model()
    cfg = _MODELS[("pixel", 32, (1, 2), 16)][1]
    sd = _host_state(m)
    op = _step_operators(G, (3, 16, 16))[which]
    k = 2
    tables, use = m._guided_tables("20", False, 0.0, G.zeta_table(2.0, 20))()
    host_tables = {n: v.cpu() for n, v in tables.items()}
    x = 0.9 * syn.synthetic_input((2, 3, 16, 16), "g5.x")
    z = syn.synthetic_normal((2, 3, 16, 16), "g5.z")
    y = GR.measure(op, 0.8 * syn.synthetic_input((2, 3, 16, 16), "g5.truth").double()).float()
    eps_model = lambda xx, kk: GR.unet(sd, cfg, xx, torch.full((2,), use[kk]), pre="latent_model.")
    e_r, d_r, g_r, x_r = GR.guided_step(eps_model, host_tables, op, y.double(), x.double(), k, z.double())
    xd = to_nhwc(x).to(DEV)
    op.to(DEV)
    with G.frozen(m):
        e, d, g = m._guided_step(xd, to_nhwc(y).to(DEV), op, torch.full((2,), use[k], device=DEV), torch.full((2,), k, device=DEV), tables,
                                 noise=to_nhwc(z).to(DEV))
    errs = (rel_err(to_nchw(e.cpu()), e_r), float(((d.cpu().double() - d_r).abs() / d_r).max()), _per_image_rel(to_nchw(g.cpu()), g_r),
            rel_err(to_nchw(xd.cpu()), x_r))
    print(f"\n{which}: eps_hat {errs[0]:.2e} dist {errs[1]:.2e} g {errs[2]:.2e} x_prev {errs[3]:.2e}; |zeta g| max {2.0 * float(g_r.abs().max()):.3g}")
    assert float(g_r.abs().max()) > 1e-3
    assert errs[0] < 5e-5 and errs[1] < 5e-5 and errs[2] < 2e-4 and errs[3] < 2e-4


# ---------------------------------------------------------------- 6. the autograd path when nothing is trained
def _grad_state(model):
    return ([p.grad.clone() for p in model.parameters()], [p.requires_grad for p in model.parameters()], [mod.training for mod in model.modules()])


def _same_state(model, state):
    grads, flags, modes = state
    return (all(torch.equal(p.grad, g) for p, g in zip(model.parameters(), grads)) and [p.requires_grad for p in model.parameters()] == flags
            and [mod.training for mod in model.modules()] == modes)


def test_the_input_only_backward_and_what_a_guided_chain_leaves_behind(monkeypatch):
    """the input gradient with every weight frozen equals the input gradient of a full backward, within the full backward's own bound
    (2e-4 relative, tests/test_backward_gpu.py); no `.grad`, requires_grad flag or training mode differs after restore_guided, nor after
    an exception in the middle of its chain"""
    from models import DDPM, Unet
    G, ops = _G(), _ops()
    cfg = ddpm_cfg(32, 3, 16)
    cfg["unet_dims"] = (1, 2)
    m = det_load(DDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).train()
    m.latent_model.mid_attn.eval()
    list(m.parameters())[2].requires_grad_(False)
    unet = m.latent_model
    x = to_nhwc(syn.synthetic_input((2, 3, 16, 16), "g6.x")).to(DEV)
    w = to_nhwc(syn.synthetic_normal((2, 3, 16, 16), "g6.w")).to(DEV)
    t = torch.tensor([3, 700], device=DEV)
    xf = x.clone().requires_grad_(True)
    (unet.forward_nhwc(xf, t) * w).sum().backward()                 # the full backward: every parameter gradient is made too
    assert all(p.grad is not None for p in m.parameters() if p.requires_grad)
    for i, p in enumerate(m.parameters()):
        p.grad = torch.full_like(p, 0.5 + i)
    state = _grad_state(m)
    with G.frozen(m):
        xi = x.clone().requires_grad_(True)
        (gi,) = torch.autograd.grad((unet.forward_nhwc(xi, t) * w).sum(), xi)
    err = rel_err(gi.cpu(), xf.grad.cpu())
    print(f"\ninput-only against full backward: {err:.2e}")
    assert err < 2e-4 and _same_state(m, state)
    y = torch.zeros(2, 3, 4, 4)
    out = m.restore_guided(y, ("mean", 4), zeta=1.0, respacing="3", seed=1)
    assert out.shape == (2, 3, 16, 16) and bool(torch.isfinite(out).all()) and _same_state(m, state)
    calls = []
    real = ops.p_sample_update_guided_

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("mid-chain")
        return real(*a, **k)
    monkeypatch.setattr(ops, "p_sample_update_guided_", failing)
    with pytest.raises(RuntimeError, match="mid-chain"):
        m.restore_guided(y, ("mean", 4), zeta=1.0, respacing="3", seed=1)
    assert len(calls) == 2 and _same_state(m, state)


# ---------------------------------------------------------------- 7. a 4-step chain
@pytest.mark.parametrize("ddim,eta", [(False, 0.0), (True, 0.5)])
def test_four_step_chain_against_the_reference_chain(ddim, eta):
    """respacing "4", injected noise, A = 2 x 2 block means with a saturating sensor, against the float64 reference chain.  The bound is
    measured here: the reference chain is also run in fp32 on the CPU, and the device may differ from the float64 chain by 8 x their
    deviation (four steps compound the forward's rounding through a gradient).
    Measured, max |x_0 - x_0(float64)| with max |x_0| = 1.03: torch fp32 on the CPU 8.0e-5 (ancestral) and 6.2e-5 (DDIM eta 0.5) on
    one host, 7.7e-5 and 1.3e-4 on another; an MI355X 7.5e-5 and 1.5e-4, against bounds of 6.4e-4 and 4.9e-4.
    Philox draws: the same seed and x_T twice give the same bits, another seed other bits."""
    G = _G()
    m = _pixel_model()
    cfg = _MODELS[("pixel", 32, (1, 2), 16)][1]
    op = G.make_operator(("mean", 2), (3, 16, 16), response="saturate", gain=1.5)
    zeta = [0.5, 1.0, 1.5, 2.0]
    y = GR.measure(op, 0.8 * syn.synthetic_input((2, 3, 16, 16), "g7.truth").double()).float()
    x_T = syn.synthetic_normal((2, 3, 16, 16), "g7.xT")
    noise = torch.stack([syn.synthetic_normal((2, 3, 16, 16), f"g7.z{j}") for j in range(4)])
    tables, use = m._guided_tables("4", ddim, eta, G.zeta_table(zeta, 4))()
    host_tables = {n: v.cpu() for n, v in tables.items()}
    assert len(use) == 4
    refs = {}
    for dt in (torch.float32, torch.float64):
        sd = {k: (v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu()) for k, v in m.state_dict().items()}
        eps_model = lambda xx, kk: GR.unet(sd, cfg, xx, torch.full((2,), use[kk]), pre="latent_model.")
        refs[dt] = GR.guided_chain(eps_model, host_tables, op, y.to(dt), x_T.to(dt), noise.to(dt))
    dev32 = float((refs[torch.float32].double() - refs[torch.float64]).abs().max())
    got = m.restore_guided(y, ("mean", 2), zeta=zeta, response="saturate", gain=1.5, respacing="4", ddim=ddim, eta=eta, x_T=x_T, noise=noise)
    err = float((got.cpu().double() - refs[torch.float64]).abs().max())
    print(f"\nddim={ddim}: torch fp32 chain {dev32:.2e}, device chain {err:.2e} (max |x_0| {float(refs[torch.float64].abs().max()):.3g})")
    assert dev32 > 0 and err <= 8 * dev32
    a = m.restore_guided(y, ("mean", 2), zeta=zeta, response="saturate", gain=1.5, respacing="4", ddim=ddim, eta=eta, x_T=x_T, seed=77)
    b = m.restore_guided(y, ("mean", 2), zeta=zeta, response="saturate", gain=1.5, respacing="4", ddim=ddim, eta=eta, x_T=x_T, seed=77)
    c = m.restore_guided(y, ("mean", 2), zeta=zeta, response="saturate", gain=1.5, respacing="4", ddim=ddim, eta=eta, x_T=x_T, seed=78)
    assert torch.equal(a, b) and not torch.equal(a, c) and bool(torch.isfinite(a).all())


# ---------------------------------------------------------------- 8. dDDPM: one step through the decoder
def _latent_model(u_mode):
    from models import DownsampleDDPM, Unet
    unet_in = 3 if u_mode == "deterministic" else 8
    cfg = dddpm_cfg(32, 16, 1)
    cfg.update(d_mode=u_mode, u_mode=u_mode, unet_in=unet_in, d_n_blocks=1, u_n_blocks=1)
    key = ("latent", u_mode)
    if key not in _MODELS:
        _MODELS[key] = (det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval(), cfg)
    return _MODELS[key]


@pytest.mark.parametrize("which", ["mean2", "psf"])
@pytest.mark.parametrize("u_mode", ["convolutional_res", "convolutional", "deterministic"])
def test_one_guided_step_through_the_decoder(u_mode, which):
    """the smallest dddpm_cfg (32 channels, a 16 x 16 image, an 8 x 8 latent, one block per resampler), every u_mode: one step in the
    latent with the measurement in pixels, behind the decoder, against the float64 reference.  Bounds as for the pixel model's step.
    Measured on an MI355X over the six cases: eps_hat 2.7e-6 .. 3.0e-6, dist 7.1e-8 .. 2.2e-7, g 4.7e-6 .. 7.5e-6, x_{t-1} 1.7e-6 .. 4.0e-6."""
    G, AG = _G(), _AG()
    m, cfg = _latent_model(u_mode)
    sd = _host_state(m)
    C = cfg["unet_in"]
    op = G.make_operator(("mean", 2) if which == "mean2" else "disk", (3, 16, 16))
    k = 2
    tables, use = m._guided_tables("20", False, 0.0, G.zeta_table(2.0, 20))()
    host_tables = {n: v.cpu() for n, v in tables.items()}
    x = 0.9 * syn.synthetic_input((2, C, 8, 8), "g8.x")
    z = syn.synthetic_normal((2, C, 8, 8), "g8.z")
    y = GR.measure(op, 0.8 * syn.synthetic_input((2, 3, 16, 16), "g8.truth").double()).float()
    eps_model = lambda xx, kk: GR.unet(sd, cfg, xx, torch.full((2,), use[kk]), pre="latent_model.")
    e_r, d_r, g_r, x_r = GR.guided_step(eps_model, host_tables, op, y.double(), x.double(), k, z.double(), decode=GR.decoder(sd, cfg))

    def decode(x0):
        img = m.rescaled_upsample(AG.NhwcToNchwFn.apply(x0, x0.shape[-1]))
        return AG.NchwToNhwcFn.apply(img.contiguous(), img.shape[1])
    xd = to_nhwc(x).to(DEV)
    op.to(DEV)
    with G.frozen(m):
        e, d, g = m._guided_step(xd, to_nhwc(y).to(DEV), op, torch.full((2,), use[k], device=DEV), torch.full((2,), k, device=DEV), tables,
                                 noise=to_nhwc(z).to(DEV), decode=decode)
    errs = (rel_err(to_nchw(e.cpu()), e_r), float(((d.cpu().double() - d_r).abs() / d_r).max()), _per_image_rel(to_nchw(g.cpu()), g_r),
            rel_err(to_nchw(xd.cpu()), x_r))
    print(f"\n{u_mode} {which}: eps_hat {errs[0]:.2e} dist {errs[1]:.2e} g {errs[2]:.2e} x_prev {errs[3]:.2e}; |zeta g| max {2.0 * float(g_r.abs().max()):.3g}")
    assert float(g_r.abs().max()) > 1e-4
    assert errs[0] < 5e-5 and errs[1] < 5e-5 and errs[2] < 2e-4 and errs[3] < 2e-4


@pytest.mark.parametrize("task,kw", [("sr", dict(scale=4, saturate=2.5, sigma_y=0.05)), ("inpaint", dict(mask="half")), ("deblur", dict(kernel="gauss")),
                                     ("deconv", dict(psf="disk", ddim=True, eta=0.5))])
def test_the_evaluator_scores_the_method_on_both_model_kinds(task, kw):
    """evaluate_restoration(method="dps") end to end on three steps: the measurement made on the device, the chain, the scores"""
    from utils import restoration_metrics as RMx
    images = (syn.synthetic_input((3, 16, 16, 3), f"g9.{task}") * 127.5 + 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
    for model in (_pixel_model(), _latent_model("convolutional_res")[0]):
        r = RMx.evaluate_restoration(model, images, task, method="dps", zeta=0.5, respacing="3", batch_size=2, seed=5, **kw)
        assert r["method"] == "dps" and r["unet_forwards"] == r["unet_backwards"] == 3 and r["zeta"] == 0.5 and r["n_images"] == 3
        assert set(r["methods"]) == {"restored", "measured"} and r["images"]["restored"].shape == (3, 16, 16, 3)
        assert r["consistency"].shape == (3,) and bool(np.isfinite(r["consistency"]).all()) and bool(np.isfinite(r["methods"]["restored"]["psnr"]).all())
        assert ("psnr_hidden" in r["methods"]["restored"]) == (task == "inpaint")


def test_guided_cli(tmp_path):
    """guided_model_samples.py on a dDDPM with synthetic weights: clean images measured here through a sensor that clips, with noise,
    restored in three steps; both files written"""
    cfg_path, images_path, _, env = CC.cli_files(tmp_path, CC.cli_cfg("dddpm"), 3, 32)
    CC.run_script("guided_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--task", "sr",
                  "--scale", "4", "--measure_input", "--saturate", "2.5", "--sigma_y", "0.05", "--zeta", "0.5", "--timestep_respacing", "3",
                  "--batch_size", "2", "--out_dir", tmp_path, env=env)
    name = "clitest_guided_sr_x4_sat2.5_z0.5_3_sy0.05"
    out, measured = np.load(tmp_path / f"{name}.npy"), np.load(tmp_path / f"{name}_measured.npy")
    assert out.shape == (3, 32, 32, 3) and out.dtype == np.float32 and out.min() >= 0 and out.max() <= 255 and np.isfinite(out).all()
    assert measured.shape == (3, 8, 8, 3) and measured.dtype == np.uint8
    assert measured.std() > 20                  # gain 2.5 spreads the block means of uniform noise (std 0.14 / 2 of the range) by as much


def test_restore_guided_in_the_latent_returns_image_and_latent():
    m, cfg = _latent_model("convolutional_res")
    state = ([p.requires_grad for p in m.parameters()], m.training)
    x_out, z = m.restore_guided(torch.zeros(2, 3, 16, 16), "disk", zeta=0.5, respacing="2", seed=3)
    assert x_out.shape == (2, 3, 16, 16) and z.shape == (2, 8, 8, 8) and bool(torch.isfinite(x_out).all())
    assert ([p.requires_grad for p in m.parameters()], m.training) == state
    with torch.no_grad():
        assert torch.equal(x_out, m.rescaled_upsample(z))
