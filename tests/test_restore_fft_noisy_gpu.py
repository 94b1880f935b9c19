"""DDNM+ deconvolution of a noisy blurred image on the GPU (DDPM.deconvolve_noisy, ddk_sampler_run_restore_fft_noisy,
ddk_p_sample_update_restore_fft_noisy, ddk_circular_spectrum; csrc/fft_conv.hip) against tests/fft_noisy_ref.py, the method restated in
float64 (numpy.fft) with float32 multipliers around oracle/unet_ref with oracle/philox_ref draws.

The bar of the lone step, per plane in the 2-norm, with u = 2^-24, N = H W and L = log2 N (DESIGN.md sections 3.18 and 3.19):

  ||got - ref|| <= |c1| (16 L u (||x0|| + ||Yp||) + 4 u ||x0'||) + 16 L u max(phi) ||z|| + 4 u (||c1 x0'|| + ||c2 x|| + ||n||)

      section 3.18's lone-step bar with each transformed signal entering on its own: x0 goes through two transforms (16 L u ||x0||,
      Higham Thm 24.2 with 8 u per bit); Yp = Re F2^-1(M Y^), an fp32 spectrum both sides read, through the inverse one and the
      blend (0 <= lam <= 1 enlarges no norm), counted as x0 is; the blend X^ + lam (Y^ - X^) rounds three times and the scaling by
      1 / N is exact: 4 u ||x0'||; the draw goes through two transforms and one multiply by phi <= max(phi): 16 L u max(phi) ||z||;
      the update's roundings are half an ulp of each of its terms, 4 u each as in section 3.18.  Derived, not fitted.

Shapes: the plane form with W != H both ways and an odd channel count, the largest plane it holds, and the multi-launch form.  Chains:
1e-4 abs against the restatement with the same argmax and 1e-5 between the Python loop and the native sampler, as for the other
restore kinds; graph replay equals eager launches bit for bit."""
import json
import math

import numpy as np
import pytest
import torch

import chain_cases as CC
import fft_conv_ref as FR
import fft_noisy_ref as FN
from helpers import ddpm_cfg, to_nchw as nchw, to_nhwc as nhwc
from oracle import diffusion_ref as D
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SEED = 1409
U24 = 2.0 ** -24
PRESETS = ("diag", "disk")
# (C, H, W, B): the plane form (W != H both ways, an odd channel count), the largest plane it holds, the multi-launch form
SHAPES = [(3, 16, 16, 3), (1, 32, 16, 3), (2, 16, 64, 2), (2, 128, 128, 1), (1, 128, 256, 1)]
PSF_TOL = 3e-2
KINDS = [dict(), dict(ddim=True, eta=0.5)]
IDS = ["ancestral", "ddim_eta0.5"]


def _norm(v):
    """2-norm per plane of a [B, C, H, W] tensor or array, as a float64 array [B, C]"""
    v = v.detach().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
    return np.sqrt((v ** 2).sum(axis=(-2, -1)))


def _draws(B, c, h, w, t, seed, stream):
    """chain_cases.philox_draws with zeros at row 0, which this op's restatement multiplies by its own factor"""
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    z[torch.as_tensor(t) == 0] = 0.0
    return z


def _tables(ddim=False, eta=0.0):
    from models.diffusion import respace
    return respace.spaced_tables(np.asarray(BETAS, dtype=np.float64), "8", ddim, eta)[0]


def _operands(name, h, w, sigma_y, c1, tol=PSF_TOL):
    """the library's operands of a preset as (mask, P, gain, nsc) numpy arrays"""
    from models.diffusion import psf
    _, Pf, Mf, _ = psf.psf_operands(name, h, w, tol)
    gain, nsc = psf.psf_noisy_operands(name, h, w, tol, sigma_y, c1)
    return Mf, Pf, gain, nsc


def _spectrum(y, Pf):
    """(the device's own spectrum of A+ y [B, C, H W, 2] on the device, the complex128 array [B, C, H, W] in natural order it holds)"""
    from ddk import ops
    B, c, h, w = y.shape
    Yd = ops.circular_spectrum(nhwc(y).to(DEV), torch.from_numpy(Pf).to(DEV))
    v = Yd.cpu().double().numpy()
    return Yd, FN.to_natural(v[..., 0] + 1j * v[..., 1], h, w)


def _step(x, e, Md, gd, nd, Yd, t, tab, seed, stream):
    from ddk import ops
    xs = nhwc(x).to(DEV)
    ops.p_sample_update_restore_fft_noisy_(xs, nhwc(e).to(DEV), Md, gd, nd, Yd, t.to(DEV), **{k: v.to(DEV) for k, v in tab.items()},
                                           seed=seed, stream_id=stream)
    return nchw(xs.cpu())


def _rows(B):
    """the rows of the "8" tables each lone-step case visits: all three in one call where the batch allows, else one call per row"""
    return [torch.tensor([0, 7, 3][:B])] if B == 3 else [torch.tensor([0, 7])] + [torch.tensor([3, 3])] if B == 2 else \
        [torch.tensor([r]) for r in (0, 3, 7)]


# ---------------------------------------------------------------- 1. the lone step against the restatement
@pytest.mark.parametrize("sigma_y", [0.05, 0.5])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
@pytest.mark.parametrize("name", PRESETS)
@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_lone_step_within_the_derived_bar(c, h, w, B, name, kw, sigma_y):
    """see the module's docstring for the bar"""
    N = h * w
    L = math.log2(N)
    g = torch.Generator().manual_seed(31 * c + h + 3 * w + len(kw))
    shape = (B, c, h, w)
    tab = _tables(**kw)
    Mf, Pf, gain, nsc = _operands(name, h, w, sigma_y, tab["c1"])
    M = Mf != 0
    assert np.array_equal(M, FR.kept(FR.preset(name), h, w, PSF_TOL))
    Md, gd, nd = (torch.from_numpy(v).to(DEV) for v in (Mf, gain, nsc))
    clean = (0.5 * torch.randn(shape, generator=g)).clamp(-1, 1)
    y = torch.from_numpy(FR.apply(clean, FR.spectrum(FR.preset(name), h, w))).float() + sigma_y * torch.randn(shape, generator=g)
    Yd, Yhat = _spectrum(y, Pf)
    Yp = np.fft.ifft2(np.where(M, Yhat, 0.0), axes=(-2, -1)).real
    seed, stream = 97531, 4
    worst, damped, full = 0.0, 0, 0
    for t in _rows(B):
        x = torch.randn(shape, generator=g)
        e = torch.randn(shape, generator=g)
        z = _draws(B, c, h, w, t, seed, stream)
        s = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
        want, x0, x0p, n, lam, phi = FN.step(x, e, M, gain, Yhat, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], s,
                                             torch.from_numpy(nsc)[t], z)
        damped += int(((lam[:, M] > 0) & (lam[:, M] < 1)).sum())
        full += int((lam[:, M] == 1).sum())
        col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
        c1, c2 = col(tab["c1"][t]), col(tab["c2"][t])
        bar = np.abs(c1) * (16 * L * U24 * (_norm(x0) + _norm(Yp)) + 4 * U24 * _norm(x0p)) + 16 * L * U24 * col(phi.max(axis=(1, 2))) * _norm(z) + \
            4 * U24 * (np.abs(c1) * _norm(x0p) + np.abs(c2) * _norm(x) + _norm(n))
        got = _step(x, e, Md, gd, nd, Yd, t, tab, seed, stream)
        assert got.shape == want.shape and torch.isfinite(got).all()
        err = _norm(got.double() - want)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (t.tolist(), float((err / bar).max()))
    form = "plane form" if N <= 16384 else "multi-launch form"
    print(f"lone DDNM+ deconvolution step c={c} {h}x{w} B={B} psf {name} {IDS[KINDS.index(kw)]} sigma_y {sigma_y} ({form}): worst ratio to the "
          f"bar {worst:.3g}; kept frequencies with 0 < lam < 1: {damped}, with lam = 1: {full}")
    assert damped > 0 if sigma_y == 0.5 else full > 0       # both branches of the multiplier are visited over the two sigma_y


# ---------------------------------------------------------------- 2. the covariance of the draw
@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_the_shaped_draw_alone(c, h, w, B):
    """the x0 side zeroed (x, eps_hat and y zero, c1 = c2 = 0 tables): the output is n = Re F2^-1(phi F2(z)) / N, held to
    16 L u max(phi) ||z|| against the float64 shaping of the device's own draw (by Parseval the same statement as F2(n) = phi F2(z)
    within that bar times sqrt N).  x0 has to be zero itself, not only its coefficients: in the plane form it shares the complex
    transform with the draw, and the inverse transform's rounding, relative to the whole packed spectrum, lands in both parts
    (DESIGN.md section 3.19)."""
    L = math.log2(h * w)
    tab = _tables()
    tab = dict(tab, c1=torch.zeros_like(tab["c1"]), c2=torch.zeros_like(tab["c2"]))
    Mf, Pf, gain, _ = _operands("disk", h, w, 0.1, tab["c1"])
    nsc = (0.3 * tab["sigma"].numpy()).astype(np.float32)      # hand-made: g = 0.3 s gain, so kept frequencies with a gain above 3.3 are damped (phi = 0), the others shaped, the dropped ones at s
    M = Mf != 0
    shape = (B, c, h, w)
    x = e = y = torch.zeros(shape)
    Yd, _ = _spectrum(y, Pf)
    seed, stream = 24680, 2
    for t in _rows(B)[:2]:
        t = torch.clamp(t, min=1)                           # rows that draw
        z = _draws(B, c, h, w, t, seed, stream)
        s = tab["sigma"][t].numpy()
        lam, phi = FN.multipliers(M, gain, s, nsc[t.numpy()])
        assert (phi[:, M] == 0).any() and ((phi[:, M] > 0) & (phi[:, M] < s[:, None])).any()
        got = _step(x, e, *(torch.from_numpy(v).to(DEV) for v in (Mf, gain, nsc)), Yd, t, tab, seed, stream)
        want = FN.shaped(z, phi)
        err = _norm(got.double().numpy() - want)
        bar = 16 * L * U24 * phi.max(axis=(1, 2)).astype(np.float64).reshape(-1, 1) * _norm(z)
        print(f"shaped draw c={c} {h}x{w} rows {t.tolist()}: worst ratio to the bar {float((err / bar).max()):.3g}")
        assert (err <= bar).all(), float((err / bar).max())


# ---------------------------------------------------------------- 3. the tie to the deconvolution kernel
@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_zero_gain_is_the_deconvolution_step(c, h, w, B):
    """gain = 0 on the kept frequencies: g = 0, lam = 1, phi = s, the step of p_sample_update_restore_fft_ on the same inputs and seed,
    within the sum of the two bars"""
    from ddk import ops
    L = math.log2(h * w)
    tab = _tables()
    Mf, Pf, _, nsc = _operands("disk", h, w, 0.1, tab["c1"])
    M = Mf != 0
    g = torch.Generator().manual_seed(7 * h + w)
    shape = (B, c, h, w)
    x, e, y = (torch.randn(shape, generator=g) for _ in range(3))
    Yd, _ = _spectrum(y, Pf)
    Ypd = ops.circular_conv(nhwc(y).to(DEV), torch.from_numpy(Pf).to(DEV))
    Yp = nchw(Ypd.cpu())
    t = _rows(B)[-1] if B < 3 else _rows(B)[0]
    seed, stream = 1357, 3
    z = _draws(B, c, h, w, t, seed, stream)
    s = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    _, x0, x0p = FR.step(x, e, M, Yp, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], s, z)
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
    c1, c2 = np.abs(col(tab["c1"][t])), np.abs(col(tab["c2"][t]))
    upd = 4 * U24 * (c1 * _norm(x0p) + c2 * _norm(x) + col(s) * _norm(z))
    bar_fft = c1 * (16 * L * U24 * _norm(x0) + U24 * _norm(x0p)) + upd
    bar_noisy = c1 * (16 * L * U24 * (_norm(x0) + _norm(Yp)) + 4 * U24 * _norm(x0p)) + 16 * L * U24 * col(s) * _norm(z) + upd
    xs = nhwc(x).to(DEV)
    ops.p_sample_update_restore_fft_(xs, nhwc(e).to(DEV), torch.from_numpy(Mf).to(DEV), Ypd, t.to(DEV), **{k: v.to(DEV) for k, v in tab.items()},
                                     seed=seed, stream_id=stream)
    merged = nchw(xs.cpu())
    got = _step(x, e, torch.from_numpy(Mf).to(DEV), torch.zeros(h, w, device=DEV), torch.from_numpy(nsc).to(DEV), Yd, t, tab, seed, stream)
    err = _norm(got.double() - merged.double())
    print(f"zero gain against the deconvolution step c={c} {h}x{w} rows {t.tolist()}: worst ratio to the two bars' sum "
          f"{float((err / (bar_fft + bar_noisy)).max()):.3g}")
    assert (err <= bar_fft + bar_noisy).all()


# ---------------------------------------------------------------- 4. row 0
@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_row_0_returns_the_models_x0_and_nothing_of_y(c, h, w, B):
    """s_0 = 0: lam = 0 and phi = 0 everywhere, so the result is the clipped x0 up to the transform round trip, 16 L u ||x0||, whatever
    the measurement holds; NaN at the dropped frequencies of the spectrum of A+ y, which no step reads, reaches nothing"""
    L = math.log2(h * w)
    tab = _tables()
    Mf, Pf, gain, nsc = _operands("diag", h, w, 0.1, tab["c1"])
    assert float(tab["c1"][0]) == 1.0 and float(tab["c2"][0]) == 0.0 and nsc[0] > 0
    M = Mf != 0
    g = torch.Generator().manual_seed(h * 3 + w)
    shape = (B, c, h, w)
    x, e = (torch.randn(shape, generator=g) for _ in range(2))
    t = torch.zeros(B, dtype=torch.long)
    x0 = (tab["c_recip"][t].reshape(-1, 1, 1, 1) * x - tab["c_recipm1"][t].reshape(-1, 1, 1, 1) * e).clamp(-1, 1)
    dropped = torch.from_numpy(FN.to_device(np.broadcast_to(~M, (B, c, h, w)), h, w))
    outs = []
    for scale in (1.0, -3.0):
        Yd, _ = _spectrum(scale * torch.randn(shape, generator=g), Pf)
        Yd = Yd.clone()
        Yd[dropped.to(DEV)] = float("nan")
        outs.append(_step(x, e, *(torch.from_numpy(v).to(DEV) for v in (Mf, gain, nsc)), Yd, t, tab, 5, 1))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    err = _norm(outs[0].double() - x0.double())
    bar = 16 * L * U24 * _norm(x0)
    print(f"row 0 c={c} {h}x{w}: worst ratio to the bar {float((err / bar).max()):.3g}")
    assert (err <= bar).all()


def test_argument_faults_run_no_kernel():
    from ddk import lib as L
    from ddk import ops
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    nsc = torch.ones(4, device=DEV)
    for h, w, c in ((24, 16, 3), (16, 48, 3), (512, 16, 3), (8, 16, 3), (16, 16, 9)):
        x = torch.full((1, h, w, c), 0.25, device=DEV)
        before = x.clone()
        with pytest.raises(L.DDKError):
            ops.p_sample_update_restore_fft_noisy_(x, torch.ones_like(x), torch.ones(h, w, device=DEV), torch.ones(h, w, device=DEV), nsc,
                                                   torch.zeros(1, c, h * w, 2, device=DEV), t, **tab)
        torch.cuda.synchronize()
        assert torch.equal(x, before)
    x = torch.zeros(1, 16, 16, 3, device=DEV)
    one, Yh = torch.ones(16, 16, device=DEV), torch.zeros(1, 3, 256, 2, device=DEV)
    for bad in (dict(gain=torch.ones(16, 8, device=DEV)), dict(nsc=torch.ones(3, device=DEV)), dict(Yhat=torch.zeros(1, 3, 16, 16, device=DEV)),
                dict(mask=one.double())):
        a = dict(mask=one, gain=one, nsc=nsc, Yhat=Yh)
        a.update(bad)
        with pytest.raises(L.DDKError):
            ops.p_sample_update_restore_fft_noisy_(x, torch.zeros_like(x), a["mask"], a["gain"], a["nsc"], a["Yhat"], t, **tab)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# ---------------------------------------------------------------- 5. the tiny DDPM, "8" steps
@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


PSF_TINY = "disk"
K_TINY = FR.preset(PSF_TINY)
SY = 0.1


@pytest.fixture(scope="module")
def data():
    clean = 0.25 * syn.synthetic_normal(SHAPE, "deconv_noisy.x")
    y = torch.from_numpy(FR.apply(clean, FR.spectrum(K_TINY, 16, 16))).float() + SY * syn.synthetic_normal(SHAPE, "deconv_noisy.noise")
    return y.contiguous(), syn.synthetic_normal(SHAPE, "deconv_noisy.xT")


@pytest.fixture(scope="module")
def reference(tiny, data):
    """the restatement's chains, computed once and shared"""
    _, eps = tiny
    y, x_T = data
    return {i: FN.DeconvNoisy(BETAS, "8").run(eps, x_T, y, K_TINY, PSF_TOL, SY, SEED, **kw) for i, kw in zip(IDS, KINDS)}


def _same_argmax(got, want, tol):
    """the same argmax per image, ties counted: row 0 returns the clipped x0 behind a transform round trip, so the synthetic model's
    many pixels at exactly +1 come back as 1 +- a few 1e-7 on either side and the FIRST largest is decided by rounding.  Each side's
    argmax must be a largest pixel of the other side within tol."""
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    ig, iw = g.argmax(dim=1, keepdim=True), w.argmax(dim=1, keepdim=True)
    return bool((w.gather(1, ig) >= w.max(dim=1, keepdim=True).values - tol).all() and (g.gather(1, iw) >= g.max(dim=1, keepdim=True).values - tol).all())


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, reference, kw):
    m, _ = tiny
    y, x_T = data
    got = m.deconvolve_noisy(y.to(DEV), PSF_TINY, sigma_y=SY, respacing="8", x_T=x_T, seed=SEED, **kw).cpu()
    want = reference[IDS[KINDS.index(kw)]]
    err = float((got - want).abs().max())
    print(f"DDNM+ deconvolution tiny DDPM, 8 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    assert _same_argmax(got, want, TOL)
    plain = m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED, **kw).cpu()
    assert float((got - plain).abs().max()) > 1e-2          # not the deconvolution chain


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_and_python_loop_equals_native(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    native = m.deconvolve_noisy(y.to(DEV), PSF_TINY, sigma_y=SY, respacing="8", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "use_graph", False):
        eager = m.deconvolve_noisy(y.to(DEV), PSF_TINY, sigma_y=SY, respacing="8", x_T=x_T, seed=SEED, **kw)
    assert torch.equal(native, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = m.deconvolve_noisy(y.to(DEV), K_TINY, sigma_y=SY, respacing="8", x_T=x_T, seed=SEED, **kw)      # the preset as an array: the same chain
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, DDNM+ deconvolution 8 steps {kw}: {err:.3g}")
    assert err < 1e-5


def test_sigma_y_zero_is_deconvolve_and_two_sigma_y_keep_apart(tiny, data):
    m, _ = tiny
    y, x_T = data
    run = lambda sy: m.deconvolve_noisy(y.to(DEV), PSF_TINY, sigma_y=sy, respacing="8", x_T=x_T, seed=SEED)
    assert torch.equal(run(0.0), m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED))
    first = {}
    for sy in (0.05, 0.5, 0.05, 0.5, 0.5, 0.05):
        got = run(sy)
        assert torch.equal(got, first.setdefault(sy, got)), sy
    assert float((first[0.05] - first[0.5]).abs().max()) > 1e-2


def test_tail_parts_is_zero_for_every_shape(tiny):
    from models import Unet
    m, _ = tiny
    plan = m._eps_model_nhwc().plan()
    assert plan.restore_fft_noisy_tail_parts(2, 16, 16) == 0
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    for b, h, w in ((32, 32, 32), (8, 64, 64), (4, 128, 128), (1, 256, 256)):
        assert u._plan.restore_fft_noisy_tail_parts(b, h, w) == 0
    assert u._plan.restore_tail_parts(32, 32, 32, 2) == 8       # the shape has a fused tail; the plane-wide kind declines it


def test_noisy_deconvolution_and_ancestral_chains_share_a_workspace(tiny, data, reference):
    """noisy, deconvolution and ancestral chains on the same plan, workspace, state buffer, tables and t_start, alternating in two
    orders: each reproduces its own first result bit for bit (the kind and the caller's gain and nsc are in the graph key; every
    operand is staged by every call), and the noisy one is the model's own method"""
    from ddk import lib as L
    from ddk import ops
    from models.diffusion import psf
    m, _ = tiny
    y, x_T = data
    tables, use = m._spaced_tables("8", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    nbytes = lib.ddk_sampler_restore_fft_noisy_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    n = 2 * 16 * 16 * 3
    assert nbytes == lib.ddk_sampler_restore_fft_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + 4 * (256 + 8 + 2 * n)
    _, Pf, Mf, _ = psf.psf_operands(K_TINY, 16, 16, PSF_TOL)
    Md, Pd = torch.from_numpy(Mf).to(DEV), torch.from_numpy(Pf).to(DEV)
    tw = ops.fft_twiddles(16, Md.device)
    gn = {sy: tuple(torch.from_numpy(v).to(DEV) for v in psf.psf_noisy_operands(K_TINY, 16, 16, PSF_TOL, sy, tables["c1"])) for sy in (SY, 0.5)}
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    yd = ops.nchw_to_nhwc(y.to(DEV).contiguous())

    def launch(what, a, tmap, stream):
        if what is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        if what == "deconv":
            return lib.ddk_sampler_run_restore_fft(a, tmap, L.ptr(Md), L.ptr(Pd), L.ptr(tw), L.ptr(yd), stream)
        return lib.ddk_sampler_run_restore_fft_noisy(a, tmap, L.ptr(Md), L.ptr(Pd), L.ptr(gn[what][0]), L.ptr(gn[what][1]), L.ptr(tw), L.ptr(yd),
                                                     stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    with CC.workspace(plan, nbytes) as ws:
        first = {}
        for what in (SY, "deconv", None, SY, 0.5, None, "deconv", 0.5, SY, None, 0.5, "deconv", SY):
            got = sh.run(ws, what)
            assert torch.equal(got, first.setdefault(what, got)), (what, float((got - first[what]).abs().max()))
        outs = list(first.values())
        assert all(not torch.equal(a, b) for i, a in enumerate(outs) for b in outs[i + 1:])
        via_model = m.deconvolve_noisy(y.to(DEV), PSF_TINY, sigma_y=SY, respacing="8", x_T=x_T, seed=SEED)
        assert torch.equal(ops.nhwc_to_nchw(first[SY]), via_model)
        assert float((ops.nhwc_to_nchw(first[SY]).cpu() - reference["ancestral"]).abs().max()) < TOL
        assert torch.equal(ops.nhwc_to_nchw(first["deconv"]), m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED))


def test_the_five_plane_wide_kinds_in_rotation_equal_each_alone(data):
    """deblur, restore_separable, restore_cs, deconvolve and deconvolve_noisy in rotation on one model and plan, in two orders: each
    result equals, bit for bit, that of the same call made alone on a freshly built model (every call stages its own operands and
    the graph key tells the kinds apart, whichever kind used the workspace before)"""
    from models.diffusion import blur
    y, x_T = data
    yd = y.to(DEV)
    A = blur.resize_matrix(16, 2)
    y_sep = (0.25 * syn.synthetic_normal((2, 3, 8, 8), "rotation.sep")).to(DEV)
    y_cs = (0.25 * syn.synthetic_normal((2, 3, 100), "rotation.cs")).to(DEV)
    kw = dict(respacing="8", x_T=x_T, seed=SEED)
    calls = {"deblur": lambda m: m.deblur(yd, "gauss", **kw),
             "separable": lambda m: m.restore_separable(y_sep, A, A, **kw),
             "cs": lambda m: m.restore_cs(y_cs, perm_seed=3, **kw),
             "deconvolve": lambda m: m.deconvolve(yd, PSF_TINY, **kw),
             "deconvolve_noisy": lambda m: m.deconvolve_noisy(yd, PSF_TINY, sigma_y=SY, **kw)}
    fresh = lambda: CC.tiny_ddpm(CFG)[0]
    alone = {name: call(fresh()) for name, call in calls.items()}
    outs = list(alone.values())
    assert all(torch.isfinite(v).all() for v in outs) and all(not torch.equal(a, b) for i, a in enumerate(outs) for b in outs[i + 1:])
    m = fresh()
    names = list(calls)
    for name in 2 * names + 2 * [names[i] for i in (4, 2, 0, 3, 1)]:
        got = calls[name](m)
        assert torch.equal(got, alone[name]), (name, float((got - alone[name]).abs().max()))


def test_chain_faults(tiny):
    """the chain entry: injected noise, a null operand, misalignment, a shape the kind does not take and a short workspace"""
    from ddk import lib as L
    from ddk import ops
    from models.diffusion import psf
    m, _ = tiny
    tables, use = m._spaced_tables("8", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    tmap = CC.timestep_map(use)
    nbytes = lib.ddk_sampler_restore_fft_noisy_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes > 0 and lib.ddk_sampler_restore_fft_noisy_workspace_bytes(plan.handle, 2, 16, 48, K - 1) == 0
    x = torch.zeros(2, 16, 16, 3, device=DEV)
    y = torch.zeros(2, 16, 16, 3, device=DEV)
    _, Pf, Mf, _ = psf.psf_operands(K_TINY, 16, 16, PSF_TOL)
    gd, nd = (torch.from_numpy(v).to(DEV) for v in psf.psf_noisy_operands(K_TINY, 16, 16, PSF_TOL, SY, tables["c1"]))
    Md, Pd = torch.from_numpy(Mf).to(DEV), torch.from_numpy(Pf).to(DEV)
    tw = ops.fft_twiddles(16, Md.device)
    ws = CC.fresh_workspace(nbytes)
    noise = torch.zeros((K, *x.shape), device=DEV)
    args = lambda noise=None, H=16, nbytes=nbytes: CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED, noise=noise, shape=(2, H, 16))
    run = lib.ddk_sampler_run_restore_fft_noisy
    ops6 = (L.ptr(Md), L.ptr(Pd), L.ptr(gd), L.ptr(nd), L.ptr(tw), L.ptr(y))
    assert run(args(noise), tmap, *ops6, L.stream()) == -1 and "noise" in L.last_error()
    for i in range(6):
        assert run(args(), tmap, *(None if j == i else p for j, p in enumerate(ops6)), L.stream()) == -1 and "null" in L.last_error()
        assert run(args(), tmap, *(p + 4 if j == i else p for j, p in enumerate(ops6)), L.stream()) == -1 and "alignment" in L.last_error()
    assert run(args(H=48), tmap, *ops6, L.stream()) == -1 and "powers of two" in L.last_error()
    assert run(args(nbytes=nbytes - 4), tmap, *ops6, L.stream()) != 0      # a short workspace
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    with pytest.raises(L.DDKError):
        plan.sample_restore_fft_noisy_nhwc(x, y, Md, Pd, gd[:8].contiguous(), nd, tables, K - 1, timesteps=use)
    with pytest.raises(L.DDKError):
        plan.sample_restore_fft_noisy_nhwc(x, y, Md, Pd, gd, nd[:4].contiguous(), tables, K - 1, timesteps=use)


def test_multi_launch_chain_256():
    """three steps at 3 x 256 x 256, B = 1, on a 32-wide model: the three-launch form with T2 inside a chain.  Graph replay against eager
    launches, and the native chain against the Python loop over the lone op"""
    m, _ = CC.tiny_ddpm(ddpm_cfg(32, 3, 256))
    shape = (1, 3, 256, 256)
    k = FR.preset("diag")
    clean = 0.25 * syn.synthetic_normal(shape, "deconv_noisy256.x")
    y = (torch.from_numpy(FR.apply(clean, FR.spectrum(k, 256, 256))).float() + SY * syn.synthetic_normal(shape, "deconv_noisy256.n")).contiguous()
    x_T = syn.synthetic_normal(shape, "deconv_noisy256.xT")
    native = m.deconvolve_noisy(y.to(DEV), "diag", sigma_y=SY, respacing="3", x_T=x_T, seed=SEED)
    with CC.toggled(m, "use_graph", False):
        eager = m.deconvolve_noisy(y.to(DEV), "diag", sigma_y=SY, respacing="3", x_T=x_T, seed=SEED)
    assert torch.equal(native, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = m.deconvolve_noisy(y.to(DEV), "diag", sigma_y=SY, respacing="3", x_T=x_T, seed=SEED)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, DDNM+ deconvolution 256 x 256, 3 steps: {err:.3g}")
    assert torch.isfinite(native).all() and err < 1e-5


# ---------------------------------------------------------------- the command lines
def test_deconv_noisy_cli_and_evaluator(tmp_path):
    """deconv_model_samples.py --blur_input --sigma_y and evaluate_restoration.py --task deconv_noisy with synthetic weights on four
    16 x 16 images, each in a fresh process: the files, their names and shapes, and the JSON keys"""
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 4, 16)
    CC.run_script("deconv_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--blur_input",
                  "--psf", "disk", "--tol", "0.1", "--sigma_y", "0.05", "--timestep_respacing", "10", "--batch_size", "3", "--seed", "3",
                  "--out_dir", tmp_path, env=env)
    out = np.load(tmp_path / "clitest_deconv_disk_10_sy0.05.npy")
    blurred = np.load(tmp_path / "clitest_deconv_disk_10_sy0.05_blurred.npy")
    assert out.shape == (4, 16, 16, 3) and out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert blurred.shape == (4, 16, 16, 3) and blurred.dtype == np.uint8
    clean = FR.apply(torch.from_numpy(imgs.astype(np.float64)).permute(0, 3, 1, 2) / 255 * 2 - 1, FR.spectrum(FR.preset("disk"), 16, 16))
    dev = blurred.astype(np.float64) - (np.transpose(clean, (0, 2, 3, 1)) + 1) * 127.5
    assert 0.5 * 0.05 * 127.5 < dev.std() < 1.5 * 0.05 * 127.5      # the noise that was asked for is in the saved measurement
    CC.run_script("evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "deconv_noisy", "--psf", "disk",
                  "--sigma_y", "0.05", "--timestep_respacing", "10", "--batch_size", "3", "--json", tmp_path / "score.json", env=env)
    res = json.loads((tmp_path / "score.json").read_text())
    s, mt = res["settings"], res["metrics"]
    assert (s["task"], s["method"], s["psf"], s["tol"], s["sigma_y"], s["unet_forwards"], s["n_images"]) == ("deconv_noisy", "ddnm_plus", "disk", 0.03, 0.05, 10, 4)
    assert {"restored", "blurred", "pinv", "tikhonov", "consistency", "consistency_u8"} <= set(mt)
    for name in ("restored", "blurred", "pinv", "tikhonov"):
        assert set(mt[name]) == {"psnr", "ssim"} and mt[name]["psnr"]["n"] == 4 and np.isfinite(mt[name]["psnr"]["mean"])
    assert {"mean", "stderr", "n", "max"} <= set(mt["consistency"]) and np.isfinite(mt["consistency"]["mean"])
    print(f"noisy deconvolution evaluator (synthetic weights): {json.dumps(mt)}")
