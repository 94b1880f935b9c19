"""DDNM deconvolution of a 2-D point-spread function on the GPU (DDPM.deconvolve, ddk_sampler_run_restore_fft,
ddk_p_sample_update_restore_fft, ddk_circular_conv; csrc/fft_conv.hip) against tests/fft_conv_ref.py, the method restated in float64
(numpy.fft) around oracle/unet_ref with oracle/philox_ref draws.

The bars, per plane in the 2-norm, with u = 2^-24, N = H W and L = log2 N:

  circular_conv   ||got - ref|| <= (16 L + 4) u max|S| ||x||
      Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: a radix-2 transform of length n computed with twiddles of
      relative error mu has relative 2-norm error log2 n eta, eta = mu + gamma_4 (sqrt 2 + mu), about 6.7 u for correctly rounded
      twiddles; 8 u absorbs the higher-order terms.  Rows and columns add to L; two transforms give 16 L u, the complex multiply 4 u.
      The kernel's radix-4 passes are two radix-2 stages held in registers: every value is rounded as often as in radix 2.
  the lone step   ||got - ref|| <= |c1| (16 L u ||x0|| + u ||x0'||) + 4 u (||c1 x0'|| + ||c2 x|| + ||sigma z||)
      two transforms of x0 (the select between them is exact, and a projection does not enlarge a norm), the rounding of r + Yp, and
      the update's five roundings, each half an ulp of one of its terms.  Yp is an fp32 operand of both sides.
  the invariant   ||A+ A x_out - Yp|| <= 16 L u ||x0|| + u ||x0'||  at row 0 (c1 = 1, c2 = 0), the projection taken in float64.
      In a chain Yp is the library's own A+ y, one circular_conv with S = P^: its bar (16 L + 4) u max|P^| ||y|| is added, since the
      part of that error outside the kept frequencies stays in the result.

Shapes: both kernel forms (a plane of at most 16384 pixels takes one launch, a larger one three), one to three channels, W != H both
ways.  Chains: 1e-4 abs against the restatement with the same argmax and 1e-5 between the Python loop and the native sampler, as for
the other restore kinds; graph replay equals eager launches bit for bit."""
import json
import math

import numpy as np
import pytest
import torch

import chain_cases as CC
import fft_conv_ref as FR
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
KINDS = [dict(), dict(ddim=True, eta=0.0)]
IDS = ["ancestral", "ddim"]
U24 = 2.0 ** -24
PRESETS = ("diag", "disk")
# (C, H, W, B): the plane form up to N = 16384, the multi-launch form above
SHAPES = [(3, 16, 16, 3), (1, 32, 16, 3), (2, 16, 64, 2), (3, 64, 64, 2), (2, 128, 128, 2), (1, 128, 256, 2), (2, 256, 256, 1)]
PSF_TOL = 3e-2


def _c2f(S):
    """complex [H, W] -> fp32 tensor [H, W, 2] (re, im), and the complex128 array the device then reads"""
    f = np.ascontiguousarray(np.stack([S.real, S.imag], axis=-1).astype(np.float32))
    return torch.from_numpy(f), f[..., 0].astype(np.float64) + 1j * f[..., 1].astype(np.float64)


def _norm(v):
    """2-norm per plane of a [B, C, H, W] tensor or array, as a float64 array [B, C]"""
    v = v.detach().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
    return np.sqrt((v ** 2).sum(axis=(-2, -1)))


def _tables(ddim):
    from models.diffusion import respace
    return respace.spaced_tables(np.asarray(BETAS, dtype=np.float64), "8", ddim, 0.0)[0]


# ---------------------------------------------------------------- 1. circular_conv against float64
@pytest.mark.parametrize("name", PRESETS)
@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_circular_conv_within_the_derived_bar(c, h, w, B, name):
    from ddk import ops
    L = math.log2(h * w)
    g = torch.Generator().manual_seed(h * w + c)
    x = torch.randn(B, c, h, w, generator=g)
    xd = nhwc(x).to(DEV)
    worst = {}
    K = FR.spectrum(FR.preset(name), h, w)
    for what, S in (("A", K), ("A+", FR.pinv_spectrum(FR.preset(name), h, w, PSF_TOL)), ("identity", np.ones((h, w), dtype=np.complex128))):
        Sf, S32 = _c2f(S)
        got = nchw(ops.circular_conv(xd, Sf.to(DEV)).cpu())
        want = FR.apply(x, S32)
        err = _norm(got.double().numpy() - (x.double().numpy() if what == "identity" else want))
        bar = (16 * L + 4) * U24 * np.abs(S32).max() * _norm(x)
        worst[what] = float((err / bar).max())
        assert got.shape == x.shape and bool(torch.isfinite(got).all())
        assert (err <= bar).all(), (what, worst[what])
    form = "plane form" if h * w <= 16384 else "multi-launch form"
    print(f"circular_conv c={c} {h}x{w} B={B} psf {name} ({form}): worst ratios to the bar {worst}")


# ---------------------------------------------------------------- 2. the lone step
@pytest.mark.parametrize("ddim", [False, True], ids=["plain", "ddim"])
@pytest.mark.parametrize("name", PRESETS)
@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_lone_step_within_the_derived_bar(c, h, w, B, name, ddim):
    from ddk import ops
    N = h * w
    L = math.log2(N)
    g = torch.Generator().manual_seed(31 * c + h + 3 * w + ddim)
    shape = (B, c, h, w)
    x = torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    t = torch.tensor([0, 7, 3][:B]) if B > 1 else torch.tensor([3 if ddim else 0])
    tab = _tables(ddim)
    assert float(tab["c1"][0]) == 1.0 and float(tab["c2"][0]) == 0.0
    k = FR.preset(name)
    M = FR.kept(k, h, w, PSF_TOL)
    clean = (0.5 * torch.randn(shape, generator=g)).clamp(-1, 1)
    Yp = torch.from_numpy(FR.apply(FR.apply(clean, FR.spectrum(k, h, w)), FR.pinv_spectrum(k, h, w, PSF_TOL))).float()
    seed, stream = 97531, 4
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    want, x0, x0p = FR.step(x, e, M, Yp, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], sg, z)
    col = lambda v: v.reshape(-1, 1).double().numpy()
    c1, c2 = col(tab["c1"][t]), col(tab["c2"][t])
    first = np.abs(c1) * (16 * L * U24 * _norm(x0) + U24 * _norm(x0p))
    bar = first + 4 * U24 * (np.abs(c1) * _norm(x0p) + np.abs(c2) * _norm(x) + np.abs(col(sg)) * _norm(z))
    xs = nhwc(x).to(DEV)
    ops.p_sample_update_restore_fft_(xs, nhwc(e).to(DEV), torch.from_numpy(M.astype(np.float32)).to(DEV), nhwc(Yp).to(DEV), t.to(DEV),
                                     **{kk: v.to(DEV) for kk, v in tab.items()}, seed=seed, stream_id=stream)
    got = nchw(xs.cpu())
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = _norm(got.double() - want)
    ratio = float((err / bar).max())
    form = "plane form" if N <= 16384 else "multi-launch form"
    print(f"lone deconvolution step c={c} {h}x{w} B={B} psf {name} {'ddim' if ddim else 'plain'} rows {t.tolist()} ({form}): "
          f"worst ratio to the bar {ratio:.3g}")
    assert (err <= bar).all(), ratio
    if int(t[0]) == 0:
        # the invariant at row 0, which returns x0' itself: A+ A x_out = Yp, the projection applied in float64
        inv = _norm(FR.apply(got[0:1], M.astype(np.float64)) - Yp[0:1].double().numpy())
        print(f"  row 0: ||A+A x_out - Yp|| worst ratio to the first term {float((inv / first[0:1]).max()):.3g}")
        assert (inv <= first[0:1]).all()


# ---------------------------------------------------------------- 3. a one-tap PSF keeps every frequency
@pytest.mark.parametrize("c,h,w,B", [(3, 16, 16, 3), (2, 128, 128, 2), (1, 128, 256, 2), (2, 256, 256, 1)])
def test_one_tap_psf_returns_yp_bit_for_bit(c, h, w, B):
    from ddk import ops
    g = torch.Generator().manual_seed(h + w)
    shape = (B, c, h, w)
    x, e, Yp = (torch.randn(shape, generator=g) for _ in range(3))
    M = FR.kept(np.ones((1, 1)), h, w, PSF_TOL)
    assert M.all()
    tab = {kk: v.to(DEV) for kk, v in _tables(False).items()}
    xs = nhwc(x).to(DEV)
    ops.p_sample_update_restore_fft_(xs, nhwc(e).to(DEV), torch.ones(h, w, device=DEV), nhwc(Yp).to(DEV), torch.zeros(B, dtype=torch.long, device=DEV),
                                     **tab, seed=5, stream_id=1)
    assert torch.equal(nchw(xs.cpu()), Yp)


# ---------------------------------------------------------------- 4. bit identity, argument faults
@pytest.mark.parametrize("c,h,w,B", [(3, 16, 16, 3), (2, 128, 128, 2), (2, 256, 256, 1)])
def test_two_calls_of_every_op_agree_bit_for_bit(c, h, w, B):
    from ddk import ops
    g = torch.Generator().manual_seed(77 + h)
    shape = (B, c, h, w)
    x, e, Yp = (nhwc(torch.randn(shape, generator=g)).to(DEV) for _ in range(3))
    t = torch.tensor([0, 7, 3][:B]).to(DEV)
    tab = {kk: v.to(DEV) for kk, v in _tables(False).items()}
    Md = torch.from_numpy(FR.kept(FR.preset("disk"), h, w, PSF_TOL).astype(np.float32)).to(DEV)
    Kd = _c2f(FR.spectrum(FR.preset("disk"), h, w))[0].to(DEV)
    for op in (lambda: ops.p_sample_update_restore_fft_(x.clone(), e, Md, Yp, t, **tab, seed=3, stream_id=1), lambda: ops.circular_conv(x, Kd)):
        a, b = op(), op()
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_argument_faults_run_no_kernel():
    from ddk import lib as L
    from ddk import ops
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)

    def call(h, w, c):
        x = torch.full((1, h, w, c), 0.25, device=DEV)
        before = x.clone()
        with pytest.raises(L.DDKError):
            ops.p_sample_update_restore_fft_(x, torch.ones_like(x), torch.ones(h, w, device=DEV), torch.zeros_like(x), t, **tab)
        torch.cuda.synchronize()
        assert torch.equal(x, before)
        with pytest.raises(L.DDKError):
            ops.circular_conv(x, torch.ones(h, w, 2, device=DEV))

    call(24, 16, 3)
    call(16, 48, 3)
    call(512, 16, 3)
    call(8, 16, 3)
    call(16, 16, 9)
    x = torch.zeros(1, 16, 16, 3, device=DEV)
    with pytest.raises(L.DDKError):      # a multiplier or a mask of the wrong shape or type never reaches the library
        ops.circular_conv(x, torch.ones(16, 16, device=DEV))
    with pytest.raises(L.DDKError):
        ops.circular_conv(x, torch.ones(16, 16, 2, device=DEV, dtype=torch.float64))
    with pytest.raises(L.DDKError):
        ops.p_sample_update_restore_fft_(x, torch.zeros_like(x), torch.ones(16, 8, device=DEV), torch.zeros_like(x), t, **tab)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# ---------------------------------------------------------------- 5. the tiny DDPM, "8" steps
@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


PSF_TINY = "disk"
K_TINY = FR.preset(PSF_TINY)


@pytest.fixture(scope="module")
def data():
    clean = 0.25 * syn.synthetic_normal(SHAPE, "deconv.x")
    assert float(clean.abs().max()) < 1
    y = torch.from_numpy(FR.apply(clean, FR.spectrum(K_TINY, 16, 16))).float().contiguous()
    return y, syn.synthetic_normal(SHAPE, "deconv.xT")


@pytest.fixture(scope="module")
def reference(tiny, data):
    """the restatement's chains, computed once and shared"""
    _, eps = tiny
    y, x_T = data
    return {i: FR.Deconv(BETAS, "8").run(eps, x_T, y, K_TINY, PSF_TOL, SEED, **kw) for i, kw in zip(IDS, KINDS)}


def _invariant(got, y, k, tol):
    """(||A+ A x_out - Yp|| per plane with the library's own Yp, the bar: the step's first term with |x0| <= 1 plus circular_conv's bar
    for Yp itself)"""
    from ddk import ops
    h, w = got.shape[2:]
    L = math.log2(h * w)
    M = FR.kept(k, h, w, tol)
    Pf, P32 = _c2f(FR.pinv_spectrum(k, h, w, tol))
    Yp = nchw(ops.circular_conv(nhwc(y).to(DEV), Pf.to(DEV)).cpu())
    inv = _norm(FR.apply(got, M.astype(np.float64)) - Yp.double().numpy())
    bar = 16 * L * U24 * math.sqrt(h * w) + U24 * _norm(got) + (16 * L + 4) * U24 * np.abs(P32).max() * _norm(y)
    return inv, bar, Yp


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, reference, kw):
    m, _ = tiny
    y, x_T = data
    got = m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED, **kw).cpu()
    want = reference[IDS[KINDS.index(kw)]]
    err = float((got - want).abs().max())
    print(f"DDNM deconvolution tiny DDPM, 8 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    assert torch.equal(CC.argmax(got), CC.argmax(want))
    inv, bar, Yp = _invariant(got, y, K_TINY, PSF_TOL)
    print(f"  ||A+A x_out - A+y|| worst ratio to the bar {float((inv / bar).max()):.3g}")
    assert (inv <= bar).all()
    # the null-space part is the model's: the result is not A+ y
    assert float((got - Yp).abs().max()) > 1e-2


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_bit_for_bit(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    graphed = m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "use_graph", False):
        eager = m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED, **kw)
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_python_loop_equals_native(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    native = m.deconvolve(y.to(DEV), K_TINY, respacing="8", x_T=x_T, seed=SEED, **kw)      # the preset as an array: the same chain
    with CC.toggled(m, "native_sampler", False):
        loop = m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED, **kw)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, deconvolution 8 steps {kw}: {err:.3g}")
    assert err < 1e-5


def test_tail_parts_is_zero_for_every_shape(tiny):
    from models import Unet
    m, _ = tiny
    plan = m._eps_model_nhwc().plan()
    assert plan.restore_fft_tail_parts(2, 16, 16) == 0
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    for b, h, w in ((32, 32, 32), (8, 64, 64), (4, 128, 128), (1, 256, 256)):
        assert u._plan.restore_fft_tail_parts(b, h, w) == 0
    assert u._plan.restore_tail_parts(32, 32, 32, 2) == 8       # the shape has a fused tail; the plane-wide kind declines it


def _chain_operands(m, k, tol, h, w):
    from ddk import ops
    from models.diffusion import psf
    _, Pf, Mf, _ = psf.psf_operands(k, h, w, tol)
    Md = torch.from_numpy(Mf).to(DEV)
    return Md, torch.from_numpy(Pf).to(DEV), ops.fft_twiddles(max(h, w), Md.device)


def test_deconvolution_and_ancestral_chains_share_a_workspace(tiny, data, reference):
    """a deconvolution chain and a plain ancestral chain on the same plan, workspace, state buffer, tables and t_start, run
    alternately, then a chain with another batch of blurred images through the same cached graph: each reproduces its own first
    result bit for bit (the kind is in the graph key; mask, twiddles and Yp are staged by every call), and both batches come out
    right"""
    from ddk import lib as L
    from ddk import ops
    m, eps = tiny
    y, x_T = data
    tables, use = m._spaced_tables("8", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    nbytes = lib.ddk_sampler_restore_fft_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes == lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + 4 * (16 * 16 + 16 + 3 * 2 * 16 * 16 * 3)
    Md, Pd, tw = _chain_operands(m, K_TINY, PSF_TOL, 16, 16)
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    ys = {"a": ops.nchw_to_nhwc(y.to(DEV).contiguous()), "b": ops.nchw_to_nhwc((0.5 * y).to(DEV).contiguous())}

    def launch(what, a, tmap, stream):
        if what is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        return lib.ddk_sampler_run_restore_fft(a, tmap, L.ptr(Md), L.ptr(Pd), L.ptr(tw), L.ptr(ys[what]), stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    with CC.workspace(plan, nbytes) as ws:
        first = {}
        for what in ("a", None, "a", None, "b", "a", None, "b"):
            got = sh.run(ws, what)
            if what not in first:
                first[what] = got
            assert torch.equal(got, first[what]), (what, float((got - first[what]).abs().max()))
        assert not torch.equal(first["a"], first[None]) and not torch.equal(first["a"], first["b"])
        # the library's own entry and the model's method are the same chain
        via_model = m.deconvolve(y.to(DEV), PSF_TINY, respacing="8", x_T=x_T, seed=SEED)
        assert torch.equal(ops.nhwc_to_nchw(first["a"]), via_model)
        # both batches through the one graph are right
        assert float((ops.nhwc_to_nchw(first["a"]).cpu() - reference["ancestral"]).abs().max()) < TOL
        want_b = FR.Deconv(BETAS, "8").run(eps, x_T, 0.5 * y, K_TINY, PSF_TOL, SEED)
        assert float((ops.nhwc_to_nchw(first["b"]).cpu() - want_b).abs().max()) < TOL


def test_chain_faults(tiny):
    """the chain entry: injected noise, a null operand and a shape the kind does not take are DDK_ERR_ARG"""
    from ddk import lib as L
    m, _ = tiny
    tables, use = m._spaced_tables("8", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    tmap = CC.timestep_map(use)
    nbytes = lib.ddk_sampler_restore_fft_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes > 0 and lib.ddk_sampler_restore_fft_workspace_bytes(plan.handle, 2, 16, 48, K - 1) == 0
    x = torch.zeros(2, 16, 16, 3, device=DEV)
    y = torch.zeros(2, 16, 16, 3, device=DEV)
    Md, Pd, tw = _chain_operands(m, K_TINY, PSF_TOL, 16, 16)
    ws = CC.fresh_workspace(nbytes)
    noise = torch.zeros((K, *x.shape), device=DEV)
    args = lambda noise=None, H=16, nbytes=nbytes: CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED, noise=noise, shape=(2, H, 16))
    run = lib.ddk_sampler_run_restore_fft
    ops4 = (L.ptr(Md), L.ptr(Pd), L.ptr(tw), L.ptr(y))
    assert run(args(noise), tmap, *ops4, L.stream()) == -1 and "noise" in L.last_error()
    for i in range(4):
        assert run(args(), tmap, *(None if j == i else p for j, p in enumerate(ops4)), L.stream()) == -1 and "null" in L.last_error()
    assert run(args(), tmap, L.ptr(Md) + 4, *ops4[1:], L.stream()) == -1 and "alignment" in L.last_error()
    assert run(args(H=48), tmap, *ops4, L.stream()) == -1 and "powers of two" in L.last_error()
    assert run(args(nbytes=nbytes - 4), tmap, *ops4, L.stream()) != 0      # a short workspace
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    with pytest.raises(L.DDKError):
        plan.sample_restore_fft_nhwc(x, y, Md[:8].contiguous(), Pd, tables, K - 1, timesteps=use)
    with pytest.raises(L.DDKError):
        plan.sample_restore_fft_nhwc(x, y, Md, Pd[..., 0].contiguous(), tables, K - 1, timesteps=use)


def test_multi_launch_chain_256():
    """three steps at 3 x 256 x 256, B = 1, on a 32-wide model: the three-launch form inside a chain.  The native chain against the
    Python loop over the lone op, graph replay against eager launches, and the invariant"""
    m, _ = CC.tiny_ddpm(ddpm_cfg(32, 3, 256))
    shape = (1, 3, 256, 256)
    k = FR.preset("diag")
    clean = 0.25 * syn.synthetic_normal(shape, "deconv256.x")
    y = torch.from_numpy(FR.apply(clean, FR.spectrum(k, 256, 256))).float().contiguous()
    x_T = syn.synthetic_normal(shape, "deconv256.xT")
    native = m.deconvolve(y.to(DEV), "diag", respacing="3", x_T=x_T, seed=SEED)
    with CC.toggled(m, "use_graph", False):
        eager = m.deconvolve(y.to(DEV), "diag", respacing="3", x_T=x_T, seed=SEED)
    assert torch.equal(native, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = m.deconvolve(y.to(DEV), "diag", respacing="3", x_T=x_T, seed=SEED)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, deconvolution 256 x 256, 3 steps: {err:.3g}")
    assert torch.isfinite(native).all() and err < 1e-5
    inv, bar, _ = _invariant(native.cpu(), y, k, PSF_TOL)
    print(f"  ||A+A x_out - A+y|| worst ratio to the bar {float((inv / bar).max()):.3g}")
    assert (inv <= bar).all()


# ---------------------------------------------------------------- the command line
def test_deconv_cli_and_evaluator(tmp_path):
    """deconv_model_samples.py --blur_input and evaluate_restoration.py --task deconv with synthetic weights on four 16 x 16 images,
    each in a fresh process: the files, their shapes and the JSON keys"""
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 4, 16)
    rng = np.random.default_rng(0)
    rng.random((4, 16, 16, 3))                  # the images are the generator's first draw, the measured PSF its second
    kfile = tmp_path / "measured.npy"
    np.save(kfile, rng.random((5, 3)))
    CC.run_script("deconv_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--blur_input",
                  "--psf", "disk", "--tol", "0.1", "--timestep_respacing", "10", "--batch_size", "3", "--seed", "3", "--out_dir", tmp_path, env=env)
    out = np.load(tmp_path / "clitest_deconv_disk_10.npy")
    blurred = np.load(tmp_path / "clitest_deconv_disk_10_blurred.npy")
    assert out.shape == (4, 16, 16, 3) and out.dtype == np.float32
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert blurred.shape == (4, 16, 16, 3) and blurred.dtype == np.uint8
    want = FR.apply(torch.from_numpy(imgs.astype(np.float64)).permute(0, 3, 1, 2) / 255 * 2 - 1, FR.spectrum(FR.preset("disk"), 16, 16))
    assert np.abs(blurred.astype(np.float64) - (np.transpose(want, (0, 2, 3, 1)) + 1) * 127.5).max() <= 0.5 + 1e-3
    CC.run_script("evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "deconv", "--psf", kfile,
                  "--timestep_respacing", "10", "--batch_size", "3", "--json", tmp_path / "score.json", env=env)
    res = json.loads((tmp_path / "score.json").read_text())
    s, mt = res["settings"], res["metrics"]
    assert (s["task"], s["method"], s["psf"], s["tol"], s["unet_forwards"], s["n_images"]) == ("deconv", "ddnm_deconv", str(kfile), 0.03, 10, 4)
    assert {"restored", "blurred", "pinv", "consistency"} <= set(mt)
    for name in ("restored", "blurred", "pinv"):
        assert set(mt[name]) == {"psnr", "ssim"} and mt[name]["psnr"]["n"] == 4 and np.isfinite(mt[name]["psnr"]["mean"])
    assert {"mean", "stderr", "n", "max"} <= set(mt["consistency"])
    print(f"deconvolution evaluator (synthetic weights): {json.dumps(mt)}")
