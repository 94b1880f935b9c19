"""DDNM deblurring on the GPU (DDPM.deblur, ddk_sampler_run_restore_blur, ddk_p_sample_update_restore_blur, ddk_separable_apply;
csrc/separable.hip) against tests/blur_ref.py, the method restated in float64 around oracle/unet_ref with oracle/philox_ref draws.

The two matrix products run on the fp32 MFMA, whose summation order is not pinned, so the lone op is held to a derived bar instead of
bit for bit.  With u = 2^-24 (half an ulp of 1), the standard bound of an fp32 dot product of length n in any order is
n u sum |a_i b_i| (to first order).  P_h x0 P_w^T is a dot product of length H of dot products of length W: (H + W) u |P_h| |x0| |P_w|^T;
the 16 more cover the two accumulators' final add, the subtraction from x0 and the addition of Yp, whose operands are bounded by the
same three magnitudes.  c1 scales that into the result; the update's own five roundings are each half an ulp of one of its terms:

    |got - ref| <= |c1| (H + W + 16) u (|P_h| |x0| |P_w|^T + |x0| + |Yp|) + 4 u (|c1 x0'| + |c2 x| + |sigma z|)

elementwise, every element compared.  Shapes: both forms (an image of at most 64 KB takes one launch, a larger one two), one and
eight channels, W != H, sizes that are not a power of two.  Chains: 1e-4 abs against the restatement with the same argmax and 1e-5
between the Python loop and the native sampler, as for the other restore kinds; graph replay equals eager launches bit for bit."""
import json

import numpy as np
import pytest
import torch

import blur_ref as BR
import chain_cases as CC
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
ONE_LAUNCH = [(3, 16, 16), (1, 16, 16), (4, 32, 32), (3, 64, 64), (3, 16, 48), (8, 32, 16)]
TWO_LAUNCH = [(3, 128, 128), (3, 256, 256), (8, 64, 64), (3, 80, 144)]


def _first_term(P_h, P_w, x0_abs, Yp, H, W):
    """(H + W + 16) u (|P_h| |x0| |P_w|^T + |x0| + |Yp|), float64, [B, C, H, W]"""
    return (H + W + 16) * U24 * (BR.apply(x0_abs, P_h.abs(), P_w.abs()) + x0_abs.double() + Yp.double().abs())


def _mats(kernel, H, W):
    """the library's operands: the float64 matrices rounded to fp32 (as float64 for the reference, fp32 on the device)"""
    m = {k: v.float() for k, v in BR.operands(kernel, H, W).items()}
    return m, {k: v.to(DEV).contiguous() for k, v in m.items()}


def _inputs(c, h, w, B, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, c, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    yp = torch.rand(shape, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])[:B]
    return x, e, yp, t, CC.hand_tables(g)


# ---------------------------------------------------------------- the lone op against the restatement
@pytest.mark.parametrize("c,h,w", ONE_LAUNCH + TWO_LAUNCH)
def test_lone_op_within_the_derived_bar(c, h, w):
    from ddk import ops
    B = 1 if h * w >= 256 * 256 else 3
    x, e, yp, t, tab = _inputs(c, h, w, B, 31 * c + h + w)
    seed, stream = 97531, 4
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    m, md = _mats("uniform" if h >= 32 else "gauss", h, w)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    want, x0, x0p = BR.step(x, e, m["P_h"].double(), m["P_w"].double(), yp, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t],
                            tab["c2"][t], sg, z)
    col = lambda v: v.reshape(-1, 1, 1, 1).double()
    c1, c2 = col(tab["c1"][t]), col(tab["c2"][t])
    bar = c1.abs() * _first_term(m["P_h"].double(), m["P_w"].double(), x0.abs(), yp, h, w) + \
        4 * U24 * ((c1 * x0p).abs() + (c2 * x.double()).abs() + (col(sg) * z.double()).abs())
    xs = nhwc(x).to(DEV)
    ops.p_sample_update_restore_blur_(xs, nhwc(e).to(DEV), md["P_h"], md["P_w"], nhwc(yp).to(DEV), t.to(DEV),
                                      **{k: v.to(DEV) for k, v in tab.items()}, seed=seed, stream_id=stream)
    got = nchw(xs.cpu())
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = (got.double() - want).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    form = "one launch" if h * w * c * 4 <= 65536 else "two launches"
    print(f"lone blur op c={c} {h}x{w} B={B} ({form}): max abs error {float(err.max()):.3g}, worst ratio to the bar {ratio:.3g}")
    assert bool((err <= bar).all()), ratio
    # row 0 returns x0' itself: its projection is Yp's
    inv = (BR.apply(got[0:1], m["P_h"], m["P_w"]) - BR.apply(yp[0:1], m["P_h"], m["P_w"])).abs()
    print(f"  row 0: |P x P^T - P Yp P^T| max {float(inv.max()):.3g}")


@pytest.mark.parametrize("c,h,w", [(3, 16, 16), (3, 128, 128)])
def test_exact_cases(c, h, w):
    """P = 0 and Yp = 0: the Ancestral kind's Philox-drawn lone op, bit for bit.  P = I: row 0 returns Yp.  Two calls agree."""
    from ddk import ops
    B = 3
    x, e, yp, t, tab = _inputs(c, h, w, B, 7 + h)
    tabd = {k: v.to(DEV) for k, v in tab.items()}
    seed, stream = 1234, 2
    xs, es, td = nhwc(x).to(DEV), nhwc(e).to(DEV), t.to(DEV)
    zero_h, zero_w = torch.zeros(h, h, device=DEV), torch.zeros(w, w, device=DEV)
    got = ops.p_sample_update_restore_blur_(xs.clone(), es, zero_h, zero_w, torch.zeros_like(xs), td, **tabd, seed=seed, stream_id=stream)
    want = ops.p_sample_update_(xs.clone(), es, td, **tabd, seed=seed, stream_id=stream)
    assert torch.equal(got, want), float((got - want).abs().max())
    eye_h, eye_w = torch.eye(h, device=DEV), torch.eye(w, device=DEV)
    yd = nhwc(yp).to(DEV)
    got = ops.p_sample_update_restore_blur_(xs.clone(), es, eye_h, eye_w, yd, td, **tabd, seed=seed, stream_id=stream)
    assert torch.equal(got[0], yd[0])
    assert not torch.equal(got[1], yd[1])
    _, md = _mats("uniform", h, w)
    a = ops.p_sample_update_restore_blur_(xs.clone(), es, md["P_h"], md["P_w"], yd, td, **tabd, seed=seed, stream_id=stream)
    b = ops.p_sample_update_restore_blur_(xs.clone(), es, md["P_h"], md["P_w"], yd, td, **tabd, seed=seed, stream_id=stream)
    assert torch.equal(a, b) and not torch.equal(a, got)


# ---------------------------------------------------------------- ops.separable_apply
@pytest.mark.parametrize("c,h,w", [(3, 16, 16), (3, 64, 64), (3, 128, 128), (1, 256, 256)])
def test_separable_apply(c, h, w):
    from ddk import ops
    g = torch.Generator().manual_seed(h + c)
    B = 2
    x = torch.randn(B, c, h, w, generator=g)
    Lm, Rm = torch.randn(h, h, generator=g) / h ** 0.5, torch.randn(w, w, generator=g) / w ** 0.5
    got = nchw(ops.separable_apply(nhwc(x).to(DEV), Lm.to(DEV), Rm.to(DEV)).cpu())
    want = BR.apply(x, Lm, Rm)
    bar = (h + w + 16) * U24 * BR.apply(x.abs(), Lm.abs(), Rm.abs())
    err = (got.double() - want).abs()
    print(f"separable_apply c={c} {h}x{w}: max abs error {float(err.max()):.3g}, worst ratio {float((err / bar).max()):.3g}")
    assert bool((err <= bar).all())
    # with (A_h, A_w) it is the zero-padded blur
    m, md = _mats("uniform", h, w)
    k_h, k_w = BR.taps("uniform")
    k2 = torch.from_numpy(np.outer(k_h, k_w)).reshape(1, 1, 9, 9)
    conv = torch.nn.functional.conv2d(x.double().reshape(B * c, 1, h, w), k2, padding=4).reshape(B, c, h, w)
    xd = nhwc(x).to(DEV)
    blurred = nchw(ops.separable_apply(xd, md["A_h"], md["A_w"], out=xd).cpu())      # in place
    bar = (h + w + 16) * U24 * BR.apply(x.abs(), m["A_h"].abs(), m["A_w"].abs())
    err = (blurred.double() - conv).abs()
    print(f"  blur vs conv2d: max abs error {float(err.max()):.3g}, worst ratio {float((err / bar).max()):.3g}")
    assert bool((err <= bar).all())


# ---------------------------------------------------------------- argument faults
def test_argument_faults_run_no_kernel():
    from ddk import lib as L
    from ddk import ops
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)

    def call(h, w, c, P_h="ok", P_w="ok"):
        x = torch.full((1, h, w, c), 0.25, device=DEV)
        before = x.clone()
        P_h = torch.eye(h, device=DEV) if isinstance(P_h, str) else P_h
        P_w = torch.eye(w, device=DEV) if isinstance(P_w, str) else P_w
        with pytest.raises(L.DDKError):
            ops.p_sample_update_restore_blur_(x, torch.ones_like(x), P_h, P_w, torch.zeros_like(x), t, **tab)
        torch.cuda.synchronize()
        assert torch.equal(x, before)
        if P_h is not None and P_w is not None:
            with pytest.raises(L.DDKError):
                ops.separable_apply(x, P_h, P_w)

    call(24, 16, 3)
    call(16, 24, 3)
    call(272, 16, 3)
    call(16, 16, 9)
    call(16, 16, 3, P_h=None)
    call(16, 16, 3, P_w=None)


def test_chain_faults(tiny):
    """the chain entry: injected noise, a null matrix and a shape the kind does not take are DDK_ERR_ARG"""
    from ddk import lib as L
    m, _ = tiny
    tables, use = m._spaced_tables("20", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    tmap = CC.timestep_map(use)
    nbytes = lib.ddk_sampler_restore_blur_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes > 0
    _, md = _mats("gauss", 16, 16)
    x = torch.zeros(2, 16, 16, 3, device=DEV)
    y = torch.zeros_like(x)
    ws = CC.fresh_workspace(nbytes)
    noise = torch.zeros((K, *x.shape), device=DEV)
    args = lambda noise=None, H=16: CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED, noise=noise, shape=(2, H, 16))
    mats = [L.ptr(md[k]) for k in ("P_h", "P_w", "Q_h", "Q_w")]
    assert lib.ddk_sampler_run_restore_blur(args(noise), tmap, *mats, L.ptr(y), L.stream()) == -1 and "noise" in L.last_error()
    for i in range(4):
        bad = list(mats)
        bad[i] = None
        assert lib.ddk_sampler_run_restore_blur(args(), tmap, *bad, L.ptr(y), L.stream()) == -1 and "null" in L.last_error()
    assert lib.ddk_sampler_run_restore_blur(args(), tmap, *mats, None, L.stream()) == -1
    assert lib.ddk_sampler_run_restore_blur(args(H=24), tmap, *mats, L.ptr(y), L.stream()) == -1 and "multiples of 16" in L.last_error()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    with pytest.raises(L.DDKError):
        plan.sample_restore_blur_nhwc(x, y, md["P_h"], md["P_w"], md["Q_h"][:8, :8].contiguous(), md["Q_w"], tables, K - 1, timesteps=use)


# ---------------------------------------------------------------- the tiny DDPM, "20" steps
@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


KERNELS = ["gauss", "uniform"]      # at 16 x 16 the gauss kernel keeps all 16 singular values of an axis (x_out is A+ y whatever the
                                    # model says), the uniform one 14: there the null-space part of the result is the model's


@pytest.fixture(scope="module")
def data():
    m = {k: BR.operands(k, 16, 16) for k in KERNELS}
    # a quarter of a standard normal image: inside [-1, 1] without clamping (max 0.79), so its largest value is not one of many ties at 1
    # (top two 0.022 and 0.10 apart).  The gauss kernel keeps every singular value at 16 x 16, so the result is close to this image.
    clean = 0.25 * syn.synthetic_normal(SHAPE, "deblur.x")
    assert float(clean.abs().max()) < 1
    return {k: BR.apply(clean, m[k]["A_h"], m[k]["A_w"]).float().contiguous() for k in KERNELS}, syn.synthetic_normal(SHAPE, "deblur.xT")


@pytest.fixture(scope="module")
def reference(tiny, data):
    """the restatement's chains, computed once and shared"""
    _, eps = tiny
    ys, x_T = data
    return {(k, i): BR.Deblur(BETAS, "20").run(eps, x_T, ys[k], k, SEED, **kw) for k in KERNELS for i, kw in zip(IDS, KINDS)}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, reference, kw, kernel):
    m, _ = tiny
    y, x_T = data[0][kernel], data[1]
    got = m.deblur(y.to(DEV), kernel, respacing="20", x_T=x_T, seed=SEED, **kw).cpu()
    want = reference[(kernel, IDS[KINDS.index(kw)])]
    err = float((got - want).abs().max())
    print(f"DDNM deblur ({kernel}) tiny DDPM, 20 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    assert torch.equal(CC.argmax(got), CC.argmax(want))
    # the invariant: the range-space part of the result is A+ y.  Row 0 has c1 = 1 and |x0| <= 1 (clamped), which bounds the first term.
    mm = {k: v.float().double() for k, v in BR.operands(kernel, 16, 16).items()}
    Yp = BR.apply(y, mm["Q_h"], mm["Q_w"])
    inv = (BR.apply(got, mm["P_h"], mm["P_w"]) - Yp).abs()
    bar = _first_term(mm["P_h"], mm["P_w"], torch.ones(SHAPE), Yp, 16, 16)
    print(f"  |P x_out P^T - Yp| max {float(inv.max()):.3g}, worst ratio to the first term {float((inv / bar).max()):.3g}")
    assert bool((inv <= bar).all())
    gap = float((BR.apply(got, mm["A_h"], mm["A_w"]) - y.double()).abs().max())
    print(f"  max|A(x_out) - y| = {gap:.3g} (limited by the truncation; not asserted)")
    if kernel == "uniform":      # the null space is not empty: the chain kind shows in the result
        assert float((got - BR.apply(y, mm["Q_h"], mm["Q_w"]).float()).abs().max()) > 1e-2


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_bit_for_bit(tiny, data, kw, kernel):
    m, _ = tiny
    y, x_T = data[0][kernel], data[1]
    graphed = m.deblur(y.to(DEV), kernel, respacing="20", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "use_graph", False):
        eager = m.deblur(y.to(DEV), kernel, respacing="20", x_T=x_T, seed=SEED, **kw)
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_python_loop_equals_native(tiny, data, kw, kernel):
    m, _ = tiny
    y, x_T = data[0][kernel], data[1]
    native = m.deblur(y.to(DEV), kernel, respacing="20", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "native_sampler", False):
        loop = m.deblur(y.to(DEV), kernel, respacing="20", x_T=x_T, seed=SEED, **kw)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, deblur ({kernel}) 20 steps {kw}: {err:.3g}")
    assert err < 1e-5


def test_tail_parts_is_zero_for_every_shape(tiny):
    from models import Unet
    m, _ = tiny
    plan = m._eps_model_nhwc().plan()
    assert plan.restore_blur_tail_parts(2, 16, 16) == 0
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    for b, h, w in ((32, 32, 32), (8, 64, 64), (1, 16, 48), (4, 128, 128), (1, 256, 256)):
        assert u._plan.restore_blur_tail_parts(b, h, w) == 0
    assert u._plan.restore_tail_parts(32, 32, 32, 2) == 8       # the shape has a fused tail; the plane-wide kind declines it


# ---------------------------------------------------------------- one workspace, two kinds of chain
def test_blur_and_ancestral_chains_share_a_workspace(tiny, data):
    """a blur chain and a plain ancestral chain on the same plan, workspace, state buffer, tables and t_start, run alternately, then a
    blur chain with another y: each reproduces its own first result bit for bit (the kind is in the graph key; the matrices and y are
    staged by every call)"""
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    y, x_T = data[0]["uniform"], data[1]
    tables, use = m._spaced_tables("20", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    nbytes = lib.ddk_sampler_restore_blur_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes == lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + 4 * (2 * 16 * 16 + 2 * 2 * 16 * 16 * 3)
    md = m._blur_operands("uniform", 3e-2)       # the model's own cached operands
    mats = [L.ptr(md[k]) for k in ("P_h", "P_w", "Q_h", "Q_w")]
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    ys = {"a": ops.nchw_to_nhwc(y.to(DEV)), "b": ops.nchw_to_nhwc((0.5 * y).to(DEV))}

    def launch(what, a, tmap, stream):
        if what is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        return lib.ddk_sampler_run_restore_blur(a, tmap, *mats, L.ptr(ys[what]), stream)

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
        via_model = m.deblur(y.to(DEV), "uniform", respacing="20", x_T=x_T, seed=SEED)
        assert torch.equal(ops.nhwc_to_nchw(first["a"]), via_model)


# ---------------------------------------------------------------- the command line
def test_deblur_cli_and_evaluator(tmp_path):
    """deblur_model_samples.py (already blurred input, then --blur_input) and evaluate_restoration.py --task deblur with synthetic
    weights on four 16 x 16 images, each in a fresh process: the files, their shapes and the JSON keys"""
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 4, 16)
    for extra, kernel, spec in (([], "gauss", "10"), (["--blur_input", "--kernel", "uniform", "--use_ddim", "--eta", "0.5"], "uniform", "10_ddim_eta0.5")):
        CC.run_script("deblur_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path,
                      "--timestep_respacing", "10", "--batch_size", "3", "--seed", "3", "--out_dir", tmp_path, *extra, env=env)
        out = np.load(tmp_path / f"clitest_deblur_{kernel}_{spec}.npy")
        blurred = np.load(tmp_path / f"clitest_deblur_{kernel}_{spec}_blurred.npy")
        assert out.shape == (4, 16, 16, 3) and out.dtype == np.float32
        assert blurred.shape == (4, 16, 16, 3) and blurred.dtype == np.uint8
        assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
        if not extra:
            assert np.array_equal(blurred, imgs)
        else:
            m = BR.operands("uniform", 16, 16)
            want = BR.apply(torch.from_numpy(imgs.astype(np.float64)).permute(0, 3, 1, 2) / 255 * 2 - 1, m["A_h"], m["A_w"])
            want = ((want + 1) * 127.5).round().clamp(0, 255).permute(0, 2, 3, 1).numpy()
            assert np.abs(blurred.astype(np.float64) - want).max() <= 1      # a rounding tie may fall either way in fp32
    CC.run_script("evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "deblur", "--kernel", "uniform",
                  "--timestep_respacing", "10", "--batch_size", "3", "--json", tmp_path / "score.json", env=env)
    res = json.loads((tmp_path / "score.json").read_text())
    s, mt = res["settings"], res["metrics"]
    assert (s["task"], s["method"], s["kernel"], s["tol"], s["unet_forwards"], s["n_images"]) == ("deblur", "ddnm_blur", "uniform", 0.03, 10, 4)
    assert set(mt) == {"restored", "blurred", "pinv", "consistency", "consistency_u8"}
    for name in ("restored", "blurred", "pinv"):
        assert set(mt[name]) == {"psnr", "ssim"} and mt[name]["psnr"]["n"] == 4 and np.isfinite(mt[name]["psnr"]["mean"])
    assert {"mean", "stderr", "n", "max"} <= set(mt["consistency"])
    print(f"deblur evaluator (synthetic weights): {json.dumps(mt)}")
