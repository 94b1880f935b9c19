"""DDNM for size-changing separable operators on the GPU: ddk_separable_apply_rect, the lone deblurring op
against the block-local super-resolution op on the block-mean operator, and DDPM.restore_separable / super_resolve(downsample="bicubic")
through ddk_sampler_run_restore_sep, against tests/resize_ref.py (the method restated in float64 around oracle/unet_ref with
oracle/philox_ref draws).

The bars.  u = 2^-24.  L . in . R^T is a dot product of length Hi of dot products of length Wi, each in an order the MFMA does not pin:
|got - ref| <= (Hi + Wi + 16) u (|L| |in| |R|^T) elementwise (section 3.14's bound with the contracted lengths; the 16 cover the two
accumulators' final adds).  The lone op's bar is test_restore_blur_gpu.py's.  Chains: 1e-4 abs against the restatement with the same
argmax, the TOL of the deblurring tests for the same model and the same step kernels, and 1e-5 between the Python loop and the native
sampler; graph replay equals eager launches bit for bit."""
import json

import numpy as np
import pytest
import torch

import blur_ref as BR
import chain_cases as CC
import resize_ref as ZR
from helpers import dddpm_cfg, ddpm_cfg, to_nchw as nchw, to_nhwc as nhwc
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
SCALES = [2, 4]
U24 = 2.0 ** -24
# (C, Hi, Wi, Ho, Wo): K = 8 tail and a 24-wide partial strip; K = 4; K = 12 and 20, not square; whole tiles; the largest; half an
# output tile in the reducing direction; a quarter tile; eight channels, not square; the largest reduction
RECT = [(3, 8, 8, 32, 32), (1, 4, 4, 16, 16), (3, 12, 20, 48, 80), (3, 16, 16, 64, 64), (3, 64, 64, 256, 256), (3, 32, 32, 8, 8),
        (1, 16, 16, 4, 4), (8, 64, 32, 16, 8), (3, 256, 256, 64, 64)]
B = 2


def _rect_inputs(c, hi, wi, ho, wo):
    g = torch.Generator().manual_seed(1000 * c + 7 * hi + wi + ho)
    x = torch.randn(B, c, hi, wi, generator=g)
    return x, torch.randn(ho, hi, generator=g) / hi ** 0.5, torch.randn(wo, wi, generator=g) / wi ** 0.5


# ---------------------------------------------------------------- ops.separable_apply_rect
@pytest.mark.parametrize("c,hi,wi,ho,wo", RECT)
def test_rect_apply_within_the_derived_bar(c, hi, wi, ho, wo):
    from ddk import ops
    x, Lm, Rm = _rect_inputs(c, hi, wi, ho, wo)
    xd, Ld, Rd = nhwc(x).to(DEV), Lm.to(DEV), Rm.to(DEV)
    got_d = ops.separable_apply_rect(xd, Ld, Rd)
    again = ops.separable_apply_rect(xd, Ld, Rd, out=torch.full_like(got_d, float("nan")))
    assert tuple(got_d.shape) == (B, ho, wo, c) and torch.equal(got_d, again)
    got = nchw(got_d.cpu())
    want = BR.apply(x, Lm, Rm)
    bar = (hi + wi + 16) * U24 * BR.apply(x.abs(), Lm.abs(), Rm.abs())
    err = (got.double() - want).abs()
    print(f"separable_apply_rect c={c} {hi}x{wi} -> {ho}x{wo}: max abs error {float(err.max()):.3g}, worst ratio {float((err / bar).max()):.3g}")
    assert torch.isfinite(got).all() and bool((err <= bar).all())


@pytest.mark.parametrize("c,hi,wi,ho,wo", RECT)
def test_rect_apply_exact_cases(c, hi, wi, ho, wo):
    """rows of the identity pick a strided slice, repeated rows repeat the input: no arithmetic but x 1 and + 0, so any slip of an index
    or a guard shows exactly"""
    from ddk import ops
    x = nhwc(_rect_inputs(c, hi, wi, ho, wo)[0]).to(DEV)
    if ho > hi:
        nh, nw = ho // hi, wo // wi
        Lm = torch.eye(hi, device=DEV).repeat_interleave(nh, dim=0)
        Rm = torch.eye(wi, device=DEV).repeat_interleave(nw, dim=0)
        want = x.repeat_interleave(nh, dim=1).repeat_interleave(nw, dim=2)
    else:
        sh, sw = hi // ho, wi // wo
        Lm = torch.eye(hi, device=DEV)[0::sh].contiguous()
        Rm = torch.eye(wi, device=DEV)[sw - 1::sw].contiguous()
        want = x[:, 0::sh, sw - 1::sw]
    got = ops.separable_apply_rect(x, Lm, Rm)
    assert tuple(got.shape) == (B, ho, wo, c) and torch.equal(got, want)


@pytest.mark.parametrize("c,hi,wi,ho,wo", RECT)
def test_rect_apply_reads_and_writes_inside_its_tensors(c, hi, wi, ho, wo):
    """in, L, R, scratch and out carved out of one NaN-filled buffer, 16-byte aligned with NaN between them: a read past a row's end
    puts a NaN into the result, a write past a tile shows outside the out and scratch slices"""
    from ddk import lib as L
    x, Lm, Rm = _rect_inputs(c, hi, wi, ho, wo)
    sizes = dict(inp=B * hi * wi * c, Lm=ho * hi, Rm=wo * wi, scr=B * ho * wi * c, out=B * ho * wo * c)
    off, at = {}, 64
    for k, n in sizes.items():
        off[k] = at
        at += (n + 3) // 4 * 4 + 64          # 64 NaNs between two tensors, every start on a 16-byte boundary
    buf = torch.full((at,), float("nan"), device=DEV)
    view = lambda k: buf[off[k]:off[k] + sizes[k]]
    view("inp").copy_(nhwc(x).reshape(-1))
    view("Lm").copy_(Lm.reshape(-1))
    view("Rm").copy_(Rm.reshape(-1))
    before = buf.clone()
    rc = L.load().ddk_separable_apply_rect(L.ptr(view("inp")), L.ptr(view("Lm")), L.ptr(view("Rm")), L.ptr(view("out")), L.ptr(view("scr")),
                                           B, hi, wi, ho, wo, c, L.stream())
    assert rc == 0, L.last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(view("out")).all() and torch.isfinite(view("scr")).all()
    written = torch.zeros(at, dtype=torch.bool, device=DEV)
    for k in ("out", "scr"):
        written[off[k]:off[k] + sizes[k]] = True
    same = buf.view(torch.int32) == before.view(torch.int32)
    assert bool(same[~written].all())
    from ddk import ops
    assert torch.equal(view("out").reshape(B, ho, wo, c), ops.separable_apply_rect(nhwc(x).to(DEV), Lm.to(DEV), Rm.to(DEV)))


@pytest.mark.parametrize("c,h,w", [(3, 16, 16), (3, 64, 64), (8, 32, 16), (3, 128, 128), (1, 256, 256), (3, 80, 144)])
def test_rect_apply_equals_the_square_form_bit_for_bit(c, h, w):
    from ddk import ops
    x, Lm, Rm = _rect_inputs(c, h, w, h, w)
    xd, Ld, Rd = nhwc(x).to(DEV), Lm.to(DEV), Rm.to(DEV)
    assert torch.equal(ops.separable_apply_rect(xd, Ld, Rd), ops.separable_apply(xd, Ld, Rd))


def test_rect_apply_argument_faults_run_no_kernel():
    from ddk import lib as L
    from ddk import ops
    lib = L.load()

    def call(hi=8, wi=8, ho=32, wo=32, c=3, shift=None, alias=None):
        t = dict(inp=torch.ones(B * hi * wi * c + 4, device=DEV), Lm=torch.ones(ho * hi + 4, device=DEV), Rm=torch.ones(wo * wi + 4, device=DEV),
                 scr=torch.zeros(B * ho * wi * c + 4, device=DEV), out=torch.full((B * ho * wo * c + 4,), 0.25, device=DEV))
        p = {k: (v[1:] if k == shift else v) for k, v in t.items()}
        if alias:
            p["out"] = p[alias]
        before = {k: v.clone() for k, v in t.items()}
        rc = lib.ddk_separable_apply_rect(L.ptr(p["inp"]), L.ptr(p["Lm"]), L.ptr(p["Rm"]), L.ptr(p["out"]), L.ptr(p["scr"]), B, hi, wi, ho, wo, c,
                                          L.stream())
        torch.cuda.synchronize()
        assert rc == -1 and "separable_apply_rect" in L.last_error(), (rc, L.last_error())
        assert all(torch.equal(t[k], before[k]) for k in t)

    call(hi=6)
    call(wo=30)
    call(ho=260)
    call(wi=2)
    call(c=9)
    for k in ("inp", "Lm", "Rm", "scr", "out"):
        call(shift=k)
    call(hi=32, wi=32, alias="inp")
    call(alias="scr")
    x = torch.ones(B, 8, 8, 3, device=DEV)
    with pytest.raises(L.DDKError):
        ops.separable_apply_rect(x, torch.ones(32, 12, device=DEV), torch.ones(32, 8, device=DEV))
    with pytest.raises(L.DDKError):
        ops.separable_apply_rect(x, torch.ones(32, 8, device=DEV), torch.ones(32, 8, device=DEV), out=torch.ones(B, 32, 16, 3, device=DEV))
    with pytest.raises(L.DDKError):
        ops.separable_apply_rect(x, torch.ones(8, 8, device=DEV), torch.ones(8, 8, device=DEV), out=x)


# ---------------------------------------------------------------- the lone op on the block-mean operator: two kernels, one operator
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("c,h,w", [(3, 16, 16), (3, 128, 128)])
def test_plane_wide_op_agrees_with_the_block_local_op(c, h, w, n):
    """P = A+ A of resize_matrix(kind="mean") is the block-mean projection and A+ y repeats y, so p_sample_update_restore_blur_ and the
    block-local p_sample_update_restore_ compute one step by two independent kernels.  They may differ by the plane-wide op's derived
    bar (test_restore_blur_gpu.py): |c1| (H + W + 16) u (|P_h| |x0| |P_w|^T + |x0| + |Yp|) + 4 u (|c1 x0'| + |c2 x| + |sigma z|)."""
    from ddk import ops
    from models.diffusion import blur
    g = torch.Generator().manual_seed(31 * c + h + n)
    Bn = 3
    shape = (Bn, c, h, w)
    x, e = 2 * torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    y = torch.rand((Bn, c, h // n, w // n), generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])
    tab = CC.hand_tables(g)
    seed, stream = 97531, 4
    m = dict(zip(("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w"), blur.separable_operands(blur.resize_matrix(h, n, "mean"), blur.resize_matrix(w, n, "mean"))))
    assert float((m["Q_h"] - torch.eye(h // n).repeat_interleave(n, dim=0)).abs().max()) <= 1e-6       # A+ repeats
    yp = y.repeat_interleave(n, dim=2).repeat_interleave(n, dim=3)            # both ops get the exact A+ y
    tabd = {k: v.to(DEV) for k, v in tab.items()}
    xs, es, td = nhwc(x).to(DEV), nhwc(e).to(DEV), t.to(DEV)
    yp_dev = nhwc(yp).to(DEV)
    formed = ops.separable_apply_rect(nhwc(y).to(DEV), m["Q_h"].to(DEV), m["Q_w"].to(DEV))
    assert float((formed - yp_dev).abs().max()) <= 1e-5      # (what the chain entry would form; Q's zeros are 1e-17 after the SVD)
    wide = ops.p_sample_update_restore_blur_(xs.clone(), es, m["P_h"].to(DEV), m["P_w"].to(DEV), yp_dev, td, **tabd, seed=seed, stream_id=stream)
    local = ops.p_sample_update_restore_(xs.clone(), es, nhwc(y).to(DEV), n, td, **tabd, seed=seed, stream_id=stream)
    z = nchw(torch.stack([ops.randn((Bn, h, w, c), DEV, seed, int(tb), stream)[b] for b, tb in enumerate(t)]).cpu())
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(Bn))
    P_h, P_w = m["P_h"].double(), m["P_w"].double()
    want, x0, x0p = BR.step(x, e, P_h, P_w, yp, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], sg, z)
    col = lambda v: v.reshape(-1, 1, 1, 1).double()
    c1, c2 = col(tab["c1"][t]), col(tab["c2"][t])
    bar = c1.abs() * (h + w + 16) * U24 * (BR.apply(x0.abs(), P_h.abs(), P_w.abs()) + x0.abs().double() + yp.double().abs()) + \
        4 * U24 * ((c1 * x0p).abs() + (c2 * x.double()).abs() + (col(sg) * z.double()).abs())
    diff = (nchw(wide.cpu()).double() - nchw(local.cpu()).double()).abs()
    e_wide = (nchw(wide.cpu()).double() - want).abs()
    print(f"plane-wide vs block-local, c={c} {h}x{w} n={n}: max diff {float(diff.max()):.3g}, worst ratio to the bar "
          f"{float((diff / bar.clamp_min(1e-300)).max()):.3g}; plane-wide vs float64 ratio {float((e_wide / bar.clamp_min(1e-300)).max()):.3g}")
    assert bool((diff <= bar).all()) and bool((e_wide <= bar).all())


# ---------------------------------------------------------------- the tiny DDPM, "20" steps
@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    """y[scale]: the bicubic reduction of a quarter of a standard normal image (inside [-1, 1], its largest value no tie at 1), formed in
    float64 with the restatement's matrix; x_T"""
    clean = 0.25 * syn.synthetic_normal(SHAPE, "resize.x")
    assert float(clean.abs().max()) < 1
    A = {n: torch.from_numpy(ZR.matrix(16, n)) for n in SCALES}
    return {n: BR.apply(clean, A[n], A[n]).float().contiguous() for n in SCALES}, syn.synthetic_normal(SHAPE, "resize.xT")


@pytest.fixture(scope="module")
def reference(tiny, data):
    """the restatement's chains, computed once and shared"""
    _, eps = tiny
    ys, x_T = data
    return {(n, i): ZR.Separable(BETAS, "20").run(eps, x_T, ys[n], ZR.matrix(16, n), ZR.matrix(16, n), SEED, **kw)
            for n in SCALES for i, kw in zip(IDS, KINDS)}


@pytest.mark.parametrize("n", SCALES)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, reference, kw, n):
    m, _ = tiny
    y, x_T = data[0][n], data[1]
    got = m.super_resolve(y.to(DEV), n, downsample="bicubic", respacing="20", x_T=x_T, seed=SEED, **kw).cpu()
    want = reference[(n, IDS[KINDS.index(kw)])]
    err = float((got - want).abs().max())
    print(f"DDNM bicubic x{n} tiny DDPM, 20 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    assert torch.equal(CC.argmax(got), CC.argmax(want))
    # full row rank: A P = A, so A(x_out) = y as far as fp32 goes.  Whatever the chain's distance from the restatement (< TOL per
    # element) does to the gap is at most the largest absolute row sums of the two matrices times TOL.
    mm = {k: v.float().double() for k, v in ZR.operands(ZR.matrix(16, n), ZR.matrix(16, n)).items()}
    gap = lambda v: float((BR.apply(v, mm["A_h"], mm["A_w"]) - y.double()).abs().max())
    r_h, r_w = float(mm["A_h"].abs().sum(dim=1).max()), float(mm["A_w"].abs().sum(dim=1).max())
    print(f"  max|A(x_out) - y| = {gap(got):.3g}, the restatement's {gap(want):.3g}, row sums {r_h:.3f} {r_w:.3f}")
    assert gap(got) <= gap(want) + r_h * r_w * TOL
    # the null space is 3/4 (15/16) of the image: the model's part shows
    assert float((got - BR.apply(y, mm["Q_h"], mm["Q_w"]).float()).abs().max()) > 1e-2


@pytest.mark.parametrize("n", SCALES)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_bit_for_bit(tiny, data, kw, n):
    m, _ = tiny
    y, x_T = data[0][n], data[1]
    run = lambda: m.super_resolve(y.to(DEV), n, downsample="bicubic", respacing="20", x_T=x_T, seed=SEED, **kw)
    graphed = run()
    with CC.toggled(m, "use_graph", False):
        eager = run()
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("n", SCALES)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_python_loop_equals_native(tiny, data, kw, n):
    m, _ = tiny
    y, x_T = data[0][n], data[1]
    run = lambda: m.super_resolve(y.to(DEV), n, downsample="bicubic", respacing="20", x_T=x_T, seed=SEED, **kw)
    native = run()
    with CC.toggled(m, "native_sampler", False):
        loop = run()
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, bicubic x{n} 20 steps {kw}: {err:.3g}")
    assert err < 1e-5


@pytest.mark.parametrize("n", SCALES)
def test_super_resolve_is_restore_separable(tiny, data, n):
    from models.diffusion import blur
    m, _ = tiny
    y, x_T = data[0][n], data[1]
    a = m.super_resolve(y.to(DEV), n, downsample="bicubic", respacing="20", x_T=x_T, seed=SEED)
    b = m.restore_separable(y.to(DEV), blur.resize_matrix(16, n), torch.from_numpy(blur.resize_matrix(16, n)), respacing="20", x_T=x_T, seed=SEED)
    assert torch.equal(a, b)
    # not the block-mean chain
    assert not torch.equal(a, m.super_resolve(y.to(DEV), n, respacing="20", x_T=x_T, seed=SEED))


def test_an_operator_of_the_planes_size_is_deblur_bit_for_bit(tiny, data):
    """h = H, w = W with a blur's matrices: the new entry runs the old entry's chain"""
    from models.diffusion import blur
    m, _ = tiny
    x_T = data[1]
    k_h, k_w = blur.blur_kernel("uniform")
    A_h, A_w = blur.blur_matrix(16, k_h), blur.blur_matrix(16, k_w)
    y = BR.apply(0.25 * syn.synthetic_normal(SHAPE, "resize.x"), torch.from_numpy(A_h), torch.from_numpy(A_w)).float().contiguous()
    for kw in KINDS:
        a = m.restore_separable(y.to(DEV), A_h, A_w, respacing="20", x_T=x_T, seed=SEED, **kw)
        b = m.deblur(y.to(DEV), "uniform", respacing="20", x_T=x_T, seed=SEED, **kw)
        assert torch.equal(a, b)


def test_chain_faults(tiny, data):
    """the chain entry: h or w off the grid, larger than the plane, a null matrix and injected noise are DDK_ERR_ARG; x is not touched"""
    from ddk import lib as L
    m, _ = tiny
    tables, use = m._spaced_tables("20", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    tmap = CC.timestep_map(use)
    nbytes = lib.ddk_sampler_restore_blur_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    md = m._sep_operands(ZR.matrix(16, 2), ZR.matrix(16, 2), 3e-2)
    x = torch.zeros(2, 16, 16, 3, device=DEV)
    y = torch.zeros(2, 8, 8, 3, device=DEV)
    ws = CC.fresh_workspace(nbytes)
    noise = torch.zeros((K, *x.shape), device=DEV)
    mats = [L.ptr(md[k]) for k in ("P_h", "P_w", "Q_h", "Q_w")]

    def run(mats=mats, noise=None, h=8, w=8):
        a = CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED, noise=noise)
        return lib.ddk_sampler_run_restore_sep(a, tmap, *mats, L.ptr(y), h, w, L.stream())
    assert run(noise=noise) == -1 and "noise" in L.last_error()
    for h, w in ((6, 8), (8, 2), (0, 8), (20, 8), (8, 32)):
        assert run(h=h, w=w) == -1 and "multiples of 4" in L.last_error()
    for i in range(4):
        bad = list(mats)
        bad[i] = None
        assert run(mats=bad) == -1 and "null" in L.last_error()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    with pytest.raises(L.DDKError):
        plan.sample_restore_sep_nhwc(x, y, md["P_h"], md["P_w"], md["Q_h"], md["Q_w"][:, :4].contiguous(), tables, K - 1, timesteps=use)
    with pytest.raises(L.DDKError):
        plan.sample_restore_sep_nhwc(x, y[:, :4].contiguous(), md["P_h"], md["P_w"], md["Q_h"], md["Q_w"], tables, K - 1, timesteps=use)


def test_sep_and_ancestral_chains_share_a_workspace(tiny, data):
    """a restore_sep chain and a plain ancestral chain on the same plan, workspace, state buffer, tables and t_start, run alternately,
    then restore_sep chains with another y and with a y of another size: each reproduces its own first result bit for bit"""
    from ddk import lib as L
    from ddk import ops
    from models.diffusion import blur
    m, _ = tiny
    ys, x_T = data
    tables, use = m._spaced_tables("20", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    nbytes = lib.ddk_sampler_restore_blur_workspace_bytes(plan.handle, 2, 16, 16, len(use) - 1)
    md = {n: m._sep_operands(blur.resize_matrix(16, n), blur.resize_matrix(16, n), 3e-2) for n in SCALES}       # the model's own cached operands
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    runs = {"a": (2, ops.nchw_to_nhwc(ys[2].to(DEV))), "b": (2, ops.nchw_to_nhwc((0.5 * ys[2]).to(DEV))), "c": (4, ops.nchw_to_nhwc(ys[4].to(DEV)))}

    def launch(what, a, tmap, stream):
        if what is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        n, y = runs[what]
        mats = [L.ptr(md[n][k]) for k in ("P_h", "P_w", "Q_h", "Q_w")]
        return lib.ddk_sampler_run_restore_sep(a, tmap, *mats, L.ptr(y), 16 // n, 16 // n, stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    with CC.workspace(plan, nbytes) as ws:
        first = {}
        for what in ("a", None, "a", "c", None, "b", "a", "c", None, "b"):
            got = sh.run(ws, what)
            if what not in first:
                first[what] = got
            assert torch.equal(got, first[what]), (what, float((got - first[what]).abs().max()))
        assert len({tuple(v.flatten()[:64].tolist()) for v in first.values()}) == 4
        # the library's own entry and the model's method are the same chain
        via_model = m.super_resolve(ys[2].to(DEV), 2, downsample="bicubic", respacing="20", x_T=x_T, seed=SEED)
        assert torch.equal(ops.nhwc_to_nchw(first["a"]), via_model)


def test_the_downsampled_model_refuses():
    from models import DownsampleDDPM, Unet
    from models.diffusion import blur
    cfg = dddpm_cfg(32, 32, 2)
    m = DownsampleDDPM(cfg, Unet(cfg), "cpu", 3)      # the refusal comes before any device work
    A = blur.resize_matrix(32, 4)
    with pytest.raises(ValueError, match="latent"):
        m.restore_separable(torch.zeros(1, 3, 8, 8), A, A)
    with pytest.raises(ValueError, match="downsample"):
        m.super_resolve(torch.zeros(1, 3, 8, 8), 4, downsample="bicubic")


# ---------------------------------------------------------------- the command lines
def test_upscale_cli_and_evaluator_with_bicubic(tmp_path):
    """upscale_model_samples.py and evaluate_restoration.py --task sr with synthetic weights on three 16 x 16 images, each in a fresh
    process, with --downsample bicubic and with the defaults: the files, their names, the reduced images and the JSON keys"""
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    for extra, name in ((["--downsample", "bicubic"], "clitest_sr2_bicubic_5"), ([], "clitest_sr2_5")):
        CC.run_script("upscale_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--scale", "2",
                      "--timestep_respacing", "5", "--batch_size", "2", "--seed", "3", "--out_dir", tmp_path, *extra, env=env)
        out, lowres = np.load(tmp_path / f"{name}.npy"), np.load(tmp_path / f"{name}_lowres.npy")
        assert out.shape == (3, 16, 16, 3) and out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
        assert lowres.shape == (3, 8, 8, 3) and lowres.dtype == np.uint8
        x = torch.from_numpy(imgs.astype(np.float64)).permute(0, 3, 1, 2) / 255 * 2 - 1
        A = torch.from_numpy(ZR.matrix(16, 2, "bicubic" if extra else "mean"))
        want = ((BR.apply(x, A, A) + 1) * 127.5).round().clamp(0, 255).permute(0, 2, 3, 1).numpy()
        assert np.abs(lowres.astype(np.float64) - want).max() <= 1      # a rounding tie may fall either way in fp32
    assert sorted(p.name for p in tmp_path.glob("clitest_*")) == ["clitest_sr2_5.npy", "clitest_sr2_5_lowres.npy", "clitest_sr2_bicubic_5.npy",
                                                                 "clitest_sr2_bicubic_5_lowres.npy"]
    base = ["evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "sr", "--scale", "2",
            "--timestep_respacing", "5", "--batch_size", "2", "--json", tmp_path / "score.json"]
    keys = {"checkpoint", "synthetic", "model", "task", "images", "n_images", "batch_size", "seed", "method", "unet_forwards", "respacing",
            "scale", "ddim", "eta"}
    for extra in (["--downsample", "bicubic"], []):
        CC.run_script(*base, *extra, env=env)
        res = json.loads((tmp_path / "score.json").read_text())
        s, mt = res["settings"], res["metrics"]
        assert set(s) == (keys | {"downsample"} if extra else keys)
        assert (s["task"], s["method"], s["scale"], s["unet_forwards"], s["n_images"]) == ("sr", "ddnm", 2, 5, 3)
        assert set(mt) == {"restored", "replicate", "bicubic", "consistency", "consistency_u8"}
        for name in ("restored", "replicate", "bicubic"):
            assert set(mt[name]) == {"psnr", "ssim"} and mt[name]["psnr"]["n"] == 3 and np.isfinite(mt[name]["psnr"]["mean"])
        # the last step returns x0' = (x0 - P x0 P^T) + Yp and A P = A (block means likewise): |A(x_out) - y| is fp32 rounding,
        # (16 + 16 + 16) u (|P| |x0| |P|^T + |x0| + |Yp|) <= 48 u 6 spread by row sums <= 1.7, times 127.5: 4e-3 of a uint8 level
        assert mt["consistency"]["max"] < 0.01
        print(f"sr evaluator {extra} (synthetic weights): {json.dumps(mt)}")
