"""DDNM super-resolution on the GPU (DDPM.super_resolve, DownsampleDDPM.super_resolve, ddk_sampler_run_restore,
p_update_restore_kernel and final_tail_kernel<.., StepKind::Restore>) against tests/restore_ref.py, the method restated around
oracle/unet_ref with oracle/philox_ref draws in NHWC order.

The tiny DDPM (unet_chan 32, 3x16x16) has no Winograd final conv, so its steps end in the unfused p_update_restore_kernel.  The cfg4
latent at B = 32 ends in the fused tail for n = 2 and 4.  Bars: the lone op bit for bit (the order of the fp32 operations is
pinned); chains 1e-4 abs against the restatement with the same argmax and 1e-5 between the Python loop and the native sampler, as
for the spaced and RePaint chains; the block means of the output within 8 n^2 2^-24 of y (derived worst case (n^2 + 4) 2^-24)."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import restore_ref as RR
from helpers import dddpm_cfg, ddpm_cfg, det_load, to_nhwc, unet_cfg
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SEED = 613
KINDS = [dict(), dict(ddim=True, eta=0.0)]
IDS = ["ancestral", "ddim"]


def _bar(n):
    return 8 * n * n * 2.0 ** -24


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    return CC.pooled_y(SHAPE, 4, "restore.x"), syn.synthetic_normal(SHAPE, "restore.xT")


# ---------------------------------------------------------------- the lone op, bit for bit
@pytest.mark.parametrize("n,c,h,w", [(2, 3, 16, 16), (2, 4, 32, 32), (4, 3, 16, 16), (4, 4, 32, 32), (8, 3, 16, 16), (8, 4, 32, 32),
                                     (8, 3, 32, 24), (4, 4, 8, 64), (2, 4, 4, 128), (2, 3, 6, 10), (4, 1, 4, 4)])
def test_lone_op_equals_restatement_bit_for_bit(n, c, h, w):
    """ops.p_sample_update_restore_ given eps_hat against restore_ref.step on the same inputs.  The draws are the device's own
    (ddk_randn: the same Philox call and keying), first checked against oracle/philox_ref, so the comparison of the update is exact;
    row 0 has no draw.  Shapes with W n > 128 and 3-channel maps included."""
    from ddk import ops
    g = torch.Generator().manual_seed(17 * n + c + h)
    B = 3
    shape = (B, c, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    y = torch.rand(B, c, h // n, w // n, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])
    tab = CC.hand_tables(g)
    seed, stream = 24680, 5
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    want = RR.step(x, e, y, n, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], sg, z)
    xs = to_nhwc(x).to(DEV)
    ops.p_sample_update_restore_(xs, to_nhwc(e).to(DEV), to_nhwc(y).to(DEV), n, t.to(DEV), **{k: v.to(DEV) for k, v in tab.items()},
                                 seed=seed, stream_id=stream)
    got = xs.cpu().permute(0, 3, 1, 2)
    diff = float((got - want).abs().max())
    print(f"lone op n={n} c={c} {h}x{w}: max abs difference {diff:.3g}")
    assert torch.equal(got, want), diff
    # row 0 returns x0' itself: its block means are y
    assert float((RR.pool(got[0:1].double(), n) - y[0:1].double()).abs().max()) <= _bar(n)


def test_lone_op_rejects_bad_arguments():
    from ddk import lib as L
    from ddk import ops
    x = torch.zeros(1, 8, 8, 3, device=DEV)
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    with pytest.raises(L.DDKError):
        ops.p_sample_update_restore_(x, x.clone(), torch.zeros(1, 2, 2, 3, device=DEV), 3, t, **tab)
    with pytest.raises(L.DDKError):
        ops.p_sample_update_restore_(x, x.clone(), torch.zeros(1, 0, 0, 3, device=DEV), 16, t, **tab)
    with pytest.raises(L.DDKError):
        ops.p_sample_update_restore_(x, x.clone(), torch.zeros(1, 4, 4, 3, device=DEV), 4, t, **tab)


# ---------------------------------------------------------------- the tiny DDPM, "20" steps
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, kw):
    m, eps = tiny
    y, x_T = data
    got = m.super_resolve(y.to(DEV), 4, respacing="20", x_T=x_T, seed=SEED, **kw).cpu()
    want = RR.Restore(BETAS, "20").run(eps, x_T, y, 4, SEED, **kw)
    err = float((got - want).abs().max())
    print(f"DDNM x4 tiny DDPM, 20 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    assert torch.equal(CC.argmax(got), CC.argmax(want))


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_bit_for_bit(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    graphed = m.super_resolve(y.to(DEV), 4, respacing="20", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "use_graph", False):
        eager = m.super_resolve(y.to(DEV), 4, respacing="20", x_T=x_T, seed=SEED, **kw)
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_python_loop_equals_native(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    native = m.super_resolve(y.to(DEV), 4, respacing="20", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "native_sampler", False):
        loop = m.super_resolve(y.to(DEV), 4, respacing="20", x_T=x_T, seed=SEED, **kw)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, DDNM 20 steps {kw}: {err:.3g}")
    assert err < 1e-5


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_output_block_means_equal_y(tiny, n, kw):
    m, _ = tiny
    y = CC.pooled_y(SHAPE, n, f"restore.cons.{n}")
    out = m.super_resolve(y.to(DEV), n, respacing="20", x_T=syn.synthetic_normal(SHAPE, "restore.xT"), seed=SEED + n, **kw).cpu()
    assert out.dtype == torch.float32
    err = float((RR.pool(out.double(), n) - y.double()).abs().max())
    print(f"consistency n={n} {kw}: block means off by {err:.3g} (bar {_bar(n):.3g})")
    assert err <= _bar(n), err
    detail = float((out - RR.replicate(y, n)).abs().max())
    print(f"  null-space content: max |out - replicate(y)| = {detail:.3g}")
    assert detail > 1e-2


# ---------------------------------------------------------------- cfg4, B = 32: the benchmark's shape and plan options
@pytest.fixture(scope="module")
def cfg4():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(128, 256, 3)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    return m


@pytest.mark.parametrize("n", [2, 4])
def test_cfg4_b32_fused_tail(cfg4, n):
    """"8" steps on the cfg4 latent at B = 32, default options (level chain, in-launch GroupNorm): the fused tail is taken, and
    its result equals the unfused tail's bit for bit, the Python loop's within 1e-5 and the restatement's within 1e-4"""
    from ddk import ops
    from models import DDPM
    m = cfg4
    plan = m._eps_model_nhwc().plan()
    before, cluster = ops.cluster_timeouts(), plan._cluster
    shape = (32, 8, 32, 32)
    assert plan.restore_tail_parts(32, 32, 32, n) == 8
    y = CC.pooled_y(shape, n, f"restore.cfg4.{n}")
    x_T = syn.synthetic_normal(shape, "restore.cfg4.xT")
    run = lambda: DDPM.super_resolve(m, y.to(DEV), n, respacing="8", x_T=x_T, seed=SEED)
    fused = run()
    plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 0)
    try:
        assert plan.restore_tail_parts(32, 32, 32, n) == 0
        unfused = run()
    finally:
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())
    with CC.toggled(m, "native_sampler", False):
        loop = run()
    err_loop = float((loop - fused).abs().max())
    torch.cuda.synchronize()
    err_means = float((RR.pool(fused.cpu().double(), n) - y.double()).abs().max())
    print(f"cfg4 B=32 DDNM x{n}: loop vs native {err_loop:.3g}, block means off by {err_means:.3g}")
    assert torch.isfinite(fused).all() and err_loop < 1e-5, err_loop
    assert err_means <= _bar(n)
    assert ops.cluster_timeouts() == before and plan._cluster == cluster
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    eps = lambda x, t: U.unet_forward(sd, unet_cfg(128, 8), x, t, pre="latent_model.")
    if n == 2:      # one restatement run at this size is enough (the oracle UNet at B = 32 is slow)
        want = RR.Restore(BETAS, "8").run(eps, x_T, y, n, SEED)
        err = float((fused.cpu() - want).abs().max())
        print(f"cfg4 B=32 DDNM x{n} vs restatement: {err:.3g}")
        assert err < TOL, err


def test_cfg4_n8_takes_the_unfused_tail(cfg4):
    """W n = 256 > 128: the tile does not hold whole rows of blocks, so the step ends in p_update_restore_kernel"""
    from ddk import ops
    from models import DDPM
    m = cfg4
    plan = m._eps_model_nhwc().plan()
    before = ops.cluster_timeouts()
    assert plan.restore_tail_parts(4, 32, 32, 8) == 0
    shape = (4, 8, 32, 32)
    y = CC.pooled_y(shape, 8, "restore.cfg4.8")
    x_T = syn.synthetic_normal(shape, "restore.cfg4.xT8")
    run = lambda: DDPM.super_resolve(m, y.to(DEV), 8, respacing="8", x_T=x_T, seed=SEED)
    native = run()
    with CC.toggled(m, "native_sampler", False):
        loop = run()
    assert float((loop - native).abs().max()) < 1e-5
    assert float((RR.pool(native.cpu().double(), 8) - y.double()).abs().max()) <= _bar(8)
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- one workspace, two kinds of chain
def test_restore_and_ancestral_chains_share_a_workspace(tiny, data):
    """a restore chain then a plain ancestral chain on the same workspace, state buffer, tables and t_start, and the reverse
    order, then a restore chain with another y: each equals its own single run on a fresh workspace bit for bit (the kind and n are
    in the graph key, y is staged by every call)"""
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    y, x_T = data
    tables, use = m._spaced_tables("20", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    nbytes = lib.ddk_sampler_restore_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes >= lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + 2 * 4 * 4 * 3 * 4
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    ys = {4: ops.nchw_to_nhwc(y.to(DEV)), 2: ops.nchw_to_nhwc(CC.pooled_y(SHAPE, 2, "restore.other").to(DEV)),
          -4: ops.nchw_to_nhwc(CC.pooled_y(SHAPE, 4, "restore.third").to(DEV))}

    def launch(what, a, tmap, stream):
        if what is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        return lib.ddk_sampler_run_restore(a, tmap, L.ptr(ys[what]), abs(what), stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    x, tmap = sh.x, sh.tmap
    single = {what: sh.alone(what) for what in (4, None, 2, -4)}
    assert not torch.equal(single[4], single[None]) and not torch.equal(single[4], single[-4])
    for order in ((4, None, -4, 2, None), (None, 4, None, 2, -4, 4)):
        sh.interleaved(order, single)
    # injected noise is rejected
    a = CC.sampler_args(plan, x, tables, K - 1, CC.fresh_workspace(nbytes), nbytes, seed=SEED, noise=torch.zeros((K, *x.shape), device=DEV))
    assert lib.ddk_sampler_run_restore(a, tmap, L.ptr(ys[4]), 4, L.stream()) == -1 and "noise" in L.last_error()
    a.noise = None
    assert lib.ddk_sampler_run_restore(a, tmap, L.ptr(ys[4]), 3, L.stream()) == -1 and "n must be" in L.last_error()


# ---------------------------------------------------------------- dDDPM and the command line
def test_dddpm_super_resolve_holds_the_latent_constraint():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    y = CC.pooled_y((2, 3, 32, 32), 8, "restore.dd.x")
    z_T = syn.synthetic_normal((2, 8, 8, 8), "restore.dd.zT")
    x_out, z = m.super_resolve(y.to(DEV), 8, respacing="10", x_T=z_T, seed=SEED)
    assert x_out.shape == (2, 3, 32, 32) and z.shape == (2, 8, 8, 8)
    with torch.no_grad():
        z_ref = m.rescaled_downsample(RR.replicate(y, 8).to(DEV))
        y_lat = torch.nn.functional.avg_pool2d(z_ref, 2).cpu()
        assert torch.equal(x_out, m.rescaled_upsample(z))
    err = float((RR.pool(z.cpu().double(), 2) - y_lat.double()).abs().max())
    print(f"dDDPM x8 (latent n = 2): latent block means off by {err:.3g} (bar {_bar(2):.3g}); "
          f"pixels: |pool(x_out) - y| max {float((RR.pool(x_out.cpu(), 8) - y).abs().max()):.3g} (not guaranteed)")
    assert err <= _bar(2), err


def test_upscale_cli(tmp_path):
    cfg_path, _, _, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)      # imgs.npy: the full-size images, from the generator's first draw
    rng = np.random.default_rng(0)
    rng.random((3, 16, 16, 3))
    low = (rng.random((3, 4, 4, 3)) * 255).astype(np.uint8)             # its second draw
    np.save(tmp_path / "low.npy", low)
    for images, extra, spec in (("low.npy", [], "10"), ("imgs.npy", ["--use_ddim", "--eta", "0.5"], "10_ddim_eta0.5")):
        CC.run_script("upscale_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", tmp_path / images, "--scale",
                      "4", "--timestep_respacing", "10", "--batch_size", "2", "--seed", "3", "--out_dir", tmp_path, *extra, env=env)
        out = np.load(tmp_path / f"clitest_sr4_{spec}.npy")
        lowres = np.load(tmp_path / f"clitest_sr4_{spec}_lowres.npy")
        assert out.shape == (3, 16, 16, 3) and out.dtype == np.float32
        assert lowres.shape == (3, 4, 4, 3) and lowres.dtype == np.uint8
        assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
        if images == "low.npy":
            assert np.array_equal(lowres, low)
