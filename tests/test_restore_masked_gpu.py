"""DDNM with a mask on the GPU (DDPM.restore, DownsampleDDPM.restore, ddk_sampler_run_restore_masked, p_update_restore_kernel<RestoreMasked>,
p_update_restore_point_kernel<RestoreMasked> and final_tail_kernel<.., StepKind::RestoreMasked>) against tests/restore_masked_ref.py, the method
restated around oracle/unet_ref with oracle/philox_ref draws in NHWC order.

The tiny DDPM (unet_chan 32, 3x16x16) has no Winograd final conv, so its steps end in the unfused kernels; a 128-channel UNet on
8x32x32 latents at B = 16 ends in the fused tail for n = 1, 2 and 4 and not for n = 8 (the smallest such shape: the final conv leaves
its GroupNorm partials, which the fused tail needs, only unsplit, i.e. from 16 images of 128 channels on; 32 channels at B = 2 never do).  Bars: the lone op bit for bit (the order of the fp32
operations is pinned, the added operation is a select); chains 1e-4 abs against the restatement and 1e-5 between the Python loop
and the native sampler, as for the unmasked chain; measured pixels of the output equal y exactly at n = 1, measured block means
within 8 n^2 2^-24 at n >= 2; fused and unfused tails, graph and eager, masked-with-ones and unmasked: the same bits."""
import json

import numpy as np
import pytest
import torch

import chain_cases as CC
import restore_masked_ref as RM
import restore_ref as RR
from helpers import dddpm_cfg, ddpm_cfg, det_load, to_nhwc
from oracle import diffusion_ref as D
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


def _means_err(out, y, mk, n):
    """max over the measured blocks of |block mean of out - y| (n = 1: of |out - y|)"""
    return float((RR.pool(out.double(), n) - y.double())[CC.sel(mk, y)].abs().max())


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    """y and mask per block, one start state: computed once, never changed"""
    x_T = syn.synthetic_normal(SHAPE, "restore_masked.xT")
    ys = {n: CC.pooled_y(SHAPE, n, f"restore_masked.x{n}") for n in (1, 2, 4, 8)}
    mks = {n: CC.mask("checker", 2, 16 // n, 16 // n) for n in (1, 2, 4, 8)}
    return ys, mks, x_T


@pytest.fixture(scope="module")
def native(tiny, data):
    """the native chain's results on the tiny model, shared by the tests that compare against them"""
    m, _ = tiny
    ys, mks, x_T = data
    return {(n, i): m.restore(ys[n].to(DEV), mks[n], n, respacing="20", x_T=x_T, seed=SEED, **kw).cpu()
            for n in (1, 2) for i, kw in zip(IDS, KINDS)}


# ---------------------------------------------------------------- the lone op, bit for bit
@pytest.mark.parametrize("hw", [(16, 16), (8, 32)], ids=["16x16", "8x32"])
@pytest.mark.parametrize("c", [3, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_lone_op_equals_restatement_bit_for_bit(n, c, hw):
    """ops.p_sample_update_restore_masked_ given eps_hat against restore_masked_ref.step on the same inputs, for the three masks.  The
    draws are the device's own (ddk_randn: the same Philox call and keying), first checked against oracle/philox_ref, so the
    comparison of the update is exact; row 0 has no draw.  y is NaN wherever the mask is 0: the result must not see it."""
    from ddk import ops
    h, w = hw
    g = torch.Generator().manual_seed(17 * n + c + h)
    B = 3
    shape = (B, c, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    y0 = torch.rand(B, c, h // n, w // n, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])
    tab = CC.hand_tables(g)
    seed, stream = 24680, 5
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    dtab = {k: v.to(DEV) for k, v in tab.items()}
    for kind in ("checker", "one_measured", "one_hidden"):
        mk = CC.mask(kind, B, h // n, w // n)
        y = torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
        want = RM.step(x, e, y, mk, n, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], sg, z)
        xs = to_nhwc(x).to(DEV)
        ops.p_sample_update_restore_masked_(xs, to_nhwc(e).to(DEV), to_nhwc(y).to(DEV), mk.to(DEV), n, t.to(DEV), **dtab, seed=seed,
                                            stream_id=stream)
        got = xs.cpu().permute(0, 3, 1, 2)
        assert torch.isfinite(got).all(), kind
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))
        # row 0 returns x0' itself: measured pixels are y (n = 1: exactly), measured block means are y
        if n == 1:
            assert torch.equal(got[0:1][CC.sel(mk[0:1], y[0:1])], y[0:1][CC.sel(mk[0:1], y[0:1])])
        else:
            assert _means_err(got[0:1], y[0:1], mk[0:1], n) <= _bar(n)
    if n > 1:   # no mask: the unmasked op, bit for bit
        a, b = to_nhwc(x).to(DEV), to_nhwc(x).to(DEV)
        ops.p_sample_update_restore_masked_(a, to_nhwc(e).to(DEV), to_nhwc(y0).to(DEV), None, n, t.to(DEV), **dtab, seed=seed, stream_id=stream)
        ops.p_sample_update_restore_(b, to_nhwc(e).to(DEV), to_nhwc(y0).to(DEV), n, t.to(DEV), **dtab, seed=seed, stream_id=stream)
        assert torch.equal(a, b)
        ops.p_sample_update_restore_masked_(b.copy_(to_nhwc(x)), to_nhwc(e).to(DEV), to_nhwc(y0).to(DEV), torch.ones(B, h // n, w // n, device=DEV), n,
                                            t.to(DEV), **dtab, seed=seed, stream_id=stream)
        assert torch.equal(a, b)


def test_lone_op_rejects_bad_arguments():
    from ddk import lib as L
    from ddk import ops
    x = torch.zeros(1, 8, 8, 3, device=DEV)
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    lib = L.load()
    with pytest.raises(L.DDKError):                                                        # n = 3
        ops.p_sample_update_restore_masked_(x, x.clone(), torch.zeros(1, 2, 2, 3, device=DEV), torch.ones(1, 2, 2, device=DEV), 3, t, **tab)
    with pytest.raises(L.DDKError):                                                        # n = 1 without a mask
        ops.p_sample_update_restore_masked_(x, x.clone(), x.clone(), None, 1, t, **tab)
    x6 = torch.zeros(1, 6, 8, 4, device=DEV)
    with pytest.raises(L.DDKError):                                                        # H % n != 0
        ops.p_sample_update_restore_masked_(x6, x6.clone(), torch.zeros(1, 1, 2, 4, device=DEV), torch.ones(1, 1, 2, device=DEV), 4, t, **tab)
    # misaligned x / y (4 bytes into a buffer): rejected before any launch
    buf, y, mk = torch.zeros(8 * 8 * 4 + 4, device=DEV), torch.zeros(8 * 8 * 4 + 4, device=DEV), torch.ones(1, 8, 8, device=DEV)
    args = lambda xp, yp: (xp, buf.data_ptr(), yp, mk.data_ptr(), 1, t.data_ptr(), *(tab[k].data_ptr() for k in tab), 1, 8, 8, 4, 0, 0,
                           L.stream())
    assert lib.ddk_p_sample_update_restore_masked(*args(buf.data_ptr() + 4, y.data_ptr())) == -1
    assert lib.ddk_p_sample_update_restore_masked(*args(y.data_ptr(), buf.data_ptr() + 4)) == -1 and "align" in L.last_error()
    assert lib.ddk_p_sample_update_restore_masked(*args(y.data_ptr(), buf.data_ptr() + 16)) == 0, L.last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the tiny DDPM, "20" steps
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, native, kw, n):
    _, eps = tiny
    ys, mks, x_T = data
    got = native[n, IDS[KINDS.index(kw)]]
    want = RM.RestoreMasked(BETAS, "20").run(eps, x_T, ys[n], mks[n], n, SEED, **kw)
    err = float((got - want).abs().max())
    print(f"masked DDNM n={n} tiny DDPM, 20 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_and_python_loop_is_close(tiny, data, native, kw, n):
    m, _ = tiny
    ys, mks, x_T = data
    graphed = native[n, IDS[KINDS.index(kw)]]
    run = lambda: m.restore(ys[n].to(DEV), mks[n], n, respacing="20", x_T=x_T, seed=SEED, **kw).cpu()
    with CC.toggled(m, "use_graph", False):
        eager = run()
    assert torch.equal(graphed, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = run()
    err = float((loop - graphed).abs().max())
    print(f"Python loop vs native, masked DDNM n={n} 20 steps {kw}: {err:.3g}")
    assert err < 1e-5


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_constraint_and_agreement_with_the_unmasked_entry(tiny, data, native, kw):
    """n = 1: measured pixels of the output are y exactly, NaN under the zero mask changes nothing; n >= 2: measured block means
    within 8 n^2 2^-24, and a null mask and an all-ones mask equal sample_restore_nhwc (super_resolve) bit for bit"""
    m, _ = tiny
    ys, mks, x_T = data
    i = IDS[KINDS.index(kw)]
    out = native[1, i]
    s1 = CC.sel(mks[1], ys[1])
    assert torch.equal(out[s1], ys[1][s1]) and float((out - ys[1])[~s1].abs().max()) > 1e-2
    y_nan = torch.where(s1, ys[1], torch.full_like(ys[1], float("nan"))).to(DEV)
    plan = m._eps_model_nhwc().plan()
    from ddk import ops
    tables, use = m._spaced_tables("20", kw.get("ddim", False), kw.get("eta", 0.0))
    x = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    plan.sample_restore_masked_nhwc(x, ops.nchw_to_nhwc(y_nan), mks[1].to(DEV), 1, tables, len(use) - 1, seed=SEED,
                                    stream_id=int(m.rng_stream_id), timesteps=use)
    assert torch.equal(ops.nhwc_to_nchw(x).cpu(), out)
    assert _means_err(native[2, i], ys[2], mks[2], 2) <= _bar(2)
    for n in (2, 4):
        want = m.super_resolve(ys[n].to(DEV), n, respacing="20", x_T=x_T, seed=SEED, **kw)
        assert torch.equal(m.restore(ys[n].to(DEV), None, n, respacing="20", x_T=x_T, seed=SEED, **kw), want)
        ones = m.restore(ys[n].to(DEV), torch.ones(16 // n, 16 // n), n, respacing="20", x_T=x_T, seed=SEED, **kw)
        assert torch.equal(ones, want)
        assert _means_err(ones.cpu(), ys[n], torch.ones(2, 16 // n, 16 // n), n) <= _bar(n)


# ---------------------------------------------------------------- the fused tail: 128 channels, 8x32x32 latents, B = 16
@pytest.fixture(scope="module")
def wide():
    from models import DDPM, Unet
    cfg = ddpm_cfg(128, 8, 32)
    m = det_load(DDPM(cfg, Unet(cfg), DEV, 8)).to(DEV).eval()       # an 8-channel "image": the cfg4 latent's shape without the codec
    return m


@pytest.mark.parametrize("n", [1, 2, 8])
def test_fused_tail_equals_unfused_bit_for_bit(wide, n):
    """ "6" steps: n = 1 and n = 2 end in final_tail_kernel<.., RestoreMasked>, n = 8 (W n = 256 > 128) in p_update_restore_kernel<RestoreMasked>
    whatever the option says; with DDK_OPT_RESTORE_FUSED_TAIL = 0 all end in the unfused kernels, with the same bits"""
    from ddk import ops
    m = wide
    plan = m._eps_model_nhwc().plan()
    before = ops.cluster_timeouts()
    B = 16
    shape = (B, 8, 32, 32)
    assert plan.restore_masked_tail_parts(B, 32, 32, n) == (0 if n == 8 else 8)
    assert plan.restore_masked_tail_parts(B, 32, 32, 1) > 0 and plan.restore_masked_tail_parts(B, 32, 32, 8) == 0
    y0 = CC.pooled_y(shape, n, f"restore_masked.wide.{n}")
    mk = CC.mask("checker", B, 32 // n, 32 // n)
    y = torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
    x_T = syn.synthetic_normal(shape, "restore_masked.wide.xT")
    run = lambda: m.restore(y.to(DEV), mk, n, respacing="6", ddim=True, eta=0.5, x_T=x_T, seed=SEED).cpu()
    fused = run()
    plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 0)
    try:
        assert plan.restore_masked_tail_parts(B, 32, 32, n) == 0
        unfused = run()
    finally:
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())
    if n == 1:
        assert torch.equal(fused[CC.sel(mk, y)], y[CC.sel(mk, y)])
    else:
        assert _means_err(fused, y, mk, n) <= _bar(n)
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- one workspace, three kinds of chain, two masks
def test_chains_share_a_workspace_and_masks_share_a_graph(tiny, data):
    """a masked chain, an unmasked restore chain and a plain ancestral chain on the same workspace, state buffer, tables and t_start,
    in two orders, and two different masks back to back: each equals its own single run on a fresh workspace bit for bit (the kind
    and n are in the graph key, y and the mask are staged by every call)"""
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    ys, mks, x_T = data
    tables, use = m._spaced_tables("20", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    before = ops.cluster_timeouts()
    K = len(use)
    nbytes = lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    assert nbytes >= lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + (2 * 16 * 16 * 3 + 2 * 16 * 16) * 4
    assert nbytes >= lib.ddk_sampler_restore_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    yd = {n: ops.nchw_to_nhwc(ys[n].to(DEV)) for n in (1, 2)}
    md = {"m1": mks[1].to(DEV), "m1b": (1 - mks[1]).to(DEV), "m2": mks[2].to(DEV)}
    jobs = {"m1": (1, "m1"), "m1b": (1, "m1b"), "m2": (2, "m2"), "r2": (2, None), "anc": None}

    def launch(what, a, tmap, stream):
        if jobs[what] is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        if what == "r2":
            return lib.ddk_sampler_run_restore(a, tmap, L.ptr(yd[2]), 2, stream)
        n, mk = jobs[what]
        return lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[n]), L.ptr(md[mk]), n, stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    x, tmap = sh.x, sh.tmap
    single = {what: sh.alone(what) for what in jobs}
    assert not torch.equal(single["m1"], single["m1b"]) and not torch.equal(single["m2"], single["r2"])
    assert not torch.equal(single["m1"], single["anc"])
    for order in (("m1", "r2", "anc", "m1b", "m2", "m1"), ("anc", "m2", "r2", "m1b", "m1", "anc")):
        sh.interleaved(order, single)
    # the measured pixels of the two masks' results are their own
    for what in ("m1", "m1b"):
        out = ops.nhwc_to_nchw(single[what]).cpu()
        s = CC.sel(md[what].cpu(), ys[1])
        assert torch.equal(out[s], ys[1][s])
    # a null mask on this entry is the unmasked chain; n = 1 without a mask, injected noise and a bad n are rejected
    with CC.workspace(plan, nbytes) as ws:
        a = CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED)
        x.copy_(x0)                                       # eager (the legacy stream cannot be captured): the same bits as the graph
        assert lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[2]), None, 2, L.stream()) == 0, L.last_error()
        torch.cuda.synchronize()
        assert torch.equal(x, single["r2"])
        assert lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[1]), None, 1, L.stream()) == -1 and "mask" in L.last_error()
        assert lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[1]), L.ptr(md["m1"]), 3, L.stream()) == -1
        noise = torch.zeros((K, *x.shape), device=DEV)
        a.noise = L.ptr(noise)
        assert lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[1]), L.ptr(md["m1"]), 1, L.stream()) == -1 and "noise" in L.last_error()
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- dDDPM
def test_dddpm_restore_holds_the_latent_constraint_and_pastes():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    z_T = syn.synthetic_normal((2, 8, 8, 8), "restore_masked.dd.zT")
    # scale 1: inpainting in the latent, the left half and one far block measured
    img = syn.synthetic_normal((2, 3, 32, 32), "restore_masked.dd.x").clamp(-1, 1)
    mk = torch.zeros(32, 32)
    mk[:, :14] = 1
    mk[8:12, 24:28] = 1
    x_out, z = m.restore(img.to(DEV), mk, 1, respacing="10", ddim=True, x_T=z_T, seed=SEED)
    assert x_out.shape == (2, 3, 32, 32) and z.shape == (2, 8, 8, 8) and torch.isfinite(x_out).all()
    sel = (mk != 0).expand(2, 3, 32, 32)
    assert torch.equal(x_out.cpu()[sel], img[sel])                                    # paste
    with torch.no_grad():
        z_ref = m.rescaled_downsample(torch.where(sel, img, torch.zeros_like(img)).to(DEV)).cpu()
    m_lat = -torch.nn.functional.max_pool2d(-mk[None, None], 4)[0, 0]
    assert m_lat.sum() == 8 * 3 + 1
    s_lat = (m_lat != 0).expand(2, 8, 8, 8)
    assert torch.equal(z.cpu()[s_lat], z_ref[s_lat])                                  # the constraint, held in the latent
    raw, _ = m.restore(img.to(DEV), mk, 1, respacing="10", ddim=True, x_T=z_T, seed=SEED, paste=False)
    assert not torch.equal(raw.cpu()[sel], img[sel]) and torch.equal(raw.cpu()[~sel], x_out.cpu()[~sel])
    # scale 8: a 4 x 4 low-resolution image with holes, latent block 2
    y = CC.pooled_y((2, 3, 32, 32), 8, "restore_masked.dd.y")
    mk8 = CC.mask("checker", 2, 4, 4)
    x8, z8 = m.restore(y.to(DEV), mk8, 8, respacing="10", x_T=z_T, seed=SEED)
    with torch.no_grad():
        zr = m.rescaled_downsample(RR.replicate(torch.where(CC.sel(mk8, y), y, torch.zeros_like(y)), 8).to(DEV))
        y_lat = torch.nn.functional.avg_pool2d(zr, 2).cpu()
        assert torch.equal(x8, m.rescaled_upsample(z8))
    err = _means_err(z8.cpu(), y_lat, mk8, 2)
    print(f"dDDPM x8 with holes (latent n = 2): measured latent block means off by {err:.3g} (bar {_bar(2):.3g})")
    assert err <= _bar(2), err


# ---------------------------------------------------------------- the command line (a fresh child process each)
def test_inpaint_cli_with_ddnm(tmp_path):
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    base = ["inpaint_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--mask", "left",
            "--timestep_respacing", "10", "--batch_size", "2", "--seed", "3", "--out_dir", tmp_path, "--method", "ddnm"]
    CC.run_script(*base, "--use_ddim", "--eta", "0.5", env=env)
    out = np.load(tmp_path / "clitest_inpaint_left_10_ddnm_ddim_eta0.5.npy")
    masked = np.load(tmp_path / "clitest_inpaint_left_10_ddnm_ddim_eta0.5_masked.npy")
    assert out.shape == (3, 16, 16, 3) and out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert np.abs(out[:, :, 8:] - imgs[:, :, 8:]).max() < 1e-3             # the known half comes back
    assert np.abs(out[:, :, :8] - imgs[:, :, :8]).max() > 1 and (masked[:, :, :8] == 0).all()
    r = CC.run_script(*base, "--jump_length", "5", env=env, check=False)
    assert r.returncode != 0 and "jump" in r.stderr


def test_evaluate_cli_with_ddnm(tmp_path):
    cfg_path, images_path, _, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    np.save(tmp_path / "ones.npy", np.ones((16, 16), dtype=np.float32))
    CC.run_script("evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "inpaint", "--method", "ddnm",
                  "--use_ddim", "--mask", tmp_path / "ones.npy", "--timestep_respacing", "10", "--batch_size", "2", "--seed", "9", "--json",
                  tmp_path / "out.json", env=env)
    out = json.loads((tmp_path / "out.json").read_text())
    st, me = out["settings"], out["metrics"]
    assert (st["task"], st["method"], st["unet_forwards"], st["respacing"], st["ddim"], st["eta"]) == ("inpaint", "ddnm", 10, "10", True, 0.0)
    assert "jump_length" not in st
    # everything known: the restored images are the inputs
    assert me["restored"]["psnr"]["mean"] == float("inf") and me["restored"]["ssim"]["mean"] == 1.0


def test_scorer_methods_side_by_side_and_masked_super_resolution(tiny):
    """RePaint and DDNM on the same images and mask report their forwards per image; masked super-resolution scores the model and the
    baselines on the same holes, and its measured block means are consistent"""
    from utils import restoration_metrics as RMx
    m, _ = tiny
    imgs = (np.random.default_rng(1).random((3, 16, 16, 3)) * 255).astype(np.uint8)
    rp = RMx.evaluate_restoration(m, imgs, "inpaint", batch_size=3, seed=5, mask="center", respacing="5", jump_length=2, jump_n_sample=2)
    dn = RMx.evaluate_restoration(m, imgs, "inpaint", batch_size=3, seed=5, mask="center", method="ddnm", respacing="5", ddim=True)
    assert (rp["method"], rp["unet_forwards"]) == ("repaint", 9) and (dn["method"], dn["unet_forwards"]) == ("ddnm", 5)
    assert np.array_equal(rp["images"]["mean_fill"], dn["images"]["mean_fill"])
    known = RMx.make_mask("center", 3, 16, 16)[:, 0].numpy() != 0
    assert np.array_equal(dn["images"]["restored"][known], imgs[known])
    sr = RMx.evaluate_restoration(m, imgs, "sr", batch_size=3, seed=5, scale=2, sr_mask="half", respacing="5")
    assert sr["method"] == "ddnm" and sr["unet_forwards"] == 5 and set(sr["methods"]) == {"restored", "replicate", "bicubic"}
    assert float(sr["consistency"].max()) <= 8 * 4 * 2.0 ** -24 * 127.5
    plain = RMx.evaluate_restoration(m, imgs, "sr", batch_size=3, seed=5, scale=2, respacing="5")
    assert not np.array_equal(plain["images"]["replicate"], sr["images"]["replicate"])
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(m, imgs, "sr", method="repaint")
