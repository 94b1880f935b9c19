"""RePaint inpainting on the GPU (DDPM.inpaint, DownsampleDDPM.inpaint, ddk_sampler_run_inpaint, p_update_kernel<StepKind::Inpaint> and
final_tail_kernel's inpainting mode) against tests/repaint_ref.py, RePaint restated around oracle/unet_ref with oracle/philox_ref
draws in NHWC order.

The tiny DDPM (unet_chan 32, 3x16x16) has no Winograd final conv, so its ops end in the unfused p_update_kernel<StepKind::Inpaint>; its
"20", j = 5, r = 3 chain has 50 ops, so the one-step and the 16-step graphs both run.  The cfg4 latent at B = 32 ends in
final_tail_kernel's inpainting instantiation.  Bars as for the spaced chains: 1e-4 abs against the restatement, 1e-5 between the
Python loop and the native sampler."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import repaint_ref as RP
from helpers import dddpm_cfg, ddpm_cfg, det_load, unet_cfg
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SEED = 977
KW = dict(respacing="20", jump_length=5, jump_n_sample=3)


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    x = syn.synthetic_normal(SHAPE, "inpaint.x").clamp(-1, 1)
    mask = torch.ones(SHAPE[0], 1, 16, 16)
    mask[:, :, 4:12, 4:12] = 0
    mask[1, :, :, :3] = 0
    return x, mask, syn.synthetic_normal(SHAPE, "inpaint.xT")


def _check(got, want, tol=TOL):
    err = float((got.cpu() - want).abs().max())
    assert torch.isfinite(got).all()
    assert err < tol, err
    assert torch.equal(CC.argmax(got.cpu()), CC.argmax(want))
    return err


def _want(eps, x, mask, x_T, spec="20", j=5, r=3, seed=SEED):
    m = mask.expand_as(x)
    return RP.RePaint(BETAS, spec, j, r).run(eps, x_T, x, m, seed)


def test_tiny_vs_restatement(tiny, data):
    m, eps = tiny
    x, mask, x_T = data
    got = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    err = _check(got, _want(eps, x, mask, x_T))
    print(f"RePaint tiny DDPM, 50 ops: max abs error {err:.3g}")


def test_known_region_is_x_bit_for_bit(tiny, data):
    m, _ = tiny
    x, mask, x_T = data
    got = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW).cpu()
    known = mask.expand_as(x) != 0
    assert torch.equal(got[known], x[known])
    assert float((got[~known] - x[~known]).abs().max()) > 1e-2


def test_graph_equals_eager_bit_for_bit(tiny, data):
    m, _ = tiny
    x, mask, x_T = data
    graphed = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    with CC.toggled(m, "use_graph", False):
        eager = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    assert torch.equal(graphed, eager)


def test_python_loop_equals_native(tiny, data):
    m, _ = tiny
    x, mask, x_T = data
    native = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    with CC.toggled(m, "native_sampler", False):
        loop = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, RePaint 50 ops: {err:.3g}")
    assert err < 1e-5


def test_hidden_pixels_of_x_are_never_read(tiny, data):
    m, _ = tiny
    x, mask, x_T = data
    hidden = mask.expand_as(x) == 0
    x2 = x.clone()
    x2[hidden] = -x2[hidden] + 0.5
    a = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    b = m.inpaint(x2.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    assert torch.equal(a, b)


def test_two_images_on_one_workspace_replay_one_graph(tiny, data):
    """two calls with different images and masks of one shape: the second replays the first call's cached graph (same
    workspace and state buffers; known / mask are copied into the workspace), and both match the restatement"""
    m, eps = tiny
    x, mask, x_T = data
    xb = syn.synthetic_normal(SHAPE, "inpaint.x.other").clamp(-1, 1)
    maskb = torch.ones(SHAPE[0], 1, 16, 16)
    maskb[:, :, :, 8:] = 0
    plan = m._eps_model_nhwc().plan()
    got_a = m.inpaint(x.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, **KW)
    ws_before = [k for k in plan._ws if k[0] == "sin"]
    got_b = m.inpaint(xb.to(DEV), maskb.to(DEV), x_T=x_T, seed=SEED + 1, **KW)
    assert [k for k in plan._ws if k[0] == "sin"] == ws_before
    _check(got_a, _want(eps, x, mask, x_T))
    err = _check(got_b, _want(eps, xb, maskb, x_T, seed=SEED + 1))
    print(f"second image on the cached graph: {err:.3g}")


def test_update_kernel_matches_torch_expression():
    """ops.p_sample_update_inpaint_ against the fp32 torch expression with philox_ref draws, rows with and without a jump and
    row 0 (tau = 0: the known value exactly)"""
    from ddk import ops
    from oracle import philox_ref as PR
    g = torch.Generator().manual_seed(5)
    B, per = 3, 4 * 97
    x = (2 * torch.randn(B, per, generator=g))
    e = torch.randn(B, per, generator=g)
    kn = torch.rand(B, per, generator=g) * 2 - 1
    mk = (torch.rand(B, per, generator=g) > 0.5).float()
    t = torch.tensor([0, 7, 3])
    tab = {k: torch.rand(8, generator=g) * s for k, s in
           (("c_recip", 3.0), ("c_recipm1", 2.0), ("c1", 1.0), ("c2", 1.0), ("sigma", 0.5), ("ka", 1.0), ("kb", 1.0), ("ja", 1.0))}
    tab["jb"] = torch.tensor([0.0, 0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.7])
    tab["ka"][0], tab["kb"][0] = 1.0, 0.0
    seed, stream = 12345, 3
    z = {s: torch.from_numpy(np.stack([PR.philox_normal(B * per, seed, int(tb), s).reshape(B, per)[b] for b, tb in enumerate(t)]))
         for s in (stream, stream | (1 << 30), stream | (1 << 29))}
    col = lambda k: tab[k][t].unsqueeze(1)
    x0 = (col("c_recip") * x - col("c_recipm1") * e).clamp(-1, 1)
    x_unk = (col("c1") * x0 + col("c2") * x) + (t > 0).float().unsqueeze(1) * col("sigma") * z[stream]
    x_kn = col("ka") * kn + col("kb") * z[stream | (1 << 30)]
    want = torch.where(mk != 0, x_kn, x_unk)
    want = torch.where(col("jb") != 0, col("ja") * want + col("jb") * z[stream | (1 << 29)], want)
    xs = x.to(DEV)
    ops.p_sample_update_inpaint_(xs, e.to(DEV), kn.to(DEV), mk.to(DEV), t.to(DEV), **{k: v.to(DEV) for k, v in tab.items()},
                                 seed=seed, stream_id=stream)
    got = xs.cpu()
    err = float((got - want).abs().max())
    assert err < 1e-5, err
    assert torch.equal(got[0][mk[0] != 0], kn[0][mk[0] != 0])


def test_library_rejects_bad_arguments(tiny, data):
    import ctypes as C
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    tables, use = m._inpaint_tables("20", 5, 3)
    plan = m._eps_model_nhwc().plan()
    x = ops.nchw_to_nhwc(data[2].to(DEV).contiguous())
    known = torch.zeros_like(x)
    n = len(use)
    nbytes = plan._lib.ddk_sampler_inpaint_workspace_bytes(plan.handle, 2, 16, 16, n)
    assert nbytes > plan._lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, n - 1)
    ws = torch.empty(nbytes // 4, device=DEV)

    def run(tmap, noise=None, stream_id=0):
        a = CC.sampler_args(plan, x, tables, n - 1, ws, nbytes, seed=0, stream_id=stream_id, noise=noise)
        ip = L.InpaintArgs((C.c_int64 * n)(*tmap), L.ptr(known), L.ptr(known), L.ptr(tables["ka"]), L.ptr(tables["kb"]),
                           L.ptr(tables["ja"]), L.ptr(tables["jb"]))
        return plan._lib.ddk_sampler_run_inpaint(C.byref(a), C.byref(ip), L.stream())

    assert run(use, noise=torch.zeros((n, *x.shape), device=DEV)) == -1 and "noise" in L.last_error()
    assert run(use, stream_id=1 << 29) == -1 and "stream_id" in L.last_error()
    assert run([5] + list(use[1:])) == -1 and "timestep_map" in L.last_error()
    assert run(list(use[:-1]) + [0]) == -1 and "timestep_map" in L.last_error()


# ---------------------------------------------------------------- cfg4, B = 32: the benchmark's shape and plan options
def test_cfg4_b32_fused_tail():
    """"8", j = 2, r = 2 (14 ops) on the cfg4 latent at B = 32, default options (fused tail, level chain, in-launch GroupNorm)"""
    from ddk import ops
    from models import DDPM, DownsampleDDPM, Unet
    cfg = dddpm_cfg(128, 256, 3)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    eps = lambda x, t: U.unet_forward(sd, unet_cfg(128, 8), x, t, pre="latent_model.")
    plan = m._eps_model_nhwc().plan()
    before, cluster = ops.cluster_timeouts(), plan._cluster
    shape = (32, 8, 32, 32)
    z0 = syn.synthetic_normal(shape, "inpaint.cfg4.z").clamp(-1, 1)
    mask = torch.ones(32, 1, 32, 32)
    mask[:, :, 8:24, 8:24] = 0
    x_T = syn.synthetic_normal(shape, "inpaint.cfg4.xT")
    got = DDPM.inpaint(m, z0.to(DEV), mask.to(DEV), x_T=x_T, seed=SEED, respacing="8", jump_length=2, jump_n_sample=2)
    want = RP.RePaint(BETAS, "8", 2, 2).run(eps, x_T, z0, mask.expand(shape), SEED)
    err = float((got.cpu() - want).abs().max())
    torch.cuda.synchronize()
    print(f"cfg4 B=32 RePaint 14 ops: {err:.3g}")
    assert torch.isfinite(got).all() and err < TOL, err
    assert ops.cluster_timeouts() == before and plan._cluster == cluster


# ---------------------------------------------------------------- dDDPM and the command line
def test_dddpm_inpaint_hidden_pixels_never_read():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    x = syn.synthetic_normal((2, 3, 32, 32), "inpaint.dd.x").clamp(-1, 1)
    mask = torch.ones(2, 1, 32, 32)
    mask[:, :, 6:26, 10:22] = 0
    x2 = x.clone()
    x2[mask.expand_as(x) == 0] = 0.9
    z_T = syn.synthetic_normal((2, 8, 8, 8), "inpaint.dd.zT")
    kw = dict(respacing="10", jump_length=3, jump_n_sample=2, x_T=z_T, seed=SEED)
    xa, za = m.inpaint(x.to(DEV), mask.to(DEV), **kw)
    xb, zb = m.inpaint(x2.to(DEV), mask.to(DEV), **kw)
    assert xa.shape == (2, 3, 32, 32) and za.shape == (2, 8, 8, 8)
    assert torch.equal(xa, xb) and torch.equal(za, zb)
    known = mask.expand_as(x) != 0
    assert torch.equal(xa.cpu()[known], x[known])
    raw, _ = m.inpaint(x.to(DEV), mask.to(DEV), paste=False, **kw)
    with torch.no_grad():
        assert torch.equal(raw, m.rescaled_upsample(za))


def test_inpaint_cli(tmp_path):
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg("dddpm"), 3, 32)
    CC.run_script("inpaint_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--mask", "center",
                  "--timestep_respacing", "10", "--jump_length", "3", "--jump_n_sample", "2", "--batch_size", "2", "--out_dir", tmp_path, env=env)
    out = np.load(tmp_path / "clitest_inpaint_center_10_j3r2.npy")
    masked = np.load(tmp_path / "clitest_inpaint_center_10_j3r2_masked.npy")
    assert out.shape == (3, 32, 32, 3) and masked.shape == (3, 32, 32, 3)
    assert out.min() >= 0 and out.max() <= 255 and np.isfinite(out).all()
    # the known border comes back as given (up to the u8 -> [-1, 1] -> [0, 255] round trip)
    assert np.abs(out[:, :8] - imgs[:, :8]).max() < 1e-3
    assert (masked[:, 8:24, 8:24] == 0).all()
