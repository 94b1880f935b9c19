"""Respaced and DDIM sampling on the GPU (DDPM.p_sample_loop(respacing=, ddim=, eta=), ddk_sampler_run_spaced) against
tests/spaced_ref.py, improved-diffusion's SpacedDiffusion / ddim_sample in their direct form around oracle/unet_ref at map[k].

The tiny DDPM (unet_chan 32, 3x16x16, linear schedule, T = 1000) has no Winograd final conv, so its steps end in the unfused
p_update_kernel; the cfg4 window at B = 32 ends in final_tail_kernel.  Bars as for the plain chains: 1e-4 abs against the
restatement with the same argmax, 1e-6 between full respacing and the plain chain, 1e-5 between the Python loop and the
native sampler.  Each comparison with injected draws has a negative control."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import spaced_ref as SR
from helpers import dddpm_cfg, ddpm_cfg, det_load, golden_keys, unet_cfg
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def draws():
    x_T = syn.synthetic_normal(SHAPE, "spaced.xT")
    noise = torch.stack([syn.synthetic_normal(SHAPE, f"spaced.n{k}") for k in range(1000)])
    return x_T, noise


def _ref(spec, x_T, noise, ddim=False, eta=0.0, k_end=0):
    use = SR.space_timesteps(1000, spec) if spec else set(range(1000))
    sd = SR.SpacedDiffusion(BETAS, use)
    return sd, (lambda eps: sd.run(eps, x_T, lambda j: noise[j], k_end=k_end, ddim=ddim, eta=eta))


def _check(got, want, tol=TOL):
    err = float((got.cpu() - want).abs().max())
    assert torch.isfinite(got).all()
    assert err < tol, err
    assert torch.equal(CC.argmax(got.cpu()), CC.argmax(want))
    return err


@pytest.mark.parametrize("spec", ["ddim50", "250", "10,10,10"])
def test_spaced_ancestral_vs_restatement(tiny, draws, spec):
    m, eps = tiny
    x_T, noise = draws
    sd, run = _ref(spec, x_T, noise)
    K = sd.num_timesteps
    got = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise[:K], respacing=spec)
    err = _check(got, run(eps))
    print(f"spaced ancestral {spec} ({K} steps): max abs error {err:.3g}")


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_vs_restatement(tiny, draws, eta):
    m, eps = tiny
    x_T, noise = draws
    _, run = _ref("ddim50", x_T, noise, ddim=True, eta=eta)
    got = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise[:50], respacing="ddim50", ddim=True, eta=eta)
    err = _check(got, run(eps))
    print(f"DDIM ddim50 eta {eta}: max abs error {err:.3g}")


def test_changed_draw_misses_the_bar(tiny, draws):
    """negative control: spaced step k = 30 of ddim50 (eta 0.5) gets another draw; the chain must miss the restatement by > 10x"""
    m, eps = tiny
    x_T, noise = draws
    _, run = _ref("ddim50", x_T, noise, ddim=True, eta=0.5)
    bad = noise[:50].clone()
    bad[49 - 30] = syn.synthetic_normal(SHAPE, "spaced.control")
    got = m.p_sample_loop(SHAPE, x_T=x_T, noise=bad, respacing="ddim50", ddim=True, eta=0.5)
    err = float((got.cpu() - run(eps)).abs().max())
    print(f"ddim50 eta 0.5, draw of k = 30 changed: max abs error {err:.3g}")
    assert err > 10 * TOL


def test_ddim_eta0_ignores_the_seed(tiny, draws):
    m, _ = tiny
    x_T, _ = draws
    a = m.p_sample_loop(SHAPE, x_T=x_T, seed=1, respacing="ddim50", ddim=True)
    b = m.p_sample_loop(SHAPE, x_T=x_T, seed=2, respacing="ddim50", ddim=True)
    assert torch.equal(a, b)


def test_full_respacing_equals_plain_chain(tiny, draws):
    m, _ = tiny
    x_T, noise = draws
    plain = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise)
    full = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise, respacing="1000")
    err = float((full - plain).abs().max())
    print(f"respacing '1000' vs plain: {err:.3g}")
    assert err < 1e-6


def test_full_ddim_eta1_equals_plain_chain(tiny, draws):
    m, _ = tiny
    x_T, noise = draws
    plain = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise)
    ddim = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise, ddim=True, eta=1.0)
    err = float((ddim - plain).abs().max())
    print(f"DDIM eta 1 over all T vs plain: {err:.3g}")
    assert err < 1e-4


@pytest.mark.parametrize("spec,ddim,eta", [("10,10,10", False, 0.0), ("ddim50", True, 0.5)])
def test_python_loop_equals_native(tiny, draws, spec, ddim, eta):
    m, _ = tiny
    x_T, noise = draws
    K = len(SR.space_timesteps(1000, spec))
    native = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise[:K], respacing=spec, ddim=ddim, eta=eta)
    with CC.toggled(m, "native_sampler", False):
        loop = m.p_sample_loop(SHAPE, x_T=x_T, noise=noise[:K], respacing=spec, ddim=ddim, eta=eta)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, {spec} ddim={ddim}: {err:.3g}")
    assert err < 1e-5


def test_spaced_philox_seed_and_stream(tiny, draws):
    m, _ = tiny
    x_T, _ = draws
    kw = dict(x_T=x_T, respacing="ddim50", ddim=True, eta=1.0)
    a = m.p_sample_loop(SHAPE, seed=77, **kw)
    b = m.p_sample_loop(SHAPE, seed=77, **kw)
    assert torch.equal(a, b)
    with CC.toggled(m, "rng_stream_id", 1):
        c = m.p_sample_loop(SHAPE, seed=77, **kw)
    assert float((a - c).abs().max()) > 1e-3


def test_early_stop_runs_the_kept_steps_above_it(tiny, draws):
    """ddim50 keeps 0, 20, ..., 980: early_stop 500 runs k = 49 .. 25 (25 draws); 981 runs none"""
    from ddk.lib import DDKError
    m, eps = tiny
    x_T, noise = draws
    _, run = _ref("ddim50", x_T, noise, ddim=True, eta=0.5, k_end=25)
    got = m.p_sample_loop(SHAPE, early_stop=500, x_T=x_T, noise=noise[:25], respacing="ddim50", ddim=True, eta=0.5)
    _check(got, run(eps))
    _, run2 = _ref("ddim50", x_T, noise, ddim=True, eta=0.5, k_end=26)
    got2 = m.p_sample_loop(SHAPE, early_stop=501, x_T=x_T, noise=noise[:24], respacing="ddim50", ddim=True, eta=0.5)
    _check(got2, run2(eps))
    with pytest.raises(DDKError):
        m.p_sample_loop(SHAPE, early_stop=500, x_T=x_T, noise=noise[:26], respacing="ddim50", ddim=True, eta=0.5)
    same = m.p_sample_loop(SHAPE, early_stop=981, x_T=x_T, respacing="ddim50", ddim=True)
    assert torch.equal(same.cpu(), x_T)


def test_plain_and_ddim_chains_share_a_workspace_without_sharing_rows(tiny, draws):
    """a plain t_start = 49 chain and a ddim50 chain have the same workspace size, so the plan hands both the same "smp"
    workspace and its shift table; alternated three times each must equal its own first result and its restatement"""
    from ddk import ops
    m, eps = tiny
    x_T, noise = draws
    plan = m._eps_model_nhwc().plan()
    nz = noise[:50].to(DEV).permute(0, 1, 3, 4, 2).contiguous()
    buf = D.schedule_buffers("linear", 1000)

    def plain():
        x = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
        plan.sample_nhwc(x, m._tables(), 49, 0, noise=nz, seed=3)
        return ops.nhwc_to_nchw(x).cpu()

    def ddim():
        return m.p_sample_loop(SHAPE, x_T=x_T, noise=noise[:50], respacing="ddim50", ddim=True, eta=0.5).cpu()

    want_plain = D.p_sample_loop(buf, eps, x_T, list(noise[:50]), 50)[0]
    _, run = _ref("ddim50", x_T, noise, ddim=True, eta=0.5)
    want_ddim = run(eps)
    first = {}
    for _ in range(3):
        for name, f, want in (("plain", plain, want_plain), ("ddim", ddim, want_ddim)):
            got = f()
            first.setdefault(name, got)
            assert torch.equal(got, first[name]), name
            _check(got, want)
    nbytes = plan._lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, 49)
    assert len([k for k in plan._ws if k[0] == "smp" and k[1] == nbytes]) == 1


def test_unfused_tail_ddim_b4(tiny):
    """B = 4 on the tiny UNet (no Winograd final conv: p_update_kernel ends every step), ddim50 eta 0.5 vs the restatement"""
    m, eps = tiny
    shape = (4, 3, 16, 16)
    x_T = syn.synthetic_normal(shape, "spaced.b4.xT")
    noise = torch.stack([syn.synthetic_normal(shape, f"spaced.b4.n{k}") for k in range(50)])
    _, run = _ref("ddim50", x_T, noise, ddim=True, eta=0.5)
    got = m.p_sample_loop(shape, x_T=x_T, noise=noise, respacing="ddim50", ddim=True, eta=0.5)
    err = _check(got, run(eps))
    print(f"unfused tail, B = 4, ddim50 eta 0.5: {err:.3g}")


def test_state_dict_keys_unchanged_after_spaced_sample():
    from models import DDPM, Unet
    cfg = ddpm_cfg(128, 3, 32)
    m = DDPM(cfg, Unet(cfg), DEV, 3).to(DEV).eval()
    m.p_sample_loop((1, 3, 32, 32), respacing="ddim25", ddim=True, seed=1)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    ks = golden_keys()["ddpm_c3"]
    assert got == ks and list(got) == list(ks)


# ---------------------------------------------------------------- cfg4, B = 32: the benchmark's shape and plan options
B4, C4, S4 = 32, 8, 32
CFG4 = dddpm_cfg(128, 256, 3)


def test_cfg4_b32_ddim50_windows():
    """ddim50 eta 0 at the benchmark's shape, default options (fused tail, level chain, in-launch GroupNorm): k = 49 .. 45
    (early_stop = map[45] = 900) and k = 4 .. 0 (a chain started at t_start = 4 with the first five map entries)."""
    from ddk import ops
    from models import DownsampleDDPM, Unet
    m = det_load(DownsampleDDPM(CFG4, Unet(CFG4), DEV, 3)).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    eps = lambda x, t: U.unet_forward(sd, unet_cfg(128, C4), x, t, pre="latent_model.")
    plan = m._eps_model_nhwc().plan()
    before, cluster = ops.cluster_timeouts(), plan._cluster
    spaced = SR.SpacedDiffusion(BETAS, SR.space_timesteps(1000, "ddim50"))
    shape = (B4, C4, S4, S4)
    x0 = syn.synthetic_normal(shape, "spaced.cfg4.x")
    got = m.p_sample_loop(shape, early_stop=900, x_T=x0, seed=9, respacing="ddim50", ddim=True)
    want = spaced.run(eps, x0, lambda j: torch.zeros(shape), k_start=49, k_end=45, ddim=True)
    e1 = _check(got, want)
    tables, use = m._spaced_tables("ddim50", True, 0.0)
    x = ops.nchw_to_nhwc(x0.to(DEV).contiguous())
    plan.sample_nhwc(x, tables, 4, 0, seed=9, stream_id=3, timesteps=use[:5])
    got2 = ops.nhwc_to_nchw(x)
    want2 = spaced.run(eps, x0, lambda j: torch.zeros(shape), k_start=4, k_end=0, ddim=True)
    e2 = _check(got2, want2)
    torch.cuda.synchronize()
    print(f"cfg4 B=32 ddim50: k=49..45 {e1:.3g}, k=4..0 {e2:.3g}")
    assert ops.cluster_timeouts() == before and plan._cluster == cluster


# ---------------------------------------------------------------- dDDPM and the command line
def test_dddpm_sample_ddim50():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    torch.manual_seed(11)
    x, z = m.sample(2, respacing="ddim50", ddim=True)
    assert x.shape == (2, 3, 32, 32) and z.shape == (2, 8, 8, 8)
    torch.manual_seed(11)
    z2 = m.p_sample_loop((2, 8, 8, 8), respacing="ddim50", ddim=True)
    assert torch.equal(z, z2)
    with torch.no_grad():
        assert torch.equal(x, m.rescaled_upsample(z))


def test_generate_model_samples_respacing_cli(tmp_path):
    cfg_path, _, _, env = CC.cli_files(tmp_path, CC.cli_cfg("dddpm"), 0, 32)
    base = ["generate_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--fid_samples", "4", "--batch_size", "2",
            "--out_dir", tmp_path]
    CC.run_script(*base, "--timestep_respacing", "ddim50", "--use_ddim", env=env)
    imgs = np.load(tmp_path / "clitest_ddim50_ddim_eta0.npy")
    assert imgs.shape == (2, 2, 32, 32, 3) and imgs.min() == 0.0 and abs(imgs.max() - 255.0) < 1e-3
    assert np.load(tmp_path / "clitest_ddim50_ddim_eta0_latent.npy").shape == (2, 2, 8, 8, 8)
    assert not (tmp_path / "clitest.npy").exists()
    CC.run_script(*base, "--early_stop", "95", env=env)
    assert np.load(tmp_path / "clitest.npy").shape == (2, 2, 32, 32, 3)
