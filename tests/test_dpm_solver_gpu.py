"""DPM-Solver++(2M) on the GPU (DDPM.p_sample_loop(solver="dpm++2m"), ddk_sampler_run_multistep, p_update_kernel<StepKind::Multistep> and
final_tail_kernel's multistep mode) against tests/dpm_solver_ref.py, Algorithm 2 in its direct form around oracle/unet_ref at map[k].

The tiny DDPM (unet_chan 32, 3x16x16, linear schedule, T = 1000) has no Winograd final conv, so its steps end in the unfused
p_update_kernel<StepKind::Multistep>; the cfg4 window at B = 32 ends in final_tail_kernel's multistep instantiation.  Bars as for the spaced chains:
1e-4 abs against the restatement with the same argmax, 1e-5 between the Python loop and the native sampler."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import dpm_solver_ref as DR
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
SOLVER = "dpm++2m"


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def x_T():
    return syn.synthetic_normal(SHAPE, "dpm.xT")


def _check(got, want, tol=TOL):
    err = float((got.cpu() - want).abs().max())
    assert torch.isfinite(got).all()
    assert err < tol, err
    assert torch.equal(CC.argmax(got.cpu()), CC.argmax(want))
    return err


@pytest.mark.parametrize("spec", ["logsnr20", "ddim50"])
def test_2m_vs_restatement(tiny, x_T, spec):
    """logsnr20: one-step graphs; ddim50 (K = 50): the 16-step graph too"""
    m, eps = tiny
    got = m.p_sample_loop(SHAPE, x_T=x_T, respacing=spec, solver=SOLVER)
    err = _check(got, DR.DPMSolver(BETAS, spec).run(eps, x_T))
    print(f"2M {spec}: max abs error {err:.3g}")


def test_order1_tables_miss_the_2m_restatement(tiny, x_T):
    """negative control: the same chain with order-1 tables (c3 = 0, no history used) matches the order-1 restatement and misses
    the 2M one by more than 10x the bar"""
    from ddk import ops
    from models.diffusion import respace
    m, eps = tiny
    tab, use = respace.dpm_solver_tables(m._betas64, "logsnr20", order=1)
    tab = {k: v.to(DEV) for k, v in tab.items()}
    x = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    m._eps_model_nhwc().plan().sample_multistep_nhwc(x, tab, len(use) - 1, 0, timesteps=use)
    got = ops.nhwc_to_nchw(x).cpu()
    _check(got, DR.DPMSolver(BETAS, "logsnr20", order=1).run(eps, x_T))
    err = float((got - DR.DPMSolver(BETAS, "logsnr20").run(eps, x_T)).abs().max())
    print(f"order-1 tables vs the 2M restatement: {err:.3g}")
    assert err > 10 * TOL


def test_graph_equals_eager_bit_for_bit(tiny, x_T):
    m, _ = tiny
    graphed = m.p_sample_loop(SHAPE, x_T=x_T, respacing="ddim50", solver=SOLVER)
    with CC.toggled(m, "use_graph", False):
        eager = m.p_sample_loop(SHAPE, x_T=x_T, respacing="ddim50", solver=SOLVER)
    assert torch.equal(graphed, eager)


def test_python_loop_equals_native(tiny, x_T):
    m, _ = tiny
    native = m.p_sample_loop(SHAPE, x_T=x_T, respacing="logsnr20", solver=SOLVER)
    with CC.toggled(m, "native_sampler", False):
        loop = m.p_sample_loop(SHAPE, x_T=x_T, respacing="logsnr20", solver=SOLVER)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, 2M logsnr20: {err:.3g}")
    assert err < 1e-5


def test_early_stop_cuts_the_bottom(tiny, x_T):
    """logsnr20: early_stop = map[12] runs k = 19 .. 12; above map[19] = 999 nothing runs"""
    from models.diffusion import respace
    m, eps = tiny
    use = respace.space_timesteps(1000, "logsnr20", respace.schedule_arrays(BETAS)["alphas_cumprod"])
    got = m.p_sample_loop(SHAPE, early_stop=use[12], x_T=x_T, respacing="logsnr20", solver=SOLVER)
    _check(got, DR.DPMSolver(BETAS, "logsnr20").run(eps, x_T, k_end=12))
    same = m.p_sample_loop(SHAPE, early_stop=1000, x_T=x_T, respacing="logsnr20", solver=SOLVER)
    assert torch.equal(same.cpu(), x_T)


def test_ddim_and_2m_chains_alternate(tiny, x_T):
    """a DDIM logsnr20 chain and a 2M logsnr20 chain on one model and shape, alternated three times: each equals its own first
    result and its restatement (graph key, shift table, history reset)"""
    m, eps = tiny
    sd = SR.SpacedDiffusion(BETAS, set(DR.logsnr_grid(BETAS, 20)))
    want = {"ddim": sd.run(eps, x_T, lambda j: torch.zeros(SHAPE), ddim=True),
            "2m": DR.DPMSolver(BETAS, "logsnr20").run(eps, x_T)}
    runs = {"ddim": lambda: m.p_sample_loop(SHAPE, x_T=x_T, respacing="logsnr20", ddim=True).cpu(),
            "2m": lambda: m.p_sample_loop(SHAPE, x_T=x_T, respacing="logsnr20", solver=SOLVER).cpu()}
    first = {}
    for _ in range(3):
        for name in ("ddim", "2m"):
            got = runs[name]()
            first.setdefault(name, got)
            assert torch.equal(got, first[name]), name
            _check(got, want[name])
    assert float((first["ddim"] - first["2m"]).abs().max()) > 10 * TOL


def test_injected_noise_is_rejected_by_the_library(tiny, x_T):
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    tables, use = m._solver_tables("logsnr20", SOLVER)
    plan = m._eps_model_nhwc().plan()
    x = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    noise = torch.zeros((20, *x.shape), device=DEV)
    nbytes = plan._lib.ddk_sampler_multistep_workspace_bytes(plan.handle, 2, 16, 16, 19)
    assert nbytes > plan._lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, 19)
    ws = torch.empty(nbytes // 4, device=DEV)
    a = CC.sampler_args(plan, x, tables, 19, ws, nbytes, seed=0, noise=noise)        # the solver's tables have no sigma: NULL
    assert plan._lib.ddk_sampler_run_multistep(a, CC.timestep_map(use), L.ptr(tables["c3"]), L.stream()) == -1     # DDK_ERR_ARG
    assert "noise" in L.last_error()


def test_update_kernel_bit_exact():
    """ops.p_sample_update_multistep_ against the fp32 torch expression in the kernel's order"""
    from ddk import ops
    g = torch.Generator().manual_seed(5)
    B, per = 3, 4 * 97
    x = (2 * torch.randn(B, per, generator=g)).to(DEV)
    e = torch.randn(B, per, generator=g).to(DEV)
    h = torch.rand(B, per, generator=g).to(DEV) * 2 - 1
    t = torch.tensor([0, 7, 3], device=DEV)
    tab = {k: (torch.rand(8, generator=g) * s).to(DEV) for k, s in
           (("c_recip", 3.0), ("c_recipm1", 2.0), ("c1", 1.0), ("c2", 1.0), ("c3", -0.5))}
    col = lambda k: tab[k][t].unsqueeze(1)
    x0 = (col("c_recip") * x - col("c_recipm1") * e).clamp(-1, 1)
    want = (col("c1") * x0 + col("c2") * x) + col("c3") * h
    xs, hs = x.clone(), h.clone()
    ops.p_sample_update_multistep_(xs, e, hs, t, **tab)
    assert torch.equal(xs, want)
    assert torch.equal(hs, x0)


# ---------------------------------------------------------------- cfg4, B = 32: the benchmark's shape and plan options
def test_cfg4_b32_2m_window():
    """logsnr20 at the benchmark's shape, default options (fused tail, level chain, in-launch GroupNorm): k = 19 .. 15 via
    early_stop = map[15]"""
    from ddk import ops
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(128, 256, 3)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    eps = lambda x, t: U.unet_forward(sd, unet_cfg(128, 8), x, t, pre="latent_model.")
    plan = m._eps_model_nhwc().plan()
    before, cluster = ops.cluster_timeouts(), plan._cluster
    _, use = m._solver_tables("logsnr20", SOLVER)
    shape = (32, 8, 32, 32)
    x0 = syn.synthetic_normal(shape, "dpm.cfg4.x")
    got = m.p_sample_loop(shape, early_stop=use[15], x_T=x0, respacing="logsnr20", solver=SOLVER)
    want = DR.DPMSolver(BETAS, "logsnr20").run(eps, x0, k_end=15)
    err = _check(got, want)
    torch.cuda.synchronize()
    print(f"cfg4 B=32 2M logsnr20 k=19..15: {err:.3g}")
    assert ops.cluster_timeouts() == before and plan._cluster == cluster


# ---------------------------------------------------------------- dDDPM, state_dict and the command line
def test_dddpm_sample_2m():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    torch.manual_seed(11)
    x, z = m.sample(2, respacing="logsnr20", solver=SOLVER)
    assert x.shape == (2, 3, 32, 32) and z.shape == (2, 8, 8, 8)
    with torch.no_grad():
        assert torch.equal(x, m.rescaled_upsample(z))


def test_state_dict_keys_unchanged_after_2m_sample():
    from models import DDPM, Unet
    cfg = ddpm_cfg(128, 3, 32)
    m = DDPM(cfg, Unet(cfg), DEV, 3).to(DEV).eval()
    m.p_sample_loop((1, 3, 32, 32), respacing="logsnr20", solver=SOLVER)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    ks = golden_keys()["ddpm_c3"]
    assert got == ks and list(got) == list(ks)


def test_generate_model_samples_dpm_solver_cli(tmp_path):
    cfg_path, _, _, env = CC.cli_files(tmp_path, CC.cli_cfg("dddpm"), 0, 32)
    CC.run_script("generate_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--fid_samples", "4", "--batch_size", "2",
                  "--out_dir", tmp_path, "--timestep_respacing", "logsnr10", "--dpm_solver", env=env)
    imgs = np.load(tmp_path / "clitest_logsnr10_dpmpp2m.npy")
    assert imgs.shape == (2, 2, 32, 32, 3) and imgs.min() == 0.0 and abs(imgs.max() - 255.0) < 1e-3
    assert np.load(tmp_path / "clitest_logsnr10_dpmpp2m_latent.npy").shape == (2, 2, 8, 8, 8)
    assert not (tmp_path / "clitest.npy").exists()
