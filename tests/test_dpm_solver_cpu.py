"""DPM-Solver++(2M) and the log-SNR grid (models/diffusion/respace.py) on the CPU: the "logsnrN" map against the restatement
(tests/dpm_solver_ref.py), the order-1 tables against DDIM eta 0, the first / last rows, the convergence of the product's own
float64 coefficients on Gaussian data with the exact denoiser, and the keyword / flag checks that come before any device work."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dpm_solver_ref as DR
from helpers import ddpm_cfg
from models import DDPM, Unet
from models.diffusion import respace
from oracle import diffusion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = D.beta_schedule("linear", 1000)


def _acp(betas):
    return respace.schedule_arrays(betas)["alphas_cumprod"]


@pytest.mark.parametrize("schedule,n", [("linear", n) for n in (2, 5, 10, 20, 40, 80, 250)] + [("cosine", n) for n in (2, 5, 8)])
def test_logsnr_map_matches_restatement(schedule, n):
    betas = D.beta_schedule(schedule, 1000)
    got = respace.space_timesteps(1000, f"logsnr{n}", _acp(betas))
    assert got == DR.logsnr_grid(betas, n)
    assert len(got) == n and got[0] == 0 and got[-1] == 999
    assert all(b > a for a, b in zip(got, got[1:]))


def test_logsnr_grid_follows_the_schedule():
    lin = respace.space_timesteps(1000, "logsnr8", _acp(BETAS))
    cos = respace.space_timesteps(1000, "logsnr8", _acp(D.beta_schedule("cosine", 1000)))
    assert lin != cos


@pytest.mark.parametrize("schedule,n", [("linear", 1), ("linear", 988), ("linear", 1001), ("cosine", 9), ("cosine", 20)])
def test_logsnr_impossible_counts_raise(schedule, n):
    """cosine: the clipped last beta puts lambda_999 = -9.9 far below lambda_998 = -6.5, so from 9 steps on the targets below
    -6.5 all land on 999 and the grid does not fit"""
    with pytest.raises(ValueError):
        respace.space_timesteps(1000, f"logsnr{n}", _acp(D.beta_schedule(schedule, 1000)))
    with pytest.raises(ValueError):
        DR.logsnr_grid(D.beta_schedule(schedule, 1000), n)


def test_logsnr_needs_the_schedule():
    with pytest.raises(ValueError):
        respace.space_timesteps(1000, "logsnr20")


@pytest.mark.parametrize("spec", ["logsnr20", "ddim50", "250"])
def test_order1_tables_equal_ddim_eta0(spec):
    one, use1 = respace.dpm_solver_tables(BETAS, spec, order=1)
    ddim, use2 = respace.spaced_tables(BETAS, spec, ddim=True, eta=0.0)
    assert use1 == use2
    for k in ("c_recip", "c_recipm1", "c1", "c2"):
        assert float((one[k] - ddim[k]).abs().max()) <= 1e-6, k
    assert torch.equal(one["c3"], torch.zeros_like(one["c3"]))


@pytest.mark.parametrize("spec", ["logsnr10", "logsnr20", "ddim50"])
def test_first_and_last_rows(spec):
    tab, use = respace.dpm_solver_tables(BETAS, spec)
    K = len(use)
    assert all(v.dtype == torch.float32 and v.shape == (K,) for v in tab.values())
    assert float(tab["c3"][K - 1]) == 0.0
    assert (float(tab["c1"][0]), float(tab["c2"][0]), float(tab["c3"][0])) == (1.0, 0.0, 0.0)
    assert (tab["c3"][1:K - 1] < 0).all()                 # every inner row is second order
    # a second-order row's c1 + c3 is the first-order phi
    one, _ = respace.dpm_solver_tables(BETAS, spec, order=1)
    assert float((tab["c1"][1:] + tab["c3"][1:] - one["c1"][1:]).abs().max()) < 1e-6


def test_coefficients_match_restatement_steps():
    """one step of the product's linear form against the restatement's direct form, float64 coefficients"""
    sched = respace.schedule_arrays(respace.respaced_betas(_acp(BETAS), respace.space_timesteps(1000, "logsnr20", _acp(BETAS))))
    c1, c2, c3 = respace.dpm_solver_coefficients(sched["alphas_cumprod"])
    ref = DR.DPMSolver(BETAS, "logsnr20")
    x = torch.linspace(-2, 2, 9, dtype=torch.float64)
    x0, x0p = 0.3 * x, -0.2 * x
    for k in range(1, 19):
        want = ref.step(x.float(), x0.float(), [x0p.float()], k).double()
        got = c1[k] * x0 + c2[k] * x + c3[k] * x0p
        assert float((got - want).abs().max()) < 1e-6, k


# ---------------------------------------------------------------- convergence on Gaussian data with the exact denoiser
S = 0.5                                          # x0 ~ N(0, S^2)
U = np.linspace(-2.0, 2.0, 41)                   # x_T grid, in units of the marginal's standard deviation


def _pf_error(spec, solver):
    """max-abs error of the final sample against the closed-form probability-flow solution, float64 throughout"""
    acp = _acp(BETAS)
    use = respace.space_timesteps(1000, spec, acp)
    sched = respace.schedule_arrays(respace.respaced_betas(acp, use))
    a = sched["alphas_cumprod"]
    if solver == "ddim":
        c1, c2, _ = respace.ddim_coefficients(a, 0.0)
        c3 = np.zeros_like(c1)
    else:
        c1, c2, c3 = respace.dpm_solver_coefficients(a, order=2)
    K = len(a)
    x = np.sqrt(a[K - 1] * S ** 2 + 1 - a[K - 1]) * U
    hist = np.zeros_like(x)
    for k in range(K - 1, -1, -1):
        eps = np.sqrt(1 - a[k]) * x / (a[k] * S ** 2 + 1 - a[k])            # E[eps | x_k]
        x0 = np.clip(sched["sqrt_recip_alphas_cumprod"][k] * x - sched["sqrt_recipm1_alphas_cumprod"][k] * eps, -1, 1)
        x = c1[k] * x0 + c2[k] * x + c3[k] * hist
        hist = x0
    return float(np.abs(x - S * U).max())


def test_2m_beats_ddim_on_logsnr20():
    e2m, eddim = _pf_error("logsnr20", "2m"), _pf_error("logsnr20", "ddim")
    print(f"logsnr20: 2M {e2m:.3g}, DDIM {eddim:.3g}")
    assert e2m <= eddim / 5


def test_observed_orders():
    o2m = np.log2(_pf_error("logsnr40", "2m") / _pf_error("logsnr80", "2m"))
    oddim = np.log2(_pf_error("logsnr40", "ddim") / _pf_error("logsnr80", "ddim"))
    print(f"observed order between logsnr40 and logsnr80: 2M {o2m:.3f}, DDIM {oddim:.3f}")
    assert o2m >= 1.7
    assert oddim < 1.3


# ---------------------------------------------------------------- keyword and flag checks (before any device work)
@pytest.mark.parametrize("solver,kw", [("dpm++2m", dict(ddim=True)), ("dpm++2m", dict(eta=0.5)),
                                       ("dpm++2m", dict(noise=torch.zeros(20, 1, 3, 16, 16))), ("dpm++3m", dict())])
def test_p_sample_loop_rejects_bad_combinations(solver, kw):
    """ValueError on the CPU model: raised before the device check (which would raise DDKError)"""
    cfg = ddpm_cfg(32, 3, 16)
    m = DDPM(cfg, Unet(cfg), "cpu", 3)
    with pytest.raises(ValueError):
        m.p_sample_loop((1, 3, 16, 16), respacing="logsnr20", solver=solver, **kw)


def test_solver_tables_are_cached_and_not_buffers():
    cfg = ddpm_cfg(32, 3, 16)
    m = DDPM(cfg, Unet(cfg), "cpu", 3)
    keys = list(m.state_dict())
    a = m._solver_tables("logsnr20", "dpm++2m")
    assert a is m._solver_tables("logsnr20", "dpm++2m")
    assert a[1] == respace.space_timesteps(1000, "logsnr20", _acp(BETAS))
    assert list(m.state_dict()) == keys


@pytest.mark.parametrize("extra", [["--use_ddim"], ["--eta", "0.5"]])
def test_cli_rejects_dpm_solver_with_ddim_flags(extra, tmp_path):
    script = os.path.join(ROOT, "downsampled-diffusion_amd", "generate_model_samples.py")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "downsampled-diffusion_amd"))
    r = subprocess.run([sys.executable, script, "--synthetic", str(tmp_path / "missing.json"), "--timestep_respacing", "logsnr20",
                        "--dpm_solver"] + extra, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2, r.stderr[-2000:]
    assert "--dpm_solver" in r.stderr
