"""Timestep respacing and DDIM schedules (models/diffusion/respace.py) on the CPU: improved-diffusion's space_timesteps, the
respaced tables against the model's own buffers, DDIM's linear c1 / c2 form against its direct formula, the keyword checks of
p_sample_loop, and the state_dict layout (the spaced tables are not buffers)."""
import numpy as np
import pytest
import torch

import spaced_ref as SR
from helpers import ddpm_cfg, golden_keys
from models import DDPM, Unet
from models.diffusion import respace
from oracle import diffusion_ref as D


def test_space_timesteps_ddim_stride():
    assert respace.space_timesteps(1000, "ddim50") == list(range(0, 1000, 20))
    assert respace.space_timesteps(200, "ddim25") == list(range(0, 200, 8))


def test_space_timesteps_sections():
    s = respace.space_timesteps(1000, "250")
    assert len(s) == 250 and s[:4] == [0, 4, 8, 12] and s[-2:] == [995, 999]
    s3 = respace.space_timesteps(1000, "10,10,10")
    assert len(s3) == 30 and {333, 334, 666, 667, 999} <= set(s3)
    assert respace.space_timesteps(1000, "1000") == list(range(1000))


@pytest.mark.parametrize("spec", ["ddim50", "ddim25", "ddim10", "250", "100", "10,10,10", "7,3,20", "1000", "5"])
def test_space_timesteps_matches_restatement(spec):
    for T in (1000, 200):
        try:
            want = sorted(SR.space_timesteps(T, spec))
        except ValueError:
            with pytest.raises(ValueError):
                respace.space_timesteps(T, spec)
            continue
        assert respace.space_timesteps(T, spec) == want


@pytest.mark.parametrize("spec", ["ddim999", "2000", "400,400,400"])
def test_space_timesteps_impossible_specs_raise(spec):
    with pytest.raises(ValueError):
        respace.space_timesteps(1000, spec)


def test_model_buffers_unchanged_by_shared_table_code():
    """the buffers made through respace.fp32_tables equal the oracle's (the reference's expressions) bit for bit"""
    m = DDPM(ddpm_cfg(32, 3, 16), Unet(ddpm_cfg(32, 3, 16)), "cpu", 3)
    buf = D.schedule_buffers("linear", 1000)
    for k in D.SCHEDULE_KEYS:
        assert torch.equal(getattr(m, k), buf[k]), k
    assert torch.equal(m.posterior_sigma, (0.5 * buf["posterior_log_variance_clipped"]).exp())


def _ulps(a, b):
    a, b = a.float().numpy(), b.float().numpy()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


def test_full_respacing_reproduces_model_tables():
    m = DDPM(ddpm_cfg(32, 3, 16), Unet(ddpm_cfg(32, 3, 16)), "cpu", 3)
    tables, use = respace.spaced_tables(m._betas64, "1000")
    assert use == list(range(1000))
    for k, v in m._tables().items():
        assert _ulps(tables[k], v) <= 1, k


def test_ddim_eta1_full_chain_is_the_posterior():
    a = respace.schedule_arrays(D.beta_schedule("linear", 1000))
    c1, c2, sigma = respace.ddim_coefficients(a["alphas_cumprod"], 1.0)
    assert np.abs(c1 - a["posterior_mean_coef1"]).max() < 1e-12
    assert np.abs(c2 - a["posterior_mean_coef2"]).max() < 1e-12
    assert np.abs(sigma[1:] - np.sqrt(a["posterior_variance"][1:])).max() < 1e-12
    assert c1[0] == 1.0 and c2[0] == 0.0 and sigma[0] == 0.0


@pytest.mark.parametrize("spec,eta", [("ddim50", 0.0), ("ddim50", 0.5), ("250", 1.0), ("10,10,10", 0.3)])
def test_ddim_linear_form_equals_direct_formula(spec, eta):
    """float64, random x and eps: clamp(c_recip x - c_recipm1 eps) -> c1 x0 + c2 x + sigma z equals ddim_sample's own steps"""
    betas = D.beta_schedule("linear", 1000)
    use = respace.space_timesteps(1000, spec)
    sched = respace.schedule_arrays(respace.respaced_betas(respace.schedule_arrays(betas)["alphas_cumprod"], use))
    c1, c2, sigma = respace.ddim_coefficients(sched["alphas_cumprod"], eta)
    g = np.random.default_rng(7)
    for k in (len(use) - 1, len(use) // 2, 1, 0):
        x, eps, z = g.standard_normal((3, 4096)) * np.array([[1.5], [1.0], [1.0]])
        a = sched["alphas_cumprod"][k]
        ap = sched["alphas_cumprod_prev"][k]
        x0 = np.clip(np.sqrt(1 / a) * x - np.sqrt(1 / a - 1) * eps, -1, 1)
        eps2 = (np.sqrt(1 / a) * x - x0) / np.sqrt(1 / a - 1)
        sg = eta * np.sqrt((1 - ap) / (1 - a)) * np.sqrt(1 - a / ap)
        direct = x0 * np.sqrt(ap) + np.sqrt(1 - ap - sg ** 2) * eps2 + (k != 0) * sg * z
        linear = c1[k] * x0 + c2[k] * x + (k != 0) * sigma[k] * z
        assert np.abs(direct - linear).max() < 1e-12, k


def test_spaced_tables_are_cached_and_not_buffers():
    cfg = ddpm_cfg(128, 3, 32)
    m = DDPM(cfg, Unet(cfg), "cpu", 3)
    t1, use = m._spaced_tables("ddim50", True, 0.0)
    t2, _ = m._spaced_tables("ddim50", True, 0.0)
    assert all(t1[k] is t2[k] for k in t1) and len(use) == 50 and t1["c1"].shape == (50,)
    m._spaced_tables("250", False, 0.0)
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    ks = golden_keys()["ddpm_c3"]
    assert got == ks and list(got) == list(ks)


def test_eta_without_ddim_and_negative_eta_are_errors():
    m = DDPM(ddpm_cfg(32, 3, 16), Unet(ddpm_cfg(32, 3, 16)), "cpu", 3)
    with pytest.raises(ValueError):
        m.p_sample_loop((1, 3, 16, 16), eta=0.5)
    with pytest.raises(ValueError):
        m.p_sample_loop((1, 3, 16, 16), respacing="ddim50", ddim=True, eta=-0.1)
    with pytest.raises(ValueError):
        respace.spaced_tables(m._betas64, "ddim50", ddim=False, eta=1.0)


@pytest.mark.parametrize("bad", [[1, 2, 3], [0, 2, 2], [0, 5, 3], [0, 1, 2 ** 31]])
def test_sampler_run_spaced_rejects_bad_maps(bad):
    """host-side validation of ddk_sampler_run_spaced: map[0] == 0, strictly increasing, < 2^31 -> DDK_ERR_ARG before any device
    work (the pointers are never dereferenced)"""
    import ctypes as C
    from ddk import lib as L
    from ddk.plan import UnetPlan
    plan = UnetPlan(3, 32, (1, 2, 2, 2))
    fake = 1 << 20
    a = L.SamplerArgs(plan.handle, fake, fake, None, fake, fake, fake, fake, fake, 2, 16, 16, 2, 0, 1, 0, 0, fake, 1 << 40)
    tmap = (C.c_int64 * 3)(*bad)
    assert L.load().ddk_sampler_run_spaced(C.byref(a), tmap, None) == -1
    assert "timestep_map" in L.last_error()
