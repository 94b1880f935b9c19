"""RePaint inpainting (models/diffusion/respace.py repaint_schedule / repaint_tables, DDPM.inpaint) on the CPU: the schedule
against a literal restatement of RePaint's get_schedule_jump pair walk (tests/repaint_ref.py), the op count, the row tables
(jumps as composed forward steps, r = 1 as the plain spaced chain), the argument checks that come before any device work, and the
restatement's conditional mean on Gaussian data with the exact eps against the true Gaussian conditional."""
import numpy as np
import pytest
import torch

import repaint_ref as RP
import spaced_ref as SR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import respace
from oracle import diffusion_ref as D

BETAS = D.beta_schedule("linear", 1000)
CASES = [(250, 10, 10), (20, 5, 3), (20, 5, 1), (10, 3, 2), (7, 10, 4), (1, 1, 3), (12, 4, 5), (50, 1, 2)]


def _n_ops(K, j, r):
    return K + (r - 1) * j * len(range(0, K - j, j))


@pytest.mark.parametrize("K,j,r", CASES)
def test_schedule_matches_repaint_pair_walk(K, j, r):
    taus, jl = respace.repaint_schedule(K, j, r)
    want_taus, want_fwd = RP.ops_from_pairs(K, j, r)
    assert taus == want_taus
    assert jl == want_fwd
    assert len(taus) == _n_ops(K, j, r)
    assert taus.count(0) == 1 and taus[-1] == 0 and jl[-1] == 0
    assert set(v for v in jl) <= {0, j}


def test_op_counts_of_the_issue_examples():
    assert len(respace.repaint_schedule(250, 10, 10)[0]) == 2410
    assert len(respace.repaint_schedule(20, 5, 3)[0]) == 50


@pytest.mark.parametrize("K,j", [(20, 5), (250, 10), (7, 3)])
def test_r1_is_k_plain_steps(K, j):
    taus, jl = respace.repaint_schedule(K, j, 1)
    assert taus == list(range(K - 1, -1, -1)) and not any(jl)


@pytest.mark.parametrize("spec,j,r", [("20", 5, 3), ("250", 10, 10), (None, 10, 2), ("8", 2, 2)])
def test_tables_rows_and_map(spec, j, r):
    tab, use = respace.repaint_tables(BETAS, spec, j, r)
    K = 1000 if spec is None else len(SR.space_timesteps(1000, spec))
    N = _n_ops(K, j, r)
    assert len(use) == N and all(v.shape == (N,) and v.dtype == torch.float32 for v in tab.values())
    assert use[0] == 0 and all(0 < t < 2 ** 31 for t in use[1:])
    assert float(tab["ka"][0]) == 1.0 and float(tab["kb"][0]) == 0.0 and float(tab["jb"][0]) == 0.0


@pytest.mark.parametrize("spec,j,r", [("20", 5, 3), ("250", 10, 10), ("8", 2, 2)])
def test_jumps_equal_composed_forward_steps(spec, j, r):
    """(ja, jb) of every jump equal the float64 composition of j single forward steps of the respaced DDPM to 1e-12; the fp32
    tables are their cast"""
    acp = respace.schedule_arrays(BETAS)["alphas_cumprod"]
    use = respace.space_timesteps(1000, spec, acp)
    sched = respace.schedule_arrays(respace.respaced_betas(acp, use))
    taus, jl = respace.repaint_schedule(len(use), j, r)
    ka, kb, ja, jb = respace.repaint_coefficients(sched["alphas_cumprod"], taus, jl)
    betas = sched["betas"]
    n_jumps = 0
    for i, (tau, jj) in enumerate(zip(taus, jl)):
        if not jj:
            assert ja[i] == 1.0 and jb[i] == 0.0
            continue
        n_jumps += 1
        a, v = 1.0, 0.0
        for s in range(tau, tau + jj):               # state tau - 1 -> tau - 1 + j, one step q(x_{s} | x_{s-1}) at a time
            a, v = a * np.sqrt(1.0 - betas[s]), v * (1.0 - betas[s]) + betas[s]
        assert abs(ja[i] - a) < 1e-12 and abs(jb[i] - np.sqrt(v)) < 1e-12
    assert n_jumps == (r - 1) * len(range(0, len(use) - j, j))
    tab, _ = respace.repaint_tables(BETAS, spec, j, r)
    for name, v in (("ka", ka), ("kb", kb), ("ja", ja), ("jb", jb)):
        assert torch.equal(tab[name], torch.tensor(v[::-1].copy(), dtype=torch.float32)), name


@pytest.mark.parametrize("spec", ["20", "250", None])
def test_r1_tables_equal_spaced_tables(spec):
    rp, use_rp = respace.repaint_tables(BETAS, spec, 5, 1)
    sp, use_sp = respace.spaced_tables(BETAS, spec)
    assert use_rp == use_sp
    for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma"):
        assert torch.equal(rp[k], sp[k]), k


def test_bad_schedule_arguments_raise():
    for args in ((0, 1, 1), (10, 0, 1), (10, 2, 0)):
        with pytest.raises(ValueError):
            respace.repaint_schedule(*args)


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


@pytest.mark.parametrize("mask", [torch.full((2, 1, 16, 16), 0.5), torch.ones(2, 2, 16, 16), torch.ones(3, 1, 16, 16),
                                  torch.ones(2, 1, 8, 16), torch.ones(1, 2, 1, 16, 16), torch.full((16, 16), float("nan")),
                                  torch.full((16, 16), -1.0)])
def test_bad_masks_raise(mask):
    with pytest.raises(ValueError):
        _tiny().inpaint(torch.zeros(2, 3, 16, 16), mask)


@pytest.mark.parametrize("kw", [dict(ddim=True), dict(solver="dpm++2m"), dict(eta=0.0), dict(noise=torch.zeros(1)),
                                dict(early_stop=10), dict(jump_length=0), dict(jump_n_sample=0), dict(jump_length=2.5)])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError):
        _tiny().inpaint(torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16), **kw)


def test_bad_images_and_stream_raise():
    m = _tiny()
    with pytest.raises(ValueError):
        m.inpaint(torch.zeros(2, 3, 8, 8), torch.ones(8, 8))
    with pytest.raises(ValueError):
        m.inpaint(torch.full((1, 3, 16, 16), float("inf")), torch.ones(16, 16))
    m.rng_stream_id = 2 ** 29
    with pytest.raises(ValueError):
        m.inpaint(torch.zeros(1, 3, 16, 16), torch.ones(16, 16))


def test_dddpm_checks_the_image_shape():
    cfg = dddpm_cfg(32, 32, 2)
    m = DownsampleDDPM(cfg, Unet(cfg), "cpu", 3)
    with pytest.raises(ValueError):
        m.inpaint(torch.zeros(1, 8, 8, 8), torch.ones(8, 8))        # a latent is not an image
    with pytest.raises(ValueError):
        m.inpaint(torch.zeros(1, 3, 32, 32), torch.ones(32, 32), solver="dpm++2m")


def test_inpaint_tables_are_cached_and_not_buffers():
    m = _tiny()
    keys = list(m.state_dict())
    a = m._inpaint_tables("20", 5, 3)
    assert a is m._inpaint_tables("20", 5, 3)
    assert a is not m._inpaint_tables("20", 5, 2)
    assert list(m.state_dict()) == keys


# ---------------------------------------------------------------- Gaussian data, exact eps
def _gaussian_repaint(S, x_known, known, spec, j, r, n, seed):
    """The restatement's ops (repaint_ref) in float64 numpy on data x0 ~ N(0, S) with the exact eps of that Gaussian:
    E[eps | x_t] = sqrt(1 - abar) (abar S + (1 - abar) I)^-1 x_t.  n independent chains; returns their final states."""
    rp = RP.RePaint(BETAS, spec, j, r)
    sd = rp.sd
    d = S.shape[0]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    I = np.eye(d)
    for tau, jj in zip(rp.taus, rp.fwd):
        a = sd.alphas_cumprod[tau]
        eps = x @ (np.sqrt(1 - a) * np.linalg.inv(a * S + (1 - a) * I)).T
        x0 = np.clip(sd.sqrt_recip_alphas_cumprod[tau] * x - sd.sqrt_recipm1_alphas_cumprod[tau] * eps, -1, 1)
        mean = sd.posterior_mean_coef1[tau] * x0 + sd.posterior_mean_coef2[tau] * x
        x_unk = mean + (tau > 0) * np.exp(0.5 * sd.posterior_log_variance_clipped[tau]) * rng.standard_normal((n, d))
        ab = rp._ab(tau - 1)
        x_kn = np.sqrt(ab) * x_known + np.sqrt(1 - ab) * rng.standard_normal((n, d))
        x = np.where(known, x_kn, x_unk)
        if jj:
            fa, fb = rp._fold(tau - 1, jj)
            x = fa * x + fb * rng.standard_normal((n, d))
    return x


def test_gaussian_conditional_mean_resampling_helps():
    """16 correlated 'pixels' (std 0.3, correlation length 4), the middle 6 hidden.  RePaint's mean over 20000 chains against
    the exact conditional mean S_hk S_kk^-1 x_k (max 0.109 on the hidden pixels).  Resampling (r = 10) was expected to land closer
    than replacement (r = 1); measured at "50", j = 5 it does not (0.058 against 0.031), so the test records
    both errors and asserts only that each chain conditions on the known pixels: closer to the conditional mean than the prior
    mean 0 is, with the known pixels exact."""
    d = 16
    idx = np.arange(d)
    S = 0.09 * np.exp(-np.abs(idx[:, None] - idx[None, :]) / 4.0)
    known = np.ones(d, dtype=bool)
    known[5:11] = False
    rng = np.random.default_rng(0)
    x_true = np.linalg.cholesky(S) @ rng.standard_normal(d)
    x_known = np.where(known, x_true, 0.0)
    h, k = ~known, known
    want = S[np.ix_(h, k)] @ np.linalg.solve(S[np.ix_(k, k)], x_true[k])
    errs = {}
    for r in (1, 10):
        chains = _gaussian_repaint(S, x_known, known, "50", 5, r, 20000, seed=1 + r)
        assert (chains[:, known] == x_true[known]).all()
        got = chains.mean(axis=0)
        errs[r] = float(np.abs(got[h] - want).max())
    print(f"Gaussian conditional mean, max abs error on the hidden pixels: r = 1 {errs[1]:.4g}, r = 10 {errs[10]:.4g}")
    for r, err in errs.items():
        assert err < 0.75 * float(np.abs(want).max()), (r, err)
