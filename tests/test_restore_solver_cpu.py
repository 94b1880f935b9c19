"""DDNM on the DPM-Solver++(2M) chain (DDPM.restore_solver, DownsampleDDPM.restore_solver, ddk_sampler_run_restore_multistep) on
the CPU: the tables' first and last rows, every argument error before any device work, the restatement
(tests/restore_solver_ref.py) holding A x = y, reducing to the plain 2M chain under a mask that measures nothing and to DDNM on
DDIM eta 0 at order 1, its conditional mean on Gaussian data with the exact eps, and the C ABI of the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dpm_solver_ref as DR
import restore_ref as RR
import restore_solver_ref as RS
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import respace
from ddk import lib as L
from oracle import diffusion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = D.beta_schedule("linear", 1000)
NEW = ("ddk_p_sample_update_restore_multistep", "ddk_sampler_restore_multistep_workspace_bytes",
       "ddk_sampler_restore_multistep_tail_parts", "ddk_sampler_run_restore_multistep")


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


def _dd():
    cfg = dddpm_cfg(32, 32, 2)
    return DownsampleDDPM(cfg, Unet(cfg), "cpu", 3)


def _half(h, w):
    m = torch.ones(h, w)
    m[:, w // 2:] = 0
    return m


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("spec", ["logsnr6", "logsnr8", "logsnr20"])
@pytest.mark.parametrize("order", [1, 2])
def test_first_and_last_rows_are_first_order_and_row_0_returns_x0(spec, order):
    tab, use = respace.dpm_solver_tables(BETAS, spec, order=order)
    K = len(use)
    assert float(tab["c3"][0]) == 0.0 and float(tab["c3"][K - 1]) == 0.0
    assert tab["c1"].dtype == torch.float32 and float(tab["c1"][0]) == 1.0 and float(tab["c2"][0]) == 0.0


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
@pytest.mark.parametrize("kw", [dict(solver="dpm++3m"), dict(solver=None), dict(order=3), dict(order=0), dict(order=2.0), dict(order=True),
                                dict(ddim=True), dict(eta=0.5), dict(seed=1), dict(noise=torch.zeros(1)), dict(early_stop=10),
                                dict(jump_length=3)])
def test_rejected_keywords_raise(kw):
    with pytest.raises(ValueError):
        _tiny().restore_solver(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, **kw)
    with pytest.raises(ValueError):
        _dd().restore_solver(torch.zeros(1, 3, 32, 32), _half(32, 32), 1, **kw)


def test_the_errors_of_restore_are_raised_here_too():
    m = _tiny()
    with pytest.raises(ValueError):
        m.restore_solver(torch.zeros(2, 3, 16, 16))                                    # scale 1 without a mask
    for scale in (0, 3, 16, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            m.restore_solver(torch.zeros(2, 3, 8, 8), torch.ones(8, 8), scale)
    for mask in (torch.full((16, 16), 0.5), torch.zeros(16, 16), torch.stack([torch.ones(16, 16), torch.zeros(16, 16)]),
                 torch.ones(2, 3, 16, 16), torch.ones(8, 16), [[1.0]]):
        with pytest.raises(ValueError):
            m.restore_solver(torch.zeros(2, 3, 16, 16), mask, 1)
    for y, scale in ((torch.zeros(2, 3, 8, 8), 1), (torch.zeros(3, 16, 16), 1), (torch.zeros(2, 3, 16, 16, dtype=torch.long), 1),
                     (torch.zeros(2, 3, 16, 16), 2)):
        with pytest.raises(ValueError):
            m.restore_solver(y, _half(16 // scale, 16 // scale), scale)
    y = torch.zeros(2, 3, 16, 16)
    y[0, 1, 3, 2] = float("nan")                       # measured (left half)
    with pytest.raises(ValueError):
        m.restore_solver(y, _half(16, 16), 1)
    with pytest.raises(ValueError):
        m.restore_solver(torch.full((2, 3, 8, 8), float("inf")), None, 2)
    d = _dd()
    for y, mask, scale in ((torch.zeros(1, 8, 8, 8), torch.ones(8, 8), 1), (torch.zeros(1, 3, 32, 32), torch.eye(32), 1),
                           (torch.zeros(1, 3, 8, 8), torch.ones(8, 8), 3), (torch.zeros(1, 3, 8, 8), None, 4),
                           (torch.zeros(1, 3, 1, 1), torch.ones(1, 1), 64)):
        with pytest.raises(ValueError):
            d.restore_solver(y, mask, scale)


@pytest.mark.parametrize("mask,scale,kw", [
    (_half(16, 16), 1, dict(respacing="logsnr8")),
    (_half(16, 16).bool(), 1, dict(respacing="logsnr8", order=1)),
    (_half(16, 16).expand(2, 1, 16, 16), 1, dict(respacing="20", solver="dpm++2m", order=2)),
    (_half(8, 8), 2, dict(respacing="logsnr8")),
    (None, 4, dict(respacing="logsnr8")),
    (_half(2, 2), 8, {}),
])
def test_good_arguments_reach_the_device_check(mask, scale, kw):
    """everything valid: the first complaint is the missing device, not an argument (hidden NaN included)"""
    y = torch.zeros(2, 3, 16 // scale, 16 // scale)
    if mask is not None:
        y[0, 1, 0, -1] = float("nan")                  # hidden by every mask above: never read
    with pytest.raises(L.DDKError):
        _tiny().restore_solver(y, mask, scale, **kw)


@pytest.mark.parametrize("y,mask,scale", [(torch.zeros(1, 3, 32, 32), _half(32, 32), 1), (torch.zeros(1, 3, 8, 8), _half(8, 8), 4),
                                          (torch.zeros(1, 3, 4, 4), _half(4, 4), 8), (torch.zeros(1, 3, 4, 4), None, 8)])
def test_dddpm_good_arguments_reach_the_device_check(y, mask, scale):
    with pytest.raises(L.DDKError):
        _dd().restore_solver(y, mask, scale, respacing="logsnr8", paste=False)


def test_the_older_entries_still_reject_a_solver():
    m = _tiny()
    for call in (lambda: m.restore(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, solver="dpm++2m"),
                 lambda: m.super_resolve(torch.zeros(2, 3, 4, 4), 4, solver="dpm++2m"),
                 lambda: m.inpaint(torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16), solver="dpm++2m")):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------- the restatement's identities
def _toy_eps(x, t):
    return 0.3 * x + 0.1 * torch.roll(x, 1, dims=3) - 0.05 * t.reshape(-1, 1, 1, 1).float() / 1000.0


@pytest.mark.parametrize("order", [1, 2])
def test_the_restatement_ends_with_the_constraint_and_never_reads_hidden_y(order):
    g = torch.Generator().manual_seed(3 + order)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.rand(2, 3, 8, 8, generator=g) * 2 - 1
    mk = (torch.rand(2, 8, 8, generator=g) < 0.5).float()
    sel = (mk != 0).unsqueeze(1).expand_as(y)
    chain = RS.RestoreSolver(BETAS, "logsnr8", order)
    zeroed = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.zeros_like(y)), mk, 1)
    assert torch.equal(zeroed[sel], y[sel]) and not torch.equal(zeroed[~sel], y[~sel])         # exact at n = 1
    poisoned = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.full_like(y, float("nan"))), mk, 1)
    assert torch.isfinite(poisoned).all() and torch.equal(poisoned, zeroed)
    for n in (2, 4):
        yn = RR.pool(y, n)
        mkn = (torch.rand(2, 8 // n, 8 // n, generator=g) < 0.5).float()
        mkn[:, 0, 0] = 1
        seln = (mkn != 0).unsqueeze(1).expand_as(yn)
        a = chain.run(_toy_eps, x_T, torch.where(seln, yn, torch.zeros_like(yn)), mkn, n)
        b = chain.run(_toy_eps, x_T, torch.where(seln, yn, torch.full_like(yn, float("nan"))), mkn, n)
        assert torch.isfinite(b).all() and torch.equal(a, b)
        assert float((RR.pool(a.double(), n) - yn.double())[seln].abs().max()) <= 8 * n * n * 2.0 ** -24     # section 3.6's bound
        full = chain.run(_toy_eps, x_T, yn, None, n)
        assert float((RR.pool(full.double(), n) - yn.double()).abs().max()) <= 8 * n * n * 2.0 ** -24
        assert torch.equal(full, chain.run(_toy_eps, x_T, yn, torch.ones(2, 8 // n, 8 // n), n))


@pytest.mark.parametrize("n", [1, 2])
def test_a_mask_that_measures_nothing_is_the_plain_2m_chain_bit_for_bit(n):
    g = torch.Generator().manual_seed(n)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.full((2, 3, 8 // n, 8 // n), float("nan"))
    want = DR.DPMSolver(BETAS, "logsnr8").run(_toy_eps, x_T)
    assert torch.equal(RS.RestoreSolver(BETAS, "logsnr8").run(_toy_eps, x_T, y, torch.zeros(2, 8 // n, 8 // n), n), want)


@pytest.mark.parametrize("n,masked", [(1, True), (2, True), (2, False)])
def test_order_1_is_ddnm_on_ddim_eta_0(n, masked):
    """the two restatements state the step in different forms (the solver's direct form with fp32-cast float64 coefficients; DDIM
    through eps): 8 steps of a contractive toy model, each a handful of fp32 roundings of O(1) values -- 1e-5 abs"""
    g = torch.Generator().manual_seed(10 + n)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.rand(2, 3, 8 // n, 8 // n, generator=g) * 2 - 1
    mk = (torch.rand(2, 8 // n, 8 // n, generator=g) < 0.5).float() if masked else None
    got = RS.RestoreSolver(BETAS, "logsnr8", order=1).run(_toy_eps, x_T, y, mk, n)
    want = RS.masked_chain(BETAS, "logsnr8").run(_toy_eps, x_T, y, mk, n, seed=1, ddim=True, eta=0.0)
    assert float((got - want).abs().max()) < 1e-5
    two = RS.RestoreSolver(BETAS, "logsnr8", order=2).run(_toy_eps, x_T, y, mk, n)
    assert float((two - want).abs().max()) > 1e-4                                             # the history term is really there


def test_the_two_restatements_share_the_grid():
    assert RS.RestoreSolver(BETAS, "logsnr8").timestep_map == RS.masked_chain(BETAS, "logsnr8").sd.timestep_map
    assert RS.RestoreSolver(BETAS, "logsnr8").timestep_map == respace.dpm_solver_tables(BETAS, "logsnr8")[1]


# ---------------------------------------------------------------- Gaussian data, exact eps
def test_gaussian_conditional_mean():
    """The toy problem of tests/test_restore_masked_cpu.py: 16 correlated 'pixels' (std 0.3, correlation length 4), the middle 6
    hidden, the exact eps of that Gaussian.  The restatement's chain at "logsnr20" (20 forwards), 20000 x_T draws as the batch; the
    mean over the draws against the exact conditional mean S_hk S_kk^-1 x_k on the hidden pixels.  The bar, the only order
    asserted: below the prior mean's error (0.109), computed here.  The measured pixels are exact.  Measured values: DESIGN.md
    section 3.9."""
    d = 16
    idx = np.arange(d)
    S = 0.09 * np.exp(-np.abs(idx[:, None] - idx[None, :]) / 4.0)
    known = np.ones(d, dtype=bool)
    known[5:11] = False
    rng = np.random.default_rng(0)
    x_true = np.linalg.cholesky(S) @ rng.standard_normal(d)
    h, k = ~known, known
    want = S[np.ix_(h, k)] @ np.linalg.solve(S[np.ix_(k, k)], x_true[k])
    prior_err = float(np.abs(want).max())
    assert abs(prior_err - 0.109) < 1e-3
    acp = np.cumprod(1.0 - np.asarray(BETAS, dtype=np.float64))
    I = np.eye(d)

    def eps_model(x, t):
        a = acp[int(t[0])]
        M = np.sqrt(1 - a) * np.linalg.inv(a * S + (1 - a) * I)
        return torch.from_numpy(x.double().numpy().reshape(-1, d) @ M.T).float().reshape(x.shape)

    n = 20000
    y = torch.from_numpy(np.where(known, x_true, np.nan)).float().reshape(1, 1, 1, d).expand(n, 1, 1, d).contiguous()
    mk = torch.from_numpy(known.astype(np.float32)).reshape(1, 1, d).expand(n, 1, d).contiguous()
    errs = {}
    for name, order in (("2M", 2), ("order 1", 1)):
        x_T = torch.from_numpy(np.random.default_rng(7).standard_normal((n, 1, 1, d))).float()
        out = RS.RestoreSolver(BETAS, "logsnr20", order).run(eps_model, x_T, y, mk, 1).reshape(n, d).double().numpy()
        assert (out[:, known] == y.reshape(n, d).numpy()[:, known]).all()
        errs[name] = float(np.abs(out.mean(axis=0)[h] - want).max())
    print("Gaussian conditional mean at logsnr20, max abs error on the hidden pixels: " + ", ".join(f"{k} {v:.4g}" for k, v in errs.items()) +
          f" (prior mean {prior_err:.4g})")
    assert errs["2M"] < prior_err, errs


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_multistep"][1]) == 17
    assert len(L.SIGNATURES["ddk_sampler_run_restore_multistep"][1]) == 7
    assert len(L.SIGNATURES["ddk_sampler_restore_multistep_workspace_bytes"][1]) == 6


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only.  The workspace: the sampler layout, the history (a whole latent), then y and the mask for this n; the
    queries of the merged chains are unchanged.  The fused tail: as the masked kind's (n = 1 wherever the plain kinds with at most
    128 channels are, n >= 2 with whole rows of blocks per tile), off with DDK_OPT_RESTORE_FUSED_TAIL = 0."""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 8, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    B, S, Cl = 32, 32, 8
    lat, pix = B * S * S * Cl * 4, B * S * S * 4          # bytes
    plain = lib.ddk_sampler_workspace_bytes(h, B, S, S, 19)
    assert lib.ddk_sampler_multistep_workspace_bytes(h, B, S, S, 19) == plain + lat
    assert lib.ddk_sampler_restore_masked_workspace_bytes(h, B, S, S, 19, 1) == plain + lat + pix
    q = {n: lib.ddk_sampler_restore_multistep_workspace_bytes(h, B, S, S, 19, n) for n in (1, 2, 4, 8)}
    assert q == {n: plain + lat + lat // (n * n) + pix // (n * n) for n in (1, 2, 4, 8)}
    assert lib.ddk_sampler_restore_multistep_workspace_bytes(h, B, S, S, 19, 3) == 0
    assert lib.ddk_sampler_restore_multistep_workspace_bytes(h, B, 30, S, 19, 1) == 0
    parts = {n: lib.ddk_sampler_restore_multistep_tail_parts(h, B, S, S, n) for n in (1, 2, 4, 8)}
    assert parts == {1: 8, 2: 8, 4: 8, 8: 0}
    assert parts == {n: lib.ddk_sampler_restore_masked_tail_parts(h, B, S, S, n) for n in (1, 2, 4, 8)}
    assert lib.ddk_sampler_restore_multistep_tail_parts(h, B, S, S, 3) < 0
    assert lib.ddk_sampler_restore_multistep_tail_parts(h, B, 64, 64, 4) == 0
    assert lib.ddk_unet_set_option(h, 12, 0) == 0
    assert [lib.ddk_sampler_restore_multistep_tail_parts(h, B, S, S, n) for n in (1, 2, 8)] == [0, 0, 0]
    assert lib.ddk_unet_set_option(h, 12, 1) == 0
    u256 = Unet(ddpm_cfg(256, 8, 32))
    u256.flops(1, 32, 32)
    assert lib.ddk_sampler_restore_multistep_tail_parts(u256._plan.handle, B, S, S, 1) == 0
