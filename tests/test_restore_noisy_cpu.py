"""DDNM+ for a noisy measurement (DDPM.restore_noisy, DownsampleDDPM.restore_noisy, ddk_sampler_run_restore_noisy) on the CPU: the
properties of the two per-row tables lam and sgm, every argument error before any device work, sigma_y = 0 handed to restore, the
library's tables against the restatement's (tests/restore_noisy_ref.py), the restatement's conditional mean on Gaussian data with the
exact eps and a noisy measurement, and the header, the ctypes signatures, the built library and the host-side workspace and
eligibility queries on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import restore_masked_ref as RM
import restore_noisy_ref as RN
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import respace
from ddk import lib as L
from oracle import diffusion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = D.beta_schedule("linear", 1000)
NEW = ("ddk_p_sample_update_restore_noisy", "ddk_sampler_restore_noisy_workspace_bytes", "ddk_sampler_restore_noisy_tail_parts",
       "ddk_sampler_run_restore_noisy")
# the four table sets of tests/test_restore_cpu.py
TABLE_SETS = [dict(respacing=None), dict(respacing="20"), dict(respacing="20", ddim=True), dict(respacing="ddim50", ddim=True, eta=0.7)]
SIGMAS = (0.0, 0.05, 0.5)


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


# ---------------------------------------------------------------- the tables
def _f64(m, kw):
    """float64 (c1, s with row 0 zeroed) of a table set: c1 from the float64 schedule, s the fp32 sigma the kernels apply, widened"""
    ddim, eta = kw.get("ddim", False), kw.get("eta", 0.0)
    if kw["respacing"] is None and not ddim:
        c1 = respace.schedule_arrays(m._betas64)["posterior_mean_coef1"]
    else:
        sched, _ = respace._respaced_schedule(m._betas64, kw["respacing"])
        c1 = respace.ddim_coefficients(sched["alphas_cumprod"], eta)[0] if ddim else sched["posterior_mean_coef1"]
    return np.asarray(c1, dtype=np.float64)


@pytest.mark.parametrize("kw", TABLE_SETS)
def test_table_properties(kw):
    m = _tiny()
    ddim, eta = kw.get("ddim", False), kw.get("eta", 0.0)
    c1 = _f64(m, kw)
    prev = None
    for sy in SIGMAS:
        tab, _ = m._noisy_tables(kw["respacing"], ddim, eta, sy)
        assert tab["lam"].dtype == tab["sgm"].dtype == torch.float32 and tab["lam"].shape == tab["sgm"].shape == tab["c1"].shape
        s32 = tab["sigma"].clone()
        s32[0] = 0.0
        s = s32.double().numpy()
        lam64, sgm64 = respace.noisy_coefficients(c1, tab["sigma"].double().numpy(), sy)
        assert torch.equal(tab["lam"], torch.tensor(lam64, dtype=torch.float32)) and torch.equal(tab["sgm"], torch.tensor(sgm64, dtype=torch.float32))
        assert (lam64 >= 0).all() and (lam64 <= 1).all()
        assert lam64[0] == 0 and sgm64[0] == 0 and float(tab["lam"][0]) == 0 and float(tab["sgm"][0]) == 0
        if sy == 0:
            assert (lam64[1:] == 1).all() and torch.equal(tab["lam"][1:], torch.ones(len(s) - 1))
            assert torch.equal(tab["sgm"], s32)                        # bit for bit the fp32 sigma
        one = lam64 == 1
        total = (c1 * lam64 * sy) ** 2 + sgm64 ** 2
        assert np.allclose(total[one], s[one] ** 2, rtol=16 * np.finfo(np.float64).eps, atol=0)
        assert (sgm64[~one] == 0).all()
        # where lam < 1 the measurement's share alone is the whole variance
        part = ~one & (np.arange(len(s)) > 0)
        assert np.allclose(np.abs(c1[part]) * lam64[part] * sy, s[part], rtol=16 * np.finfo(np.float64).eps, atol=0)
        if prev is not None:
            assert (lam64 <= prev).all()                               # non-increasing in sigma_y
        prev = lam64
    assert (prev[1:] < 1).any()                                        # sigma_y = 0.5 bites somewhere in every set


@pytest.mark.parametrize("kw", [dict(), dict(ddim=True, eta=0.5)])
@pytest.mark.parametrize("sy", [0.05, 0.5])
def test_library_tables_agree_with_the_restatement(kw, sy):
    """two derivations (the library's c1 / c2 tables, the restatement's from the direct DDIM form) of "8" rows: the same to fp32 rounding"""
    tab, use = _tiny()._noisy_tables("8", kw.get("ddim", False), kw.get("eta", 0.0), sy)
    chain = RN.RestoreNoisy(BETAS, "8")
    ref = chain.tables(sy, **kw)
    assert list(use) == chain.sd.timestep_map
    for name in ("c1", "c2", "lam", "sgm"):
        assert torch.allclose(tab[name], ref[name], rtol=1e-5, atol=1e-7), name
    assert torch.allclose(tab["sigma"][1:], ref["sigma"][1:], rtol=1e-6, atol=0)


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
@pytest.mark.parametrize("sy", [-0.1, float("nan"), float("inf"), "0.1", None, True, [0.1], torch.tensor(0.1), 1j])
def test_bad_sigma_y_raises(sy):
    with pytest.raises(ValueError):
        _tiny().restore_noisy(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, sigma_y=sy)
    with pytest.raises(ValueError):
        _dd().restore_noisy(torch.zeros(1, 3, 32, 32), _half(32, 32), 1, sigma_y=sy)


def test_sigma_y_is_required():
    with pytest.raises(TypeError):
        _tiny().restore_noisy(torch.zeros(2, 3, 16, 16), _half(16, 16), 1)


@pytest.mark.parametrize("kw", [dict(solver="dpm++2m"), dict(noise=torch.zeros(1)), dict(early_stop=10), dict(jump_length=3),
                                dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(paste=True)])
@pytest.mark.parametrize("sy", [0.0, 0.1])
def test_rejected_keywords_raise(kw, sy):
    with pytest.raises(ValueError):
        _tiny().restore_noisy(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, sigma_y=sy, **kw)
    with pytest.raises(ValueError):
        _dd().restore_noisy(torch.zeros(1, 3, 32, 32), _half(32, 32), 1, sigma_y=sy, **kw)


@pytest.mark.parametrize("kw", [dict(ddim=True), dict(ddim=True, eta=0.0), dict(respacing="20", ddim=True)])
def test_a_chain_without_draws_is_rejected(kw):
    with pytest.raises(ValueError, match="eta"):
        _tiny().restore_noisy(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, sigma_y=0.1, **kw)
    with pytest.raises(ValueError, match="eta"):
        _dd().restore_noisy(torch.zeros(1, 3, 32, 32), _half(32, 32), 1, sigma_y=0.1, **kw)
    with pytest.raises(L.DDKError):                                    # sigma_y = 0 is restore, which takes eta = 0
        _tiny().restore_noisy(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, sigma_y=0.0, **kw)


@pytest.mark.parametrize("y,mask,scale", [
    (torch.zeros(2, 3, 16, 16), None, 1),                               # scale 1 without a mask
    (torch.zeros(2, 3, 8, 8), torch.ones(8, 8), 3), (torch.zeros(2, 3, 8, 8), torch.ones(8, 8), 2.0),
    (torch.zeros(2, 3, 8, 8), torch.ones(8, 8), True),                  # bad scales
    (torch.zeros(2, 3, 16, 16), torch.full((16, 16), 0.5), 1), (torch.zeros(2, 3, 16, 16), torch.zeros(16, 16), 1),
    (torch.zeros(2, 3, 16, 16), torch.stack([torch.ones(16, 16), torch.zeros(16, 16)]), 1),
    (torch.zeros(2, 3, 16, 16), torch.ones(2, 3, 16, 16), 1), (torch.zeros(2, 3, 16, 16), [[1.0]], 1),      # bad masks
    (torch.zeros(2, 3, 8, 8), _half(16, 16), 1), (torch.zeros(2, 1, 16, 16), _half(16, 16), 1),
    (torch.zeros(2, 3, 16, 16, dtype=torch.long), _half(16, 16), 1), ([[0.0]], _half(16, 16), 1),
    (torch.zeros(2, 3, 16, 16), _half(8, 8), 2),                        # misshapen y
    (torch.full((2, 3, 8, 8), float("inf")), None, 2),                  # not finite
])
def test_restores_value_errors_are_raised(y, mask, scale):
    with pytest.raises(ValueError):
        _tiny().restore_noisy(y, mask, scale, sigma_y=0.1)


def test_non_finite_measured_pixels_raise_and_hidden_ones_do_not():
    y = torch.zeros(2, 3, 16, 16)
    y[0, 1, 3, 2] = float("nan")                       # measured (left half)
    with pytest.raises(ValueError):
        _tiny().restore_noisy(y, _half(16, 16), 1, sigma_y=0.1)
    y = torch.zeros(2, 3, 16, 16)
    y[0, 1, 3, 12] = float("nan")                      # hidden: never read, so the first complaint is the missing device
    with pytest.raises(L.DDKError):
        _tiny().restore_noisy(y, _half(16, 16), 1, sigma_y=0.1)


@pytest.mark.parametrize("mask,scale,kw", [
    (_half(16, 16), 1, dict(respacing="20", ddim=True, eta=0.5, seed=1)),
    (_half(16, 16).bool(), 1, {}),
    (_half(16, 16).expand(2, 1, 16, 16), 1, dict(respacing="20")),
    (_half(8, 8), 2, dict(respacing="20")),
    (None, 4, dict(respacing="20")),
    (_half(2, 2), 8, dict(sigma_y=2)),
])
def test_good_arguments_reach_the_device_check(mask, scale, kw):
    kw = dict(dict(sigma_y=0.1), **kw)
    with pytest.raises(L.DDKError):
        _tiny().restore_noisy(torch.zeros(2, 3, 16 // scale, 16 // scale), mask, scale, **kw)


@pytest.mark.parametrize("y,mask,scale", [
    (torch.zeros(1, 8, 8, 8), torch.ones(8, 8), 1), (torch.zeros(1, 3, 32, 32), torch.eye(32), 1),
    (torch.zeros(1, 3, 8, 8), torch.ones(8, 8), 3), (torch.zeros(1, 3, 16, 16), torch.ones(16, 16), 2),
    (torch.zeros(1, 3, 8, 8), None, 4),                                 # one latent pixel per measurement and no mask
])
def test_dddpm_bad_arguments_raise(y, mask, scale):
    with pytest.raises(ValueError):
        _dd().restore_noisy(y, mask, scale, sigma_y=0.1)


@pytest.mark.parametrize("y,mask,scale", [(torch.zeros(1, 3, 32, 32), _half(32, 32), 1), (torch.zeros(1, 3, 8, 8), _half(8, 8), 4),
                                          (torch.zeros(1, 3, 4, 4), None, 8)])
def test_dddpm_good_arguments_reach_the_device_check(y, mask, scale):
    with pytest.raises(L.DDKError):
        _dd().restore_noisy(y, mask, scale, sigma_y=0.1, respacing="10", ddim=True, eta=0.5)


def test_sigma_y_zero_dispatches_to_restore(monkeypatch):
    calls = []

    def fake(self, y, mask=None, scale=1, **kw):
        calls.append((y, mask, scale, kw))
        return "restored"

    monkeypatch.setattr(DDPM, "restore", fake)
    y, mk, x_T = torch.zeros(2, 3, 8, 8), _half(8, 8), torch.zeros(2, 3, 16, 16)
    for zero in (0, 0.0, np.float32(0)):
        assert _tiny().restore_noisy(y, mk, 2, sigma_y=zero, respacing="20", ddim=True, eta=0.3, x_T=x_T, seed=4) == "restored"
    assert len(calls) == 3
    got = calls[0]
    assert got[0] is y and got[1] is mk and got[2] == 2
    assert got[3] == dict(respacing="20", ddim=True, eta=0.3, x_T=x_T, seed=4)
    calls.clear()
    monkeypatch.setattr(DownsampleDDPM, "restore", fake)
    assert _dd().restore_noisy(torch.zeros(1, 3, 8, 8), _half(8, 8), 4, sigma_y=0) == "restored"
    assert calls[0][3]["paste"] is False                               # a noisy entry never pastes
    calls.clear()
    with pytest.raises(L.DDKError):                                    # sigma_y > 0 does not go through restore
        _tiny().restore_noisy(y, mk, 2, sigma_y=0.1)
    assert not calls


def test_the_older_entries_keep_their_signatures_and_errors():
    import inspect
    m = _tiny()
    for name in ("restore", "super_resolve", "inpaint", "restore_solver"):
        assert "sigma_y" not in inspect.signature(getattr(DDPM, name)).parameters
        assert "sigma_y" not in inspect.signature(getattr(DownsampleDDPM, name)).parameters
    with pytest.raises(ValueError):
        m.restore(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, sigma_y=0.1)
    with pytest.raises(ValueError):
        m.restore_solver(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, sigma_y=0.1)
    with pytest.raises(ValueError):
        m.super_resolve(torch.zeros(2, 3, 4, 4), 4, sigma_y=0.1)
    assert "paste" not in inspect.signature(DownsampleDDPM.restore_noisy).parameters


# ---------------------------------------------------------------- the restatement's identities
def _toy_eps(x, t):
    return 0.3 * x + 0.1 * torch.roll(x, 1, dims=3) - 0.05 * t.reshape(-1, 1, 1, 1).float() / 1000.0


@pytest.mark.parametrize("n", [1, 2])
def test_restatement_never_uses_unmeasured_y_and_lam_one_is_ddnm(n):
    g = torch.Generator().manual_seed(n)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.rand(2, 3, 8 // n, 8 // n, generator=g) * 2 - 1
    mk = (torch.rand(2, 8 // n, 8 // n, generator=g) < 0.5).float()
    sel = (mk != 0).unsqueeze(1).expand_as(y)
    chain = RN.RestoreNoisy(BETAS, "10")
    a = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.zeros_like(y)), mk, n, 0.2, 9)
    b = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.full_like(y, float("nan"))), mk, n, 0.2, 9)
    assert torch.isfinite(b).all() and torch.equal(a, b)
    # one step with lam = 1 and sgm = sigma is the masked DDNM step (n >= 2: operation for operation; n = 1: x0 + (y - x0), within 2^-23 of y)
    x, e, z = (torch.randn(2, 3, 8, 8, generator=g) for _ in range(3))
    co = {k: torch.rand(2, generator=g) for k in ("cr", "crm1", "c1", "c2", "sg")}
    got = RN.step(x, e, y, mk, n, co["cr"], co["crm1"], co["c1"], co["c2"], co["sg"], torch.ones(2), co["sg"], z)
    want = RM.step(x, e, torch.where(sel, y, torch.zeros_like(y)), mk, n, co["cr"], co["crm1"], co["c1"], co["c2"], co["sg"], z)
    if n >= 2:
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 4 * 2.0 ** -23


# ---------------------------------------------------------------- Gaussian data, exact eps, a noisy measurement
def test_gaussian_posterior_mean_with_a_noisy_measurement():
    """The toy problem of tests/test_restore_masked_cpu.py: 16 correlated 'pixels' (std 0.3, correlation length 4), the middle 6
    hidden, the exact eps of that Gaussian; the 10 known pixels are measured with noise, y = clean + 0.1 n.  The exact answer is the
    posterior mean given the NOISY measurement, S_hk (S_kk + sigma_y^2 I)^-1 y_k.  The restatement's DDNM+ chain runs at "50",
    ancestral, 20000 chains as the batch; the bar, as there: the error of the chains' mean on the hidden pixels is below the prior
    mean's (max |posterior mean|).  Plain DDNM on the same noisy y (which takes y for exact) is printed beside it; no order between
    the two is asserted.  Measured: see DESIGN.md section 3.10."""
    d, sy = 16, 0.1
    idx = np.arange(d)
    S = 0.09 * np.exp(-np.abs(idx[:, None] - idx[None, :]) / 4.0)
    known = np.ones(d, dtype=bool)
    known[5:11] = False
    rng = np.random.default_rng(0)
    x_true = np.linalg.cholesky(S) @ rng.standard_normal(d)
    y_noisy = x_true + sy * np.random.default_rng(5).standard_normal(d)
    h, k = ~known, known
    want = S[np.ix_(h, k)] @ np.linalg.solve(S[np.ix_(k, k)] + sy ** 2 * np.eye(int(k.sum())), y_noisy[k])
    want_k = S[np.ix_(k, k)] @ np.linalg.solve(S[np.ix_(k, k)] + sy ** 2 * np.eye(int(k.sum())), y_noisy[k])
    prior_err = float(np.abs(want).max())
    acp = np.cumprod(1.0 - np.asarray(BETAS, dtype=np.float64))
    I = np.eye(d)

    def eps_model(x, t):
        a = acp[int(t[0])]
        M = np.sqrt(1 - a) * np.linalg.inv(a * S + (1 - a) * I)
        return torch.from_numpy(x.double().numpy().reshape(-1, d) @ M.T).float().reshape(x.shape)

    n = 20000
    y = torch.from_numpy(np.where(known, y_noisy, np.nan)).float().reshape(1, 1, 1, d).expand(n, 1, 1, d).contiguous()
    mk = torch.from_numpy(known.astype(np.float32)).reshape(1, 1, d).expand(n, 1, d).contiguous()
    x_T = lambda: torch.from_numpy(np.random.default_rng(7).standard_normal((n, 1, 1, d))).float()
    plus = RN.RestoreNoisy(BETAS, "50").run(eps_model, x_T(), y, mk, 1, sy, seed=11).reshape(n, d).double().numpy()
    plain = RM.RestoreMasked(BETAS, "50").run(eps_model, x_T(), y, mk, 1, seed=11).reshape(n, d).double().numpy()
    assert np.isfinite(plus).all()
    err_plus = float(np.abs(plus.mean(axis=0)[h] - want).max())
    err_plain = float(np.abs(plain.mean(axis=0)[h] - want).max())
    # on the measured pixels: plain DDNM returns the noisy y; DDNM+ returns the model's x0, whose mean is compared with the posterior's
    kn_plus = float(np.abs(plus.mean(axis=0)[k] - want_k).max())
    kn_plain = float(np.abs(plain.mean(axis=0)[k] - want_k).max())
    print(f"Gaussian posterior mean with sigma_y = {sy}, max abs error on the hidden pixels: DDNM+ {err_plus:.4g}, plain DDNM on the same "
          f"noisy y {err_plain:.4g} (prior mean {prior_err:.4g}); on the measured pixels: DDNM+ {kn_plus:.4g}, plain DDNM {kn_plain:.4g}")
    assert err_plus < prior_err, (err_plus, prior_err)


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_noisy"][1]) == 20
    assert len(L.SIGNATURES["ddk_sampler_run_restore_noisy"][1]) == 8
    assert len(L.SIGNATURES["ddk_sampler_restore_noisy_workspace_bytes"][1]) == 6
    assert L.load().ddk_version() == L.ABI_VERSION == 400


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only.  The workspace is the masked chain's, byte for byte, for every n; the fused tail's eligibility is the
    masked kind's: n = 1 wherever the plain kinds with at most 128 channels are, n >= 2 where the tile holds whole rows of blocks;
    the option that switches the restore tails off switches this one off."""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 8, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    B, S = 32, 32
    for n in (1, 2, 4, 8):
        assert lib.ddk_sampler_restore_noisy_workspace_bytes(h, B, S, S, 49, n) == lib.ddk_sampler_restore_masked_workspace_bytes(h, B, S, S, 49, n) > 0
    assert lib.ddk_sampler_restore_noisy_workspace_bytes(h, B, S, S, 49, 3) == 0
    assert lib.ddk_sampler_restore_noisy_workspace_bytes(h, B, 30, S, 49, 1) == 0
    parts = {n: lib.ddk_sampler_restore_noisy_tail_parts(h, B, S, S, n) for n in (1, 2, 4, 8)}
    assert parts == {n: lib.ddk_sampler_restore_masked_tail_parts(h, B, S, S, n) for n in (1, 2, 4, 8)} == {1: 8, 2: 8, 4: 8, 8: 0}
    assert lib.ddk_sampler_restore_noisy_tail_parts(h, B, S, S, 3) < 0
    assert lib.ddk_sampler_restore_noisy_tail_parts(h, B, 64, 64, 4) == 0
    assert lib.ddk_unet_set_option(h, 12, 0) == 0
    assert lib.ddk_sampler_restore_noisy_tail_parts(h, B, S, S, 1) == 0 and lib.ddk_sampler_restore_noisy_tail_parts(h, B, S, S, 2) == 0
    assert lib.ddk_unet_set_option(h, 12, 1) == 0
    u256 = Unet(ddpm_cfg(256, 8, 32))
    u256.flops(1, 32, 32)
    assert lib.ddk_sampler_restore_noisy_tail_parts(u256._plan.handle, B, S, S, 1) == 0
