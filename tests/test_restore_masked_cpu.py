"""DDNM with a mask (DDPM.restore, DownsampleDDPM.restore, ddk_sampler_run_restore_masked) on the CPU: every argument error comes
before any device work, the restatement (tests/restore_masked_ref.py) reduces to tests/restore_ref.py for an all-measured mask,
returns measured pixels exactly at n = 1 and never uses what is not measured, its conditional mean on Gaussian data with the exact
eps is closer to the true conditional mean than the prior mean is, and the header, the ctypes signatures, the built library and
the host-side workspace and eligibility queries agree on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import restore_masked_ref as RM
import restore_ref as RR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from ddk import lib as L
from oracle import diffusion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = D.beta_schedule("linear", 1000)
NEW = ("ddk_p_sample_update_restore_masked", "ddk_sampler_restore_masked_workspace_bytes", "ddk_sampler_restore_masked_tail_parts",
       "ddk_sampler_run_restore_masked")


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


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
@pytest.mark.parametrize("kw", [dict(solver="dpm++2m"), dict(noise=torch.zeros(1)), dict(early_stop=10), dict(jump_length=3),
                                dict(eta=0.5), dict(ddim=True, eta=-1.0)])
def test_rejected_keywords_raise(kw):
    with pytest.raises(ValueError):
        _tiny().restore(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, **kw)
    with pytest.raises(ValueError):
        _dd().restore(torch.zeros(1, 3, 32, 32), _half(32, 32), 1, **kw)


def test_scale_1_without_a_mask_raises():
    with pytest.raises(ValueError):
        _tiny().restore(torch.zeros(2, 3, 16, 16))
    with pytest.raises(ValueError):
        _dd().restore(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        _dd().restore(torch.zeros(1, 3, 8, 8), None, 4)            # dim_reduc = 4: one latent pixel per measurement, as unconstrained


@pytest.mark.parametrize("scale", [0, 3, 16, 2.0, True, "2", None])
def test_bad_scale_raises(scale):
    with pytest.raises(ValueError):
        _tiny().restore(torch.zeros(2, 3, 8, 8), torch.ones(8, 8), scale)


@pytest.mark.parametrize("mask", [torch.full((16, 16), 0.5), torch.full((16, 16), float("nan")), torch.full((16, 16), -1.0),
                                  torch.zeros(16, 16),                                        # all zero
                                  torch.stack([torch.ones(16, 16), torch.zeros(16, 16)]),     # all zero in one image
                                  torch.ones(2, 3, 16, 16), torch.ones(3, 16, 16), torch.ones(8, 16), torch.ones(2, 1, 8, 8),
                                  torch.ones(1, 2, 1, 16, 16), [[1.0]]])
def test_bad_masks_raise(mask):
    with pytest.raises(ValueError):
        _tiny().restore(torch.zeros(2, 3, 16, 16), mask, 1)


@pytest.mark.parametrize("y,scale", [(torch.zeros(2, 3, 8, 8), 1), (torch.zeros(2, 1, 16, 16), 1), (torch.zeros(3, 16, 16), 1),
                                     (torch.zeros(2, 3, 16, 16, dtype=torch.long), 1), ([[0.0]], 1), (torch.zeros(2, 3, 16, 16), 2),
                                     (torch.zeros(2, 3, 4, 8), 4)])
def test_misshapen_y_raises(y, scale):
    h = 16 // scale
    with pytest.raises(ValueError):
        _tiny().restore(y, _half(h, h), scale)


def test_non_finite_measured_pixels_raise_and_hidden_ones_do_not():
    y = torch.zeros(2, 3, 16, 16)
    y[0, 1, 3, 2] = float("nan")                       # measured (left half)
    with pytest.raises(ValueError):
        _tiny().restore(y, _half(16, 16), 1)
    y = torch.zeros(2, 3, 16, 16)
    y[0, 1, 3, 12] = float("nan")                      # hidden: never read, so the first complaint is the missing device
    with pytest.raises(L.DDKError):
        _tiny().restore(y, _half(16, 16), 1)
    with pytest.raises(ValueError):
        _tiny().restore(torch.full((2, 3, 8, 8), float("inf")), None, 2)


@pytest.mark.parametrize("mask,scale,kw", [
    (_half(16, 16), 1, dict(respacing="20", ddim=True, eta=0.5, seed=1)),
    (_half(16, 16).bool(), 1, {}),
    (_half(16, 16).expand(2, 16, 16), 1, dict(respacing="20")),
    (_half(16, 16).expand(2, 1, 16, 16), 1, dict(ddim=True)),
    (_half(8, 8), 2, dict(respacing="20")),
    (None, 4, dict(respacing="20")),
    (_half(2, 2), 8, {}),
])
def test_good_arguments_reach_the_device_check(mask, scale, kw):
    """everything valid: the first complaint is the missing device, not an argument"""
    with pytest.raises(L.DDKError):
        _tiny().restore(torch.zeros(2, 3, 16 // scale, 16 // scale), mask, scale, **kw)


@pytest.mark.parametrize("y,mask,scale,kw", [
    (torch.zeros(1, 8, 8, 8), torch.ones(8, 8), 1, {}),                      # a latent is not an image
    (torch.zeros(1, 3, 32, 32), torch.ones(16, 16), 1, {}),                   # the mask is the image's, not the latent's
    (torch.zeros(1, 3, 32, 32), torch.eye(32), 1, {}),                        # no 4 x 4 footprint wholly measured
    (torch.zeros(1, 3, 8, 8), torch.ones(8, 8), 3, {}),                       # not a multiple of dim_reduc
    (torch.zeros(1, 3, 16, 16), torch.ones(16, 16), 2, {}),                   # below dim_reduc
    (torch.zeros(1, 3, 1, 1), torch.ones(1, 1), 64, {}),                      # n_lat = 16
    (torch.zeros(1, 3, 8, 8), torch.ones(8, 8), 8, {}),                       # 32 / 8 = 4, not 8
    (torch.zeros(1, 3, 4, 4), torch.ones(4, 4), 8, dict(eta=0.3)),
    (torch.zeros(1, 3, 4, 4), torch.ones(4, 4), 8, dict(solver="dpm++2m")),
])
def test_dddpm_bad_arguments_raise(y, mask, scale, kw):
    with pytest.raises(ValueError):
        _dd().restore(y, mask, scale, **kw)


@pytest.mark.parametrize("y,mask,scale", [(torch.zeros(1, 3, 32, 32), _half(32, 32), 1), (torch.zeros(1, 3, 8, 8), _half(8, 8), 4),
                                          (torch.zeros(1, 3, 4, 4), _half(4, 4), 8), (torch.zeros(1, 3, 4, 4), None, 8)])
def test_dddpm_good_arguments_reach_the_device_check(y, mask, scale):
    with pytest.raises(L.DDKError):
        _dd().restore(y, mask, scale, respacing="10", ddim=True)


def test_the_older_entries_keep_their_errors():
    m = _tiny()
    with pytest.raises(ValueError):
        m.super_resolve(torch.zeros(2, 3, 4, 4), 4, solver="dpm++2m")
    with pytest.raises(ValueError):
        m.inpaint(torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16), ddim=True)
    with pytest.raises(ValueError):
        m.inpaint(torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16), solver="dpm++2m")
    with pytest.raises(ValueError):
        m.super_resolve(torch.zeros(2, 3, 16, 16), 1)


# ---------------------------------------------------------------- the restatement's identities
def _toy_eps(x, t):
    return 0.3 * x + 0.1 * torch.roll(x, 1, dims=3) - 0.05 * t.reshape(-1, 1, 1, 1).float() / 1000.0


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("kw", [dict(), dict(ddim=True, eta=0.5)])
def test_all_ones_mask_is_the_unmasked_chain_bit_for_bit(n, kw):
    g = torch.Generator().manual_seed(n)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.rand(2, 3, 8 // n, 8 // n, generator=g) * 2 - 1
    want = RR.Restore(BETAS, "10").run(_toy_eps, x_T, y, n, 5, **kw)
    ones = torch.ones(2, 8 // n, 8 // n)
    assert torch.equal(RM.RestoreMasked(BETAS, "10").run(_toy_eps, x_T, y, ones, n, 5, **kw), want)
    assert torch.equal(RM.RestoreMasked(BETAS, "10").run(_toy_eps, x_T, y, None, n, 5, **kw), want)


@pytest.mark.parametrize("kw", [dict(), dict(ddim=True, eta=0.0), dict(ddim=True, eta=0.85)])
def test_measured_pixels_come_back_exactly_and_hidden_y_is_never_used(kw):
    g = torch.Generator().manual_seed(3)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.rand(2, 3, 8, 8, generator=g) * 2 - 1
    mk = (torch.rand(2, 8, 8, generator=g) < 0.5).float()
    sel = (mk != 0).unsqueeze(1).expand_as(y)
    chain = RM.RestoreMasked(BETAS, "10")
    zeroed = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.zeros_like(y)), mk, 1, 9, **kw)
    assert torch.equal(zeroed[sel], y[sel])
    assert not torch.equal(zeroed[~sel], y[~sel])
    poisoned = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.full_like(y, float("nan"))), mk, 1, 9, **kw)
    assert torch.isfinite(poisoned).all() and torch.equal(poisoned, zeroed)
    # the same at n = 2: blocks that are not measured never see y
    y2 = RR.pool(y, 2)
    mk2 = (torch.rand(2, 4, 4, generator=g) < 0.5).float()
    sel2 = (mk2 != 0).unsqueeze(1).expand_as(y2)
    a = chain.run(_toy_eps, x_T, torch.where(sel2, y2, torch.zeros_like(y2)), mk2, 2, 9, **kw)
    b = chain.run(_toy_eps, x_T, torch.where(sel2, y2, torch.full_like(y2, float("nan"))), mk2, 2, 9, **kw)
    assert torch.isfinite(b).all() and torch.equal(a, b)
    err = float((RR.pool(a.double(), 2) - y2.double())[sel2].abs().max())
    assert err <= 8 * 4 * 2.0 ** -24, err


# ---------------------------------------------------------------- Gaussian data, exact eps
def test_gaussian_conditional_mean():
    """The toy problem of tests/test_inpaint_cpu.py: 16 correlated 'pixels' (std 0.3, correlation length 4), the middle 6 hidden,
    the exact eps of that Gaussian.  The restatement's chain itself runs at "50" (fp32, Philox draws), 20000 chains as the batch,
    as DDIM with eta 0, DDIM with eta 0.85 and ancestral steps; the mean over the chains against the exact conditional mean
    S_hk S_kk^-1 x_k.  The bar: below the prior mean's error (max |conditional mean| = 0.109 on the hidden pixels).
    Measured: eta 0: 0.0227, eta 0.85: 0.0254, ancestral: 0.0309 (RePaint at "50", j = 5: 0.031 with r = 1, 0.058 with r = 10; no
    order between the methods is asserted).  The measured pixels are exact."""
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
    chain = RM.RestoreMasked(BETAS, "50")
    errs = {}
    for name, kw in (("ddim eta 0", dict(ddim=True, eta=0.0)), ("ddim eta 0.85", dict(ddim=True, eta=0.85)), ("ancestral", dict())):
        x_T = torch.from_numpy(np.random.default_rng(7).standard_normal((n, 1, 1, d))).float()
        out = chain.run(eps_model, x_T, y, mk, 1, seed=11, **kw).reshape(n, d).double().numpy()
        assert (out[:, known] == y.reshape(n, d).numpy()[:, known]).all()
        errs[name] = float(np.abs(out.mean(axis=0)[h] - want).max())
    print("Gaussian conditional mean, max abs error on the hidden pixels: " + ", ".join(f"{k} {v:.4g}" for k, v in errs.items()) +
          f" (prior mean {prior_err:.4g})")
    for name, err in errs.items():
        assert err < prior_err, (name, err)


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_masked"][1]) == 18
    assert len(L.SIGNATURES["ddk_sampler_run_restore_masked"][1]) == 6
    assert len(L.SIGNATURES["ddk_sampler_restore_masked_workspace_bytes"][1]) == 6
    assert L.load().ddk_version() == L.ABI_VERSION == 400


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only.  The workspace holds y and the mask behind the sampler layout, sized by n: a whole latent plus B H W at
    n = 1, a quarter of each at n = 2, and never less than the unmasked restore chain's at n >= 2 (a call without a mask is that
    chain); the existing query is unchanged.  The fused tail: n = 1 wherever the plain kinds with at most 128 channels are (no
    whole-blocks condition), n >= 2 as the unmasked kind."""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 8, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    B, S, Cl = 32, 32, 8
    lat, pix = B * S * S * Cl * 4, B * S * S * 4          # bytes
    plain = lib.ddk_sampler_workspace_bytes(h, B, S, S, 49)
    restore = lib.ddk_sampler_restore_workspace_bytes(h, B, S, S, 49)
    assert restore == plain + lat // 4                    # what it returned before this entry existed
    q = {n: lib.ddk_sampler_restore_masked_workspace_bytes(h, B, S, S, 49, n) for n in (1, 2, 4, 8)}
    assert q[1] == plain + lat + pix
    assert q[2] == plain + lat // 4 + pix // 4
    assert q[4] == q[8] == restore
    assert all(q[n] >= restore for n in (2, 4, 8))
    assert lib.ddk_sampler_restore_masked_workspace_bytes(h, B, S, S, 49, 3) == 0
    assert lib.ddk_sampler_restore_masked_workspace_bytes(h, B, 30, S, 49, 1) == 0
    parts = {n: lib.ddk_sampler_restore_masked_tail_parts(h, B, S, S, n) for n in (1, 2, 4, 8)}
    assert parts[1] == parts[2] == parts[4] == 8 and parts[8] == 0, parts
    assert {n: lib.ddk_sampler_restore_tail_parts(h, B, S, S, n) for n in (2, 4, 8)} == {2: 8, 4: 8, 8: 0}
    assert lib.ddk_sampler_restore_masked_tail_parts(h, B, S, S, 3) < 0
    assert lib.ddk_sampler_restore_masked_tail_parts(h, B, 64, 64, 1) == lib.ddk_sampler_restore_tail_parts(h, B, 64, 64, 2)
    assert lib.ddk_sampler_restore_masked_tail_parts(h, B, 64, 64, 4) == 0
    assert lib.ddk_unet_set_option(h, 12, 0) == 0
    assert lib.ddk_sampler_restore_masked_tail_parts(h, B, S, S, 1) == 0 and lib.ddk_sampler_restore_masked_tail_parts(h, B, S, S, 2) == 0
    assert lib.ddk_unet_set_option(h, 12, 1) == 0
    u256 = Unet(ddpm_cfg(256, 8, 32))
    u256.flops(1, 32, 32)
    assert lib.ddk_sampler_restore_masked_tail_parts(u256._plan.handle, B, S, S, 1) == 0
