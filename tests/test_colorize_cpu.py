"""DDNM colourisation and grey super-resolution (DDPM.colorize, ddk_sampler_run_restore_gray) on the CPU: every argument error
before any device work, the two per-row tables, the restatement (tests/restore_gray_ref.py) against its rounding bar and on Gaussian
data with the exact eps, and the header, the ctypes signatures, the built library and the host-side workspace and eligibility queries
on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import restore_gray_ref as RG
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from ddk import lib as L
from oracle import diffusion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = D.beta_schedule("linear", 1000)
NEW = ("ddk_p_sample_update_restore_gray", "ddk_sampler_restore_gray_workspace_bytes", "ddk_sampler_restore_gray_tail_parts",
       "ddk_sampler_run_restore_gray")
# the four table sets of tests/test_restore_cpu.py
TABLE_SETS = [dict(respacing=None), dict(respacing="20"), dict(respacing="20", ddim=True), dict(respacing="ddim50", ddim=True, eta=0.7)]


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


def _half(h, w):
    m = torch.ones(h, w)
    m[:, w // 2:] = 0
    return m


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def test_a_model_that_is_not_three_channel_raises():
    cfg = ddpm_cfg(32, 8, 16)
    with pytest.raises(ValueError, match="3-channel"):
        DDPM(cfg, Unet(cfg), "cpu", 8).colorize(torch.zeros(2, 1, 16, 16))
    cfg = dddpm_cfg(32, 32, 2)
    with pytest.raises(ValueError, match="latent"):
        DownsampleDDPM(cfg, Unet(cfg), "cpu", 3).colorize(torch.zeros(1, 1, 32, 32))


@pytest.mark.parametrize("y,mask,scale", [
    (torch.zeros(2, 3, 16, 16), None, 1), (torch.zeros(2, 16, 16), None, 1), (torch.zeros(2, 1, 8, 8), None, 1),
    (torch.zeros(2, 1, 16, 16), None, 2), (torch.zeros(2, 1, 16, 16, dtype=torch.long), None, 1), ([[0.0]], None, 1),     # misshapen or not float
    (torch.full((2, 1, 16, 16), float("nan")), None, 1), (torch.full((2, 1, 8, 8), float("inf")), None, 2),               # not finite
    (torch.zeros(2, 1, 16, 16), None, 3), (torch.zeros(2, 1, 16, 16), None, 16), (torch.zeros(2, 1, 8, 8), None, 2.0),
    (torch.zeros(2, 1, 16, 16), None, True), (torch.zeros(2, 1, 16, 16), None, 0),                                         # bad scales
    (torch.zeros(2, 1, 16, 16), torch.full((16, 16), 0.5), 1), (torch.zeros(2, 1, 16, 16), torch.zeros(16, 16), 1),
    (torch.zeros(2, 1, 16, 16), torch.stack([torch.ones(16, 16), torch.zeros(16, 16)]), 1),
    (torch.zeros(2, 1, 16, 16), torch.ones(2, 3, 16, 16), 1), (torch.zeros(2, 1, 16, 16), [[1.0]], 1),
    (torch.zeros(2, 1, 8, 8), _half(16, 16), 2),                                                                           # the masks restore rejects
])
def test_bad_measurements_scales_and_masks_raise(y, mask, scale):
    with pytest.raises(ValueError):
        _tiny().colorize(y, mask, scale)


def test_a_scale_that_does_not_divide_the_image_raises():
    cfg = ddpm_cfg(32, 3, 12)
    with pytest.raises(ValueError, match="divide"):
        DDPM(cfg, Unet(cfg), "cpu", 3).colorize(torch.zeros(1, 1, 1, 1), None, 8)


@pytest.mark.parametrize("weights", ["rgb", "Mean", None, 1, ("mean",)])
def test_unknown_weights_raise(weights):
    with pytest.raises(ValueError, match="weights"):
        _tiny().colorize(torch.zeros(2, 1, 16, 16), weights=weights)


@pytest.mark.parametrize("sy", [-0.1, float("nan"), float("inf"), "0.1", None, True, [0.1], torch.tensor(0.1), 1j])
def test_bad_sigma_y_raises(sy):
    with pytest.raises(ValueError, match="sigma_y"):
        _tiny().colorize(torch.zeros(2, 1, 16, 16), sigma_y=sy)


@pytest.mark.parametrize("kw", [dict(ddim=True), dict(ddim=True, eta=0.0), dict(respacing="20", ddim=True)])
def test_sigma_y_on_a_chain_without_draws_is_rejected(kw):
    with pytest.raises(ValueError, match="eta"):
        _tiny().colorize(torch.zeros(2, 1, 16, 16), sigma_y=0.1, **kw)
    with pytest.raises(L.DDKError):                                    # an exact measurement takes eta = 0
        _tiny().colorize(torch.zeros(2, 1, 16, 16), sigma_y=0.0, **kw)


@pytest.mark.parametrize("kw", [dict(solver="dpm++2m"), dict(noise=torch.zeros(1)), dict(early_stop=10), dict(paste=True), dict(paste=False),
                                dict(jump_length=3), dict(eta=0.5), dict(ddim=True, eta=-1.0)])
def test_rejected_keywords_raise(kw):
    with pytest.raises(ValueError):
        _tiny().colorize(torch.zeros(2, 1, 16, 16), **kw)


def test_non_finite_measured_pixels_raise_and_hidden_ones_do_not():
    y = torch.zeros(2, 1, 16, 16)
    y[0, 0, 3, 2] = float("nan")                       # measured (left half)
    with pytest.raises(ValueError):
        _tiny().colorize(y, _half(16, 16))
    y = torch.zeros(2, 1, 16, 16)
    y[0, 0, 3, 12] = float("nan")                      # hidden: never read, so the first complaint is the missing device
    with pytest.raises(L.DDKError):
        _tiny().colorize(y, _half(16, 16))


@pytest.mark.parametrize("mask,scale,kw", [
    (None, 1, {}),                                                      # a grey image alone constrains something: no mask needed at scale 1
    (None, 1, dict(weights="luma", respacing="20", ddim=True, eta=0.5, seed=1)),
    (_half(16, 16), 1, dict(sigma_y=0.1)),
    (_half(16, 16).bool(), 1, dict(weights="luma")),
    (_half(16, 16).expand(2, 1, 16, 16), 1, dict(respacing="20", ddim=True)),
    (_half(8, 8), 2, dict(respacing="20", sigma_y=2)),
    (None, 4, dict(respacing="20")),
    (_half(2, 2), 8, dict(weights="luma", sigma_y=np.float32(0.3))),
])
def test_good_arguments_reach_the_device_check(mask, scale, kw):
    with pytest.raises(L.DDKError):
        _tiny().colorize(torch.zeros(2, 1, 16 // scale, 16 // scale), mask, scale, **kw)


def test_the_older_entries_keep_their_signatures_and_errors():
    import inspect
    m = _tiny()
    for name in ("restore", "restore_noisy", "super_resolve", "inpaint", "restore_solver"):
        assert "weights" not in inspect.signature(getattr(DDPM, name)).parameters
    with pytest.raises(ValueError):
        m.restore(torch.zeros(2, 3, 16, 16), _half(16, 16), 1, weights="mean")
    with pytest.raises(ValueError):                                    # restore still needs a mask at scale 1, and its message names it
        m.restore(torch.zeros(2, 3, 16, 16), None, 1)
    with pytest.raises(ValueError, match="restore: mask values"):
        m.restore(torch.zeros(2, 3, 16, 16), torch.full((16, 16), 0.5), 1)


# ---------------------------------------------------------------- the tables
@pytest.mark.parametrize("kw", TABLE_SETS)
def test_table_properties(kw):
    m = _tiny()
    ddim, eta = kw.get("ddim", False), kw.get("eta", 0.0)
    tab, use = m._gray_tables(kw["respacing"], ddim, eta, 0.0)
    base, use0 = m._spaced_tables(kw["respacing"], ddim, eta) if (kw["respacing"] is not None or ddim) else (m._tables(), None)
    assert use == use0 or list(use) == list(use0)
    for k in base:
        assert torch.equal(tab[k], base[k]), k
    assert tab["lam"].dtype == tab["sgm"].dtype == torch.float32 and tab["lam"].shape == tab["sgm"].shape == tab["c1"].shape
    assert torch.equal(tab["lam"], torch.ones_like(tab["lam"]))        # row 0 included
    want = base["sigma"].clone()
    want[0] = 0.0
    assert torch.equal(tab["sgm"], want) and float(tab["sgm"][0]) == 0.0     # the fp32 sigma bit for bit, row 0 zero
    assert m._gray_tables(kw["respacing"], ddim, eta, 0.0)[0]["lam"] is tab["lam"]      # cached: the same tensors, the same graph key
    if ddim and eta == 0:
        return                                                          # no draws: sigma_y > 0 is rejected before any table is formed
    for sy in (0.05, 0.5):
        got, _ = m._gray_tables(kw["respacing"], ddim, eta, sy)
        ref, _ = m._noisy_tables(kw["respacing"], ddim, eta, sy)
        assert set(got) == set(ref) and all(torch.equal(got[k], ref[k]) for k in ref)


@pytest.mark.parametrize("kw", [dict(), dict(ddim=True, eta=0.5)])
@pytest.mark.parametrize("sy", [0.0, 0.05, 0.5])
def test_library_tables_agree_with_the_restatement(kw, sy):
    tab, use = _tiny()._gray_tables("8", kw.get("ddim", False), kw.get("eta", 0.0), sy)
    chain = RG.RestoreGray(BETAS, "8")
    ref = chain.tables(sy, **kw)
    assert list(use) == chain.sd.timestep_map
    for name in ("c1", "c2", "lam", "sgm"):
        assert torch.allclose(tab[name], ref[name], rtol=1e-5, atol=1e-7), name
    assert torch.allclose(tab["sigma"][1:], ref["sigma"][1:], rtol=1e-6, atol=0)


# ---------------------------------------------------------------- the restatement: the rounding bar, the select on the mask
def _bar(n, weights):
    """tests/test_restore_gpu.py's _bar, 8 n^2 2^-24 for a block of n^2 terms, with the group's 3 n^2 terms, doubled for luma's extra
    multiply per term"""
    return (8 if weights == "mean" else 16) * 3 * n * n * 2.0 ** -24


@pytest.mark.parametrize("weights", ["mean", "luma"])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
@pytest.mark.parametrize("data", ["uniform", "saturated"])
def test_one_step_with_lam_one_meets_the_rounding_bar(data, n, weights):
    """row 0 of an exact chain (lam = 1, c1 = 1, c2 = 0, no draw) returns x0'; A x0', evaluated in float64 with the exact weights, is y
    to the bar.  x0 uniform in [-1, 1], and saturated at +-1 (the clamp's output on large inputs: the worst case for the sum)."""
    g = torch.Generator().manual_seed(100 * n + len(weights))
    B, H, W = 4, 16, 16
    x = torch.rand(B, 3, H, W, generator=g) * 2 - 1 if data == "uniform" else 5 * torch.randn(B, 3, H, W, generator=g)
    y = torch.rand(B, 1, H // n, W // n, generator=g) * 2 - 1
    one, zero = torch.ones(B), torch.zeros(B)
    out = RG.step(x, torch.zeros_like(x), y, None, n, weights, one, zero, one, zero, zero, one, zero, torch.zeros_like(x))
    if data == "saturated":
        assert float(x.clamp(-1, 1).abs().mean()) > 0.8
    err = float((RG.apply_exact(out, n, weights) - y[:, 0].double()).abs().max())
    print(f"restatement, {weights}, n = {n}, {data} x0: |A x0' - y| = {err:.3g} (bar {_bar(n, weights):.3g})")
    assert err <= _bar(n, weights), err


def _toy_eps(x, t):
    return 0.3 * x + 0.1 * torch.roll(x, 1, dims=3) - 0.05 * t.reshape(-1, 1, 1, 1).float() / 1000.0


@pytest.mark.parametrize("weights", ["mean", "luma"])
@pytest.mark.parametrize("n", [1, 2])
def test_restatement_never_uses_unmeasured_y_and_leaves_unmeasured_groups_alone(n, weights):
    g = torch.Generator().manual_seed(n)
    x_T = torch.randn(2, 3, 8, 8, generator=g)
    y = torch.rand(2, 1, 8 // n, 8 // n, generator=g) * 2 - 1
    mk = (torch.rand(2, 8 // n, 8 // n, generator=g) < 0.5).float()
    sel = (mk != 0).unsqueeze(1)
    chain = RG.RestoreGray(BETAS, "10")
    for sy in (0.0, 0.2):
        a = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.zeros_like(y)), mk, n, weights, sy, 9)
        b = chain.run(_toy_eps, x_T, torch.where(sel, y, torch.full_like(y, float("nan"))), mk, n, weights, sy, 9)
        assert torch.isfinite(b).all() and torch.equal(a, b)
    # an exact chain's result meets the bar on the measured groups
    err = float(((RG.apply_exact(chain.run(_toy_eps, x_T, y, mk, n, weights, 0.0, 9), n, weights) - y[:, 0].double()) * mk).abs().max())
    assert err <= _bar(n, weights), err
    # one step: unmeasured groups take the plain ancestral step
    x, e, z = (torch.randn(2, 3, 8, 8, generator=g) for _ in range(3))
    co = {k: torch.rand(2, generator=g) for k in ("cr", "crm1", "c1", "c2", "sg", "lam", "sgm")}
    got = RG.step(x, e, y, mk, n, weights, co["cr"], co["crm1"], co["c1"], co["c2"], co["sg"], co["lam"], co["sgm"], z)
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(co["cr"]) * x - col(co["crm1"]) * e).clamp(-1, 1)
    plain = (col(co["c1"]) * x0 + col(co["c2"]) * x) + col(co["sg"]) * z
    hid = ~RG.measured(mk, x, n)
    assert torch.equal(got[hid], plain[hid]) and not torch.equal(got[~hid], plain[~hid])


# ---------------------------------------------------------------- Gaussian data, exact eps
@pytest.mark.parametrize("weights,sy", [("mean", 0.0), ("luma", 0.1)])
def test_gaussian_posterior_mean(weights, sy):
    """8 'pixels' x 3 channels, jointly Gaussian: pixel covariance exp(-|i - j| / 4), channel stds (0.3, 0.2, 0.1) with correlations
    0.6 (R-G), 0.3 (R-B), 0.6 (G-B), channel means (0.3, 0, -0.3), and the exact eps of that Gaussian.  y = A x_true + sigma_y noise
    with A the grey operator at n = 1.  The exact answer is mu + S A^T (A S A^T + sigma_y^2 I)^-1 (y - A mu).  20000 chains of the
    restatement at "50", ancestral.  The bar: the max error of the chains' mean over all 24 elements is below both the grey-replicated
    image's and the prior mean's.  Measured: see DESIGN.md section 3.11."""
    d = 8
    idx = np.arange(d)
    P = np.exp(-np.abs(idx[:, None] - idx[None, :]) / 4.0)
    std = np.array([0.3, 0.2, 0.1])
    R = np.array([[1.0, 0.6, 0.3], [0.6, 1.0, 0.6], [0.3, 0.6, 1.0]])
    S = np.kron(R * std[:, None] * std[None, :], P)                    # element (c, i) at c * d + i: the NCHW order of [3, 1, d]
    mu = np.repeat(np.array([0.3, 0.0, -0.3]), d)
    w = np.array(RG.EXACT[weights])
    A = np.kron(w[None, :], np.eye(d))                                 # [d, 3 d]
    x_true = mu + np.linalg.cholesky(S) @ np.random.default_rng(0).standard_normal(3 * d)
    y_np = A @ x_true + sy * np.random.default_rng(5).standard_normal(d)
    want = mu + S @ A.T @ np.linalg.solve(A @ S @ A.T + sy ** 2 * np.eye(d), y_np - A @ mu)
    gray_err = float(np.abs(np.tile(y_np, 3) - want).max())
    prior_err = float(np.abs(mu - want).max())
    acp = np.cumprod(1.0 - np.asarray(BETAS, dtype=np.float64))
    I = np.eye(3 * d)

    def eps_model(x, t):
        a = acp[int(t[0])]
        M = np.sqrt(1 - a) * np.linalg.inv(a * S + (1 - a) * I)
        return torch.from_numpy((x.double().numpy().reshape(-1, 3 * d) - np.sqrt(a) * mu) @ M.T).float().reshape(x.shape)

    n = 20000
    y = torch.from_numpy(y_np).float().reshape(1, 1, 1, d).expand(n, 1, 1, d).contiguous()
    x_T = torch.from_numpy(np.random.default_rng(7).standard_normal((n, 3, 1, d))).float()
    out = RG.RestoreGray(BETAS, "50").run(eps_model, x_T, y, None, 1, weights, sy, seed=11).reshape(n, 3 * d).double().numpy()
    assert np.isfinite(out).all()
    err = float(np.abs(out.mean(axis=0) - want).max())
    print(f"Gaussian posterior mean, {weights}, sigma_y = {sy}: max abs error of the chains' mean {err:.4g}; the grey-replicated image "
          f"{gray_err:.4g}, the prior mean {prior_err:.4g}")
    assert err < gray_err and err < prior_err, (err, gray_err, prior_err)


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_gray"][1]) == 21
    assert len(L.SIGNATURES["ddk_sampler_run_restore_gray"][1]) == 9
    assert len(L.SIGNATURES["ddk_sampler_restore_gray_workspace_bytes"][1]) == 6
    assert len(L.SIGNATURES["ddk_sampler_restore_gray_tail_parts"][1]) == 5
    # the header's parameter counts are the ctypes ones
    for name in NEW:
        params = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[name][1]), name
    assert L.GRAY_WEIGHTS == {"mean": 1, "luma": 2}
    assert L.load().ddk_version() == L.ABI_VERSION == 400


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only.  The workspace is the masked chain's, byte for byte, for every n; the fused tail takes 3-channel models
    only: n = 1 wherever the plain kinds with at most 128 channels are, n >= 2 where the tile holds whole rows of blocks; the option
    that switches the restore tails off switches this one off."""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    B, S = 32, 32
    for n in (1, 2, 4, 8):
        assert lib.ddk_sampler_restore_gray_workspace_bytes(h, B, S, S, 49, n) == lib.ddk_sampler_restore_masked_workspace_bytes(h, B, S, S, 49, n) > 0
    assert lib.ddk_sampler_restore_gray_workspace_bytes(h, B, S, S, 49, 3) == 0
    assert lib.ddk_sampler_restore_gray_workspace_bytes(h, B, 30, S, 49, 1) == 0
    parts = {n: lib.ddk_sampler_restore_gray_tail_parts(h, B, S, S, n) for n in (1, 2, 4, 8)}
    assert parts == {1: 8, 2: 8, 4: 8, 8: 0}                           # n = 8 on W = 32: 128 % 256 != 0
    assert lib.ddk_sampler_restore_gray_tail_parts(h, B, S, S, 3) < 0
    assert lib.ddk_sampler_restore_gray_tail_parts(h, B, 64, 64, 4) == 0 and lib.ddk_sampler_restore_gray_tail_parts(h, B, 64, 64, 1) == 32
    assert lib.ddk_unet_set_option(h, 12, 0) == 0
    assert lib.ddk_sampler_restore_gray_tail_parts(h, B, S, S, 1) == 0 and lib.ddk_sampler_restore_gray_tail_parts(h, B, S, S, 2) == 0
    assert lib.ddk_unet_set_option(h, 12, 1) == 0
    u8 = Unet(ddpm_cfg(128, 8, 32))                                    # an 8-channel model has no grey operator: never fused (and never run)
    u8.flops(1, 32, 32)
    assert {n: lib.ddk_sampler_restore_gray_tail_parts(u8._plan.handle, B, S, S, n) for n in (1, 2, 4, 8)} == {1: 0, 2: 0, 4: 0, 8: 0}
    assert lib.ddk_sampler_restore_masked_tail_parts(u8._plan.handle, B, S, S, 1) == 8
    u256 = Unet(ddpm_cfg(256, 3, 32))
    u256.flops(1, 32, 32)
    assert lib.ddk_sampler_restore_gray_tail_parts(u256._plan.handle, B, S, S, 1) == 0


def test_the_evaluator_and_the_cli_know_the_task():
    import evaluate_restoration as cli
    from utils import restoration_metrics as RMx
    assert RMx.TASKS == ("inpaint", "sr", "colorize")
    a = cli.parse_args(["--task", "colorize"])
    assert (a.scale, a.weights, a.method, a.mask) == (1, "mean", "ddnm", None)
    assert cli.chain_options(a) == dict(respacing=None, scale=1, weights="mean", ddim=False, eta=0.0)
    a = cli.parse_args(["--task", "colorize", "--weights", "luma", "--scale", "2", "--sigma_y", "0.1", "--mask", "half"])
    assert cli.chain_options(a) == dict(respacing=None, scale=2, weights="luma", ddim=False, eta=0.0, sigma_y=0.1)
    # the existing tasks parse to what they did
    assert cli.chain_options(cli.parse_args(["--task", "sr"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    assert cli.parse_args(["--task", "inpaint"]).mask == "center"
    for bad in (["--task", "sr", "--weights", "luma"], ["--task", "colorize", "--scale", "3"], ["--task", "colorize", "--dpm_solver"],
                ["--task", "colorize", "--method", "repaint"], ["--task", "colorize", "--weights", "rgb"],
                ["--task", "colorize", "--sigma_y", "0.1", "--use_ddim"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    x = torch.rand(2, 3, 4, 4)
    assert torch.allclose(RMx.gray(x, "mean"), x.mean(dim=1, keepdim=True), atol=1e-7)
    assert torch.allclose(RMx.gray(x, "luma")[:, 0], 0.299 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2], atol=1e-7)
    with pytest.raises(ValueError):
        RMx.gray(x[:, :1], "mean")
