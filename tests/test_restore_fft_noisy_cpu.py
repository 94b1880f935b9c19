"""DDNM+ deconvolution of a noisy blurred image on the CPU: the per-frequency multipliers of the restatement
tests/fft_noisy_ref.py on the library's own operands (models/diffusion/psf.py psf_noisy_operands), the restatement's tie to
tests/fft_conv_ref.py, every argument error of DDPM.deconvolve_noisy / DownsampleDDPM.deconvolve_noisy before any device work, what
stays refused, the header, the ctypes signatures and the built library on the new entries, and a Gaussian problem whose posterior
mean is known in closed form."""
import ctypes
import os
import re
import time

import numpy as np
import pytest
import torch

import fft_conv_ref as FR
import fft_noisy_ref as FN
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import psf
from oracle import diffusion_ref as D
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = D.beta_schedule("linear", 1000)
NEW = ("ddk_p_sample_update_restore_fft_noisy", "ddk_sampler_run_restore_fft_noisy", "ddk_sampler_restore_fft_noisy_workspace_bytes",
       "ddk_sampler_restore_fft_noisy_tail_parts")
SIZES = [(16, 16), (32, 16), (16, 64)]
TABLE_SETS = [dict(respacing=None), dict(respacing="20"), dict(respacing="20", ddim=True), dict(respacing="ddim50", ddim=True, eta=0.7)]
U24 = 2.0 ** -24


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


def _mirror(a):
    H, W = a.shape[-2:]
    return a[..., (-np.arange(H)) % H, :][..., (-np.arange(W)) % W]


# ---------------------------------------------------------------- the operands and the multipliers
@pytest.mark.parametrize("kw", TABLE_SETS, ids=["plain", "20", "ddim20", "ddim50eta"])
@pytest.mark.parametrize("name", psf.PRESETS)
def test_multiplier_properties(name, kw):
    """per frequency and row: the noise that y brings, lam g, and the draw's phi add up to the chain's own s^2 (eq. 19).  The bar 8 u s^2:
    lam = 1: phi^2 carries the roundings of s s, g g, their difference and the root (twice), 5 u s^2 at most; lam < 1: lam g =
    s (1 + d), |d| <= u, so 2 u s^2."""
    m = _tiny()
    ddim, eta = kw.get("ddim", False), kw.get("eta", 0.0)
    draws = not (ddim and eta == 0)
    tab = (m._spaced_tables(kw["respacing"], ddim, eta) if kw["respacing"] is not None or ddim else (m._tables(), None))[0]
    s32 = tab["sigma"].numpy().astype(np.float32).copy()
    s32[0] = 0.0
    s = s32.astype(np.float64)[:, None, None]
    for H, W in SIZES:
        for tol in (0.03, 0.1):
            M = FR.kept(FR.preset(name), H, W, tol)
            inside = 0
            for sy in (0.02, 0.1, 0.5):
                gain, nsc = psf.psf_noisy_operands(name, H, W, tol, sy, tab["c1"])
                assert gain.dtype == nsc.dtype == np.float32 and gain.shape == (H, W) and nsc.shape == s32.shape
                assert gain.flags["C_CONTIGUOUS"] and np.array_equal(gain > 0, M) and np.array_equal(gain, _mirror(gain))
                assert np.allclose(gain, FN.gain(FR.preset(name), H, W, tol), rtol=2.0 ** -22, atol=0) and gain.max() < 1.0 / tol
                assert np.array_equal(nsc, (np.abs(tab["c1"].double().numpy()) * sy).astype(np.float32))
                lam, phi = FN.multipliers(M, gain, s32, nsc)
                assert lam.shape == phi.shape == (len(s32), H, W)
                assert (lam >= 0).all() and (lam <= 1).all() and (phi >= 0).all() and (phi <= s32[:, None, None]).all()
                assert (lam[0] == 0).all() and (phi[0] == 0).all()                          # row 0: the model's own x0, no draw
                assert (lam[:, ~M] == 0).all() and np.array_equal(phi[:, ~M], np.broadcast_to(s32[:, None], phi[:, ~M].shape))
                assert np.array_equal(lam, _mirror(lam)) and np.array_equal(phi, _mirror(phi))
                g = (nsc[:, None, None] * gain[None]).astype(np.float32).astype(np.float64)
                total = (lam.astype(np.float64) * g) ** 2 + phi.astype(np.float64) ** 2
                assert (np.abs(total - s ** 2)[1:, M] <= 8 * U24 * (s[1:, 0, 0] ** 2)[:, None]).all()
                assert ((phi == 0) | (lam == 1))[:, M].all()                                # one of the two carries the whole variance
                inside += int(((lam[1:, M] > 0) & (lam[1:, M] < 1)).any(axis=1).sum())
                if not draws:
                    assert (lam[:, M] == 0).all() and (phi == 0).all()                      # nothing is drawn: nothing can be constrained
            if draws:
                assert inside > 0, (H, W, tol)                                               # some row damps some kept frequency
            # sigma_y -> 0: lam is 1 on every kept frequency above row 0 and phi the chain's own s: the deconvolution step
            gain, nsc = psf.psf_noisy_operands(name, H, W, tol, 0.0, tab["c1"])
            lam, phi = FN.multipliers(M, gain, s32, nsc)
            assert (nsc == 0).all() and (lam[1:, M] == 1).all() and np.array_equal(phi, np.broadcast_to(s32[:, None, None], phi.shape))


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), "0.1", None, True])
def test_operands_refuse_a_bad_sigma_y(bad):
    with pytest.raises(ValueError):
        psf.psf_noisy_operands("disk", 16, 16, 0.03, bad, np.ones(4))


# ---------------------------------------------------------------- the restatement's tie to the deconvolution step
@pytest.mark.parametrize("name", psf.PRESETS)
def test_forced_multipliers_give_the_deconvolution_step(name):
    """lam = 1 and phi = s on every frequency: x0' = x0 - A+A x0 + A+y and n = s z, tests/fft_conv_ref.py's step"""
    g = torch.Generator().manual_seed(11)
    shape = (3, 2, 16, 32)
    x, e, z = (torch.randn(shape, generator=g) for _ in range(3))
    k = FR.preset(name)
    M = FR.kept(k, 16, 32, 0.03)
    Yp = FR.apply(torch.randn(shape, generator=g), M.astype(np.float64))
    B = shape[0]
    cr, crm1, c1, c2 = (torch.rand(B, generator=g) + 0.5 for _ in range(4))
    sg = torch.tensor([0.0, 0.3, 0.7])
    want, x0, x0p = FR.step(x, e, M, torch.from_numpy(Yp), cr, crm1, c1, c2, sg, z)
    lam = np.ones((B, 16, 32), dtype=np.float32)
    phi = np.broadcast_to(sg.numpy()[:, None, None], lam.shape).astype(np.float32)
    Yhat = np.fft.fft2(Yp, axes=(-2, -1))
    Yhat[..., ~M] = np.nan                                  # never read there
    got, x0n, x0pn, n, _, _ = FN.step(x, e, M, FN.gain(k, 16, 32, 0.03).astype(np.float32), Yhat, cr, crm1, c1, c2, sg, torch.zeros(B), z,
                                      lam_phi=(lam, phi))
    assert torch.equal(x0, x0n) and float((x0p - x0pn).abs().max()) <= 1e-12 and float((got - want).abs().max()) <= 1e-12
    # and through multipliers() itself: nsc = 0 is lam = 1, phi = s
    got2 = FN.step(x, e, M, FN.gain(k, 16, 32, 0.03).astype(np.float32), Yhat, cr, crm1, c1, c2, sg, torch.zeros(B), z)[0]
    assert float((got2[1:] - want[1:]).abs().max()) <= 1e-12


def test_device_order_round_trip():
    H, W = 16, 64
    u, v = np.arange(H)[:, None], np.arange(W)[None, :]
    nat = (u * 1000 + v).astype(np.float64)
    brev = lambda i, bits: int(format(i, f"0{bits}b")[::-1], 2)
    dev = np.zeros(H * W)
    for a in range(H):
        for b in range(W):
            dev[brev(a, 4) * W + brev(b, 6)] = nat[a, b]
    assert np.array_equal(FN.to_natural(dev, H, W), nat)


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def test_the_downsampled_model_has_no_deconvolve_noisy():
    cfg = dddpm_cfg(32, 32, 2)
    with pytest.raises(ValueError, match="latent"):
        DownsampleDDPM(cfg, Unet(cfg), "cpu", 3).deconvolve_noisy(torch.zeros(1, 3, 32, 32), "disk", sigma_y=0.1)


@pytest.mark.parametrize("sy", [0.0, 0.1])
@pytest.mark.parametrize("y", [torch.zeros(2, 3, 64), torch.zeros(2, 1, 16, 16), torch.zeros(2, 3, 16, 32), torch.zeros(2, 3, 16, 16, dtype=torch.long),
                               torch.zeros(0, 3, 16, 16), torch.full((2, 3, 16, 16), float("nan")), torch.full((2, 3, 16, 16), float("inf")), [[0.0]]])
def test_bad_y_raises(y, sy):
    with pytest.raises(ValueError):
        _tiny().deconvolve_noisy(y, "disk", sigma_y=sy)


@pytest.mark.parametrize("sy", [0.0, 0.1])
@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(eta=True), dict(solver="dpm++2m"), dict(noise=torch.zeros(1)),
                                dict(early_stop=10), dict(paste=True), dict(mask=torch.ones(16, 16)), dict(tol=1.0),
                                dict(tol=-0.1), dict(tol=True), dict(tol="x"), dict(kernel="gauss"), dict(perm_seed=1)])
def test_unsupported_arguments_raise(kw, sy):
    with pytest.raises(ValueError):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "disk", sigma_y=sy, **kw)


@pytest.mark.parametrize("k", ["motion", "gauss", np.ones((4, 4)), np.ones((17, 3)), np.ones((3, 17)), np.zeros((3, 3)), np.full((3, 3), np.nan)])
def test_bad_psf_is_refused_by_the_model(k):
    with pytest.raises(ValueError):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), k, sigma_y=0.1)


@pytest.mark.parametrize("size", [24, 48, 8])
def test_an_image_size_off_the_grid_raises(size):
    cfg = ddpm_cfg(32, 3, size)
    with pytest.raises(ValueError, match="powers of two"):
        DDPM(cfg, Unet(cfg), "cpu", 3).deconvolve_noisy(torch.zeros(1, 3, size, size), np.ones((1, 1)), sigma_y=0.1)


@pytest.mark.parametrize("sy", [-0.1, float("nan"), float("inf"), "0.1", None, True, [0.1], torch.tensor(0.1), 1j])
def test_bad_sigma_y_raises(sy):
    with pytest.raises(ValueError, match="sigma_y"):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "disk", sigma_y=sy)


def test_sigma_y_is_required():
    with pytest.raises(TypeError):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "disk")


@pytest.mark.parametrize("kw", [dict(ddim=True), dict(ddim=True, eta=0.0), dict(respacing="20", ddim=True)])
def test_a_chain_without_draws_is_rejected(kw):
    with pytest.raises(ValueError, match="draws"):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "disk", sigma_y=0.1, **kw)
    with pytest.raises(L.DDKError, match="ROCm"):           # sigma_y = 0 is deconvolve, which takes such a chain
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "disk", sigma_y=0.0, **kw)


def test_good_arguments_reach_the_device_check():
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "diag", sigma_y=0.1, respacing="20", ddim=True, eta=0.3)
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), np.random.default_rng(0).standard_normal((5, 3)), sigma_y=0.5, tol=0.1)
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().deconvolve_noisy(torch.zeros(2, 3, 16, 16), "disk", sigma_y=np.float32(0.05), respacing="8")


def test_sigma_y_zero_dispatches_to_deconvolve(monkeypatch):
    m = _tiny()
    seen = {}
    monkeypatch.setattr(m, "deconvolve", lambda y, k, **kw: seen.update(kw, y=y, psf=k) or "out")
    y = torch.zeros(1, 3, 16, 16)
    assert m.deconvolve_noisy(y, "diag", sigma_y=0, tol=0.1, respacing="20", seed=4) == "out"
    assert seen == dict(y=y, psf="diag", tol=0.1, respacing="20", ddim=False, eta=0.0, x_T=None, seed=4)


# ---------------------------------------------------------------- what stays refused
def test_deconvolve_keeps_refusing_sigma_y():
    with pytest.raises(ValueError, match="sigma_y"):
        _tiny().deconvolve(torch.zeros(2, 3, 16, 16), "disk", sigma_y=0.1)
    import evaluate_restoration as cli
    with pytest.raises(SystemExit):
        cli.parse_args(["--task", "deconv", "--psf", "disk", "--sigma_y", "0.1"])


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    from ddk import ops, plan
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW + ("ddk_circular_spectrum",):
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
        params = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[name][1]), name
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_fft_noisy"][1]) == 21
    assert len(L.SIGNATURES["ddk_sampler_run_restore_fft_noisy"][1]) == 9
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert callable(ops.p_sample_update_restore_fft_noisy_) and callable(ops.circular_spectrum)
    assert plan.UnetPlan.RESTORE_ENTRIES["sfn"] == ("sampler_run_restore_fft_noisy", "sampler_restore_fft_noisy_workspace_bytes",
                                                   "sampler_restore_fft_noisy_tail_parts")
    assert "sfn" in plan.SAMPLERS and "sfn" in plan.CHAIN_WORKSPACES and callable(plan.UnetPlan.sample_restore_fft_noisy_nhwc)
    assert callable(plan.UnetPlan.restore_fft_noisy_tail_parts)
    # the older entries are what they were
    assert plan.SAMPLERS["srn"][0] == "sample_restore_noisy" and plan.SAMPLERS["srf"][0] == "sample_restore_fft"
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_fft"][1]) == 19 and len(L.SIGNATURES["ddk_sampler_run_restore_fft"][1]) == 7


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only: the deconvolution workspace plus gain (H W floats), nsc (one float per row, rounded up to four), the complex
    spectrum of A+ y (twice the latent's size) and, where a plane takes the multi-launch form, T2 (twice the latent's size)"""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    al4 = lambda v: (v + 3) // 4 * 4
    for t_start in (49, 7):
        for B, H, W in ((32, 32, 32), (2, 16, 64), (1, 256, 256)):
            base = lib.ddk_sampler_restore_fft_workspace_bytes(h, B, H, W, t_start)
            got = lib.ddk_sampler_restore_fft_noisy_workspace_bytes(h, B, H, W, t_start)
            n = B * H * W * 3
            assert base > 0 and got == base + 4 * (H * W + al4(t_start + 1) + 2 * n + (2 * n if H * W > 16384 else 0)), (B, H, W)
            assert lib.ddk_sampler_restore_fft_noisy_tail_parts(h, B, H, W) == 0
    for H, W in ((24, 24), (16, 48), (512, 512), (8, 16)):
        assert lib.ddk_sampler_restore_fft_noisy_workspace_bytes(h, 2, H, W, 49) == 0


def test_off_grid_arguments_are_err_arg_before_any_launch():
    """the lone entries refuse every off-grid shape, null pointer and misalignment on the host: no device is needed to be told so"""
    lib = L.load()
    buf = (ctypes.c_char * 272)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 16-byte aligned host memory: never read, no call gets as far as a launch
    step = lib.ddk_p_sample_update_restore_fft_noisy
    spec = lib.ddk_circular_spectrum

    def call(B, H, W, C, scratch=None, **over):
        a = dict(x=p, eps=p, mask=p, gain=p, nsc=p, tw=p, yhat=p)
        a.update(over)
        return step(a["x"], a["eps"], a["mask"], a["gain"], a["nsc"], a["tw"], a["yhat"], scratch, p, p, p, p, p, p, B, H, W, C, 0, 0, None)
    for B, H, W, C in ((1, 24, 16, 3), (1, 16, 48, 3), (1, 512, 16, 3), (1, 8, 16, 3), (1, 16, 16, 9), (1, 16, 16, 0), (0, 16, 16, 3),
                       (30000, 16, 16, 3)):
        assert call(B, H, W, C) == -1, (B, H, W, C)
        assert spec(p, p, p, p, None, B, H, W, C, None) == -1, (B, H, W, C)
    assert call(1, 256, 256, 3) == -1 and "scratch" in L.last_error()
    assert spec(p, p, p, p, None, 1, 128, 256, 3, None) == -1 and "scratch" in L.last_error()
    for name in ("mask", "gain", "nsc", "tw", "yhat"):
        assert call(1, 16, 16, 3, **{name: None}) == -1 and "null" in L.last_error(), name
    q = ctypes.c_void_p(p.value + 4)
    for name in ("mask", "gain", "nsc", "tw", "yhat"):
        assert call(1, 16, 16, 3, **{name: q}) == -1 and "alignment" in L.last_error(), name
    assert call(1, 256, 256, 3, scratch=q) == -1 and "alignment" in L.last_error()
    assert spec(q, p, p, p, None, 1, 16, 16, 3, None) == -1 and "alignment" in L.last_error()


# ---------------------------------------------------------------- Gaussian data, exact eps, a noisy blurred image
def test_gaussian_posterior_mean_of_a_noisy_blurred_image():
    """The toy problem of tests/test_restore_noisy_cpu.py in two dimensions: a 16 x 16 periodic image with a stationary Gaussian prior of
    pixel std 0.3 and correlation length 4 along each axis, covariance 0.09 exp(-(d_i + d_j) / 4) with d the distance around the
    torus.  The covariance is circulant, so prior, blur and posterior are all diagonal in the 2-D Fourier basis.  The exact eps of that
    prior, y = A x + 0.1 noise with the disk point-spread function.  The exact answer is the Wiener posterior mean
    S conj K^ / (|K^|^2 S + sigma_y^2) y^.  tol = sigma_y = 0.1: the frequencies kept are those the measurement knows at least as well
    as its noise, gain sigma_y <= 1 (max |K^| = 1 for a PSF that sums to 1), the usual truncation of a pseudo-inverse at the noise level.
    The restatement's DDNM+ chains run at "50", ancestral, 1500 chains as the batch; the bar: the error of the chains' mean is below
    the prior mean's (max |posterior mean|).  Plain DDNM on the same noisy y, which copies the noise into the kept frequencies times
    1 / |K^|, runs beside it; where this CPU shows DDNM+ at least 2x closer the order is asserted too.

    At the default tol = 0.03 the method itself misses this bar (measured: 0.75 against a prior mean of 0.58; 95 % of the error's
    power at frequencies with gain > 5; 1.21 at "250" steps): y's noise is one fixed draw, so what every step lets in of it, up to
    the step's whole s, adds up coherently along the chain where independent draws would add in quadrature, and a Gaussian prior
    this weak does not pull it back.  DESIGN.md section 3.19 says so and tells the caller to keep tol at or above sigma_y."""
    H = W = 16
    sy, tol = 0.1, 0.1
    d = np.minimum(np.arange(H), H - np.arange(H))
    S = np.fft.fft2(0.09 * np.exp(-(d[:, None] + d[None, :]) / 4.0)).real      # eigenvalues of the covariance: their mean is the pixel variance
    assert S.min() > 0
    rng = np.random.default_rng(0)
    x_true = np.fft.ifft2(np.sqrt(S) * np.fft.fft2(rng.standard_normal((H, W)))).real
    k = FR.preset("disk")
    K = FR.spectrum(k, H, W)
    y_noisy = np.fft.ifft2(K * np.fft.fft2(x_true)).real + sy * np.random.default_rng(5).standard_normal((H, W))
    want = np.fft.ifft2(S * np.conj(K) / (np.abs(K) ** 2 * S + sy ** 2) * np.fft.fft2(y_noisy)).real
    prior_err = float(np.abs(want).max())
    acp = np.cumprod(1.0 - np.asarray(BETAS, dtype=np.float64))

    def eps_model(x, t):
        a = acp[int(t[0])]
        mult = np.sqrt(1 - a) / (a * S + (1 - a))
        return torch.from_numpy(np.fft.ifft2(mult * np.fft.fft2(x.double().numpy(), axes=(-2, -1)), axes=(-2, -1)).real).float()

    n = 1500
    y = torch.from_numpy(y_noisy).float().reshape(1, 1, H, W).expand(n, 1, H, W).contiguous()
    x_T = lambda: torch.from_numpy(np.random.default_rng(7).standard_normal((n, 1, H, W))).float()
    t0 = time.time()
    plus = FN.DeconvNoisy(BETAS, "50").run(eps_model, x_T(), y, k, tol, sy, seed=11).reshape(n, H, W).double().numpy()
    plain = FR.Deconv(BETAS, "50").run(eps_model, x_T(), y, k, tol, seed=11).reshape(n, H, W).double().numpy()
    assert np.isfinite(plus).all()
    err_plus = float(np.abs(plus.mean(axis=0) - want).max())
    err_plain = float(np.abs(plain.mean(axis=0) - want).max())
    rms = lambda v: float(np.sqrt((v ** 2).mean()))
    print(f"Gaussian posterior mean of a noisy blurred image, sigma_y = {sy}: max abs error of the chains' mean: DDNM+ {err_plus:.4g}, plain DDNM "
          f"on the same noisy y {err_plain:.4g} (prior mean {prior_err:.4g}); rms: DDNM+ {rms(plus.mean(axis=0) - want):.4g}, plain "
          f"{rms(plain.mean(axis=0) - want):.4g}; {time.time() - t0:.1f} s")
    assert err_plus < prior_err, (err_plus, prior_err)
    assert 2 * err_plus <= err_plain, (err_plus, err_plain)      # measured: see DESIGN.md section 3.19


# ---------------------------------------------------------------- the command lines and the evaluator
def test_the_evaluator_and_the_cli_know_the_task():
    import deconv_model_samples as dms
    import evaluate_restoration as cli
    from models.diffusion import blur
    from utils import restoration_metrics as RMx
    assert RMx.DECONV_NOISY_TASK == "deconv_noisy" and RMx.DECONV_TASK == "deconv" and RMx.TASKS == ("inpaint", "sr", "colorize")
    a = cli.parse_args(["--task", "deconv_noisy", "--psf", "disk", "--sigma_y", "0.05"])
    assert cli.chain_options(a) == dict(respacing=None, psf="disk", tol=3e-2, ddim=False, eta=0.0, sigma_y=0.05)
    a = cli.parse_args(["--task", "deconv_noisy", "--psf", "k.npy", "--sigma_y", "0.1", "--tol", "0.1", "--use_ddim", "--eta", "0.5",
                        "--timestep_respacing", "20"])
    assert cli.chain_options(a) == dict(respacing="20", psf="k.npy", tol=0.1, ddim=True, eta=0.5, sigma_y=0.1)
    # the deconvolution task parses to what it did and keeps refusing --sigma_y
    assert cli.chain_options(cli.parse_args(["--task", "deconv", "--psf", "disk"])) == dict(respacing=None, psf="disk", tol=3e-2, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "sr", "--sigma_y", "0.1"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0, sigma_y=0.1)
    d = ["--task", "deconv_noisy", "--psf", "diag", "--sigma_y", "0.1"]
    for bad in (["--task", "deconv", "--psf", "disk", "--sigma_y", "0.1"], ["--task", "deconv_noisy", "--psf", "disk"],
                ["--task", "deconv_noisy", "--psf", "disk", "--sigma_y", "0"], ["--task", "deconv_noisy", "--psf", "disk", "--sigma_y", "-0.1"],
                ["--task", "deconv_noisy", "--psf", "disk", "--sigma_y", "nan"], ["--task", "deconv_noisy", "--sigma_y", "0.1"],
                ["--task", "deconv_noisy", "--psf", "motion", "--sigma_y", "0.1"], ["--task", "sr", "--psf", "disk", "--sigma_y", "0.1"],
                d + ["--use_ddim"], d + ["--use_ddim", "--eta", "0"], d + ["--eta", "0.5"], d + ["--scale", "2"], d + ["--mask", "half"],
                d + ["--dpm_solver"], d + ["--method", "repaint"], d + ["--method", "ddnm"], d + ["--kernel", "gauss"], d + ["--ratio", "0.5"],
                d + ["--perm_seed", "1"], d + ["--tol", "1"], d + ["--tol", "-0.5"], d + ["--jump_length", "5"], d + ["--weights", "luma"],
                d + ["--downsample", "bicubic"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    a = dms.parse_args(["--images", "x.npy", "--psf", "disk", "--blur_input", "--sigma_y", "0.05"])
    assert (a.psf, a.tol, a.blur_input, a.sigma_y, a.use_ddim, a.eta) == ("disk", blur.DEFAULT_TOL, True, 0.05, False, 0.0)
    assert dms.parse_args(["--images", "x.npy", "--psf", "disk"]).sigma_y == 0.0
    assert dms.parse_args(["--images", "x.npy", "--psf", "disk", "--use_ddim"]).sigma_y == 0.0      # the exact measurement takes a chain without draws
    assert dms.parse_args(["--images", "x.npy", "--psf", "disk", "--sigma_y", "0.1", "--use_ddim", "--eta", "0.5"]).eta == 0.5
    for bad in (["--images", "x.npy", "--psf", "disk", "--sigma_y", "-1"], ["--images", "x.npy", "--psf", "disk", "--sigma_y", "nan"],
                ["--images", "x.npy", "--psf", "disk", "--sigma_y", "0.1", "--use_ddim"], ["--images", "x.npy", "--sigma_y", "0.1"],
                ["--images", "x.npy", "--psf", "motion", "--sigma_y", "0.1"], ["--images", "x.npy", "--psf", "disk", "--sigma_y", "0.1", "--tol", "1"],
                ["--images", "x.npy", "--psf", "disk", "--sigma_y", "0.1", "--eta", "0.5"]):
        with pytest.raises(SystemExit):
            dms.parse_args(bad)
    u8 = np.zeros((1, 16, 16, 3), np.uint8)
    for kw in (dict(psf="disk"), dict(psf="disk", sigma_y=0.0), dict(psf="disk", sigma_y=-0.1), dict(psf="disk", sigma_y=True), dict(sigma_y=0.1),
               dict(psf="disk", sigma_y=0.1, scale=2), dict(psf="disk", sigma_y=0.1, dpm_solver=True), dict(psf="disk", sigma_y=0.1, method="repaint"),
               dict(psf="disk", sigma_y=0.1, kernel="gauss")):
        with pytest.raises(ValueError):
            RMx.evaluate_restoration(_tiny(), u8, "deconv_noisy", **kw)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(_tiny(), u8, "deconv", psf="disk", sigma_y=0.1)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(_tiny(), u8, "sr", psf="disk", sigma_y=0.1)
