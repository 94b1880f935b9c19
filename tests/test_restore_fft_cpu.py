"""DDNM deconvolution of a 2-D point-spread function on the CPU: the restatement tests/fft_conv_ref.py against
the operator's definition, the host side of models/diffusion/psf.py, every argument error of DDPM.deconvolve /
DownsampleDDPM.deconvolve before any device work, both command lines' parsers, and the header, the ctypes signatures and the built
library on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fft_conv_ref as FR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import blur, psf
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddk_circular_conv", "ddk_p_sample_update_restore_fft", "ddk_sampler_restore_fft_workspace_bytes",
       "ddk_sampler_restore_fft_tail_parts", "ddk_sampler_run_restore_fft")
SIZES = [(16, 16), (32, 16), (16, 64), (64, 64)]


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


# ---------------------------------------------------------------- the PSF and the projection
def test_presets():
    assert psf.PRESETS == ("diag", "disk") and blur.PRESETS == ("uniform", "gauss", "aniso")
    for name in psf.PRESETS:
        k = psf.psf_array(name)
        assert k.shape == (9, 9) and k.dtype == np.float64 and abs(k.sum() - 1.0) <= 1e-15 and (k >= 0).all()
        assert np.linalg.matrix_rank(k) > 1                 # no product of two 1-D kernels
        assert np.array_equal(k, FR.preset(name))
    assert np.array_equal(psf.psf_array("diag"), np.eye(9) / 9) and int((psf.psf_array("disk") > 0).sum()) == 37


@pytest.mark.parametrize("bad", ["box", np.ones((4, 3)), np.ones((3, 4)), np.ones(9), np.ones((3, 3, 3)), np.full((3, 3), np.nan),
                                 np.array([[1.0, -1.0, 0.0]]), [[1.0, float("inf"), 0.0]], None, [["a"]]])
def test_bad_psf_raises(bad):
    with pytest.raises(ValueError):
        psf.psf_array(bad)


def test_psf_array_takes_arrays_and_tensors():
    k = np.arange(15.0).reshape(3, 5)
    assert np.array_equal(psf.psf_array(k), k) and np.array_equal(psf.psf_array(torch.from_numpy(k).float()), k)
    assert psf.psf_array(k.tolist()).dtype == np.float64
    with pytest.raises(ValueError):
        psf.psf_spectrum(np.ones((17, 3)), 16, 16)          # larger than the plane


def test_the_definition_equals_a_direct_double_loop_at_16():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((16, 16))
    for k in (psf.psf_array("diag"), psf.psf_array("disk"), rng.standard_normal((5, 3)), rng.standard_normal((1, 7)), np.ones((1, 1)) * 0.5):
        want = FR.blur_direct(X, k)
        for K in (psf.psf_spectrum(k, 16, 16), FR.spectrum(k, 16, 16)):
            assert K.dtype == np.complex128
            assert np.abs(FR.apply(X[None, None], K)[0, 0] - want).max() <= 1e-13
    # the correlation form is blur.blur_matrix's: a separable PSF on a plane it cannot wrap around gives the same interior
    kh, kw = np.array([1.0, 2.0, 4.0]), np.array([3.0, 1.0, -1.0])
    sep = blur.blur_matrix(16, kh) @ X @ blur.blur_matrix(16, kw).T
    got = FR.apply(X[None, None], psf.psf_spectrum(np.outer(kh, kw), 16, 16))[0, 0]
    assert np.abs(got[1:-1, 1:-1] - sep[1:-1, 1:-1]).max() <= 1e-13


@pytest.mark.parametrize("name", psf.PRESETS)
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("tol", [0.03, 0.1])
def test_projection(name, H, W, tol):
    P, M, kept = psf.psf_projection(name, H, W, tol)
    K = psf.psf_spectrum(name, H, W)
    assert P.dtype == np.complex128 and M.dtype == np.bool_ and kept == int(M.sum()) and 0.16 * H * W <= kept <= 0.90 * H * W
    # the library's mask and the restatement's own agree, and M is symmetric under (u, v) -> (-u, -v)
    assert np.array_equal(M, FR.kept(FR.preset(name), H, W, tol))
    assert np.array_equal(M, M[(-np.arange(H)) % H][:, (-np.arange(W)) % W])
    assert np.abs(P - FR.pinv_spectrum(FR.preset(name), H, W, tol)).max() <= 1e-12 * np.abs(P).max()
    assert np.abs(np.abs(K) / np.abs(K).max() - tol).min() > 9e-7
    x = np.random.default_rng(H + W).standard_normal((2, 1, H, W))
    AtA = lambda v: FR.apply(FR.apply(v, K), P)
    p1 = AtA(x)
    assert np.abs(p1 - FR.apply(x, M.astype(np.float64))).max() <= 1e-12          # A+ A = F2^-1 M F2
    assert np.abs(AtA(p1) - p1).max() <= 1e-12                                     # idempotent
    assert np.abs(FR.apply(p1, K) - FR.apply(x, K * M)).max() <= 1e-12             # A A+ A = A on the kept set
    # the step's projection: the null-space part of x0' is x0's, the range-space part is Yp
    y = FR.apply(x, K)
    Yp = FR.apply(y, P)
    x0 = np.random.default_rng(1).standard_normal((2, 1, H, W))
    x0p = FR.project(torch.from_numpy(x0), Yp, M)
    null = lambda v: v - FR.apply(v, M.astype(np.float64))
    assert np.abs(null(x0p) - null(x0)).max() <= 1e-12
    assert np.abs(FR.apply(x0p, M.astype(np.float64)) - Yp).max() <= 1e-12


def test_one_tap_keeps_every_frequency_and_operands():
    P, M, kept = psf.psf_projection(np.array([[2.0]]), 16, 32, 0.5)
    assert kept == 512 and M.all() and np.abs(P - 0.5).max() <= 1e-15
    Kf, Pf, Mf, tw = psf.psf_operands("disk", 32, 16, 0.1)
    assert Kf.shape == Pf.shape == (32, 16, 2) and Mf.shape == (32, 16) and tw.shape == (16, 2)
    assert all(a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] for a in (Kf, Pf, Mf, tw))
    j = np.arange(16)
    assert np.abs(tw - np.stack([np.cos(2 * np.pi * j / 32), -np.sin(2 * np.pi * j / 32)], axis=1)).max() <= 2.0 ** -24
    assert set(np.unique(Mf)) == {0.0, 1.0}
    for tol in (-0.1, 1.0, True, "x", None):
        with pytest.raises(ValueError):
            psf.psf_projection("disk", 16, 16, tol)
    assert psf.size_ok(3, 16, 256) and not any(psf.size_ok(*s) for s in ((3, 8, 16), (3, 24, 16), (3, 16, 48), (3, 512, 16), (0, 16, 16), (9, 16, 16)))


def test_restatement_step_at_row_0_returns_the_projection():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    M = FR.kept(FR.preset("disk"), 16, 16, 0.1)
    Yp = torch.from_numpy(FR.apply(torch.randn(2, 3, 16, 16, generator=g), M.astype(np.float64)))
    one = torch.ones(2)
    out, x0, x0p = FR.step(x, torch.zeros_like(x), M, Yp, one, 0 * one, one, 0 * one, 0 * one, torch.zeros_like(x))
    assert torch.equal(x0, x) and torch.equal(out, x0p)
    assert np.abs(FR.apply(out, M.astype(np.float64)) - Yp.numpy()).max() <= 1e-13


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def test_the_downsampled_model_has_no_deconvolve():
    cfg = dddpm_cfg(32, 32, 2)
    with pytest.raises(ValueError, match="latent"):
        DownsampleDDPM(cfg, Unet(cfg), "cpu", 3).deconvolve(torch.zeros(1, 3, 32, 32), "disk")


@pytest.mark.parametrize("y", [torch.zeros(2, 3, 64), torch.zeros(2, 1, 16, 16), torch.zeros(2, 3, 16, 32), torch.zeros(2, 3, 16, 16, dtype=torch.long),
                               torch.zeros(0, 3, 16, 16), torch.full((2, 3, 16, 16), float("nan")), torch.full((2, 3, 16, 16), float("inf")), [[0.0]]])
def test_bad_y_raises(y):
    with pytest.raises(ValueError):
        _tiny().deconvolve(y, "disk")


@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(eta=True), dict(solver="dpm++2m"), dict(noise=torch.zeros(1)),
                                dict(early_stop=10), dict(paste=True), dict(mask=torch.ones(16, 16)), dict(sigma_y=0.1), dict(tol=1.0),
                                dict(tol=-0.1), dict(tol=True), dict(tol="x"), dict(kernel="gauss"), dict(perm_seed=1)])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError):
        _tiny().deconvolve(torch.zeros(2, 3, 16, 16), "disk", **kw)


@pytest.mark.parametrize("k", ["motion", "gauss", np.ones((4, 4)), np.ones((17, 3)), np.ones((3, 17)), np.zeros((3, 3)), np.full((3, 3), np.nan)])
def test_bad_psf_is_refused_by_the_model(k):
    with pytest.raises(ValueError):
        _tiny().deconvolve(torch.zeros(2, 3, 16, 16), k)


@pytest.mark.parametrize("size", [24, 48, 8])
def test_an_image_size_off_the_grid_raises(size):
    cfg = ddpm_cfg(32, 3, size)
    with pytest.raises(ValueError, match="powers of two"):
        DDPM(cfg, Unet(cfg), "cpu", 3).deconvolve(torch.zeros(1, 3, size, size), np.ones((1, 1)))


def test_good_arguments_reach_the_device_check():
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().deconvolve(torch.zeros(2, 3, 16, 16), "diag", respacing="20", ddim=True, eta=0.3)
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().deconvolve(torch.zeros(2, 3, 16, 16), np.random.default_rng(0).standard_normal((5, 3)), tol=0.1)


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    from ddk import ops, plan
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
        params = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[name][1]), name
    assert len(L.SIGNATURES["ddk_circular_conv"][1]) == 10
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_fft"][1]) == 19
    assert len(L.SIGNATURES["ddk_sampler_run_restore_fft"][1]) == 7
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert callable(ops.circular_conv) and callable(ops.p_sample_update_restore_fft_)
    assert plan.UnetPlan.RESTORE_ENTRIES["srf"] == ("sampler_run_restore_fft", "sampler_restore_fft_workspace_bytes", "sampler_restore_fft_tail_parts")
    assert "srf" in plan.SAMPLERS and "srf" in plan.CHAIN_WORKSPACES and callable(plan.UnetPlan.sample_restore_fft_nhwc)
    assert callable(plan.UnetPlan.restore_fft_tail_parts)


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only: the workspace holds the plain sampler's plus the mask (H W floats), the twiddles (max(H, W) floats), Yp
    (the latent's size) and the complex T (twice the latent's size); no shape takes the fused tail; off-grid shapes give 0"""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    for B, H, W in ((32, 32, 32), (2, 16, 64), (1, 256, 256)):
        plain = lib.ddk_sampler_workspace_bytes(h, B, H, W, 49)
        got = lib.ddk_sampler_restore_fft_workspace_bytes(h, B, H, W, 49)
        assert plain > 0 and got == plain + 4 * (H * W + max(H, W) + 3 * B * H * W * 3), (B, H, W)
        assert lib.ddk_sampler_restore_fft_tail_parts(h, B, H, W) == 0
    assert lib.ddk_sampler_restore_tail_parts(h, 32, 32, 32, 2) == 8      # the shape does have a fused tail: the plane-wide kind declines it
    for H, W in ((24, 24), (16, 48), (512, 512), (8, 16)):
        assert lib.ddk_sampler_restore_fft_workspace_bytes(h, 2, H, W, 49) == 0
    # the older queries are what they were
    assert lib.ddk_sampler_restore_cs_workspace_bytes(h, 2, 16, 64, 49) == lib.ddk_sampler_workspace_bytes(h, 2, 16, 64, 49) + \
        4 * (16 * 64 + 2 * 2 * 16 * 64 * 3)


def test_off_grid_arguments_are_err_arg_before_any_launch():
    """the lone entries refuse every off-grid shape on the host: no device is needed to be told so"""
    lib = L.load()
    buf = (ctypes.c_char * 272)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 16-byte aligned host memory: never read, no call gets as far as a launch
    for B, H, W, C in ((1, 24, 16, 3), (1, 16, 48, 3), (1, 512, 16, 3), (1, 8, 16, 3), (1, 16, 16, 9), (1, 16, 16, 0), (0, 16, 16, 3),
                       (30000, 16, 16, 3)):
        assert lib.ddk_circular_conv(p, p, p, p, None, B, H, W, C, None) == -1, (B, H, W, C)
        assert lib.ddk_p_sample_update_restore_fft(p, p, p, p, p, None, p, p, p, p, p, p, B, H, W, C, 0, 0, None) == -1, (B, H, W, C)
    assert lib.ddk_circular_conv(p, p, p, p, None, 1, 128, 256, 3, None) == -1 and "scratch" in L.last_error()
    assert lib.ddk_p_sample_update_restore_fft(p, p, p, p, p, None, p, p, p, p, p, p, 1, 256, 256, 3, 0, 0, None) == -1 and "scratch" in L.last_error()
    assert lib.ddk_circular_conv(p, None, p, p, None, 1, 16, 16, 3, None) == -1 and "null" in L.last_error()
    assert lib.ddk_p_sample_update_restore_fft(p, p, None, p, p, None, p, p, p, p, p, p, 1, 16, 16, 3, 0, 0, None) == -1 and "null" in L.last_error()
    q = ctypes.c_void_p(p.value + 4)
    assert lib.ddk_circular_conv(q, p, p, p, None, 1, 16, 16, 3, None) == -1 and "alignment" in L.last_error()


def test_the_evaluator_and_the_cli_know_the_task():
    import deconv_model_samples as dms
    import evaluate_restoration as cli
    from utils import restoration_metrics as RMx
    assert RMx.DECONV_TASK == "deconv" and RMx.CS_TASK == "cs" and RMx.DEBLUR_TASK == "deblur"
    assert RMx.TASKS == ("inpaint", "sr", "colorize") and RMx.BLUR_KERNELS == ("uniform", "gauss", "aniso")
    a = cli.parse_args(["--task", "deconv", "--psf", "disk"])
    assert cli.chain_options(a) == dict(respacing=None, psf="disk", tol=3e-2, ddim=False, eta=0.0)
    a = cli.parse_args(["--task", "deconv", "--psf", "k.npy", "--tol", "0.1", "--use_ddim", "--eta", "0.5", "--timestep_respacing", "20"])
    assert cli.chain_options(a) == dict(respacing="20", psf="k.npy", tol=0.1, ddim=True, eta=0.5)
    # the existing tasks parse to what they did
    assert cli.chain_options(cli.parse_args(["--task", "sr"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "deblur", "--kernel", "gauss"])) == dict(respacing=None, kernel="gauss", tol=3e-2, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "cs", "--ratio", "0.25"])) == dict(respacing=None, ratio=0.25, perm_seed=0, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "inpaint"])) == dict(respacing=None, jump_length=10, jump_n_sample=10)
    assert cli.chain_options(cli.parse_args(["--task", "colorize"])) == dict(respacing=None, scale=1, weights="mean", ddim=False, eta=0.0)
    d = ["--task", "deconv", "--psf", "diag"]
    for bad in (["--task", "sr", "--psf", "disk"], ["--task", "inpaint", "--psf", "disk"], ["--task", "deblur", "--kernel", "gauss", "--psf", "disk"],
                ["--task", "cs", "--ratio", "0.5", "--psf", "disk"], ["--task", "colorize", "--psf", "diag"], ["--task", "sr", "--tol", "0.1"],
                ["--task", "cs", "--ratio", "0.5", "--tol", "0.1"],
                d + ["--scale", "2"], d + ["--mask", "half"], d + ["--sigma_y", "0.1"], d + ["--dpm_solver"], d + ["--method", "repaint"],
                d + ["--method", "ddnm"], d + ["--kernel", "gauss"], d + ["--ratio", "0.5"], d + ["--perm_seed", "1"], ["--task", "deconv"],
                ["--task", "deconv", "--psf", "motion"], d + ["--tol", "1"], d + ["--tol", "-0.5"], d + ["--eta", "0.5"], d + ["--jump_length", "5"],
                d + ["--weights", "luma"], d + ["--downsample", "bicubic"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    a = dms.parse_args(["--images", "x.npy", "--psf", "disk", "--blur_input", "--tol", "0.1"])
    assert (a.psf, a.tol, a.blur_input, a.use_ddim, a.eta, a.timestep_respacing) == ("disk", 0.1, True, False, 0.0, "")
    assert dms.parse_args(["--images", "x.npy", "--psf", "measured.npy"]).tol == blur.DEFAULT_TOL
    for bad in (["--images", "x.npy"], ["--images", "x.npy", "--psf", "motion"], ["--images", "x.npy", "--psf", "disk", "--tol", "1"],
                ["--images", "x.npy", "--psf", "disk", "--eta", "0.5"], ["--images", "x.npy", "--psf", "disk", "--batch_size", "0"],
                ["--psf", "disk"], []):
        with pytest.raises(SystemExit):
            dms.parse_args(bad)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(None, np.zeros((1, 16, 16, 3), np.uint8), "sr", psf="disk")
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(None, np.zeros((1, 16, 16, 3), np.uint8), "deconv", psf="disk", scale=2)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(_tiny(), np.zeros((1, 16, 16, 3), np.uint8), "deconv")
