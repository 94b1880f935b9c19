"""DDNM compressed sensing on the CPU: the restatement tests/hadamard_ref.py against the operator's definition,
the host side of models/diffusion/hadamard.py, every argument error of DDPM.restore_cs / DownsampleDDPM.restore_cs before any device
work, both command lines' parsers, and the header, the ctypes signatures and the built library on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import hadamard_ref as HR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import hadamard
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddk_hadamard_measure", "ddk_hadamard_adjoint", "ddk_p_sample_update_restore_cs", "ddk_sampler_restore_cs_workspace_bytes",
       "ddk_sampler_restore_cs_tail_parts", "ddk_sampler_run_restore_cs")


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


# ---------------------------------------------------------------- the restatement itself, at N = 256
def test_the_restatement_is_the_sylvester_matrix():
    N = 256
    W = HR.sylvester(N)
    # Sylvester's recursion, independently of the popcount definition
    S = np.ones((1, 1))
    while S.shape[0] < N:
        S = np.block([[S, S], [S, -S]])
    assert np.array_equal(W * 16.0, S)
    assert np.array_equal(W, W.T) and np.abs(W @ W.T - np.eye(N)).max() <= 1e-15
    a = np.random.default_rng(0).standard_normal((2, 3, N))
    assert np.abs(HR.fwht(a) - a @ W.T).max() <= 1e-13
    ai = np.random.default_rng(1).integers(-5, 6, size=(2, N))
    assert np.array_equal(HR.fwht_int(ai), ai @ S.astype(np.int64).T)


@pytest.mark.parametrize("m", [4, 100, 64, 252, 256])
def test_the_rows_are_orthonormal(m):
    N, shape = 256, (2, 3, 16, 16)
    perm = np.random.default_rng(3).permutation(N).astype(np.int32)
    # A as a matrix: row k of W with its columns moved to the pixels they read
    A = np.zeros((m, N))
    A[:, perm.astype(np.int64)] = HR.sylvester(N)[:m]
    assert np.abs(A @ A.T - np.eye(m)).max() <= 1e-14
    g = torch.Generator().manual_seed(m)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    y = HR.measure(x, perm, m)
    assert y.shape == (2, 3, m) and np.abs(y - HR.planes(x) @ A.T).max() <= 1e-13
    yy = np.random.default_rng(m).standard_normal((2, 3, m))
    back = HR.adjoint(yy, perm, shape)
    assert np.abs(HR.planes(back) - yy @ A).max() <= 1e-13
    assert np.abs(HR.measure(back, perm, m) - yy).max() <= 1e-13          # A (A^T y) = y
    # the projection keeps y and everything outside the measured coefficients
    x0p, v, w = HR.project(x, yy, perm)
    assert np.abs(HR.measure(x0p, perm, m) - yy).max() <= 1e-13
    full = HR.measure(x0p, perm, N)
    assert np.abs(full[..., m:] - v[..., m:]).max(initial=0.0) <= 1e-13 and np.array_equal(w[..., :m], yy)


def test_restatement_step_at_row_0_returns_the_projection():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    y = np.random.default_rng(0).standard_normal((2, 3, 100))
    perm = hadamard.cs_perm(256, 1)
    one = torch.ones(2)
    out, x0, x0p, _ = HR.step(x, torch.zeros_like(x), y, perm, one, 0 * one, one, 0 * one, 0 * one, torch.zeros_like(x))
    assert torch.equal(x0, x) and torch.equal(out, x0p)
    assert np.abs(HR.measure(out, perm, 100) - y).max() <= 1e-13


# ---------------------------------------------------------------- the host side
def test_cs_rows_and_cs_perm():
    assert [hadamard.cs_rows(r, 256) for r in (0.5, 0.25, 0.1, 1, 1.0, 0.001, 0.99)] == [128, 64, 24, 256, 256, 4, 252]
    assert [hadamard.cs_rows(r, 65536) for r in (0.5, 0.25, 0.1)] == [32768, 16384, 6552]
    assert hadamard.cs_rows(0.3, 512) == 4 * round(0.3 * 512 / 4) == 152
    for bad in (0, -0.1, 1.5, "x", True, None, float("nan")):
        with pytest.raises(ValueError):
            hadamard.cs_rows(bad, 256)
    p = hadamard.cs_perm(256)
    assert p.dtype == np.int32 and p.shape == (256,) and np.array_equal(p, np.random.default_rng(0).permutation(256))
    assert np.array_equal(hadamard.cs_perm(1024, 7), np.random.default_rng(7).permutation(1024))
    assert not np.array_equal(hadamard.cs_perm(256, 1), p) and np.array_equal(np.sort(p), np.arange(256))
    assert np.array_equal(hadamard.check_perm(list(range(255, -1, -1)), 256), np.arange(255, -1, -1))
    assert hadamard.check_perm(torch.arange(256), 256).dtype == np.int32
    for bad in (np.arange(255), np.zeros(256, dtype=np.int64), np.arange(256) + 1, np.arange(256, dtype=np.float64), np.arange(512).reshape(2, 256),
                "perm", np.r_[np.arange(255), -1]):
        with pytest.raises(ValueError):
            hadamard.check_perm(bad, 256)
    assert hadamard.size_ok(3, 16, 16) and hadamard.size_ok(1, 16, 256) and hadamard.size_ok(8, 256, 256)
    assert not any(hadamard.size_ok(*s) for s in ((3, 8, 16), (3, 24, 16), (3, 16, 48), (3, 512, 16), (0, 16, 16), (9, 16, 16)))


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def test_the_downsampled_model_has_no_restore_cs():
    cfg = dddpm_cfg(32, 32, 2)
    with pytest.raises(ValueError, match="latent"):
        DownsampleDDPM(cfg, Unet(cfg), "cpu", 3).restore_cs(torch.zeros(1, 3, 64))


@pytest.mark.parametrize("y", [torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 64), torch.zeros(3, 64), torch.zeros(2, 3, 64, dtype=torch.long),
                               torch.zeros(2, 3, 62), torch.zeros(2, 3, 0), torch.zeros(2, 3, 260), torch.zeros(0, 3, 64),
                               torch.full((2, 3, 64), float("nan")), torch.full((2, 3, 64), float("inf")), [[0.0]]])
def test_bad_y_raises(y):
    with pytest.raises(ValueError):
        _tiny().restore_cs(y)


@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(eta=True), dict(solver="dpm++2m"), dict(noise=torch.zeros(1)),
                                dict(early_stop=10), dict(paste=True), dict(mask=torch.ones(16, 16)), dict(sigma_y=0.1), dict(perm=np.arange(255)),
                                dict(perm=np.zeros(256, dtype=np.int32)), dict(perm=np.arange(256.0)), dict(perm_seed=-1), dict(perm_seed=0.5),
                                dict(tol=0.1), dict(kernel="gauss")])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError):
        _tiny().restore_cs(torch.zeros(2, 3, 64), **kw)


@pytest.mark.parametrize("size", [24, 48, 8])
def test_an_image_size_off_the_grid_raises(size):
    cfg = ddpm_cfg(32, 3, size)
    with pytest.raises(ValueError, match="powers of two"):
        DDPM(cfg, Unet(cfg), "cpu", 3).restore_cs(torch.zeros(1, 3, 64))


def test_good_arguments_reach_the_device_check():
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().restore_cs(torch.zeros(2, 3, 64), respacing="20", ddim=True, eta=0.3)
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().restore_cs(torch.zeros(2, 3, 256), np.arange(256)[::-1].copy(), perm_seed=5)


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
    assert len(L.SIGNATURES["ddk_hadamard_measure"][1]) == len(L.SIGNATURES["ddk_hadamard_adjoint"][1]) == 10
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_cs"][1]) == 19
    assert len(L.SIGNATURES["ddk_sampler_run_restore_cs"][1]) == 6
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert callable(ops.hadamard_measure) and callable(ops.hadamard_adjoint) and callable(ops.p_sample_update_restore_cs_)
    assert plan.UnetPlan.RESTORE_ENTRIES["src"] == ("sampler_run_restore_cs", "sampler_restore_cs_workspace_bytes", "sampler_restore_cs_tail_parts")
    assert "src" in plan.SAMPLERS and "src" in plan.CHAIN_WORKSPACES and callable(plan.UnetPlan.sample_restore_cs_nhwc)
    assert callable(plan.UnetPlan.restore_cs_tail_parts)


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only: the workspace holds the plain sampler's plus perm (H W words), y (the latent's size) and T (the latent's
    size); no shape takes the fused tail; off-grid shapes give 0"""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    for B, H, W in ((32, 32, 32), (2, 16, 64), (1, 64, 64), (1, 256, 256)):
        plain = lib.ddk_sampler_workspace_bytes(h, B, H, W, 49)
        got = lib.ddk_sampler_restore_cs_workspace_bytes(h, B, H, W, 49)
        assert plain > 0 and got == plain + 4 * (H * W + 2 * B * H * W * 3), (B, H, W)
        assert lib.ddk_sampler_restore_cs_tail_parts(h, B, H, W) == 0
    assert lib.ddk_sampler_restore_tail_parts(h, 32, 32, 32, 2) == 8      # the shape does have a fused tail: the plane-wide kind declines it
    for H, W in ((24, 24), (16, 48), (512, 512), (8, 16)):
        assert lib.ddk_sampler_restore_cs_workspace_bytes(h, 2, H, W, 49) == 0
    # the older queries are what they were
    assert lib.ddk_sampler_restore_blur_workspace_bytes(h, 2, 16, 48, 49) == lib.ddk_sampler_workspace_bytes(h, 2, 16, 48, 49) + \
        4 * (16 * 16 + 48 * 48 + 2 * 2 * 16 * 48 * 3)


def test_off_grid_arguments_are_err_arg_before_any_launch():
    """the lone entries refuse every off-grid shape on the host: no device is needed to be told so"""
    lib = L.load()
    buf = (ctypes.c_char * 272)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 16-byte aligned host memory: never read, no call gets as far as a launch
    for B, H, W, C, m in ((1, 24, 16, 3, 8), (1, 16, 48, 3, 8), (1, 512, 16, 3, 8), (1, 8, 16, 3, 8), (1, 16, 16, 9, 8), (1, 16, 16, 0, 8),
                          (1, 16, 16, 3, 6), (1, 16, 16, 3, 0), (1, 16, 16, 3, 260), (0, 16, 16, 3, 8), (30000, 16, 16, 3, 8)):
        assert lib.ddk_hadamard_measure(p, p, p, None, B, H, W, C, m, None) == -1, (B, H, W, C, m)
        assert lib.ddk_hadamard_adjoint(p, p, p, None, B, H, W, C, m, None) == -1, (B, H, W, C, m)
        assert lib.ddk_p_sample_update_restore_cs(p, p, p, p, None, p, p, p, p, p, p, B, H, W, C, m, 0, 0, None) == -1, (B, H, W, C, m)
    assert lib.ddk_hadamard_measure(p, p, p, None, 1, 256, 256, 3, 8, None) == -1 and "scratch" in L.last_error()
    assert lib.ddk_p_sample_update_restore_cs(p, p, p, p, None, p, p, p, p, p, p, 1, 256, 256, 3, 8, 0, 0, None) == -1 and "scratch" in L.last_error()
    assert lib.ddk_hadamard_measure(p, None, p, None, 1, 16, 16, 3, 8, None) == -1 and "null" in L.last_error()


def test_the_evaluator_and_the_cli_know_the_task():
    import cs_model_samples as cms
    import evaluate_restoration as cli
    from utils import restoration_metrics as RMx
    assert RMx.CS_TASK == "cs" and RMx.DEBLUR_TASK == "deblur"
    assert RMx.TASKS == ("inpaint", "sr", "colorize") and RMx.MASKS == ("center", "left", "half", "lines")
    assert RMx.DOWNSAMPLES == ("mean", "bicubic") and RMx.BLUR_KERNELS == ("uniform", "gauss", "aniso")
    a = cli.parse_args(["--task", "cs", "--ratio", "0.25"])
    assert cli.chain_options(a) == dict(respacing=None, ratio=0.25, perm_seed=0, ddim=False, eta=0.0)
    a = cli.parse_args(["--task", "cs", "--ratio", "0.1", "--perm_seed", "3", "--use_ddim", "--eta", "0.5", "--timestep_respacing", "20"])
    assert cli.chain_options(a) == dict(respacing="20", ratio=0.1, perm_seed=3, ddim=True, eta=0.5)
    # the existing tasks parse to what they did
    assert cli.chain_options(cli.parse_args(["--task", "sr"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "deblur", "--kernel", "gauss"])) == dict(respacing=None, kernel="gauss", tol=3e-2, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "inpaint"])) == dict(respacing=None, jump_length=10, jump_n_sample=10)
    d = ["--task", "cs", "--ratio", "0.25"]
    for bad in (["--task", "sr", "--ratio", "0.5"], ["--task", "inpaint", "--perm_seed", "1"], ["--task", "deblur", "--kernel", "gauss", "--ratio", "0.5"],
                d + ["--scale", "2"], d + ["--mask", "half"], d + ["--sigma_y", "0.1"], d + ["--dpm_solver"], d + ["--method", "repaint"],
                d + ["--method", "ddnm"], d + ["--kernel", "gauss"], d + ["--tol", "0.1"], ["--task", "cs"], ["--task", "cs", "--ratio", "0"],
                ["--task", "cs", "--ratio", "1.5"], d + ["--perm_seed", "-1"], d + ["--eta", "0.5"], d + ["--jump_length", "5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    a = cms.parse_args(["--images", "x.npy", "--ratio", "0.5", "--measure_input", "--perm_seed", "4"])
    assert (a.ratio, a.perm_seed, a.measure_input, a.use_ddim, a.eta, a.timestep_respacing) == (0.5, 4, True, False, 0.0, "")
    assert cms.parse_args(["--images", "x.npy", "--ratio", "1"]).ratio == 1.0
    for bad in (["--images", "x.npy", "--ratio", "0"], ["--images", "x.npy", "--ratio", "1.01"], ["--images", "x.npy", "--eta", "0.5"],
                ["--images", "x.npy", "--perm_seed", "-2"], ["--images", "x.npy", "--batch_size", "0"], []):
        with pytest.raises(SystemExit):
            cms.parse_args(bad)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(None, np.zeros((1, 16, 16, 3), np.uint8), "sr", ratio=0.5)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(None, np.zeros((1, 16, 16, 3), np.uint8), "cs", ratio=0.5, scale=2)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(_tiny(), np.zeros((1, 16, 16, 3), np.uint8), "cs")
