"""DDNM deblurring on the CPU: the host mathematics of models/diffusion/blur.py (presets, band matrices, the
per-axis truncated pseudo-inverse and its projection) against their definitions and against the independent tests/blur_ref.py, the
tables' row 0, every argument error of DDPM.deblur / DownsampleDDPM.deblur before any device work, and the header, the ctypes
signatures and the built library on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import blur_ref as BR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import blur
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddk_separable_apply", "ddk_p_sample_update_restore_blur", "ddk_sampler_restore_blur_workspace_bytes",
       "ddk_sampler_restore_blur_tail_parts", "ddk_sampler_run_restore_blur")
TABLE_SETS = [dict(respacing=None), dict(respacing="20"), dict(respacing="20", ddim=True), dict(respacing="ddim50", ddim=True, eta=0.7)]
# (kernel, size) -> retained rank at tol = 3e-2
RANKS = {("gauss", 16): 16, ("uniform", 16): 14, ("uniform", 64): 57, ("uniform", 256): 228}


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


# ---------------------------------------------------------------- the host mathematics
def test_presets_give_the_stated_taps():
    k_h, k_w = blur.blur_kernel("uniform")
    assert k_h.shape == k_w.shape == (9,) and np.array_equal(k_h, np.full(9, 1.0 / 9.0)) and np.array_equal(k_w, k_h)
    k_h, k_w = blur.blur_kernel("gauss")
    want = np.exp(-0.5 * (np.arange(-2, 3) / 10.0) ** 2)
    assert k_h.shape == (5,) and np.allclose(k_h, want / want.sum(), rtol=0, atol=1e-15) and np.array_equal(k_w, k_h)
    k_h, k_w = blur.blur_kernel("aniso")
    r = np.arange(-4, 5)
    for k, s in ((k_h, 20.0), (k_w, 1.0)):
        want = np.exp(-0.5 * (r / s) ** 2)
        assert k.shape == (9,) and np.allclose(k, want / want.sum(), rtol=0, atol=1e-15)
    for name in blur.PRESETS:
        for k in blur.blur_kernel(name):
            assert k.dtype == np.float64 and abs(k.sum() - 1.0) < 1e-15 and np.array_equal(k, k[::-1])
    # an array serves both axes, a pair one each
    k_h, k_w = blur.blur_kernel([0.25, 0.5, 0.25])
    assert np.array_equal(k_h, [0.25, 0.5, 0.25]) and np.array_equal(k_w, k_h)
    k_h, k_w = blur.blur_kernel(([1.0], np.array([0.2, 0.6, 0.2])))
    assert np.array_equal(k_h, [1.0]) and np.array_equal(k_w, [0.2, 0.6, 0.2])
    assert np.array_equal(blur.blur_kernel(torch.tensor([0.5, 0.0, 0.5]))[0], [0.5, 0.0, 0.5])


@pytest.mark.parametrize("bad", ["box", [0.5, 0.5], np.ones((3, 3)), [1.0, float("nan"), 0.0], ([1.0], [0.5, 0.5]), []])
def test_bad_kernels_raise(bad):
    with pytest.raises(ValueError):
        blur.blur_kernel(bad)


@pytest.mark.parametrize("kernel", ["uniform", "gauss", "aniso", ([0.1, 0.2, 0.4, 0.2, 0.1], [0.3, 0.4, 0.3])])
def test_blur_matrix_is_the_zero_padded_convolution(kernel):
    g = torch.Generator().manual_seed(5)
    H, W = 32, 48
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    k_h, k_w = blur.blur_kernel(kernel)
    A_h, A_w = blur.blur_matrix(H, k_h), blur.blur_matrix(W, k_w)
    got = torch.einsum("ih,bchw,jw->bcij", torch.from_numpy(A_h), x, torch.from_numpy(A_w))
    # conv2d is a correlation: out[i, j] = sum k2[a, b] x[i + a - L/2, j + b - L/2], which is A[i, i + a - L/2] = k[a]
    k2 = torch.from_numpy(np.outer(k_h, k_w)).reshape(1, 1, len(k_h), len(k_w))
    want = torch.nn.functional.conv2d(x.reshape(6, 1, H, W), k2, padding=(len(k_h) // 2, len(k_w) // 2)).reshape(2, 3, H, W)
    err = float((got - want).abs().max())
    print(f"blur_matrix vs conv2d, {kernel if isinstance(kernel, str) else 'pair'}: {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("kernel,n", list(RANKS))
def test_projection_properties_and_ranks(kernel, n):
    A = blur.blur_matrix(n, blur.blur_kernel(kernel)[0])
    Q, P, rank = blur.blur_projection(A, 3e-2)
    assert Q.dtype == P.dtype == np.float64 and rank == RANKS[(kernel, n)]
    errs = dict(sym=np.abs(P - P.T).max(), idem=np.abs(P @ P - P).max(), pq=np.abs(P @ Q - Q).max())
    print(f"{kernel} {n}: rank {rank} of {n}, max|Q| {np.abs(Q).max():.3g}, {errs}")
    assert max(errs.values()) <= 1e-10
    assert np.abs(Q).max() < 12
    assert abs(np.trace(P) - rank) < 1e-9


@pytest.mark.parametrize("kernel,H,W,tol", [("gauss", 16, 16, 3e-2), ("uniform", 16, 48, 3e-2), ("aniso", 64, 32, 3e-2), ("uniform", 256, 16, 3e-2),
                                            ("uniform", 32, 32, 0.1), ([0.25, 0.5, 0.25], 16, 16, 1e-3)])
def test_blur_py_agrees_with_the_restatement(kernel, H, W, tol):
    k_h, k_w = blur.blur_kernel(kernel)
    r_h, r_w = BR.taps(kernel)
    assert np.abs(k_h - r_h).max() <= 1e-15 and np.abs(k_w - r_w).max() <= 1e-15
    ref = BR.operands(kernel, H, W, tol)
    for axis, n, k in (("h", H, k_h), ("w", W, k_w)):
        A = blur.blur_matrix(n, k)
        Q, P, _ = blur.blur_projection(A, tol)
        for name, got in (("A", A), ("Q", Q), ("P", P)):
            err = float(np.abs(got - ref[f"{name}_{axis}"].numpy()).max())
            assert err <= 1e-12, (name, axis, err)
    # the fp32 operands are those matrices rounded once, in the documented order, and cached
    ops32 = blur.blur_operands(kernel, H, W, tol)
    for got, name in zip(ops32, ("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w")):
        assert got.dtype == torch.float32 and float((got.double() - ref[name]).abs().max()) <= 2.0 ** -24 * max(1.0, float(ref[name].abs().max())) + 1e-12
    assert blur.blur_operands(kernel, H, W, tol)[0] is ops32[0]


def test_restatement_step_keeps_the_invariant():
    """P_h x0' P_w^T == Yp in float64 (P Q = Q), and the null-space part of x0 is kept"""
    g = torch.Generator().manual_seed(3)
    m = BR.operands("uniform", 32, 16)
    x0 = torch.rand(2, 3, 32, 16, generator=g) * 2 - 1
    y = BR.apply(torch.rand(2, 3, 32, 16, generator=g) * 2 - 1, m["A_h"], m["A_w"])
    Yp = BR.apply(y, m["Q_h"], m["Q_w"])
    one = torch.ones(2)
    out, _, x0p = BR.step(x0, torch.zeros_like(x0), m["P_h"], m["P_w"], Yp, one, 0 * one, one, 0 * one, 0 * one, torch.zeros_like(x0))
    assert torch.equal(out, x0p)
    assert float((BR.apply(x0p, m["P_h"], m["P_w"]) - Yp).abs().max()) <= 1e-12
    null = lambda v: v.double() - BR.apply(v, m["P_h"], m["P_w"])
    assert float((null(x0p) - null(x0)).abs().max()) <= 1e-12
    gap = float((BR.apply(x0p, m["A_h"], m["A_w"]) - y).abs().max())
    print(f"max|A(x0') - y| = {gap:.3g} (limited by the truncation; not asserted)")


@pytest.mark.parametrize("kw", TABLE_SETS, ids=lambda kw: str(kw))
def test_row_0_of_every_table_set_returns_x0(kw):
    m = _tiny()
    spaced = kw["respacing"] is not None or kw.get("ddim", False)
    tables = m._spaced_tables(kw["respacing"], kw.get("ddim", False), kw.get("eta", 0.0))[0] if spaced else m._tables()
    assert float(tables["c1"][0]) == 1.0 and float(tables["c2"][0]) == 0.0


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
def test_the_downsampled_model_has_no_deblur():
    cfg = dddpm_cfg(32, 32, 2)
    with pytest.raises(ValueError, match="latent"):
        DownsampleDDPM(cfg, Unet(cfg), "cpu", 3).deblur(torch.zeros(1, 3, 32, 32))


@pytest.mark.parametrize("y", [torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 16, 16), torch.zeros(3, 16, 16), torch.zeros(2, 3, 16, 16, dtype=torch.long),
                               torch.full((2, 3, 16, 16), float("nan")), torch.full((2, 3, 16, 16), float("inf")), [[0.0]]])
def test_bad_y_raises(y):
    with pytest.raises(ValueError):
        _tiny().deblur(y)


@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(solver="dpm++2m"), dict(noise=torch.zeros(1)), dict(early_stop=10),
                                dict(paste=True), dict(mask=torch.ones(16, 16)), dict(sigma_y=0.1), dict(tol=1.0), dict(tol=-0.1), dict(tol="x"),
                                dict(kernel="motion"), dict(kernel=[0.5, 0.5])])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError):
        _tiny().deblur(torch.zeros(2, 3, 16, 16), **kw)


def test_an_image_size_the_kernels_do_not_take_raises():
    cfg = ddpm_cfg(32, 3, 24)
    with pytest.raises(ValueError, match="multiples of 16"):
        DDPM(cfg, Unet(cfg), "cpu", 3).deblur(torch.zeros(1, 3, 24, 24))


def test_good_arguments_reach_the_device_check():
    with pytest.raises(L.DDKError, match="ROCm"):
        _tiny().deblur(torch.zeros(2, 3, 16, 16), "uniform", respacing="20", ddim=True, eta=0.3)


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
    assert len(L.SIGNATURES["ddk_separable_apply"][1]) == 9
    assert len(L.SIGNATURES["ddk_p_sample_update_restore_blur"][1]) == 19
    assert len(L.SIGNATURES["ddk_sampler_run_restore_blur"][1]) == 8
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert callable(ops.separable_apply) and callable(ops.p_sample_update_restore_blur_)
    assert plan.UnetPlan.RESTORE_ENTRIES["srb"] == ("sampler_run_restore_blur", "sampler_restore_blur_workspace_bytes",
                                                    "sampler_restore_blur_tail_parts")
    assert "srb" in plan.SAMPLERS and callable(plan.UnetPlan.sample_restore_blur_nhwc)


def test_workspace_query_and_tail_eligibility_on_the_host():
    """host arithmetic only: the workspace holds the plain sampler's plus P_h, P_w, Yp and T; no shape takes the fused tail"""
    lib = L.load()
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    h = u._plan.handle
    for B, H, W in ((32, 32, 32), (2, 16, 48), (1, 64, 64)):
        plain = lib.ddk_sampler_workspace_bytes(h, B, H, W, 49)
        got = lib.ddk_sampler_restore_blur_workspace_bytes(h, B, H, W, 49)
        assert got == plain + 4 * (H * H + W * W + 2 * B * H * W * 3), (B, H, W)
        assert lib.ddk_sampler_restore_blur_tail_parts(h, B, H, W) == 0
        assert lib.ddk_sampler_restore_tail_parts(h, B, H, W, 2) >= 0
    assert lib.ddk_sampler_restore_tail_parts(h, 32, 32, 32, 2) == 8      # the shape does have a fused tail: the blur kind declines it
    assert lib.ddk_sampler_restore_blur_workspace_bytes(h, 2, 24, 24, 49) == 0
    assert lib.ddk_sampler_restore_blur_workspace_bytes(h, 2, 272, 272, 49) == 0


def test_the_evaluator_and_the_cli_know_the_task():
    import deblur_model_samples as dms
    import evaluate_restoration as cli
    from utils import restoration_metrics as RMx
    assert RMx.DEBLUR_TASK == "deblur" and RMx.BLUR_KERNELS == blur.PRESETS
    a = cli.parse_args(["--task", "deblur", "--kernel", "gauss"])
    assert cli.chain_options(a) == dict(respacing=None, kernel="gauss", tol=3e-2, ddim=False, eta=0.0)
    a = cli.parse_args(["--task", "deblur", "--kernel", "aniso", "--tol", "0.1", "--use_ddim", "--eta", "0.5", "--timestep_respacing", "20"])
    assert cli.chain_options(a) == dict(respacing="20", kernel="aniso", tol=0.1, ddim=True, eta=0.5)
    # the existing tasks parse to what they did
    assert cli.chain_options(cli.parse_args(["--task", "sr"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    d = ["--task", "deblur", "--kernel", "gauss"]
    for bad in (["--task", "sr", "--kernel", "gauss"], ["--task", "inpaint", "--tol", "0.1"], d + ["--scale", "2"], d + ["--mask", "half"],
                d + ["--sigma_y", "0.1"], d + ["--dpm_solver"], ["--task", "deblur", "--kernel", "motion"], d + ["--tol", "1"],
                d + ["--method", "repaint"], ["--task", "deblur"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    a = dms.parse_args(["--images", "x.npy", "--kernel", "uniform", "--blur_input"])
    assert (a.kernel, a.tol, a.blur_input, a.use_ddim) == ("uniform", 3e-2, True, False)
    for bad in (["--images", "x.npy", "--kernel", "motion"], ["--images", "x.npy", "--eta", "0.5"], ["--images", "x.npy", "--tol", "2"], []):
        with pytest.raises(SystemExit):
            dms.parse_args(bad)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(None, np.zeros((1, 16, 16, 3), np.uint8), "sr", kernel="gauss")
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(None, np.zeros((1, 16, 16, 3), np.uint8), "deblur", kernel="gauss", scale=2)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(_tiny(), np.zeros((1, 16, 16, 3), np.uint8), "deblur")
