"""DDNM for size-changing separable operators on the CPU: blur.resize_matrix against torch's antialiased
bicubic interpolation and against the independent tests/resize_ref.py, the rectangular pseudo-inverse and projection against their
definitions, separable_operands against blur_operands on a square matrix, every argument error of DDPM.restore_separable /
super_resolve(downsample=...) / DownsampleDDPM before any device work, the header, the ctypes signatures and the built library on
the two new entries, and the command lines' arguments and output names."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import resize_ref as ZR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import blur
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddk_separable_apply_rect", "ddk_sampler_run_restore_sep")


def _tiny(size=16):
    cfg = ddpm_cfg(32, 3, size)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


def _torch_matrix(H, n):
    """torch's antialiased bicubic reduction applied to the identity: column j of the result is the image of unit vector j"""
    eye = torch.eye(H, dtype=torch.float64).reshape(1, 1, H, H)
    return torch.nn.functional.interpolate(eye, size=(H // n, H), mode="bicubic", antialias=True, align_corners=False)[0, 0].numpy()


# ---------------------------------------------------------------- the operator
@pytest.mark.parametrize("H,n", ZR.SIZES)
def test_resize_matrix_is_torchs_antialiased_bicubic(H, n):
    A = blur.resize_matrix(H, n)
    assert A.shape == (H // n, H) and A.dtype == np.float64
    e_torch = float(np.abs(A - _torch_matrix(H, n)).max())
    e_ref = float(np.abs(A - ZR.matrix(H, n)).max())
    e_sum = float(np.abs(A.sum(axis=1) - 1).max())
    print(f"resize_matrix H={H} n={n}: vs torch {e_torch:.3g}, vs restatement {e_ref:.3g}, |row sum - 1| {e_sum:.3g}")
    assert e_torch <= 1e-12 and e_ref <= 1e-12 and e_sum <= 1e-12


def test_the_two_d_operator_is_the_matrix_pair():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 32, 48, generator=g, dtype=torch.float64)
    A_h, A_w = torch.from_numpy(blur.resize_matrix(32, 4)), torch.from_numpy(blur.resize_matrix(48, 4))
    want = torch.nn.functional.interpolate(x, size=(8, 12), mode="bicubic", antialias=True, align_corners=False)
    err = float((torch.einsum("ih,bchw,jw->bcij", A_h, x, A_w) - want).abs().max())
    print(f"A_h X A_w^T vs interpolate: {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("H,n", [(16, 2), (32, 4), (256, 8)])
def test_mean_kind_is_the_block_mean(H, n):
    A = blur.resize_matrix(H, n, "mean")
    assert np.array_equal(A, ZR.matrix(H, n, "mean"))
    x = torch.randn(1, 1, H, H, dtype=torch.float64, generator=torch.Generator().manual_seed(H))
    At = torch.from_numpy(A)
    assert float((torch.einsum("ih,bchw,jw->bcij", At, x, At) - torch.nn.functional.avg_pool2d(x, n)).abs().max()) <= 1e-14


@pytest.mark.parametrize("bad", [dict(H=16, scale=3), dict(H=16, scale=0), dict(H=16.0, scale=2), dict(H=16, scale=2, kind="lanczos"),
                                 dict(H=True, scale=1), dict(H=4, scale=8)])
def test_bad_resize_arguments_raise(bad):
    with pytest.raises(ValueError):
        blur.resize_matrix(**bad)


@pytest.mark.parametrize("H,n", ZR.SIZES)
def test_full_row_rank_and_projection_properties(H, n):
    A = blur.resize_matrix(H, n)
    h = H // n
    S = np.linalg.svd(A, compute_uv=False)
    Q, P, rank = blur.blur_projection(A, 3e-2)
    assert Q.shape == (H, h) and P.shape == (H, H) and rank == h
    ratio = S[-1] / S[0]
    errs = dict(aq=np.abs(A @ Q - np.eye(h)).max(), sym=np.abs(P - P.T).max(), idem=np.abs(P @ P - P).max(), ap=np.abs(A @ P - A).max())
    print(f"H={H} n={n}: s_min / s_max {ratio:.4f}, max|A+| {np.abs(Q).max():.4f}, {errs}")
    assert 0.685 <= ratio <= 0.752
    assert np.abs(Q).max() <= 1.31
    assert max(errs.values()) <= 1e-10
    Qr, Pr, rr = ZR.projection(ZR.matrix(H, n), 3e-2)
    assert rr == rank and np.abs(Q - Qr).max() <= 1e-12 and np.abs(P - Pr).max() <= 1e-12


def test_separable_operands_shapes_rounding_and_cache():
    A_h, A_w = blur.resize_matrix(32, 4), blur.resize_matrix(48, 2)
    out = blur.separable_operands(A_h, A_w)
    assert [tuple(t.shape) for t in out[:6]] == [(8, 32), (24, 48), (32, 8), (48, 24), (32, 32), (48, 48)] and out[6:] == (8, 24)
    ref = ZR.operands(ZR.matrix(32, 4), ZR.matrix(48, 2))
    for got, name in zip(out, ("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w")):
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert float((got.double() - ref[name]).abs().max()) <= 2.0 ** -24 * max(1.0, float(ref[name].abs().max())) + 1e-12
    assert blur.separable_operands(A_h.copy(), torch.from_numpy(A_w))[0] is out[0]
    # a truncating tolerance drops directions: the rank says so
    assert blur.separable_operands(A_h, A_w, 0.72)[6] < 8


@pytest.mark.parametrize("kernel,H,W", [("uniform", 16, 16), ("gauss", 16, 48), ("aniso", 64, 32)])
def test_square_matrices_give_exactly_blur_operands(kernel, H, W):
    k_h, k_w = blur.blur_kernel(kernel)
    got = blur.separable_operands(blur.blur_matrix(H, k_h), blur.blur_matrix(W, k_w))
    want = blur.blur_operands(kernel, H, W)
    for a, b in zip(got[:6], want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("bad", [(np.zeros((3,)), np.eye(4)), (np.zeros((8, 4)), np.eye(4)), (np.full((2, 4), np.nan), np.eye(4)),
                                 (np.zeros((0, 4)), np.eye(4))])
def test_bad_operand_matrices_raise(bad):
    with pytest.raises(ValueError):
        blur.separable_operands(*bad)
    with pytest.raises(ValueError):
        blur.separable_operands(np.eye(4), np.eye(4), tol=1.0)


# ---------------------------------------------------------------- argument checks (ValueError before any device work)
A8 = blur.resize_matrix(16, 2)


@pytest.mark.parametrize("y", [torch.zeros(2, 3, 16, 16), torch.zeros(2, 1, 8, 8), torch.zeros(3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.long),
                               torch.full((2, 3, 8, 8), float("nan")), torch.full((2, 3, 8, 8), float("inf")), [[0.0]]])
def test_bad_y_raises(y):
    with pytest.raises(ValueError):
        _tiny().restore_separable(y, A8, A8)


@pytest.mark.parametrize("A_h,A_w", [(A8[:, :8], A8), (A8, A8.T), (np.zeros(16), A8), (np.full((8, 16), np.inf), A8), (A8[:6], A8), (A8[:2], A8),
                                     (np.zeros((20, 16)), A8), (A8, "x"), (A8, None)])
def test_bad_matrices_raise(A_h, A_w):
    h = A_h.shape[0] if hasattr(A_h, "shape") and A_h.ndim == 2 else 8
    with pytest.raises(ValueError):
        _tiny().restore_separable(torch.zeros(2, 3, h, 8), A_h, A_w)


@pytest.mark.parametrize("kw", [dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(solver="dpm++2m"), dict(noise=torch.zeros(1)), dict(early_stop=10),
                                dict(paste=True), dict(mask=torch.ones(8, 8)), dict(sigma_y=0.1), dict(tol=1.0), dict(tol=-0.1), dict(tol="x")])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError):
        _tiny().restore_separable(torch.zeros(2, 3, 8, 8), A8, A8, **kw)


def test_an_image_size_the_kernels_do_not_take_raises():
    cfg = ddpm_cfg(32, 3, 24)
    A = blur.resize_matrix(24, 2)
    with pytest.raises(ValueError, match="multiples of 16"):
        DDPM(cfg, Unet(cfg), "cpu", 3).restore_separable(torch.zeros(1, 3, 12, 12), A, A)


def test_super_resolve_downsample_argument():
    m = _tiny()
    with pytest.raises(ValueError, match="downsample"):
        m.super_resolve(torch.zeros(2, 3, 8, 8), 2, downsample="lanczos")
    with pytest.raises(ValueError, match="multiple of 4"):      # 16 / 8 = 2: off the kernels' grid
        m.super_resolve(torch.zeros(2, 3, 2, 2), 8, downsample="bicubic")
    with pytest.raises(ValueError):
        m.super_resolve(torch.zeros(2, 3, 4, 4), 2, downsample="bicubic")      # y of another scale
    with pytest.raises(ValueError):
        m.super_resolve(torch.zeros(2, 3, 8, 8), 2, downsample="bicubic", eta=0.5)
    cfg = ddpm_cfg(32, 3, 24)
    with pytest.raises(ValueError, match="multiples of 16"):
        DDPM(cfg, Unet(cfg), "cpu", 3).super_resolve(torch.zeros(1, 3, 12, 12), 2, downsample="bicubic")
    # good arguments reach the device check, by both doors; the default is today's path
    for call in (lambda: m.super_resolve(torch.zeros(2, 3, 8, 8), 2, downsample="bicubic", respacing="20"),
                 lambda: m.super_resolve(torch.zeros(2, 3, 4, 4), 4, downsample="bicubic", ddim=True, eta=0.3),
                 lambda: m.restore_separable(torch.zeros(2, 3, 8, 4), A8, blur.resize_matrix(16, 4), respacing="20"),
                 lambda: m.super_resolve(torch.zeros(2, 3, 8, 8), 2, downsample="mean"),
                 lambda: m.super_resolve(torch.zeros(2, 3, 8, 8), 2)):
        with pytest.raises(L.DDKError, match="ROCm"):
            call()


def test_the_downsampled_model_refuses():
    cfg = dddpm_cfg(32, 32, 2)
    m = DownsampleDDPM(cfg, Unet(cfg), "cpu", 3)
    A = blur.resize_matrix(32, 4)
    with pytest.raises(ValueError, match="latent"):
        m.restore_separable(torch.zeros(1, 3, 8, 8), A, A)
    with pytest.raises(ValueError, match="downsample"):
        m.super_resolve(torch.zeros(1, 3, 8, 8), 4, downsample="bicubic")


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    from ddk import ops, plan
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
        params = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr).group(1).split(",")
        sig = L.SIGNATURES[name][1]
        assert len(params) == len(sig), name
        # ints where the header has ints, pointers where it has pointers
        for p, s in zip(params, sig):
            assert (("*" in p or "ddk_stream_t" in p) and s is not ctypes.c_int) or (p.strip().startswith("int ") and s is ctypes.c_int), (name, p)
    assert len(L.SIGNATURES["ddk_separable_apply_rect"][1]) == 12
    assert len(L.SIGNATURES["ddk_sampler_run_restore_sep"][1]) == 10
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert callable(ops.separable_apply_rect) and callable(plan.UnetPlan.sample_restore_sep_nhwc)
    # the new entry has the deblurring chain's workspace and tail queries: no new contract
    assert plan.UnetPlan.RESTORE_ENTRIES["srq"] == ("sampler_run_restore_sep",) + plan.UnetPlan.RESTORE_ENTRIES["srb"][1:]
    assert "srq" in plan.SAMPLERS and "srq" in plan.CHAIN_WORKSPACES


def test_rect_entry_refuses_bad_arguments_on_the_host():
    """the checks come before any launch, so they answer without a device: null pointers, sizes off the grid, channels, alignment,
    overlap (addresses are only compared, never read)"""
    lib = L.load()
    p = lambda a: ctypes.c_void_p(a)
    base = 1 << 20
    ok = dict(inp=base, Lm=base + (1 << 16), Rm=base + (2 << 16), out=base + (3 << 16), scr=base + (4 << 16), B=2, Hi=8, Wi=8, Ho=32, Wo=32, C=3)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ddk_separable_apply_rect(p(a["inp"]), p(a["Lm"]), p(a["Rm"]), p(a["out"]), p(a["scr"]), a["B"], a["Hi"], a["Wi"], a["Ho"],
                                            a["Wo"], a["C"], None)
    for kw in (dict(inp=0), dict(scr=0), dict(Hi=6), dict(Wi=0), dict(Ho=260), dict(Wo=18), dict(C=9), dict(C=0), dict(B=0), dict(B=65536),
               dict(inp=base + 4), dict(Lm=base + (1 << 16) + 8), dict(out=base + (3 << 16) + 4), dict(scr=base + (4 << 16) + 12),
               dict(out=base), dict(scr=base), dict(out=base + (4 << 16)), dict(out=base + 16)):
        assert call(**kw) == -1, kw
        assert "separable_apply_rect" in L.last_error()


# ---------------------------------------------------------------- the command lines
def test_the_evaluator_and_the_cli_take_the_downsample_option():
    import evaluate_restoration as cli
    import upscale_model_samples as ums
    from utils import restoration_metrics as RMx
    assert RMx.DOWNSAMPLES == ("mean", "bicubic")
    # the defaults parse to what they did, and name what they did
    assert cli.chain_options(cli.parse_args(["--task", "sr"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "sr", "--downsample", "mean"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    a = cli.parse_args(["--task", "sr", "--downsample", "bicubic", "--scale", "2", "--use_ddim", "--eta", "0.5", "--timestep_respacing", "20"])
    assert cli.chain_options(a) == dict(respacing="20", scale=2, downsample="bicubic", ddim=True, eta=0.5)
    s = ["--task", "sr", "--downsample", "bicubic"]
    for bad in (["--task", "inpaint", "--downsample", "bicubic"], ["--task", "deblur", "--kernel", "gauss", "--downsample", "mean"],
                ["--task", "colorize", "--downsample", "bicubic"], s + ["--mask", "half"], s + ["--dpm_solver"], s + ["--sigma_y", "0.1"],
                ["--task", "sr", "--downsample", "lanczos"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    a = ums.parse_args(["--images", "x.npy"])
    assert (a.downsample, a.scale) == ("mean", 4) and ums.output_base("celeba_x2", 4, a.downsample, "full") == "celeba_x2_sr4_full"
    a = ums.parse_args(["--images", "x.npy", "--downsample", "bicubic", "--scale", "2", "--use_ddim"])
    assert a.downsample == "bicubic" and ums.output_base("m", 2, a.downsample, "20_ddim_eta0") == "m_sr2_bicubic_20_ddim_eta0"
    for bad in (["--images", "x.npy", "--downsample", "bicubic", "--dpm_solver"], ["--images", "x.npy", "--downsample", "bicubic", "--sigma_y", "0.1"],
                ["--images", "x.npy", "--downsample", "area"], ["--downsample", "bicubic"]):
        with pytest.raises(SystemExit):
            ums.parse_args(bad)
    z = np.zeros((1, 16, 16, 3), np.uint8)
    for kw in (dict(task="sr", downsample="lanczos"), dict(task="inpaint", downsample="bicubic"), dict(task="colorize", downsample="bicubic"),
               dict(task="deblur", kernel="gauss", downsample="bicubic"), dict(task="sr", downsample="bicubic", sr_mask="half"),
               dict(task="sr", downsample="bicubic", sigma_y=0.1), dict(task="sr", downsample="bicubic", dpm_solver=True)):
        with pytest.raises(ValueError, match="downsample"):
            RMx.evaluate_restoration(None, z, **kw)
    A_h, A_w = RMx.resize_matrices(16, 32, 4)
    assert torch.equal(A_h, torch.tensor(blur.resize_matrix(16, 4), dtype=torch.float32)) and tuple(A_w.shape) == (8, 32)
