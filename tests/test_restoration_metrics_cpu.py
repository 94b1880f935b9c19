"""Host side of the PSNR / SSIM evaluator: the float64 restatement tests/ssim_ref.py pinned with closed forms,
the fp32 figure the GPU bar is derived from, the degradations and baselines of utils/restoration_metrics.py, and the argument checks
of ops.image_metrics and of evaluate_restoration.py's parser.  Nothing here touches a device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import evaluate_restoration as cli
import inpaint_model_samples
import ssim_ref as R
import upscale_model_samples
from ddk import lib as L
from ddk import ops
from utils import restoration_metrics as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------ the restatement, against closed forms
def test_identical_images_ssim_one_psnr_inf():
    a, _ = R.pair((1, 16, 16, 4), "noise")
    assert np.array_equal(R.ssim(a, a), np.ones(1))
    assert R.psnr(a, a)[0] == math.inf
    s, k = R.sq_err(a, a)
    assert s[0] == 0 and k[0] == 16 * 16 * 4


@pytest.mark.parametrize("p,q", [(255, 254), (0, 255), (17, 200), (128, 128)])
def test_constant_images_closed_form(p, q):
    a, b = np.full((1, 13, 12, 2), p, np.uint8), np.full((1, 13, 12, 2), q, np.uint8)
    want = (2 * p * q + R.C1) / (p * p + q * q + R.C1)        # sigma = 0: the contrast-structure factor is C2 / C2
    assert abs(R.ssim(a, b)[0] - want) < 1e-12                # float64: E[x^2] - mu^2 of a constant is 0 up to ~1e-11 of 65025
    assert R.psnr(a, b)[0] == (math.inf if p == q else 10 * math.log10(255.0 ** 2 / (p - q) ** 2))


def test_symmetry():
    a, b = R.pair((1, 12, 13, 3), "noise")
    assert np.array_equal(R.ssim(a, b), R.ssim(b, a))
    assert np.array_equal(R.psnr(a, b), R.psnr(b, a))


def test_single_window_equals_hand_computed_moments():
    a, b = R.pair((1, 11, 11, 1), "noise")
    assert R.ssim_map(a, b).shape == (1, 1, 1, 1)
    g = [math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]
    tot = sum(g)
    g = [v / tot for v in g]
    ea = eb = eaa = ebb = eab = 0.0
    for i in range(11):
        for j in range(11):
            w, x, y = g[i] * g[j], float(a[0, i, j, 0]), float(b[0, i, j, 0])
            ea, eb, eaa, ebb, eab = ea + w * x, eb + w * y, eaa + w * x * x, ebb + w * y * y, eab + w * x * y
    va, vb, cab = eaa - ea * ea, ebb - eb * eb, eab - ea * eb
    want = (2 * ea * eb + R.C1) * (2 * cab + R.C2) / ((ea * ea + eb * eb + R.C1) * (va + vb + R.C2))
    assert abs(R.ssim(a, b)[0] - want) < 1e-12
    assert abs(R.window_2d().sum() - 1) < 1e-15 and R.window_2d().shape == (11, 11)


def test_masked_squared_error_counts():
    shape = (3, 45, 70, 3)
    a, b = R.pair(shape, "noise")
    s, k = R.sq_err(a, b)
    assert k.tolist() == [45 * 70 * 3] * 3
    d = a.astype(np.int64) - b.astype(np.int64)
    assert s.tolist() == [int((d[i] ** 2).sum()) for i in range(3)]
    s0, k0 = R.sq_err(a, b, R.mask_for(shape, "none"))
    assert s0.tolist() == [0, 0, 0] and k0.tolist() == [0, 0, 0] and np.isnan(R.psnr(a, b, R.mask_for(shape, "none"))).all()
    s1, k1 = R.sq_err(a, b, R.mask_for(shape, "one"))
    assert k1.tolist() == [0, 0, 3] and s1[2] == int((d[2, 43, 67] ** 2).sum())


def test_recorded_fp32_deviation_is_what_the_emulation_gives():
    """the constants the GPU bar rests on are measurements of ssim_fp32 on exactly the GPU test's inputs; re-measured here"""
    dev = {128.0: 0.0, 0.0: 0.0}
    for shape in R.SHAPES:
        for kind in R.PAIRS:
            a, b = R.pair(shape, kind)
            for shift in dev:
                got = R.ssim_fp32(a, b, shift).double().numpy()
                dev[shift] = max(dev[shift], float(np.abs(got - R.reference(shape, kind)).max()))
    print(f"fp32 separable SSIM vs float64: shifted {dev[128.0]:.3e}, unshifted {dev[0.0]:.3e}")
    assert 0.5 * R.SSIM_FP32_DEV < dev[128.0] <= R.SSIM_FP32_DEV
    assert 0.5 * R.SSIM_FP32_DEV_UNSHIFTED < dev[0.0] <= R.SSIM_FP32_DEV_UNSHIFTED
    assert dev[0.0] > 100 * dev[128.0]                        # the reason for the shift
    assert R.SSIM_BAR == 4 * R.SSIM_FP32_DEV


# ------------------------------------------------------------------ degradations and baselines
def test_mask_kinds_are_the_inpainting_cli_s():
    assert inpaint_model_samples.make_mask is RM.make_mask and inpaint_model_samples.load_mask is RM.load_mask
    assert inpaint_model_samples.MASKS is RM.MASKS
    assert RM.MASKS == ("center", "left", "half", "lines")
    m = {k: RM.make_mask(k, 2, 16, 12) for k in RM.MASKS}
    for v in m.values():
        assert v.shape == (2, 1, 16, 12) and set(v.unique().tolist()) == {0.0, 1.0}
    assert (m["center"][:, :, 4:12, 3:9] == 0).all() and m["center"].sum() == 2 * (16 * 12 - 8 * 6)
    assert (m["left"][..., :6] == 0).all() and (m["left"][..., 6:] == 1).all()
    assert (m["half"][:, :, 8:] == 0).all() and (m["half"][:, :, :8] == 1).all()
    assert (m["lines"][:, :, 1::2] == 0).all() and (m["lines"][:, :, 0::2] == 1).all()
    with pytest.raises(ValueError):
        RM.make_mask("ring", 1, 16, 16)


def test_pool_and_super_resolution_baselines():
    assert upscale_model_samples.pool is RM.pool
    imgs, _ = R.pair((2, 64, 64, 3), "noise")
    x = RM.from_u8(imgs)
    assert x.shape == (2, 3, 64, 64) and x.min() >= -1 and x.max() <= 1
    for s in (2, 4, 8):
        y = RM.pool(x, s)
        assert y.shape == (2, 3, 64 // s, 64 // s)
        assert torch.allclose(y, x.reshape(2, 3, 64 // s, s, 64 // s, s).mean(dim=(3, 5)), atol=1e-6)
        rep, bic = RM.replicate(y, s), RM.bicubic(y, s)
        assert rep.shape == bic.shape == x.shape
        assert torch.equal(RM.pool(rep, s), y) or torch.allclose(RM.pool(rep, s), y, atol=1e-6)       # A A+ = I
        assert torch.equal(rep[:, :, ::s, ::s], y) and torch.equal(rep[:, :, s - 1::s, s - 1::s], y)
        assert RM.to_u8(bic).dtype == torch.uint8 and RM.to_u8(bic).shape == (2, 64, 64, 3)             # overshoot is clamped


def test_u8_round_trip_is_exact():
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1)
    assert torch.equal(RM.to_u8(RM.from_u8(u)), u)
    assert RM.to_u8(torch.tensor([-3.0, 3.0]).reshape(1, 1, 1, 2)).flatten().tolist() == [0, 255]
    with pytest.raises(ValueError):
        RM.from_u8(np.zeros((1, 4, 4, 1), np.float32))


def test_mean_fill_baseline():
    x = RM.from_u8(R.pair((2, 64, 64, 3), "noise")[0])[:, :, :16, :16]
    m = RM.make_mask("center", 2, 16, 16)
    out = RM.mean_fill(x, m)
    assert torch.equal(out * m, x * m)
    known = x[0, 1][m[0, 0] != 0]
    assert torch.allclose(out[0, 1, 8, 8], known.mean(), atol=1e-6) and (out[0, 1][m[0, 0] == 0] == out[0, 1, 8, 8]).all()
    assert torch.equal(RM.mean_fill(x, torch.ones(2, 1, 16, 16)), x)


def test_summarise_and_report():
    s = RM.summarise([1.0, 2.0, 3.0, float("nan")])
    assert s["n"] == 3 and s["mean"] == 2.0 and abs(s["stderr"] - 1.0 / math.sqrt(3)) < 1e-12
    s = RM.summarise([math.inf, math.inf])
    assert s["mean"] == math.inf and s["n"] == 2
    assert RM.summarise([float("nan")])["n"] == 0 and math.isnan(RM.summarise([5.0])["stderr"])
    rep = RM.report(dict(methods=dict(restored=dict(psnr=np.array([30.0, 32.0]), ssim=np.array([0.9, 0.8]))),
                         consistency=np.array([0.25, 0.5])))
    assert rep["restored"]["psnr"]["mean"] == 31.0 and rep["consistency"]["max"] == 0.5


def test_evaluate_restoration_rejects_bad_requests_before_the_model_runs():
    imgs = np.zeros((2, 16, 16, 3), np.uint8)
    with pytest.raises(ValueError):
        RM.evaluate_restoration(None, imgs, "deblur")
    with pytest.raises(ValueError):
        RM.evaluate_restoration(None, imgs.astype(np.float32), "sr")


# ------------------------------------------------------------------ argument validation
@pytest.mark.parametrize("make", [
    lambda: (torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3, dtype=torch.uint8), None),                       # a not uint8
    lambda: (torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.int8), None),     # b not uint8
    lambda: (torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 17, 3, dtype=torch.uint8), None),    # shapes differ
    lambda: (torch.zeros(16, 16, 3, dtype=torch.uint8), torch.zeros(16, 16, 3, dtype=torch.uint8), None),          # not 4-d
    lambda: (torch.zeros(1, 10, 16, 3, dtype=torch.uint8), torch.zeros(1, 10, 16, 3, dtype=torch.uint8), None),    # H < 11
    lambda: (torch.zeros(1, 16, 10, 3, dtype=torch.uint8), torch.zeros(1, 16, 10, 3, dtype=torch.uint8), None),    # W < 11
    lambda: (torch.zeros(1, 16, 16, 5, dtype=torch.uint8), torch.zeros(1, 16, 16, 5, dtype=torch.uint8), None),    # C > 4
    lambda: (torch.zeros(0, 16, 16, 3, dtype=torch.uint8), torch.zeros(0, 16, 16, 3, dtype=torch.uint8), None),    # N = 0
    lambda: (torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16)),
    lambda: (torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8),
             torch.zeros(1, 16, 16, 3, dtype=torch.uint8)),                                                         # mask not [N,H,W]
])
def test_image_metrics_argument_errors_are_value_errors(make):
    a, b, mask = make()
    with pytest.raises(ValueError):
        ops.image_metrics(a, b, mask)


def test_image_metrics_refuses_host_tensors():
    z = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(L.DDKError):
        ops.image_metrics(z, z)


def test_cli_parser():
    a = cli.parse_args(["--task", "sr", "--scale", "2", "--use_ddim", "--eta", "0.5", "--timestep_respacing", "ddim10"])
    assert cli.chain_options(a) == dict(respacing="ddim10", scale=2, ddim=True, eta=0.5)
    a = cli.parse_args(["--task", "inpaint", "--mask", "lines", "--jump_length", "3", "--jump_n_sample", "2", "--max_batches", "1"])
    assert cli.chain_options(a) == dict(respacing=None, jump_length=3, jump_n_sample=2) and a.mask == "lines" and a.seed == 1234
    for bad in (["--task", "deblur"], [], ["--task", "sr", "--eta", "0.5"], ["--task", "sr", "--scale", "1"],
                ["--task", "inpaint", "--use_ddim"], ["--task", "inpaint", "--jump_length", "0"], ["--task", "sr", "--batch_size", "0"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


def test_cli_default_images_are_the_test_split():
    args = cli.parse_args(["--task", "sr", "--batch_size", "2", "--max_batches", "2"])
    imgs = cli.load_images(args, dict(dataset="celeba", image_size=16, batch_size=2), 3)
    assert imgs.dtype == np.uint8 and imgs.shape == (4, 16, 16, 3) and imgs.std() > 50
    assert np.array_equal(imgs, cli.load_images(args, dict(dataset="celeba", image_size=16, batch_size=2), 3))


def test_cli_help_lists_every_flag():
    script = os.path.join(ROOT, "downsampled-diffusion_amd", "evaluate_restoration.py")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "downsampled-diffusion_amd"))
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--saved_model", "--synthetic", "--batch_size", "--max_batches", "--seed", "--json", "--images", "--task", "--mask",
                 "--scale", "--timestep_respacing", "--use_ddim", "--eta", "--jump_length", "--jump_n_sample"):
        assert flag in r.stdout
