"""Diffusion Posterior Sampling on the CPU: the reference tests/guidance_ref.py against central differences,
the operator objects of models/diffusion/guidance.py, every argument error of DDPM.restore_guided / DownsampleDDPM.restore_guided before
any device work, the zeta table, the frozen() context, and the header, the ctypes signatures and the built library on the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref as GR
from helpers import dddpm_cfg, ddpm_cfg
from models import DDPM, DownsampleDDPM, Unet
from models.diffusion import blur, guidance as G, psf
from ddk import autograd as AG
from ddk import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddk_measure_residual_workspace_bytes", "ddk_measure_residual", "ddk_measure_adjoint", "ddk_x0_from_eps", "ddk_x0_from_eps_bwd",
       "ddk_p_sample_update_guided")


def _tiny():
    cfg = ddpm_cfg(32, 3, 16)
    return DDPM(cfg, Unet(cfg), "cpu", 3)


def _tiny_latent():
    cfg = dddpm_cfg(32, 32, 1)
    cfg.update(d_n_blocks=1, u_n_blocks=1)
    return DownsampleDDPM(cfg, Unet(cfg), "cpu", 3)


def _operators(shape, response, gain, masked):
    """one operator of every kind on an image of `shape` = (C, H, W), as restore_guided would build them"""
    C, H, W = shape
    rng = np.random.default_rng(5)
    out = []
    for spec in (("mean", 1), ("mean", 2), ("mean", 4), ("separable", blur.blur_matrix(H, blur.blur_kernel("gauss")[0])[::2], rng.standard_normal((W // 4 * 3, W)) / 4),
                 ("psf", "disk"), "uniform", "diag"):
        op = G.make_operator(spec, shape, response=response, gain=gain)
        if masked:
            op.mask = (torch.from_numpy(rng.random((2, *op.out_shape[1:]))) > 0.4).float()
        out.append(op)
    return out


# ---------------------------------------------------------------- the reference's own gradient
H_FD = 1e-4


@pytest.mark.parametrize("response,gain", [("linear", 1.0), ("saturate", 1.0), ("saturate", 2.5)])
@pytest.mark.parametrize("masked", [False, True])
def test_reference_gradient_equals_central_differences(response, gain, masked):
    """d(sum_b w_b dist_b) / d img of the float64 reference (torch autograd) against (f(x + h v) - f(x - h v)) / 2h along random
    directions v of unit maximum norm.  The tolerance is the difference's own error, not a number for the code under test: with
    h = 1e-4 the truncation term is h^2 / 6 |f'''| and the rounding term 2^-52 |f| / h; f is a sum of B = 2 Euclidean norms of vectors of a
    few hundred O(1) entries, so |f| <= 100 and |f'''| = O(|v|^3 / dist^2) <= 10 on these inputs: 10 h^2 + 100 * 2^-52 / h = 1.0e-7 + 2.2e-10.
    The inputs keep every gain u at least 1e-3 (ten difference steps) from the saturation bounds, where f has a kink."""
    shape = (2, 16, 16)
    rng = np.random.default_rng(17)
    tol = 10 * H_FD ** 2 + 100 * 2.0 ** -52 / H_FD
    saturated = 0
    for op in _operators(shape, response, gain, masked):
        y = torch.from_numpy(rng.uniform(-1, 1, (2, *op.out_shape)))
        for _ in range(64):          # (an image with an element on the kink is drawn again: about one in three at gain 2.5)
            img = torch.from_numpy(rng.uniform(-1, 1, (2, *shape)))
            gu = gain * GR.linear(op, img)
            if response == "linear" or int(((gu.abs() - 1).abs() < 1e-3).sum()) == 0:
                break
        else:
            raise AssertionError("no image off the kink in 64 draws")
        saturated += int((gu.abs() > 1).sum()) if response == "saturate" else 0
        w = torch.tensor([1.0, -0.5], dtype=torch.float64)
        dist, v = GR.dist_and_grad(op, img, y, w)
        assert dist.dtype == torch.float64 and v.shape == img.shape and float(dist.min()) > 1.0
        f = lambda x: float((GR.measure_dist(op, x, y) * w).sum())
        for _ in range(4):
            d = torch.from_numpy(rng.uniform(-1, 1, tuple(img.shape)))
            fd = (f(img + H_FD * d) - f(img - H_FD * d)) / (2 * H_FD)
            assert abs(fd - float((v * d).sum())) <= tol, (op.kind, op.n, fd, float((v * d).sum()))
    assert saturated > 0 or gain == 1.0 or response == "linear"          # the flat branch of the response was exercised


def test_reference_operators_are_their_definitions():
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((2, 2, 16, 16)))
    op = G.make_operator(("mean", 4), (2, 16, 16))
    assert (GR.linear(op, x) - x.reshape(2, 2, 4, 4, 4, 4).mean(dim=(3, 5))).abs().max() <= 1e-15
    a_h, a_w = rng.standard_normal((8, 16)), rng.standard_normal((12, 16))
    op = G.make_operator(("separable", a_h, a_w), (2, 16, 16))
    want = torch.from_numpy(a_h) @ x @ torch.from_numpy(a_w).T
    assert (GR.linear(op, x) - want).abs().max() <= 1e-13
    # the PSF operator is blur.blur_matrix's correlation wherever the plane cannot wrap around
    kh, kw = np.array([1.0, 2.0, 4.0]), np.array([3.0, 1.0, -1.0])
    op = G.make_operator(("psf", np.outer(kh, kw)), (2, 16, 16))
    sep = torch.from_numpy(blur.blur_matrix(16, kh)) @ x @ torch.from_numpy(blur.blur_matrix(16, kw)).T
    assert (GR.linear(op, x) - sep)[..., 1:-1, 1:-1].abs().max() <= 1e-13
    # the names deblur and deconvolve take
    op = G.make_operator("gauss", (2, 16, 16))
    assert op.kind == "separable" and np.array_equal(op.A_h, blur.blur_matrix(16, blur.blur_kernel("gauss")[0]))
    op = G.make_operator("disk", (2, 16, 16))
    assert op.kind == "psf" and np.array_equal(op.K, psf.psf_spectrum("disk", 16, 16))
    # the saturating response and the mask
    op = G.make_operator(("mean", 1), (2, 16, 16), response="saturate", gain=2.0)
    op.mask = torch.zeros(2, 16, 16)
    op.mask[:, ::2] = 1
    y = GR.measure(op, x)
    assert torch.equal(y[:, :, ::2], torch.clamp(2.0 * x, -1, 1)[:, :, ::2]) and float(y[:, :, 1::2].abs().max()) == 0
    assert torch.equal(GR.measure_dist(op, x, y), torch.zeros(2, dtype=torch.float64))


# ---------------------------------------------------------------- argument errors, all before any device work
GOOD_Y = torch.zeros(2, 3, 4, 4)


@pytest.mark.parametrize("kw", [
    dict(solver="dpm++2m"), dict(early_stop=3), dict(paste=True), dict(sigma_y=0.1),
    dict(eta=0.5), dict(ddim=True, eta=-1.0), dict(eta="x"),
    dict(zeta=-1.0), dict(zeta=float("nan")), dict(zeta=float("inf")), dict(zeta=True), dict(zeta="1"), dict(zeta=None),
    dict(zeta=[1.0, 2.0]), dict(zeta=[[1.0] * 1000]), dict(zeta=[1.0] * 10, respacing="20"), dict(zeta=[-1.0] * 20, respacing="20"),
    dict(response="gamma"), dict(response="saturate", gain=0.0), dict(response="saturate", gain=-2.0), dict(gain=float("nan")),
    dict(gain=float("inf")), dict(gain=True), dict(gain="2"),
    dict(mask=torch.zeros(4, 4)), dict(mask=torch.full((4, 4), 0.5)), dict(mask=torch.ones(3, 3)), dict(mask=torch.ones(2, 3, 4, 4)),
    dict(mask="half"), dict(respacing="0"),
])
def test_bad_keyword_raises_before_any_device_work(kw):
    args = dict(zeta=1.0)
    args.update(kw)
    with pytest.raises(ValueError):
        _tiny().restore_guided(GOOD_Y, ("mean", 4), **args)


@pytest.mark.parametrize("operator", [
    ("mean", 3), ("mean", 16), ("mean", 2.0), ("mean", True), ("mean",), ("mean", 2, 2), ("median", 2), "box", None, 7, (),
    ("separable", np.ones((4, 16))), ("separable", np.ones((4, 15)), np.ones((4, 16))), ("separable", np.ones((6, 16)), np.ones((4, 16))),
    ("separable", np.full((4, 16), np.nan), np.ones((4, 16))), ("separable", "a", np.ones((4, 16))), ("separable", np.ones((260, 16)), np.ones((4, 16))),
    ("psf", "motion"), ("psf", np.ones((4, 3))), ("psf", np.ones((17, 3))), ("psf", None),
])
def test_bad_operator_raises_before_any_device_work(operator):
    with pytest.raises(ValueError):
        _tiny().restore_guided(torch.zeros(2, 3, 16, 16), operator, zeta=1.0)


@pytest.mark.parametrize("y", [torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 4, 4), torch.zeros(3, 4, 4), torch.zeros(0, 3, 4, 4),
                               torch.zeros(2, 3, 4, 4, dtype=torch.int32), torch.full((2, 3, 4, 4), float("nan")), np.zeros((2, 3, 4, 4)), None])
def test_bad_measurement_raises_before_any_device_work(y):
    with pytest.raises(ValueError):
        _tiny().restore_guided(y, ("mean", 4), zeta=1.0)


def test_a_psf_needs_a_plane_the_transform_takes():
    cfg = ddpm_cfg(32, 3, 24)
    with pytest.raises(ValueError, match="powers of two"):
        DDPM(cfg, Unet(cfg), "cpu", 3).restore_guided(torch.zeros(1, 3, 24, 24), "disk", zeta=1.0)


def test_good_arguments_reach_the_device_check():
    m = _tiny()
    for y, op, kw in ((GOOD_Y, ("mean", 4), dict(zeta=0.5)),
                      (torch.zeros(2, 3, 16, 16), ("mean", 1), dict(zeta=[0.5] * 20, respacing="20", ddim=True, eta=0.3, mask=torch.eye(16))),
                      (torch.zeros(2, 3, 16, 16), "gauss", dict(zeta=1, response="saturate", gain=2.5)),
                      (torch.zeros(2, 3, 8, 12), ("separable", np.ones((8, 16)), np.ones((12, 16))), dict(zeta=np.float32(0.25))),
                      (torch.zeros(1, 3, 16, 16), ("psf", np.ones((3, 5)) / 15), dict(zeta=torch.full((1000,), 0.1))),
                      (torch.zeros(1, 3, 16, 16), "disk", dict(zeta=0.0, seed=3, x_T=torch.zeros(1, 3, 16, 16)))):
        with pytest.raises(L.DDKError, match="ROCm"):
            m.restore_guided(y, op, **kw)


def test_the_latent_model_takes_pixel_space_operators():
    """the operator, y and the mask of a DownsampleDDPM are the image's (32 x 32 here), not the 16 x 16 latent's"""
    m = _tiny_latent()
    assert m.x_shape == [3, 32, 32] and m.sample_shape == [8, 16, 16]
    for y, op, kw in ((torch.zeros(2, 3, 16, 16), ("mean", 2), dict(zeta=0.5)), (torch.zeros(2, 3, 32, 32), "disk", dict(zeta=0.5)),
                      (torch.zeros(2, 3, 32, 32), "gauss", dict(zeta=0.5, response="saturate", gain=2.0)),
                      (torch.zeros(2, 3, 32, 32), ("mean", 1), dict(zeta=0.5, mask=torch.eye(32)))):
        with pytest.raises(L.DDKError, match="ROCm"):
            m.restore_guided(y, op, **kw)
    for y, op, kw in ((torch.zeros(2, 8, 8, 8), ("mean", 2), dict(zeta=0.5)),            # the latent's shape is no measurement of the image
                      (torch.zeros(2, 3, 16, 16), ("mean", 2), dict(zeta=0.5, solver="dpm++2m")),
                      (torch.zeros(2, 3, 16, 16), ("mean", 2), dict(zeta=-0.5))):
        with pytest.raises(ValueError):
            m.restore_guided(y, op, **kw)


# ---------------------------------------------------------------- the zeta table
def test_zeta_table_from_a_float_and_from_a_sequence():
    z = G.zeta_table(0.3, 5)
    assert z.dtype == np.float64 and np.array_equal(z, np.full(5, 0.3))
    assert np.array_equal(G.zeta_table(2, 3), np.full(3, 2.0)) and np.array_equal(G.zeta_table(np.float32(0.5), 2), np.full(2, 0.5))
    seq = [0.0, 0.1, 0.2, 0.4]
    for given in (seq, tuple(seq), np.array(seq), torch.tensor(seq, dtype=torch.float64)):
        assert np.array_equal(G.zeta_table(given, 4), np.array(seq))
    for bad, rows in ((seq, 5), (seq, 3), (-0.1, 4), ([0.1, -0.1], 2), (float("nan"), 3), ([[0.1, 0.2]], 2), (True, 3), ("0.1", 3), (None, 3)):
        with pytest.raises(ValueError):
            G.zeta_table(bad, rows)


def test_the_model_caches_one_table_per_zeta():
    m = _tiny()
    z = G.zeta_table(0.3, 20)
    get = m._guided_tables("20", True, 0.5, z)
    tables, use = get()
    assert set(tables) == {"c_recip", "c_recipm1", "c1", "c2", "sigma", "zeta"} and len(use) == 20
    assert tables["zeta"].dtype == torch.float32 and torch.equal(tables["zeta"], torch.full((20,), 0.3))
    again, _ = m._guided_tables("20", True, 0.5, G.zeta_table(0.3, 20))()
    assert all(again[k] is tables[k] for k in tables)                      # the same tensors: repeated calls reuse them
    spaced, _ = m._spaced_tables("20", True, 0.5)
    assert all(tables[k] is spaced[k] for k in spaced)                     # and the chain's own rule tables as they are
    other, _ = m._guided_tables("20", True, 0.5, G.zeta_table(np.linspace(0, 1, 20), 20))()
    assert other["zeta"] is not tables["zeta"] and abs(float(other["zeta"][-1]) - 1.0) == 0
    plain, use = m._guided_tables(None, False, 0.0, G.zeta_table(1.0, 1000))()
    assert use is None and plain["c1"] is m.posterior_mean_coef1 and plain["zeta"].shape == (1000,)
    y, op, zt = m._guided_args(GOOD_Y, ("mean", 4), [0.5] * 20, None, "linear", 1.0, "20", False, 0.0, {}, m.sample_shape)
    assert zt.shape == (20,) and op.kind == "mean" and op.n == 4 and op.mask is None and op.out_shape == (3, 4, 4)


# ---------------------------------------------------------------- frozen(): flags and modes come back, _grad_slot stays away
def test_frozen_restores_flags_and_modes_also_after_an_exception():
    m = _tiny_latent()
    m.train()
    m.latent_model.mid_attn.eval()
    params = list(m.parameters())
    params[0].requires_grad_(False)
    params[3].requires_grad_(False)
    flags = [p.requires_grad for p in params]
    modes = [mod.training for mod in m.modules()]
    assert any(flags) and not all(flags) and any(modes) and not all(modes)
    with G.frozen(m) as inner:
        assert inner is m and not any(p.requires_grad for p in params) and not any(mod.training for mod in m.modules())
    assert [p.requires_grad for p in params] == flags and [mod.training for mod in m.modules()] == modes
    with pytest.raises(RuntimeError, match="mid-chain"):
        with G.frozen(m):
            raise RuntimeError("mid-chain")
    assert [p.requires_grad for p in params] == flags and [mod.training for mod in m.modules()] == modes


def test_grad_slot_is_none_for_a_parameter_that_wants_no_gradient():
    p = torch.nn.Parameter(torch.zeros(4))
    assert AG._grad_slot(p) is None                       # no buffer yet
    p.grad = torch.ones(4)
    assert AG._grad_slot(p) is p.grad                     # the training path's slot, as before
    p.requires_grad_(False)
    assert AG._grad_slot(p) is None                       # frozen: a backward must not find the buffer
    p.requires_grad_(True)
    assert AG._grad_slot(p) is p.grad and AG._grad_slot(None) is None and AG._grad_slot(p * 2) is None


# ---------------------------------------------------------------- the command line
def test_the_cli_help_lists_the_new_flags(capsys):
    import guided_model_samples as gms
    with pytest.raises(SystemExit) as e:
        gms.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--task", "{inpaint,sr,deblur,deconv}", "--zeta", "--saturate GAIN", "--sigma_y", "--measure_input", "--mask", "--scale", "--kernel",
                 "--psf", "--timestep_respacing", "--use_ddim", "--eta", "--seed", "--batch_size", "--images"):
        assert flag in text, flag


def test_the_cli_parses_every_task_and_refuses_what_it_cannot_run():
    import guided_model_samples as gms
    base = ["--images", "x.npy", "--zeta", "0.5"]
    a = gms.parse_args(base + ["--task", "inpaint"])
    assert (a.mask, a.zeta, a.saturate, a.sigma_y, a.measure_input) == ("center", 0.5, None, 0.0, False)
    assert gms.operator_spec(a) == (("mean", 1), "center") and gms.guided_kwargs(a) == dict(zeta=0.5, respacing=None, ddim=False, eta=0.0)
    a = gms.parse_args(base + ["--task", "sr", "--saturate", "2.5", "--measure_input", "--sigma_y", "0.05", "--use_ddim", "--eta", "0.5",
                               "--timestep_respacing", "20"])
    assert gms.operator_spec(a) == (("mean", 4), "x4")
    assert gms.guided_kwargs(a) == dict(zeta=0.5, respacing="20", ddim=True, eta=0.5, response="saturate", gain=2.5)
    assert gms.operator_spec(gms.parse_args(base + ["--task", "sr", "--scale", "1"])) == (("mean", 1), "x1")
    assert gms.operator_spec(gms.parse_args(base + ["--task", "deblur", "--kernel", "aniso"])) == ("aniso", "aniso")
    assert gms.operator_spec(gms.parse_args(base + ["--task", "deconv", "--psf", "disk"])) == (("psf", "disk"), "disk")
    for bad in (["--task", "inpaint"], base, base + ["--task", "colorize"], base + ["--task", "sr", "--scale", "3"],
                base + ["--task", "sr", "--mask", "half"], base + ["--task", "inpaint", "--scale", "2"], base + ["--task", "deblur"],
                base + ["--task", "deblur", "--kernel", "box"], base + ["--task", "deconv"], base + ["--task", "deconv", "--psf", "motion"],
                base + ["--task", "deconv", "--psf", "disk", "--kernel", "gauss"], base + ["--task", "inpaint", "--mask", "ring"],
                base + ["--task", "sr", "--eta", "0.5"], base + ["--task", "sr", "--sigma_y", "0.1"],
                base + ["--task", "sr", "--measure_input", "--sigma_y", "-1"], base + ["--task", "sr", "--saturate", "0"],
                base + ["--task", "sr", "--saturate", "nan"], base + ["--task", "sr", "--batch_size", "0"],
                ["--images", "x.npy", "--zeta", "-1", "--task", "sr"], ["--images", "x.npy", "--zeta", "inf", "--task", "sr"]):
        with pytest.raises(SystemExit):
            gms.parse_args(bad)


def test_the_evaluator_knows_the_method(capsys):
    import evaluate_restoration as cli
    from utils import restoration_metrics as RMx
    assert RMx.DPS_METHOD == "dps" and RMx.DPS_TASKS == ("inpaint", "sr", "deblur", "deconv") and RMx.METHODS == ("repaint", "ddnm")
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = capsys.readouterr().out
    assert "--zeta" in text and "--saturate GAIN" in text and "dps" in text
    d = ["--method", "dps", "--zeta", "0.5"]
    assert cli.chain_options(cli.parse_args(d + ["--task", "sr"])) == dict(respacing=None, ddim=False, eta=0.0, zeta=0.5, scale=4)
    a = cli.parse_args(d + ["--task", "inpaint", "--saturate", "2.5", "--sigma_y", "0.05", "--timestep_respacing", "20", "--use_ddim", "--eta", "0.5"])
    assert a.mask == "center" and cli.chain_options(a) == dict(respacing="20", ddim=True, eta=0.5, zeta=0.5, saturate=2.5, sigma_y=0.05)
    assert cli.chain_options(cli.parse_args(d + ["--task", "deblur", "--kernel", "gauss"]))["kernel"] == "gauss"
    assert cli.chain_options(cli.parse_args(d + ["--task", "deconv", "--psf", "disk"]))["psf"] == "disk"
    for bad in (["--method", "dps", "--task", "sr"], d + ["--task", "colorize"], d + ["--task", "cs", "--ratio", "0.5"], d + ["--task", "deconv_noisy", "--psf", "disk"],
                d + ["--task", "sr", "--scale", "3"], d + ["--task", "sr", "--mask", "half"], d + ["--task", "sr", "--dpm_solver"],
                d + ["--task", "sr", "--downsample", "bicubic"], d + ["--task", "deblur"], d + ["--task", "deblur", "--kernel", "gauss", "--tol", "0.1"],
                d + ["--task", "deconv"], d + ["--task", "deconv", "--psf", "motion"], d + ["--task", "inpaint", "--jump_length", "5"],
                d + ["--task", "sr", "--eta", "0.5"], d + ["--task", "sr", "--saturate", "0"], ["--method", "dps", "--zeta", "-1", "--task", "sr"],
                ["--task", "sr", "--zeta", "0.5"], ["--task", "inpaint", "--method", "ddnm", "--saturate", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    # the other methods parse to what they did
    assert cli.chain_options(cli.parse_args(["--task", "sr"])) == dict(respacing=None, scale=4, ddim=False, eta=0.0)
    assert cli.chain_options(cli.parse_args(["--task", "inpaint"])) == dict(respacing=None, jump_length=10, jump_n_sample=10)
    img = np.zeros((1, 16, 16, 3), np.uint8)
    for kw in (dict(task="sr"), dict(task="colorize", zeta=1.0), dict(task="sr", zeta=1.0, dpm_solver=True), dict(task="sr", zeta=1.0, sr_mask="half"),
               dict(task="deblur", zeta=1.0), dict(task="deconv", zeta=1.0), dict(task="sr", zeta=1.0, sigma_y=-1.0), dict(task="sr", zeta=1.0, tol=0.1)):
        with pytest.raises(ValueError):
            RMx.evaluate_restoration(_tiny(), img, method="dps", **kw)
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(_tiny(), img, "sr", zeta=1.0)                     # zeta without the method
    assert RMx.dps_operator("sr", scale=2) == (("mean", 2), None) and RMx.dps_operator("inpaint") == (("mean", 1), "center")
    assert RMx.dps_operator("deblur", kernel="aniso") == ("aniso", None) and RMx.dps_operator("deconv", psf="diag") == (("psf", "diag"), None)


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    from ddk import ops
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
        params = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[name][1]), name
    assert len(L.SIGNATURES["ddk_measure_residual"][1]) == 15 and len(L.SIGNATURES["ddk_measure_adjoint"][1]) == 10
    assert len(L.SIGNATURES["ddk_p_sample_update_guided"][1]) == len(L.SIGNATURES["ddk_p_sample_update"][1]) + 2      # g and zeta
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert "DDK_RESPONSE_LINEAR 0" in hdr and "DDK_RESPONSE_SATURATE 1" in hdr and ops.RESPONSES == {"linear": 0, "saturate": 1}
    for fn in ("measure_residual", "measure_adjoint", "x0_from_eps", "x0_from_eps_bwd", "p_sample_update_guided_"):
        assert callable(getattr(ops, fn))
    assert issubclass(AG.MeasureDistFn, torch.autograd.Function) and issubclass(AG.PredictX0Fn, torch.autograd.Function)
    assert callable(DDPM.restore_guided) and DownsampleDDPM.restore_guided is not DDPM.restore_guided


def test_bad_arguments_are_err_arg_before_any_launch():
    """every entry refuses on the host: no device is needed to be told so"""
    lib = L.load()
    buf = (ctypes.c_char * 272)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 16-byte aligned host memory: never read, no call gets as far as a launch
    q = ctypes.c_void_p(p.value + 4)
    for B, H, W, C, n in ((0, 16, 16, 3, 2), (1, 0, 16, 3, 2), (1, 16, 16, 0, 2), (1, 16, 16, 3, 3), (1, 16, 16, 3, 0), (1, 16, 16, 3, 16),
                          (1, 18, 16, 3, 4), (1, 16, 20, 3, 8), (1, 65536, 65536, 1, 1), (2 ** 26, 16, 16, 3, 1)):
        assert lib.ddk_measure_residual(p, p, None, n, 0, 1.0, p, p, B, H, W, C, None, 0, None) == -1, (B, H, W, C, n)
        assert lib.ddk_measure_adjoint(p, p, p, n, p, B, H, W, C, None) == -1, (B, H, W, C, n)
        assert lib.ddk_measure_residual_workspace_bytes(B, H, W, C, n) == 0
    assert lib.ddk_measure_residual(p, p, None, 2, 2, 1.0, p, p, 1, 16, 16, 3, None, 0, None) == -1 and "response" in L.last_error()
    for gain in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ddk_measure_residual(p, p, None, 2, 1, gain, p, p, 1, 16, 16, 3, None, 0, None) == -1 and "gain" in L.last_error()
    assert lib.ddk_measure_residual(p, None, None, 2, 0, 1.0, p, p, 1, 16, 16, 3, None, 0, None) == -1 and "null" in L.last_error()
    assert lib.ddk_measure_adjoint(p, p, None, 2, p, 1, 16, 16, 3, None) == -1 and "null" in L.last_error()
    # one launch up to 2048 measured elements per image, min(ceil(m / 2048), 64) slices of a double each above
    for (B, H, W, C, n), want in (((3, 16, 16, 8, 1), 0), ((3, 128, 128, 8, 8), 0), ((3, 19, 27, 4, 1), 3 * 2 * 8), ((2, 16, 32, 8, 1), 2 * 2 * 8),
                                  ((1, 126, 128, 8, 1), 63 * 8), ((1, 128, 128, 8, 1), 64 * 8), ((5, 128, 129, 8, 1), 5 * 64 * 8),
                                  ((1, 256, 256, 8, 1), 64 * 8)):
        assert lib.ddk_measure_residual_workspace_bytes(B, H, W, C, n) == want, (B, H, W, C, n)
    assert lib.ddk_measure_residual(p, p, None, 1, 0, 1.0, p, p, 2, 16, 32, 8, None, 0, None) == -1 and "workspace" in L.last_error()
    assert lib.ddk_measure_residual(p, p, None, 1, 0, 1.0, p, p, 2, 16, 32, 8, p, 16, None) == -1 and "workspace" in L.last_error()
    assert lib.ddk_measure_residual(p, p, None, 1, 0, 1.0, p, p, 2, 16, 32, 8, q, 64, None) == -1 and "workspace" in L.last_error()
    for per in (0, 6, -4):
        assert lib.ddk_x0_from_eps(p, p, p, p, p, 1, p, 1, per, None) == -1
        assert lib.ddk_x0_from_eps_bwd(p, p, p, p, p, p, 1, p, p, 1, per, None) == -1
        assert lib.ddk_p_sample_update_guided(p, p, None, p, p, p, p, p, p, p, p, 1, per, 0, 0, None) == -1
    assert lib.ddk_x0_from_eps(p, p, p, p, p, 1, p, 0, 8, None) == -1
    assert lib.ddk_x0_from_eps(q, p, p, p, p, 1, p, 1, 8, None) == -1 and "alignment" in L.last_error()
    assert lib.ddk_x0_from_eps_bwd(p, p, p, p, p, p, 1, p, q, 1, 8, None) == -1 and "alignment" in L.last_error()
    assert lib.ddk_x0_from_eps_bwd(p, p, None, p, p, p, 1, p, p, 1, 8, None) == -1 and "null" in L.last_error()
    assert lib.ddk_p_sample_update_guided(p, p, None, q, p, p, p, p, p, p, p, 1, 8, 0, 0, None) == -1 and "alignment" in L.last_error()
    assert lib.ddk_p_sample_update_guided(p, p, q, p, p, p, p, p, p, p, p, 1, 8, 0, 0, None) == -1 and "alignment" in L.last_error()
    assert lib.ddk_p_sample_update_guided(p, p, None, p, p, p, p, p, p, p, None, 1, 8, 0, 0, None) == -1 and "null" in L.last_error()
    assert lib.ddk_p_sample_update_guided(p, p, None, None, p, p, p, p, p, p, p, 1, 8, 0, 0, None) == -1 and "null" in L.last_error()


def test_the_ops_refuse_host_tensors_and_misshapen_ones():
    from ddk import ops
    x = torch.zeros(2, 16, 16, 3)
    for bad in (lambda: ops.measure_residual(x, torch.zeros(2, 8, 8, 3), None, 4), lambda: ops.measure_residual(x, torch.zeros(2, 4, 4, 3), None, 3),
                lambda: ops.measure_residual(x, torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 5), 4),
                lambda: ops.measure_residual(x, torch.zeros(2, 4, 4, 3), None, 4, "gamma"),
                lambda: ops.measure_residual(x, torch.zeros(2, 4, 4, 3), None, 4),                       # a host tensor: no CPU fallback
                lambda: ops.measure_adjoint(torch.zeros(2, 4, 4, 3), torch.zeros(3), torch.zeros(2), 4),
                lambda: ops.x0_from_eps(x, torch.zeros(2, 16, 16, 4), None, None, None),
                lambda: ops.p_sample_update_guided_(x, x, torch.zeros(2, 16, 16, 4), None, None, None, torch.zeros(5), None, None, torch.zeros(5)),
                lambda: ops.p_sample_update_guided_(x, x, x, None, None, None, torch.zeros(5), None, None, torch.zeros(4))):
        with pytest.raises(L.DDKError):
            bad()
