"""ddk_image_metrics (image_sq_err_kernel, ssim_tile_kernel, ssim_finish_kernel) against tests/ssim_ref.py,
and the restoration evaluator built on it (utils/restoration_metrics.py, evaluate_restoration.py) on a tiny synthetic DDPM.

Bars.  Squared-error sums and counts: equal to numpy's integers.  SSIM: within ssim_ref.SSIM_BAR = 4.8e-7 of the float64
restatement, 4 x the 1.20e-7 that the kernel's own formula costs in torch's fp32 on the CPU on these very inputs (unshifted: 6.68e-5).
Repeated runs and any split of the batch: the same bits.  With synthetic weights the quality numbers mean nothing, so the end-to-end
tests check the plumbing (what is scored against what, finiteness, the exact cases) and assert no order between methods."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssim_ref as R
from ddk import lib as L
from ddk import ops
from helpers import ddpm_cfg, det_load
from utils import restoration_metrics as RM

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = ddpm_cfg(32, 3, 16, T=100)
RAGGED = (3, 45, 70, 3)
CASES = [(s, k) for s in R.SHAPES for k in R.PAIRS]
IDS = ["x".join(map(str, s)) + "-" + k for s, k in CASES]


def _dev(x):
    return torch.tensor(np.asarray(x)).to(DEV)


def _metrics(a, b, mask=None):
    return ops.image_metrics(_dev(a), _dev(b), None if mask is None else _dev(mask))


def _same_bits(x, y):
    return np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_against_restatement(shape, kind):
    a, b = R.pair(shape, kind)
    got = _metrics(a, b)
    s, k = R.sq_err(a, b)
    err = float(np.abs(got["ssim"].double().numpy() - R.reference(shape, kind)).max())
    print(f"{shape} {kind}: sq_sum {got['sq_sum'].tolist()} ssim {got['ssim'].tolist()} |ssim - f64| {err:.3e} (bar {R.SSIM_BAR:.2e})")
    assert got["sq_sum"].tolist() == s.tolist() and got["count"].tolist() == k.tolist()
    assert got["psnr"].dtype == torch.float64 and got["mse"].dtype == torch.float64 and got["ssim"].dtype == torch.float32
    want_psnr = R.psnr(a, b)
    if kind == "same":
        assert np.isinf(got["psnr"].numpy()).all() and (got["psnr"] > 0).all() and got["ssim"].tolist() == [1.0] * shape[0]
    else:
        assert np.allclose(got["psnr"].numpy(), want_psnr, rtol=1e-14, atol=0)
    assert np.array_equal(got["mse"].numpy(), s / k)
    assert err <= R.SSIM_BAR


@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
@pytest.mark.parametrize("mkind", ["noise", "none", "one"])
def test_masked_squared_error_is_exact(shape, mkind):
    a, b = R.pair(shape, "noise")
    mask = R.mask_for(shape, mkind)
    got, plain = _metrics(a, b, mask), _metrics(a, b)
    s, k = R.sq_err(a, b, mask)
    assert got["sq_sum"].tolist() == s.tolist() and got["count"].tolist() == k.tolist()
    want = R.psnr(a, b, mask)
    assert np.array_equal(np.isnan(got["psnr"].numpy()), k == 0) and np.array_equal(np.isnan(got["mse"].numpy()), k == 0)
    assert np.allclose(got["psnr"].numpy()[k > 0], want[k > 0], rtol=1e-14, atol=0)
    if mkind == "none":
        assert got["count"].tolist() == [0] * shape[0]
    if mkind == "one":
        assert got["count"].tolist() == [0] * (shape[0] - 1) + [shape[3]]
    assert _same_bits(got["ssim"], plain["ssim"])              # the mask applies to the squared error only
    assert _metrics(a, b, mask != 0)["count"].tolist() == k.tolist()          # a bool mask is taken as well


def test_one_pixel_changes_both_metrics():
    shape = (1, 12, 13, 3)
    a, b = R.pair(shape, "noise")
    b2 = b.copy()
    step = 1 if b2[0, 5, 6, 1] < 255 else -1
    b2[0, 5, 6, 1] += step
    d = int(a[0, 5, 6, 1]) - int(b[0, 5, 6, 1])
    got, got2 = _metrics(a, b), _metrics(a, b2)
    assert int(got2["sq_sum"][0]) - int(got["sq_sum"][0]) == (d - step) ** 2 - d ** 2 != 0
    assert got2["count"].tolist() == got["count"].tolist()
    assert not _same_bits(got["ssim"], got2["ssim"])
    assert abs(float(got2["ssim"][0]) - float(R.ssim(a, b2)[0])) <= R.SSIM_BAR


def test_bit_stable_and_independent_of_the_batch():
    a, b = R.pair(RAGGED, "near")
    mask = R.mask_for(RAGGED, "noise")
    first, second = _metrics(a, b, mask), _metrics(a, b, mask)
    for key in ("ssim", "sq_sum", "count"):
        assert torch.equal(first[key], second[key])
    assert _same_bits(first["ssim"], second["ssim"])
    for i in range(RAGGED[0]):
        one = _metrics(a[i:i + 1], b[i:i + 1], mask[i:i + 1])
        assert _same_bits(one["ssim"], first["ssim"][i:i + 1])
        assert one["sq_sum"].tolist() == first["sq_sum"][i:i + 1].tolist() and one["count"].tolist() == first["count"][i:i + 1].tolist()


def test_bad_arguments_leave_the_device_untouched():
    """the Python layer raises before any allocation; the C entry point refuses before any launch: the outputs keep their fill.
    (nothing out of range is ever launched)"""
    z = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    bad = [(z.float(), z, None), (z, z[:, :, :15], None), (z[:, :10], z[:, :10], None), (z, z, torch.zeros(1, 16, 15, device=DEV))]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for a, b, m in bad:
        with pytest.raises(ValueError):
            ops.image_metrics(a, b, m)
    with pytest.raises(L.DDKError):
        ops.image_metrics(z.cpu(), z)
    assert torch.cuda.memory_allocated() == before

    lib = L.load()
    sq = torch.full((1, 2), -7, dtype=torch.int64, device=DEV)
    ssim = torch.full((1,), -7.0, device=DEV)
    ws = torch.zeros(64, device=DEV)
    n = lib.ddk_image_metrics_workspace_bytes(1, 16, 16, 3)
    assert n == 3 * 8 and lib.ddk_image_metrics_workspace_bytes(1, 10, 16, 3) == 0 and lib.ddk_image_metrics_workspace_bytes(1, 16, 16, 5) == 0
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(a=p(z), b=p(z), mask=None, N=1, H=16, W=16, C=3, sq=p(sq), ssim=p(ssim), ws=p(ws), nbytes=n)
    for change in (dict(C=0), dict(C=5), dict(H=10), dict(W=10), dict(N=0), dict(a=None), dict(b=None), dict(sq=None), dict(ssim=None),
                   dict(ws=None), dict(nbytes=n - 1)):
        k = dict(good, **change)
        rc = lib.ddk_image_metrics(k["a"], k["b"], k["mask"], k["N"], k["H"], k["W"], k["C"], k["sq"], k["ssim"], k["ws"], k["nbytes"],
                                   L.stream())
        assert rc != 0 and "image_metrics" in L.last_error(), change
        with pytest.raises(L.DDKError):
            L.check(rc, "image_metrics")
    torch.cuda.synchronize()
    assert sq.tolist() == [[-7, -7]] and ssim.tolist() == [-7.0]
    assert ops.image_metrics(z, z)["ssim"].tolist() == [1.0]


# ------------------------------------------------------------------ end to end on a tiny synthetic DDPM
@pytest.fixture(scope="module")
def tiny():
    from models import DDPM, Unet
    m = det_load(DDPM(CFG, Unet(CFG), DEV, 3)).to(DEV).eval()
    m.rng_stream_id = 0
    return m


@pytest.fixture(scope="module")
def images():
    return R.u8_image((4, 16, 16, 3), "e2e.images")


def _check_methods(res, ref, names, hidden=None):
    assert list(res["methods"]) == names and list(res["images"]) == names
    for name in names:
        img = res["images"][name]
        assert img.dtype == np.uint8 and img.shape == ref.shape
        direct = _metrics(img, ref)
        assert np.array_equal(res["methods"][name]["psnr"], direct["psnr"].numpy())
        assert np.array_equal(res["methods"][name]["ssim"], direct["ssim"].double().numpy())
        if hidden is not None:
            assert np.array_equal(res["methods"][name]["psnr_hidden"], _metrics(img, ref, hidden)["psnr"].numpy(), equal_nan=True)


@pytest.mark.parametrize("kw", [dict(scale=2, respacing="10"), dict(scale=4, respacing="ddim10", ddim=True)], ids=["x2", "x4-ddim"])
def test_super_resolution_scores(tiny, images, kw):
    res = RM.evaluate_restoration(tiny, images, "sr", batch_size=3, seed=5, **kw)
    print("sr", kw, {k: v for k, v in RM.report(res).items()})
    assert res["n_images"] == 4
    _check_methods(res, images, ["restored", "replicate", "bicubic"])
    s = kw["scale"]
    y = RM.pool(RM.from_u8(images), s)
    assert np.array_equal(res["images"]["replicate"], RM.to_u8(RM.replicate(y, s)).numpy())
    assert np.array_equal(res["images"]["bicubic"], RM.to_u8(RM.bicubic(y, s)).numpy())
    assert res["consistency"].shape == (4,) and np.isfinite(res["consistency"]).all() and res["consistency"].max() <= 1.0
    assert np.isfinite(res["consistency_u8"]).all()
    for m in res["methods"].values():
        assert np.isfinite(m["psnr"]).all() and np.isfinite(m["ssim"]).all() and (np.abs(m["ssim"]) <= 1 + 1e-6).all()
    again = RM.evaluate_restoration(tiny, images, "sr", batch_size=3, seed=5, **kw)
    assert np.array_equal(again["images"]["restored"], res["images"]["restored"])            # the seed fixes the chain


def test_inpainting_scores(tiny, images):
    kw = dict(respacing="10", jump_length=3, jump_n_sample=2)
    res = RM.evaluate_restoration(tiny, images, "inpaint", batch_size=3, seed=5, mask="center", **kw)
    print("inpaint", RM.report(res))
    hidden = (RM.make_mask("center", 4, 16, 16)[:, 0] == 0).numpy().astype(np.uint8)
    _check_methods(res, images, ["restored", "mean_fill"], hidden)
    known = hidden == 0
    for name in ("restored", "mean_fill"):
        assert np.array_equal(res["images"][name][known], images[known])                    # the known pixels come back as given
        m = res["methods"][name]
        assert np.isfinite(m["psnr"]).all() and np.isfinite(m["ssim"]).all() and np.isfinite(m["psnr_hidden"]).all()
        assert (m["psnr_hidden"] < m["psnr"]).all()            # arithmetic, not quality: the same error over a quarter of the pixels
    mean = RM.to_u8(RM.mean_fill(RM.from_u8(images), RM.make_mask("center", 4, 16, 16))).numpy()
    assert np.array_equal(res["images"]["mean_fill"], mean)


def test_inpainting_with_everything_known_is_exact(tiny, images):
    res = RM.evaluate_restoration(tiny, images, "inpaint", batch_size=4, seed=5, mask=torch.ones(1, 1, 16, 16), respacing="5",
                                  jump_length=2, jump_n_sample=1)
    for name in ("restored", "mean_fill"):
        assert np.array_equal(res["images"][name], images)
        m = res["methods"][name]
        assert np.isposinf(m["psnr"]).all() and m["ssim"].tolist() == [1.0] * 4 and np.isnan(m["psnr_hidden"]).all()
    rep = RM.report(res)["restored"]
    assert rep["psnr"]["mean"] == math.inf and rep["ssim"]["mean"] == 1.0 and rep["psnr_hidden"]["n"] == 0


@pytest.mark.parametrize("task", ["inpaint", "sr"])
def test_cli_writes_the_report(tmp_path, images, task):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(CFG, model="ddpm", dataset="celeba")
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    np.save(tmp_path / "imgs.npy", images)
    extra = (["--mask", "left", "--timestep_respacing", "5", "--jump_length", "2", "--jump_n_sample", "2"] if task == "inpaint" else
             ["--scale", "2", "--timestep_respacing", "ddim5", "--use_ddim"])
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "downsampled-diffusion_amd"))
    script = os.path.join(root, "downsampled-diffusion_amd", "evaluate_restoration.py")
    r = subprocess.run([sys.executable, script, "--synthetic", str(tmp_path / "cfg.json"), "--images", str(tmp_path / "imgs.npy"),
                        "--task", task, "--batch_size", "2", "--seed", "9", "--json", str(tmp_path / "out.json")] + extra,
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads((tmp_path / "out.json").read_text())
    st, me = out["settings"], out["metrics"]
    assert st["task"] == task and st["n_images"] == 4 and st["seed"] == 9 and st["batch_size"] == 2 and st["checkpoint"] is None
    assert st["synthetic"] == str(tmp_path / "cfg.json") and st["images"] == str(tmp_path / "imgs.npy") and st["model"] == "ddpm"
    if task == "inpaint":
        assert (st["mask"], st["respacing"], st["jump_length"], st["jump_n_sample"]) == ("left", "5", 2, 2)
        methods, keys = ["restored", "mean_fill"], ["psnr", "ssim", "psnr_hidden"]
    else:
        assert (st["scale"], st["respacing"], st["ddim"], st["eta"]) == (2, "ddim5", True, 0.0)
        methods, keys = ["restored", "replicate", "bicubic"], ["psnr", "ssim"]
        for k in ("consistency", "consistency_u8"):
            assert all(math.isfinite(me[k][f]) for f in ("mean", "stderr", "max"))
        assert me["consistency"]["max"] <= 1.0
    for name in methods:
        assert sorted(me[name]) == sorted(keys)
        for k in keys:
            assert me[name][k]["n"] == 4 and math.isfinite(me[name][k]["mean"]) and math.isfinite(me[name][k]["stderr"]), (name, k)
    assert json.loads(r.stdout[r.stdout.index("{"):]) == out
