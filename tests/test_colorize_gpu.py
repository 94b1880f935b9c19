"""DDNM colourisation and grey super-resolution on the GPU (DDPM.colorize, ddk_sampler_run_restore_gray, p_update_restore_gray_kernel
and final_tail_kernel<.., StepKind::RestoreGray>) against tests/restore_gray_ref.py, the method restated around oracle/unet_ref with
oracle/philox_ref draws in NHWC order.

Shapes and bars are those of tests/test_restore_noisy_gpu.py for the corresponding cases: the lone op bit for bit on [3, 3, 16, 16] and
[3, 3, 8, 32]; the tiny DDPM (unet_chan 32, 3x16x16, unfused tail) against the restatement's chain to 1e-4 and between the Python loop
and the native sampler to 1e-5; a 128-channel UNet on 3x32x32 images at B = 16 for the fused tail (n = 1, 2 fused, n = 8 not
eligible), the 64-channel one at B = 32 and the 32-channel one (never fused); fused and unfused tails, and chains that share a workspace: the same bits.  The
consistency bar of an exact measurement is tests/test_colorize_cpu.py's."""
import json

import numpy as np
import pytest
import torch

import chain_cases as CC
import restore_gray_ref as RG
from helpers import ddpm_cfg, det_load, to_nhwc
from oracle import diffusion_ref as D
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4                  # chains against the restatement (tests/test_restore_masked_gpu.py)
LOOP_TOL = 1e-5             # the Python loop against the native sampler (the same file)
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SEED = 811
SIGMA_Y = 0.2
KINDS = [dict(), dict(ddim=True, eta=0.5)]
IDS = ["ancestral", "ddim_eta0.5"]
# the tiny model's chains: (n, weights, with a mask, sigma_y)
CASES = [(1, "mean", False, 0.0), (2, "luma", True, 0.0), (2, "mean", True, SIGMA_Y)]
CASE_IDS = ["n1_mean", "n2_luma_masked", "n2_mean_masked_noisy"]


def _bar(n, weights):
    """tests/test_colorize_cpu.py's: 8 (mean) or 16 (luma) times the group's 3 n^2 terms times 2^-24"""
    return (8 if weights == "mean" else 16) * 3 * n * n * 2.0 ** -24


def _y(shape, n, weights, name):
    """the exact-weights grey image of a clamped synthetic one, pooled: [B, 1, H/n, W/n] fp32"""
    return RG.apply_exact(syn.synthetic_normal(shape, name).clamp(-1, 1), n, weights).float().unsqueeze(1).contiguous()


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    """a measurement and a mask per case, one start state: computed once, never changed"""
    x_T = syn.synthetic_normal(SHAPE, "colorize.xT")
    ys, mks = {}, {}
    for n, weights, masked, sy in CASES:
        y = _y(SHAPE, n, weights, f"colorize.x{n}{weights}")
        if sy:
            y = y + sy * syn.synthetic_normal(tuple(y.shape), f"colorize.n{n}{weights}")
        ys[n, weights, sy] = y
        mks[n, weights, sy] = CC.mask("checker", 2, 16 // n, 16 // n) if masked else None
    return ys, mks, x_T


def _run(m, data, case, kw):
    ys, mks, x_T = data
    n, weights, _, sy = case
    return m.colorize(ys[n, weights, sy].to(DEV), mks[n, weights, sy], n, weights=weights, sigma_y=sy, respacing="8", x_T=x_T, seed=SEED, **kw).cpu()


@pytest.fixture(scope="module")
def native(tiny, data):
    """the native chain's results on the tiny model, 8 steps of the "8"-spaced schedule, shared by the tests that compare against them"""
    m, _ = tiny
    return {(case, i): _run(m, data, case, kw) for case in CASES for i, kw in zip(IDS, KINDS)}


# ---------------------------------------------------------------- the lone op, bit for bit
@pytest.mark.parametrize("hw", [(16, 16), (8, 32)], ids=["16x16", "8x32"])
@pytest.mark.parametrize("weights", ["mean", "luma"])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_lone_op_equals_restatement_bit_for_bit(n, weights, hw):
    """ops.p_sample_update_restore_gray_ given eps_hat against restore_gray_ref.step on the same inputs, for the three masks and without
    one.  The draws are the device's own (ddk_randn: the same Philox call and keying), first checked against oracle/philox_ref; rows 7
    and 3 have lam in (0, 1) and lam = 1, row 0 has lam = 1 and no draw.  y is NaN wherever the mask is 0: the result must not see it."""
    from ddk import ops
    h, w = hw
    g = torch.Generator().manual_seed(29 * n + len(weights) + h)
    B = 3
    shape = (B, 3, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    y0 = torch.rand(B, 1, h // n, w // n, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])
    tab = CC.hand_tables(g, noisy=True)
    tab["lam"][0] = 1.0                  # this kind's row 0 has lam = 1
    seed, stream = 13579, 6
    z = CC.philox_draws(B, 3, h, w, t, seed, stream)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    dtab = {k: v.to(DEV) for k, v in tab.items()}
    row = lambda k: tab[k][t]
    cases = [(kind, CC.mask(kind, B, h // n, w // n)) for kind in ("checker", "one_measured", "one_hidden")] + [("none", None)]
    for kind, mk in cases:
        y = y0 if mk is None else torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
        want = RG.step(x, e, y, mk, n, weights, row("c_recip"), row("c_recipm1"), row("c1"), row("c2"), sg, row("lam"), row("sgm"), z)
        xs = to_nhwc(x).to(DEV)
        ops.p_sample_update_restore_gray_(xs, to_nhwc(e).to(DEV), y[:, 0].contiguous().to(DEV), None if mk is None else mk.to(DEV), n, weights,
                                          t.to(DEV), **dtab, seed=seed, stream_id=stream)
        got = xs.cpu().permute(0, 3, 1, 2)
        assert torch.isfinite(got).all(), kind
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))
        # row 0 (lam = 1, no draw, c1 = 1, c2 = 0) returns x0': its grey image is y on the measured groups, to the rounding bar
        m0 = torch.ones(h // n, w // n) if mk is None else mk[0]
        err = float(((RG.apply_exact(got[:1], n, weights)[0] - torch.nan_to_num(y[0, 0]).double()) * m0).abs().max())
        assert err <= _bar(n, weights), (kind, err)


def test_lone_op_rejects_bad_arguments():
    from ddk import lib as L
    from ddk import ops
    x = torch.zeros(1, 8, 8, 3, device=DEV)
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma", "lam", "sgm")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    y = torch.zeros(1, 8, 8, device=DEV)
    with pytest.raises(L.DDKError):                                                        # n = 3
        ops.p_sample_update_restore_gray_(x, x.clone(), torch.zeros(1, 2, 2, device=DEV), None, 3, "mean", t, **tab)
    with pytest.raises(L.DDKError):                                                        # unknown weights
        ops.p_sample_update_restore_gray_(x, x.clone(), y, None, 1, "rgb", t, **tab)
    x4 = torch.zeros(1, 8, 8, 4, device=DEV)
    with pytest.raises(L.DDKError):                                                        # not three channels
        ops.p_sample_update_restore_gray_(x4, x4.clone(), y, None, 1, "mean", t, **tab)
    with pytest.raises(L.DDKError):                                                        # a null table
        ops.p_sample_update_restore_gray_(x, x.clone(), y, None, 1, "mean", t, **dict(tab, lam=None))
    lib = L.load()
    args = [L.ptr(x), L.ptr(x.clone()), L.ptr(y), None, 1, 3, L.ptr(t)] + [L.ptr(tab[k]) for k in tab] + [1, 8, 8, 3, 0, 0, L.stream()]
    assert lib.ddk_p_sample_update_restore_gray(*args) == -1 and "weights" in L.last_error()      # weights outside {1, 2}
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0                                                     # on an error x is not touched


# ---------------------------------------------------------------- the tiny DDPM, 8 steps of "8"
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, native, kw, case):
    _, eps = tiny
    ys, mks, x_T = data
    n, weights, _, sy = case
    got = native[case, IDS[KINDS.index(kw)]]
    want = RG.RestoreGray(BETAS, "8").run(eps, x_T, ys[n, weights, sy], mks[n, weights, sy], n, weights, sy, SEED, **kw)
    err = float((got - want).abs().max())
    print(f"colorize n={n} {weights} sigma_y={sy} tiny DDPM, 8 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_and_python_loop_is_close(tiny, data, native, kw, case):
    m, _ = tiny
    graphed = native[case, IDS[KINDS.index(kw)]]
    with CC.toggled(m, "use_graph", False):
        eager = _run(m, data, case, kw)
    assert torch.equal(graphed, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = _run(m, data, case, kw)
    err = float((loop - graphed).abs().max())
    print(f"Python loop vs native, colorize {case} 8 steps {kw}: {err:.3g}")
    assert err < LOOP_TOL


@pytest.mark.parametrize("case", CASES[:2], ids=CASE_IDS[:2])
def test_an_exact_measurement_is_met_to_the_rounding_bar(data, native, case):
    """sigma_y = 0 on the ancestral chain, whose row 0 has c1 = 1, c2 = 0 and no draw: the result is x0' and its grey image is y on
    the measured groups"""
    ys, mks, _ = data
    n, weights, _, sy = case
    out = native[case, "ancestral"]
    mk = mks[n, weights, sy]
    meas = torch.ones(2, 16 // n, 16 // n) if mk is None else mk
    err = float(((RG.apply_exact(out, n, weights) - ys[n, weights, sy][:, 0].double()) * meas).abs().max())
    print(f"colorize n={n} {weights}: |A x_out - y| = {err:.3g} (bar {_bar(n, weights):.3g})")
    assert err <= _bar(n, weights), err


def test_unmeasured_y_reaches_nothing(tiny, data, native):
    m, _ = tiny
    ys, mks, x_T = data
    case = CASES[1]
    n, weights, _, sy = case
    y, mk = ys[n, weights, sy], mks[n, weights, sy]
    y_nan = torch.where(CC.sel(mk, y), y, torch.full_like(y, float("nan")))
    from ddk import ops
    tables, use = m._gray_tables("8", False, 0.0, 0.0)
    plan = m._eps_model_nhwc().plan()
    x = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    plan.sample_restore_gray_nhwc(x, y_nan[:, 0].contiguous().to(DEV), mk.to(DEV), n, weights, tables, len(use) - 1, seed=SEED,
                                  stream_id=int(m.rng_stream_id), timesteps=use)
    assert torch.equal(ops.nhwc_to_nchw(x).cpu(), native[case, "ancestral"])


# ---------------------------------------------------------------- the fused tail: 3x32x32 images, B = 16
@pytest.fixture(scope="module", params=[128, 64, 32], ids=["c128", "c64", "c32"])
def wide(request):
    from models import DDPM, Unet
    cfg = ddpm_cfg(request.param, 3, 32)
    return det_load(DDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval(), request.param


@pytest.mark.parametrize("n,masked,weights", [(1, False, "luma"), (2, True, "mean"), (2, False, "luma"), (8, True, "luma")],
                         ids=["n1", "n2", "n2_nomask", "n8"])
def test_fused_tail_equals_unfused_bit_for_bit(wide, n, masked, weights):
    """ "6" steps, DDIM eta 0.5.  On the 128-wide model n = 1 and n = 2 (with and without a mask) end in final_tail_kernel<..,
    RestoreGray>, n = 8 (W n = 256 > 128) in p_update_restore_gray_kernel whatever the option says; with DDK_OPT_RESTORE_FUSED_TAIL = 0
    all end in the unfused kernel, with the same bits.  The 64-wide model does the same at B = 32; the 32-wide model's final conv
    never runs in the one-pass form the fused tail sits behind, so there both runs take the unfused kernel
    (ddk_sampler_restore_gray_tail_parts says which tail runs)."""
    from ddk import ops
    m, chan = wide
    plan = m._eps_model_nhwc().plan()
    before = ops.cluster_timeouts()
    B = 32 if chan == 64 else 16         # the 64-wide final conv runs unsplit, which the one-launch tail needs, from B = 32 on
    shape = (B, 3, 32, 32)
    parts = plan.restore_gray_tail_parts(B, 32, 32, n)
    print(f"unet_chan {chan}, B = {B}, n = {n}: fused tail tiles {parts}")
    if chan >= 64:
        assert parts == (0 if n == 8 else 8)
    assert parts >= 0 and (n != 8 or parts == 0)
    y0 = _y(shape, n, weights, f"colorize.wide.{n}")
    mk = CC.mask("checker", B, 32 // n, 32 // n) if masked else None
    y = torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan"))) if masked else y0
    x_T = syn.synthetic_normal(shape, "colorize.wide.xT")
    run = lambda: m.colorize(y.to(DEV), mk, n, weights=weights, respacing="6", ddim=True, eta=0.5, x_T=x_T, seed=SEED).cpu()
    fused = run()
    plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 0)
    try:
        assert plan.restore_gray_tail_parts(B, 32, 32, n) == 0
        unfused = run()
    finally:
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- one workspace, three kinds of chain, two weightings
def test_chains_share_a_workspace_and_each_weighting_has_its_own_graph(tiny, data):
    """a grey, a noisy and a plain ancestral chain on the same workspace, state buffer, base tables and t_start, in two orders, and
    "mean" then "luma" back to back: each equals its own single run on a fresh workspace bit for bit (the kind, n, the presence of a
    mask, the weights and the two table buffers are in the graph key; y and the mask are staged by every call)"""
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    _, _, x_T = data
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    before = ops.cluster_timeouts()
    gtab, use = m._gray_tables("8", False, 0.0, 0.0)
    ntab, _ = m._noisy_tables("8", False, 0.0, 0.3)
    tables, _ = m._spaced_tables("8", False, 0.0)
    assert all(torch.equal(gtab[k], tables[k]) and torch.equal(ntab[k], tables[k]) for k in tables)
    K = len(use)
    nbytes = max(lib.ddk_sampler_restore_gray_workspace_bytes(plan.handle, 2, 16, 16, K - 1, n) for n in (1, 2))
    assert nbytes == lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    assert nbytes >= max(lib.ddk_sampler_restore_noisy_workspace_bytes(plan.handle, 2, 16, 16, K - 1, n) for n in (1, 2))
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    img = syn.synthetic_normal(SHAPE, "colorize.ws.x").clamp(-1, 1)
    yg = {n: RG.apply_exact(img, n, "mean").float().contiguous().to(DEV) for n in (1, 2)}            # [2, 16/n, 16/n]
    yc = {n: ops.nchw_to_nhwc(torch.nn.functional.avg_pool2d(img, n).contiguous().to(DEV)) if n > 1 else ops.nchw_to_nhwc(img.to(DEV))
          for n in (1, 2)}
    md = {n: CC.mask("checker", 2, 16 // n, 16 // n).to(DEV) for n in (1, 2)}
    # what -> (weights code, n, with a mask); "nz1": the noisy chain, "anc": the ancestral one
    jobs = {"mean1": (1, 1, False), "luma1": (2, 1, False), "mean1m": (1, 1, True), "luma2": (2, 2, True), "mean2nm": (1, 2, False),
            "nz1": None, "anc": None}

    def launch(what, a, tmap, stream):
        if what == "anc":
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        if what == "nz1":
            return lib.ddk_sampler_run_restore_noisy(a, tmap, L.ptr(ntab["lam"]), L.ptr(ntab["sgm"]), L.ptr(yc[1]), L.ptr(md[1]), 1, stream)
        wcode, n, masked = jobs[what]
        return lib.ddk_sampler_run_restore_gray(a, tmap, L.ptr(gtab["lam"]), L.ptr(gtab["sgm"]), L.ptr(yg[n]), L.ptr(md[n]) if masked else None,
                                                n, wcode, stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    x, tmap = sh.x, sh.tmap
    single = {what: sh.alone(what) for what in jobs}
    names = list(jobs)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert not torch.equal(single[p], single[q]), (p, q)
    for order in (("mean1", "luma1", "mean1", "nz1", "anc", "luma2", "mean2nm", "mean1m", "luma1"),
                  ("anc", "mean2nm", "nz1", "luma1", "mean1m", "luma2", "mean1", "anc", "nz1")):
        sh.interleaved(order, single)
    # bad weights, a bad n, a null table and injected noise are rejected
    with CC.workspace(plan, nbytes) as ws:
        a = CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED)
        call = lambda lam, sgm, y, mk, n, wc: lib.ddk_sampler_run_restore_gray(a, tmap, lam, sgm, y, mk, n, wc, L.stream())
        lam, sgm = L.ptr(gtab["lam"]), L.ptr(gtab["sgm"])
        assert call(lam, sgm, L.ptr(yg[1]), None, 1, 0) == -1 and "weights" in L.last_error()
        assert call(lam, sgm, L.ptr(yg[1]), None, 1, 3) == -1 and "weights" in L.last_error()
        assert call(lam, sgm, L.ptr(yg[1]), None, 3, 1) == -1
        assert call(None, sgm, L.ptr(yg[1]), None, 1, 1) == -1 and "table" in L.last_error()
        noise = torch.zeros((K, *x.shape), device=DEV)
        a.noise = L.ptr(noise)
        assert call(lam, sgm, L.ptr(yg[1]), None, 1, 1) == -1 and "noise" in L.last_error()
    assert ops.cluster_timeouts() == before


def test_a_model_with_other_than_three_channels_is_refused_by_the_chain_entry():
    from ddk import lib as L
    from models import DDPM, Unet
    cfg = ddpm_cfg(32, 8, 16)
    m = det_load(DDPM(cfg, Unet(cfg), DEV, 8)).to(DEV).eval()
    plan = m._eps_model_nhwc().plan()
    tables, use = m._spaced_tables("8", False, 0.0)
    tables = dict(tables, lam=torch.ones(8, device=DEV), sgm=tables["sigma"].clone())
    x = torch.zeros(2, 16, 16, 8, device=DEV)
    with pytest.raises(L.DDKError, match="3-channel"):                                     # the Python binding's own check
        plan.sample_restore_gray_nhwc(x, torch.zeros(2, 16, 16, device=DEV), None, 1, "mean", tables, 7, timesteps=use)
    lib = plan._lib
    plan._need_packed("srg")
    K = len(use)
    tmap = CC.timestep_map(use)
    nbytes = lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    ws = CC.fresh_workspace(nbytes)
    a = CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED)
    y = torch.zeros(2, 16, 16, device=DEV)
    assert lib.ddk_sampler_run_restore_gray(a, tmap, L.ptr(tables["lam"]), L.ptr(tables["sgm"]), L.ptr(y), None, 1, 1, L.stream()) == -1
    assert "3-channel" in L.last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the evaluator and the command lines
def test_evaluator_colorize(tiny):
    from utils import restoration_metrics as RMx
    m, _ = tiny
    imgs = (np.random.default_rng(2).random((2, 16, 16, 3)) * 255).astype(np.uint8)
    kw = dict(batch_size=2, seed=5, respacing="5")
    res = RMx.evaluate_restoration(m, imgs, "colorize", **kw)
    assert (res["method"], res["weights"], res["unet_forwards"]) == ("ddnm_gray", "mean", 5) and "sigma_y" not in res
    assert set(res["methods"]) == {"restored", "replicate"} and res["images"]["restored"].shape == imgs.shape
    grey = res["images"]["replicate"]
    assert (grey[..., 0] == grey[..., 1]).all() and (grey[..., 1] == grey[..., 2]).all()
    # an exact measurement: max |A x_out - y| of the float output in uint8 levels.  The chain meets _bar; the evaluator forms A x_out in
    # fp32, a weighted mean of 3 n^2 values within [-1, 1] whose own rounding is below (3 n^2 + 1) 2^-24 < _bar: twice the bar in all
    assert res["consistency"].shape == (2,) and float(res["consistency"].max()) <= 127.5 * 2 * _bar(1, "mean")
    up = RMx.evaluate_restoration(m, imgs, "colorize", scale=2, weights="luma", sr_mask="half", **kw)
    assert up["weights"] == "luma" and set(up["methods"]) == {"restored", "replicate", "bicubic"}
    assert float(up["consistency"].max()) <= 127.5 * 2 * _bar(2, "luma")
    noisy = RMx.evaluate_restoration(m, imgs, "colorize", weights="luma", sigma_y=0.1, **kw)
    assert noisy["method"] == "ddnm_gray" and noisy["sigma_y"] == 0.1 and (noisy["consistency"] > 0).all()
    again = RMx.evaluate_restoration(m, imgs, "colorize", weights="luma", sigma_y=0.1, **kw)
    assert np.array_equal(again["images"]["restored"], noisy["images"]["restored"])             # the noise is seeded
    for bad in (dict(weights="rgb"), dict(method="repaint"), dict(dpm_solver=True), dict(scale=3), dict(sigma_y=-1.0)):
        with pytest.raises(ValueError):
            RMx.evaluate_restoration(m, imgs, "colorize", **dict(kw, **bad))
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(m, imgs, "sr", weights="luma", **kw)
    # the existing task's result has the keys it had
    sr = RMx.evaluate_restoration(m, imgs, "sr", scale=2, **kw)
    assert set(sr) == {"n_images", "method", "methods", "images", "unet_forwards", "consistency", "consistency_u8"} and sr["method"] == "ddnm"


def test_evaluate_cli_colorize_and_sr_settings(tmp_path):
    cfg_path, images_path, _, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    base = ["evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--timestep_respacing", "5", "--batch_size", "2",
            "--seed", "9", "--json", tmp_path / "out.json"]
    CC.run_script(*base, "--task", "colorize", "--weights", "luma", env=env)
    out = json.loads((tmp_path / "out.json").read_text())
    st, me = out["settings"], out["metrics"]
    assert (st["task"], st["method"], st["weights"], st["scale"], st["unet_forwards"], st["respacing"]) == ("colorize", "ddnm_gray", "luma", 1, 5, "5")
    assert set(me) == {"restored", "replicate", "consistency", "consistency_u8"} and me["consistency"]["max"] <= 127.5 * 2 * _bar(1, "luma")
    CC.run_script(*base, "--task", "sr", "--scale", "2", env=env)
    out = json.loads((tmp_path / "out.json").read_text())
    assert set(out["settings"]) == {"checkpoint", "synthetic", "model", "task", "images", "n_images", "batch_size", "seed", "method",
                                    "unet_forwards", "respacing", "scale", "ddim", "eta"}
    assert (out["settings"]["method"], out["settings"]["scale"]) == ("ddnm", 2)
    assert set(out["metrics"]) == {"restored", "replicate", "bicubic", "consistency", "consistency_u8"}


def test_colorize_cli(tmp_path):
    cfg_path, _, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    grey = imgs.mean(axis=3).round().astype(np.uint8)
    np.save(tmp_path / "grey.npy", grey)
    CC.run_script("colorize_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", tmp_path / "grey.npy",
                  "--timestep_respacing", "5", "--batch_size", "2", "--seed", "3", "--out_dir", tmp_path, env=env)
    out = np.load(tmp_path / "clitest_color1_mean_5.npy")
    back = np.load(tmp_path / "clitest_color1_mean_5_gray.npy")
    assert out.shape == (3, 16, 16, 3) and out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert back.shape == (3, 16, 16, 1) and np.array_equal(back[..., 0], grey)
