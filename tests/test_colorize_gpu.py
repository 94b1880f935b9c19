"""DDNM colourisation and grey super-resolution on the GPU (DDPM.colorize, ddk_sampler_run_restore_gray, p_update_restore_gray_kernel
and final_tail_kernel<.., StepKind::RestoreGray>) against tests/restore_gray_ref.py, the method restated around oracle/unet_ref with
oracle/philox_ref draws in NHWC order.

Shapes and bars are those of tests/test_restore_noisy_gpu.py for the corresponding cases: the lone op bit for bit on [3, 3, 16, 16] and
[3, 3, 8, 32]; the tiny DDPM (unet_chan 32, 3x16x16, unfused tail) against the restatement's chain to 1e-4 and between the Python loop
and the native sampler to 1e-5; a 128-channel UNet on 3x32x32 images at B = 16 for the fused tail (n = 1, 2 fused, n = 8 not
eligible), the 64-channel one at B = 32 and the 32-channel one (never fused); fused and unfused tails, and chains that share a workspace: the same bits.  The
consistency bar of an exact measurement is tests/test_colorize_cpu.py's."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import restore_gray_ref as RG
from helpers import ddpm_cfg, det_load
from oracle import diffusion_ref as D
from oracle import philox_ref as PR
from oracle import unet_ref as U
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


def _mask(kind, b, h, w):
    """[b, h, w] {0, 1}: a checkerboard, a single measured block / pixel, a single hidden one (at another place per image)"""
    i, j = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if kind == "checker":
        return torch.stack([((i + j + k) % 2).float() for k in range(b)])
    m = torch.zeros(b, h, w) if kind == "one_measured" else torch.ones(b, h, w)
    for k in range(b):
        m[k, (k * 3 + 1) % h, (k * 5 + w - 1) % w] = 1.0 - m[k, 0, 0]
    return m


def _y(shape, n, weights, name):
    """the exact-weights grey image of a clamped synthetic one, pooled: [B, 1, H/n, W/n] fp32"""
    return RG.apply_exact(syn.synthetic_normal(shape, name).clamp(-1, 1), n, weights).float().unsqueeze(1).contiguous()


def _sel(mk, y):
    return (mk != 0).unsqueeze(1).expand_as(y)


nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def tiny():
    from models import DDPM, Unet
    m = det_load(DDPM(CFG, Unet(CFG), DEV, 3)).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    return m, (lambda x, t: U.unet_forward(sd, CFG, x, t, pre="latent_model."))


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
        mks[n, weights, sy] = _mask("checker", 2, 16 // n, 16 // n) if masked else None
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
def _hand_tables(g):
    """8 rows, made by hand: lam strictly between 0 and 1 in rows 1, 2, 5, 6, 7, exactly 1 in rows 0, 3 and 4, sgm != sigma everywhere"""
    tab = {k: torch.rand(8, generator=g) * s for k, s in (("c_recip", 3.0), ("c_recipm1", 2.0), ("c1", 1.0), ("c2", 1.0), ("sigma", 0.5))}
    tab["c1"][0], tab["c2"][0] = 1.0, 0.0
    tab["lam"] = 0.1 + 0.8 * torch.rand(8, generator=g)
    tab["lam"][0] = tab["lam"][3] = tab["lam"][4] = 1.0
    tab["sgm"] = tab["sigma"] * (0.1 + 0.8 * torch.rand(8, generator=g))
    tab["sgm"][0] = 0.0
    assert ((tab["lam"][[1, 2, 5, 6, 7]] > 0) & (tab["lam"][[1, 2, 5, 6, 7]] < 1)).all() and (tab["sgm"][1:] != tab["sigma"][1:]).all()
    return tab


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
    tab = _hand_tables(g)
    seed, stream = 13579, 6
    z_dev = torch.stack([ops.randn((B, h, w, 3), DEV, seed, int(tb), stream)[b] for b, tb in enumerate(t)]).cpu()
    z_ref = torch.from_numpy(np.stack([PR.philox_normal(B * h * w * 3, seed, int(tb), stream).reshape(B, h, w, 3)[b]
                                       for b, tb in enumerate(t)]))
    assert float((z_dev - z_ref).abs().max()) < 1e-5
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    dtab = {k: v.to(DEV) for k, v in tab.items()}
    row = lambda k: tab[k][t]
    cases = [(kind, _mask(kind, B, h // n, w // n)) for kind in ("checker", "one_measured", "one_hidden")] + [("none", None)]
    for kind, mk in cases:
        y = y0 if mk is None else torch.where(_sel(mk, y0), y0, torch.full_like(y0, float("nan")))
        want = RG.step(x, e, y, mk, n, weights, row("c_recip"), row("c_recipm1"), row("c1"), row("c2"), sg, row("lam"), row("sgm"),
                       z_dev.permute(0, 3, 1, 2))
        xs = nhwc(x).to(DEV)
        ops.p_sample_update_restore_gray_(xs, nhwc(e).to(DEV), y[:, 0].contiguous().to(DEV), None if mk is None else mk.to(DEV), n, weights,
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
    m.use_graph = False
    try:
        eager = _run(m, data, case, kw)
    finally:
        m.use_graph = True
    assert torch.equal(graphed, eager)
    m.native_sampler = False
    try:
        loop = _run(m, data, case, kw)
    finally:
        m.native_sampler = True
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
    y_nan = torch.where(_sel(mk, y), y, torch.full_like(y, float("nan")))
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
    mk = _mask("checker", B, 32 // n, 32 // n) if masked else None
    y = torch.where(_sel(mk, y0), y0, torch.full_like(y0, float("nan"))) if masked else y0
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
    tmap = (C.c_int64 * K)(*[int(v) for v in use])
    nbytes = max(lib.ddk_sampler_restore_gray_workspace_bytes(plan.handle, 2, 16, 16, K - 1, n) for n in (1, 2))
    assert nbytes == lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    assert nbytes >= max(lib.ddk_sampler_restore_noisy_workspace_bytes(plan.handle, 2, 16, 16, K - 1, n) for n in (1, 2))
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    img = syn.synthetic_normal(SHAPE, "colorize.ws.x").clamp(-1, 1)
    yg = {n: RG.apply_exact(img, n, "mean").float().contiguous().to(DEV) for n in (1, 2)}            # [2, 16/n, 16/n]
    yc = {n: ops.nchw_to_nhwc(torch.nn.functional.avg_pool2d(img, n).contiguous().to(DEV)) if n > 1 else ops.nchw_to_nhwc(img.to(DEV))
          for n in (1, 2)}
    md = {n: _mask("checker", 2, 16 // n, 16 // n).to(DEV) for n in (1, 2)}
    # what -> (weights code, n, with a mask); "nz1": the noisy chain, "anc": the ancestral one
    jobs = {"mean1": (1, 1, False), "luma1": (2, 1, False), "mean1m": (1, 1, True), "luma2": (2, 2, True), "mean2nm": (1, 2, False),
            "nz1": None, "anc": None}
    x = torch.empty_like(x0)
    side = torch.cuda.Stream()

    def run(ws, what, graph=1):
        x.copy_(x0)
        torch.cuda.synchronize()
        a = L.SamplerArgs(plan.handle, L.ptr(plan.packed), L.ptr(x), None, L.ptr(tables["c_recip"]), L.ptr(tables["c_recipm1"]),
                          L.ptr(tables["c1"]), L.ptr(tables["c2"]), L.ptr(tables["sigma"]), 2, 16, 16, K - 1, 0, SEED, 0, graph, L.ptr(ws),
                          nbytes)
        with torch.cuda.stream(side):
            if what == "anc":
                rc = lib.ddk_sampler_run_spaced(C.byref(a), tmap, side.cuda_stream)
            elif what == "nz1":
                rc = lib.ddk_sampler_run_restore_noisy(C.byref(a), tmap, L.ptr(ntab["lam"]), L.ptr(ntab["sgm"]), L.ptr(yc[1]), L.ptr(md[1]), 1,
                                                       side.cuda_stream)
            else:
                wcode, n, masked = jobs[what]
                rc = lib.ddk_sampler_run_restore_gray(C.byref(a), tmap, L.ptr(gtab["lam"]), L.ptr(gtab["sgm"]), L.ptr(yg[n]),
                                                      L.ptr(md[n]) if masked else None, n, wcode, side.cuda_stream)
        assert rc == 0, L.last_error()
        side.synchronize()
        return x.clone()

    fresh = lambda: torch.empty(nbytes // 4 + 4, device=DEV)

    def alone(what):
        ws = fresh()
        try:
            return run(ws, what)
        finally:      # the plan's cached graphs and shift table point into ws: drop them before the memory goes back
            assert lib.ddk_sampler_release_workspace(plan.handle, L.ptr(ws)) == 0

    single = {what: alone(what) for what in jobs}
    names = list(jobs)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert not torch.equal(single[p], single[q]), (p, q)
    for order in (("mean1", "luma1", "mean1", "nz1", "anc", "luma2", "mean2nm", "mean1m", "luma1"),
                  ("anc", "mean2nm", "nz1", "luma1", "mean1m", "luma2", "mean1", "anc", "nz1")):
        ws = fresh()
        for what in order:
            got = run(ws, what)
            assert torch.equal(got, single[what]), (order, what, float((got - single[what]).abs().max()))
        assert lib.ddk_sampler_release_workspace(plan.handle, L.ptr(ws)) == 0
    # bad weights, a bad n, a null table and injected noise are rejected
    ws = fresh()
    a = L.SamplerArgs(plan.handle, L.ptr(plan.packed), L.ptr(x), None, L.ptr(tables["c_recip"]), L.ptr(tables["c_recipm1"]),
                      L.ptr(tables["c1"]), L.ptr(tables["c2"]), L.ptr(tables["sigma"]), 2, 16, 16, K - 1, 0, SEED, 0, 0, L.ptr(ws), nbytes)
    call = lambda lam, sgm, y, mk, n, wc: lib.ddk_sampler_run_restore_gray(C.byref(a), tmap, lam, sgm, y, mk, n, wc, L.stream())
    lam, sgm = L.ptr(gtab["lam"]), L.ptr(gtab["sgm"])
    assert call(lam, sgm, L.ptr(yg[1]), None, 1, 0) == -1 and "weights" in L.last_error()
    assert call(lam, sgm, L.ptr(yg[1]), None, 1, 3) == -1 and "weights" in L.last_error()
    assert call(lam, sgm, L.ptr(yg[1]), None, 3, 1) == -1
    assert call(None, sgm, L.ptr(yg[1]), None, 1, 1) == -1 and "table" in L.last_error()
    noise = torch.zeros((K, *x.shape), device=DEV)
    a.noise = L.ptr(noise)
    assert call(lam, sgm, L.ptr(yg[1]), None, 1, 1) == -1 and "noise" in L.last_error()
    assert lib.ddk_sampler_release_workspace(plan.handle, L.ptr(ws)) == 0
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
    tmap = (C.c_int64 * K)(*[int(v) for v in use])
    nbytes = lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    ws = torch.empty(nbytes // 4 + 4, device=DEV)
    a = L.SamplerArgs(plan.handle, L.ptr(plan.packed), L.ptr(x), None, L.ptr(tables["c_recip"]), L.ptr(tables["c_recipm1"]),
                      L.ptr(tables["c1"]), L.ptr(tables["c2"]), L.ptr(tables["sigma"]), 2, 16, 16, K - 1, 0, SEED, 0, 0, L.ptr(ws), nbytes)
    y = torch.zeros(2, 16, 16, device=DEV)
    assert lib.ddk_sampler_run_restore_gray(C.byref(a), tmap, L.ptr(tables["lam"]), L.ptr(tables["sgm"]), L.ptr(y), None, 1, 1, L.stream()) == -1
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


def _cli_setup(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = ddpm_cfg(32, 3, 16, T=100)
    cfg.update(model="ddpm", dataset="celeba")
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    imgs = (np.random.default_rng(0).random((3, 16, 16, 3)) * 255).astype(np.uint8)
    np.save(tmp_path / "imgs.npy", imgs)
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "downsampled-diffusion_amd"))
    return root, env, imgs


def test_evaluate_cli_colorize_and_sr_settings(tmp_path):
    root, env, _ = _cli_setup(tmp_path)
    script = os.path.join(root, "downsampled-diffusion_amd", "evaluate_restoration.py")
    base = [sys.executable, script, "--synthetic", str(tmp_path / "cfg.json"), "--images", str(tmp_path / "imgs.npy"), "--timestep_respacing",
            "5", "--batch_size", "2", "--seed", "9", "--json", str(tmp_path / "out.json")]
    r = subprocess.run(base + ["--task", "colorize", "--weights", "luma"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads((tmp_path / "out.json").read_text())
    st, me = out["settings"], out["metrics"]
    assert (st["task"], st["method"], st["weights"], st["scale"], st["unet_forwards"], st["respacing"]) == ("colorize", "ddnm_gray", "luma", 1, 5, "5")
    assert set(me) == {"restored", "replicate", "consistency", "consistency_u8"} and me["consistency"]["max"] <= 127.5 * 2 * _bar(1, "luma")
    r = subprocess.run(base + ["--task", "sr", "--scale", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads((tmp_path / "out.json").read_text())
    assert set(out["settings"]) == {"checkpoint", "synthetic", "model", "task", "images", "n_images", "batch_size", "seed", "method",
                                    "unet_forwards", "respacing", "scale", "ddim", "eta"}
    assert (out["settings"]["method"], out["settings"]["scale"]) == ("ddnm", 2)
    assert set(out["metrics"]) == {"restored", "replicate", "bicubic", "consistency", "consistency_u8"}


def test_colorize_cli(tmp_path):
    root, env, imgs = _cli_setup(tmp_path)
    script = os.path.join(root, "downsampled-diffusion_amd", "colorize_model_samples.py")
    grey = imgs.mean(axis=3).round().astype(np.uint8)
    np.save(tmp_path / "grey.npy", grey)
    r = subprocess.run([sys.executable, script, "--synthetic", str(tmp_path / "cfg.json"), "--saved_model", "clitest", "--images",
                        str(tmp_path / "grey.npy"), "--timestep_respacing", "5", "--batch_size", "2", "--seed", "3", "--out_dir", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(tmp_path / "clitest_color1_mean_5.npy")
    back = np.load(tmp_path / "clitest_color1_mean_5_gray.npy")
    assert out.shape == (3, 16, 16, 3) and out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert back.shape == (3, 16, 16, 1) and np.array_equal(back[..., 0], grey)
