"""DDNM on the DPM-Solver++(2M) chain on the GPU (DDPM.restore_solver, DownsampleDDPM.restore_solver,
ddk_sampler_run_restore_multistep, p_update_restore_kernel<RestoreMultistep>, p_update_restore_point_kernel<RestoreMultistep> and
final_tail_kernel<.., StepKind::RestoreMultistep>) against tests/restore_solver_ref.py, the method restated around oracle/unet_ref.

The shapes of tests/test_restore_masked_gpu.py: the tiny DDPM (unet_chan 32, 3x16x16, B = 2) ends its steps in the unfused kernels, the
128-channel UNet on 8x32x32 latents at B = 16 in the fused tail for n = 1, 2 and not for n = 8.  Bars: the lone op bit for bit, x and
history (the order of the fp32 operations is pinned); chains at that file's TOL (1e-4 abs) against the restatement and at its 1e-5
between the Python loop and the native sampler; order 1 against the merged DDIM eta 0 chain bit for bit (their fp32 tables are
bitwise equal); measured pixels exact at n = 1, measured block means within 8 n^2 2^-24 at n >= 2; fused and unfused tails, graph
and eager, a mask that measures nothing and the plain 2M chain: the same bits."""
import json

import numpy as np
import pytest
import torch

import chain_cases as CC
import restore_ref as RR
import restore_solver_ref as RS
from helpers import dddpm_cfg, ddpm_cfg, det_load, to_nchw, to_nhwc
from oracle import diffusion_ref as D
from test_restore_masked_gpu import TOL, _bar, _means_err
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SPEC = "logsnr8"
CASES = [(1, True), (2, True), (2, False)]
CASE_IDS = ["n1-mask", "n2-mask", "n2-nomask"]


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    """y and mask per block, one start state: computed once, never changed"""
    x_T = syn.synthetic_normal(SHAPE, "restore_solver.xT")
    ys = {n: CC.pooled_y(SHAPE, n, f"restore_solver.x{n}") for n in (1, 2)}
    mks = {n: CC.mask("checker", 2, 16 // n, 16 // n) for n in (1, 2)}
    return ys, mks, x_T


@pytest.fixture(scope="module")
def native(tiny, data):
    """the native chain's results on the tiny model, shared by the tests that compare against them"""
    m, _ = tiny
    ys, mks, x_T = data
    return {(n, masked): m.restore_solver(ys[n].to(DEV), mks[n] if masked else None, n, respacing=SPEC, x_T=x_T).cpu()
            for n, masked in CASES}


# ---------------------------------------------------------------- the lone op, bit for bit
@pytest.mark.parametrize("hw", [(16, 16), (8, 32)], ids=["16x16", "8x32"])
@pytest.mark.parametrize("c", [3, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_lone_op_equals_restatement_bit_for_bit(n, c, hw):
    """ops.p_sample_update_restore_multistep_ given eps_hat and a history against restore_solver_ref.step, x and history: row 0
    (c1 = 1, c2 = 0, c3 = 0), a row with c3 = 0 and a row with c3 != 0, one per image; the three masks with NaN wherever y is not
    measured, and (n >= 2) no mask."""
    from ddk import ops
    h, w = hw
    g = torch.Generator().manual_seed(19 * n + c + h)
    B = 3
    shape = (B, c, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    hist = torch.rand(shape, generator=g) * 2 - 1
    y0 = torch.rand(B, c, h // n, w // n, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])
    tab = {k: torch.rand(8, generator=g) * s for k, s in (("c_recip", 3.0), ("c_recipm1", 2.0), ("c1", 1.0), ("c2", 1.0), ("c3", -0.5))}
    tab["c1"][0], tab["c2"][0], tab["c3"][0], tab["c3"][3] = 1.0, 0.0, 0.0, 0.0
    assert float(tab["c3"][7]) != 0.0
    dtab = {k: v.to(DEV) for k, v in tab.items()}
    rows = [tab[k][t] for k in ("c_recip", "c_recipm1", "c1", "c2", "c3")]
    masks = [CC.mask(kind, B, h // n, w // n) for kind in ("checker", "one_measured", "one_hidden")] + ([None] if n > 1 else [])
    for mk in masks:
        y = y0 if mk is None else torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
        want_x, want_h = RS.step(x, e, hist, y, mk, n, *rows)
        xs, hs = to_nhwc(x).to(DEV), to_nhwc(hist).to(DEV)
        ops.p_sample_update_restore_multistep_(xs, to_nhwc(e).to(DEV), hs, to_nhwc(y).to(DEV), None if mk is None else mk.to(DEV), n, t.to(DEV),
                                               **dtab)
        got_x, got_h = to_nchw(xs.cpu()), to_nchw(hs.cpu())
        assert torch.isfinite(got_x).all() and torch.isfinite(got_h).all()
        assert torch.equal(got_x, want_x), float((got_x - want_x).abs().max())
        assert torch.equal(got_h, want_h), float((got_h - want_h).abs().max())
        # row 0 returns x0' itself: measured pixels are y (n = 1: exactly), measured block means are y
        assert torch.equal(got_x[0], got_h[0])
        m0 = torch.ones(1, h // n, w // n) if mk is None else mk[0:1]
        if n == 1:
            assert torch.equal(got_x[0:1][CC.sel(m0, y[0:1])], y[0:1][CC.sel(m0, y[0:1])])
        else:
            assert _means_err(got_x[0:1], y[0:1], m0, n) <= _bar(n)
    if n > 1:   # an all-ones mask is no mask
        a, ha = to_nhwc(x).to(DEV), to_nhwc(hist).to(DEV)
        ops.p_sample_update_restore_multistep_(a, to_nhwc(e).to(DEV), ha, to_nhwc(y0).to(DEV), torch.ones(B, h // n, w // n, device=DEV), n,
                                               t.to(DEV), **dtab)
        assert torch.equal(a, xs) and torch.equal(ha, hs)


def test_lone_op_rejects_bad_arguments_and_touches_nothing():
    from ddk import lib as L
    lib = L.load()
    tab = [torch.ones(4, device=DEV) for _ in range(5)]
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    buf = torch.full((8 * 8 * 4 + 8,), 3.0, device=DEV)      # x, 16 bytes in
    hist = torch.full((8 * 8 * 4 + 8,), 5.0, device=DEV)
    eps, y, mk = torch.zeros(8 * 8 * 4 + 4, device=DEV), torch.zeros(8 * 8 * 4 + 4, device=DEV), torch.ones(1, 8, 8, device=DEV)
    xp, hp = buf.data_ptr() + 16, hist.data_ptr() + 16

    def call(x=xp, e=eps.data_ptr(), h=hp, yp=y.data_ptr(), m=mk.data_ptr(), n=1, H=8, W=8, ch=4, B=1, c3=tab[4].data_ptr()):
        return lib.ddk_p_sample_update_restore_multistep(x, e, h, yp, m, n, t.data_ptr(), *(v.data_ptr() for v in tab[:4]), c3, B, H, W, ch,
                                                         L.stream())

    bad = dict(n3=dict(n=3), no_mask_n1=dict(m=None), h_not_divisible=dict(n=4, H=6), x_misaligned=dict(x=xp + 4), eps_misaligned=dict(e=eps.data_ptr() + 4),
               hist_misaligned=dict(h=hp + 4), y_misaligned_n1=dict(yp=y.data_ptr() + 4), null_hist=dict(h=None), null_y=dict(yp=None),
               null_c3=dict(c3=None), zero_batch=dict(B=0), zero_channels=dict(ch=0), per_not_multiple_of_4=dict(ch=3, H=1, W=1))
    for name, kw in bad.items():
        assert call(**kw) == -1, name                                                   # DDK_ERR_ARG
        assert L.last_error(), name
    torch.cuda.synchronize()
    assert bool((buf == 3.0).all()) and bool((hist == 5.0).all())
    assert "mask" in (call(m=None), L.last_error())[1] and "align" in (call(h=hp + 4), L.last_error())[1]
    assert call() == 0, L.last_error()
    assert call(m=None, n=2, yp=y.data_ptr() + 4) == 0, L.last_error()                    # n >= 2: no mask needed, y only 4-byte aligned
    torch.cuda.synchronize()
    assert not bool((buf[4:-4] == 3.0).any()) and bool((buf[:4] == 3.0).all()) and bool((buf[-4:] == 3.0).all())
    assert bool((hist[:4] == 5.0).all()) and bool((hist[-4:] == 5.0).all())


# ---------------------------------------------------------------- the tiny DDPM, logsnr8
@pytest.mark.parametrize("n,masked", CASES, ids=CASE_IDS)
def test_tiny_vs_restatement(tiny, data, native, n, masked):
    _, eps = tiny
    ys, mks, x_T = data
    got = native[n, masked]
    want = RS.RestoreSolver(BETAS, SPEC).run(eps, x_T, ys[n], mks[n] if masked else None, n)
    err = float((got - want).abs().max())
    print(f"DDNM on 2M n={n} mask={masked} tiny DDPM, {SPEC}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    mk = mks[n] if masked else torch.ones(2, 16 // n, 16 // n)
    if n == 1:
        assert torch.equal(got[CC.sel(mk, ys[n])], ys[n][CC.sel(mk, ys[n])]) and float((got - ys[n])[~CC.sel(mk, ys[n])].abs().max()) > 1e-2
    else:
        assert _means_err(got, ys[n], mk, n) <= _bar(n)


@pytest.mark.parametrize("n,masked", CASES, ids=CASE_IDS)
def test_graph_equals_eager_and_python_loop_is_close(tiny, data, native, n, masked):
    m, _ = tiny
    ys, mks, x_T = data
    graphed = native[n, masked]
    run = lambda: m.restore_solver(ys[n].to(DEV), mks[n] if masked else None, n, respacing=SPEC, x_T=x_T).cpu()
    with CC.toggled(m, "use_graph", False):
        eager = run()
    assert torch.equal(graphed, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = run()
    err = float((loop - graphed).abs().max())
    print(f"Python loop vs native, DDNM on 2M n={n} mask={masked} {SPEC}: {err:.3g}")
    assert err < 1e-5


@pytest.mark.parametrize("n,masked", CASES, ids=CASE_IDS)
def test_order_1_equals_the_merged_ddim_eta_0_chain(tiny, data, n, masked):
    """order 1 has c3 = 0 in every row and DDIM eta 0 has sigma = 0: with bitwise equal c_recip .. c2 (checked here; else the tables'
    own 1e-6 of tests/test_dpm_solver_cpu.py test_order1_tables_equal_ddim_eta0) the new kernels and RestoreMasked's / Restore's
    compute the same bits"""
    m, _ = tiny
    ys, mks, x_T = data
    one, use1 = m._solver_tables(SPEC, "dpm++2m", 1)
    ddim, use2 = m._spaced_tables(SPEC, True, 0.0)
    assert list(use1) == list(use2)
    same = all(torch.equal(one[k], ddim[k]) for k in ("c_recip", "c_recipm1", "c1", "c2"))
    mk = mks[n] if masked else None
    got = m.restore_solver(ys[n].to(DEV), mk, n, respacing=SPEC, order=1, x_T=x_T).cpu()
    want = m.restore(ys[n].to(DEV), mk, n, respacing=SPEC, ddim=True, eta=0.0, x_T=x_T, seed=1).cpu()
    err = float((got - want).abs().max())
    print(f"order 1 vs DDIM eta 0, n={n} mask={masked}: tables bitwise equal {same}, max abs difference {err:.3g}")
    if same:
        assert torch.equal(got, want), err
    else:
        assert err <= 1e-6, err


@pytest.mark.parametrize("n", [1, 2])
def test_a_mask_that_measures_nothing_is_the_plain_solver_chain(tiny, data, n):
    from ddk import ops
    m, _ = tiny
    _, _, x_T = data
    tables, use = m._solver_tables(SPEC, "dpm++2m")
    plan = m._eps_model_nhwc().plan()
    want = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    plan.sample_multistep_nhwc(want, tables, len(use) - 1, timesteps=use)
    got = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    y = torch.full((2, 16 // n, 16 // n, 3), float("nan"), device=DEV)
    plan.sample_restore_multistep_nhwc(got, y, torch.zeros(2, 16 // n, 16 // n, device=DEV), n, tables, len(use) - 1, timesteps=use)
    assert torch.isfinite(got).all() and torch.equal(got, want)


# ---------------------------------------------------------------- the fused tail: 128 channels, 8x32x32 latents, B = 16
@pytest.fixture(scope="module")
def wide():
    from models import DDPM, Unet
    cfg = ddpm_cfg(128, 8, 32)
    return det_load(DDPM(cfg, Unet(cfg), DEV, 8)).to(DEV).eval()


@pytest.mark.parametrize("n", [1, 2, 8])
def test_fused_tail_equals_unfused_bit_for_bit(wide, n):
    """logsnr6: n = 1 and n = 2 end in final_tail_kernel<.., RestoreMultistep>, n = 8 (W n = 256 > 128) in p_update_restore_kernel<RestoreMultistep>
    whatever the option says; with DDK_OPT_RESTORE_FUSED_TAIL = 0 all end in the unfused kernels, with the same bits"""
    from ddk import ops
    m = wide
    plan = m._eps_model_nhwc().plan()
    before = ops.cluster_timeouts()
    B = 16
    shape = (B, 8, 32, 32)
    assert plan.restore_multistep_tail_parts(B, 32, 32, n) == (0 if n == 8 else 8)
    y0 = CC.pooled_y(shape, n, f"restore_solver.wide.{n}")
    mk = CC.mask("checker", B, 32 // n, 32 // n)
    y = torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
    x_T = syn.synthetic_normal(shape, "restore_solver.wide.xT")
    run = lambda: m.restore_solver(y.to(DEV), mk, n, respacing="logsnr6", x_T=x_T).cpu()
    fused = run()
    plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 0)
    try:
        assert plan.restore_multistep_tail_parts(B, 32, 32, n) == 0
        unfused = run()
    finally:
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())
    if n == 1:
        assert torch.equal(fused[CC.sel(mk, y)], y[CC.sel(mk, y)])
    else:
        assert _means_err(fused, y, mk, n) <= _bar(n)
    if n == 2:      # without a mask: the fused tail's null-mask path against the unfused kernel's
        full = m.restore_solver(y0.to(DEV), None, n, respacing="logsnr6", x_T=x_T).cpu()
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 0)
        try:
            assert torch.equal(full, m.restore_solver(y0.to(DEV), None, n, respacing="logsnr6", x_T=x_T).cpu())
        finally:
            plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
        assert _means_err(full, y0, torch.ones(B, 16, 16), n) <= _bar(n) and not torch.equal(full, fused)
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- one workspace, four kinds of chain, two masks
def test_chains_share_a_workspace_and_masks_share_a_graph(tiny, data):
    """restore-solver chains (two masks at n = 1, a mask and none at n = 2), a plain 2M chain on the same tables, a masked DDIM
    restore chain and an ancestral chain on one workspace, state buffer and t_start, in two orders: each equals its own single run
    on a fresh workspace bit for bit (the kind, c3, n and the mask's presence are in the graph key; y, the mask and the zeroed
    history are staged by every call, outside the graph, so the two masks replay one graph)"""
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    ys, mks, x_T = data
    sol, use = m._solver_tables(SPEC, "dpm++2m")
    ddim, use_d = m._spaced_tables(SPEC, True, 0.0)
    anc, use_a = m._spaced_tables(SPEC, False, 0.0)
    assert list(use) == list(use_d) == list(use_a)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    before = ops.cluster_timeouts()
    K = len(use)
    nbytes = lib.ddk_sampler_restore_multistep_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    lat = 2 * 16 * 16 * 3 * 4
    assert nbytes == lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + 2 * lat + 2 * 16 * 16 * 4
    assert nbytes >= lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    assert nbytes >= lib.ddk_sampler_multistep_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    yd = {n: ops.nchw_to_nhwc(ys[n].to(DEV)) for n in (1, 2)}
    md = {"s1": mks[1].to(DEV), "s1b": (1 - mks[1]).to(DEV), "s2": mks[2].to(DEV), "s2full": None}
    jobs = {"s1": 1, "s1b": 1, "s2": 2, "s2full": 2, "2m": None, "ddim_m1": None, "anc": None}

    def launch(what, a, tmap, s):
        if what == "anc":
            return lib.ddk_sampler_run_spaced(a, tmap, s)
        if what == "ddim_m1":
            return lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[1]), L.ptr(md["s1"]), 1, s)
        if what == "2m":
            return lib.ddk_sampler_run_multistep(a, tmap, L.ptr(sol["c3"]), s)
        n = jobs[what]
        return lib.ddk_sampler_run_restore_multistep(a, tmap, L.ptr(sol["c3"]), L.ptr(yd[n]), L.ptr(md[what]), n, s)

    sh = CC.SharedWorkspace(plan, lambda what: {"anc": anc, "ddim_m1": ddim}.get(what, sol), use, x0, nbytes, 7, launch)
    x, tmap = sh.x, sh.tmap
    single = {what: sh.alone(what) for what in jobs}
    names = list(jobs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not torch.equal(single[a], single[b]), (a, b)
    for order in (("s1", "2m", "ddim_m1", "anc", "s1b", "s2", "s2full", "s1"), ("anc", "s2full", "s2", "ddim_m1", "s1b", "2m", "s1", "anc")):
        sh.interleaved(order, single)
    for what in ("s1", "s1b"):      # the measured pixels of the two masks' results are their own
        out = ops.nhwc_to_nchw(single[what]).cpu()
        s = CC.sel(md[what].cpu(), ys[1])
        assert torch.equal(out[s], ys[1][s])
    # eager on the legacy stream: the same bits; n = 1 without a mask, a bad n and injected noise are rejected
    with CC.workspace(plan, nbytes) as ws:
        a = CC.sampler_args(plan, x, sol, K - 1, ws, nbytes, seed=7)
        x.copy_(x0)
        assert lib.ddk_sampler_run_restore_multistep(a, tmap, L.ptr(sol["c3"]), L.ptr(yd[2]), None, 2, L.stream()) == 0, L.last_error()
        torch.cuda.synchronize()
        assert torch.equal(x, single["s2full"])
        assert lib.ddk_sampler_run_restore_multistep(a, tmap, L.ptr(sol["c3"]), L.ptr(yd[1]), None, 1, L.stream()) == -1 and "mask" in L.last_error()
        assert lib.ddk_sampler_run_restore_multistep(a, tmap, L.ptr(sol["c3"]), L.ptr(yd[1]), L.ptr(md["s1"]), 3, L.stream()) == -1
        assert lib.ddk_sampler_run_restore_multistep(a, tmap, None, L.ptr(yd[1]), L.ptr(md["s1"]), 1, L.stream()) == -1
        noise = torch.zeros((K, *x.shape), device=DEV)
        a.noise = L.ptr(noise)
        assert lib.ddk_sampler_run_restore_multistep(a, tmap, L.ptr(sol["c3"]), L.ptr(yd[1]), L.ptr(md["s1"]), 1, L.stream()) == -1 and \
            "noise" in L.last_error()
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- dDDPM
def test_dddpm_restore_solver_holds_the_latent_constraint_and_pastes():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    z_T = syn.synthetic_normal((2, 8, 8, 8), "restore_solver.dd.zT")
    img = syn.synthetic_normal((2, 3, 32, 32), "restore_solver.dd.x").clamp(-1, 1)
    mk = torch.zeros(32, 32)
    mk[:, :14] = 1
    mk[8:12, 24:28] = 1
    x_out, z = m.restore_solver(img.to(DEV), mk, 1, respacing=SPEC, x_T=z_T)
    assert x_out.shape == (2, 3, 32, 32) and z.shape == (2, 8, 8, 8) and torch.isfinite(x_out).all()
    sel = (mk != 0).expand(2, 3, 32, 32)
    assert torch.equal(x_out.cpu()[sel], img[sel])                                    # paste
    with torch.no_grad():
        z_ref = m.rescaled_downsample(torch.where(sel, img, torch.zeros_like(img)).to(DEV)).cpu()
    m_lat = -torch.nn.functional.max_pool2d(-mk[None, None], 4)[0, 0]
    s_lat = (m_lat != 0).expand(2, 8, 8, 8)
    assert torch.equal(z.cpu()[s_lat], z_ref[s_lat])                                  # the constraint, held in the latent
    raw, _ = m.restore_solver(img.to(DEV), mk, 1, respacing=SPEC, x_T=z_T, paste=False)
    assert torch.equal(raw.cpu()[~sel], x_out.cpu()[~sel])
    print(f"dDDPM inpainting on 2M: pixel-space gap on the measured pixels before the paste {float((raw.cpu() - img)[sel].abs().max()):.3g}")
    # scale 8: a 4 x 4 low-resolution image with holes, latent block 2
    y = CC.pooled_y((2, 3, 32, 32), 8, "restore_solver.dd.y")
    mk8 = CC.mask("checker", 2, 4, 4)
    x8, z8 = m.restore_solver(y.to(DEV), mk8, 8, respacing=SPEC, x_T=z_T)
    with torch.no_grad():
        zr = m.rescaled_downsample(RR.replicate(torch.where(CC.sel(mk8, y), y, torch.zeros_like(y)), 8).to(DEV))
        y_lat = torch.nn.functional.avg_pool2d(zr, 2).cpu()
        assert torch.equal(x8, m.rescaled_upsample(z8))
    err = _means_err(z8.cpu(), y_lat, mk8, 2)
    gap = float((RR.pool(x8.cpu().double(), 8) - y.double())[CC.sel(mk8, y)].abs().max())
    print(f"dDDPM x8 with holes on 2M (latent n = 2): measured latent block means off by {err:.3g} (bar {_bar(2):.3g}); pixel-space gap {gap:.3g}")
    assert err <= _bar(2), err


# ---------------------------------------------------------------- the command line (a fresh child process each) and the scorer
def test_inpaint_cli_with_the_solver(tmp_path):
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    base = ["inpaint_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--mask", "left",
            "--timestep_respacing", "logsnr8", "--batch_size", "2", "--seed", "3", "--out_dir", tmp_path]
    CC.run_script(*base, "--method", "ddnm", "--dpm_solver", env=env)
    out = np.load(tmp_path / "clitest_inpaint_left_logsnr8_ddnm_dpmpp2m.npy")
    assert (tmp_path / "clitest_inpaint_left_logsnr8_ddnm_dpmpp2m_masked.npy").exists()
    assert out.shape == (3, 16, 16, 3) and out.dtype == np.float32 and np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert np.abs(out[:, :, 8:] - imgs[:, :, 8:]).max() < 1e-3             # the known half comes back
    assert np.abs(out[:, :, :8] - imgs[:, :, :8]).max() > 1
    for extra in (["--method", "ddnm", "--dpm_solver", "--use_ddim"], ["--method", "ddnm", "--dpm_solver", "--eta", "0.5"], ["--dpm_solver"]):
        r = CC.run_script(*base, *extra, env=env, check=False)      # argparse errors: no device work
        assert r.returncode != 0 and "dpm_solver" in r.stderr


def test_upscale_and_evaluate_clis_with_the_solver(tmp_path):
    cfg_path, images_path, _, env = CC.cli_files(tmp_path, CC.cli_cfg(), 3, 16)
    base = ["upscale_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--scale", "2",
            "--timestep_respacing", "logsnr8", "--batch_size", "2", "--seed", "3", "--out_dir", tmp_path, "--dpm_solver"]
    CC.run_script(*base, env=env)
    out = np.load(tmp_path / "clitest_sr2_logsnr8_dpmpp2m.npy")
    assert (tmp_path / "clitest_sr2_logsnr8_dpmpp2m_lowres.npy").exists()
    assert out.shape == (3, 16, 16, 3) and np.isfinite(out).all()
    r = CC.run_script(*base, "--use_ddim", env=env, check=False)
    assert r.returncode != 0 and "dpm_solver" in r.stderr
    np.save(tmp_path / "ones.npy", np.ones((16, 16), dtype=np.float32))
    CC.run_script("evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "inpaint", "--method", "ddnm",
                  "--dpm_solver", "--mask", tmp_path / "ones.npy", "--timestep_respacing", "logsnr8", "--batch_size", "2", "--seed", "9",
                  "--json", tmp_path / "out.json", env=env)
    res = json.loads((tmp_path / "out.json").read_text())
    st, me = res["settings"], res["metrics"]
    assert (st["task"], st["method"], st["unet_forwards"], st["respacing"], st["dpm_solver"]) == ("inpaint", "ddnm_dpmpp2m", 8, "logsnr8", True)
    assert "ddim" not in st and "jump_length" not in st
    assert me["restored"]["psnr"]["mean"] == float("inf") and me["restored"]["ssim"]["mean"] == 1.0      # everything known


def test_scorer_takes_the_solver(tiny):
    from utils import restoration_metrics as RMx
    m, _ = tiny
    imgs = (np.random.default_rng(1).random((3, 16, 16, 3)) * 255).astype(np.uint8)
    dn = RMx.evaluate_restoration(m, imgs, "inpaint", batch_size=3, seed=5, mask="center", method="ddnm", respacing=SPEC, dpm_solver=True)
    assert (dn["method"], dn["unet_forwards"]) == ("ddnm_dpmpp2m", 8)
    known = RMx.make_mask("center", 3, 16, 16)[:, 0].numpy() != 0
    assert np.array_equal(dn["images"]["restored"][known], imgs[known])
    for kw in (dict(sr_mask="half"), dict()):
        sr = RMx.evaluate_restoration(m, imgs, "sr", batch_size=3, seed=5, scale=2, respacing=SPEC, dpm_solver=True, **kw)
        assert sr["method"] == "ddnm_dpmpp2m" and sr["unet_forwards"] == 8
        assert float(sr["consistency"].max()) <= 8 * 4 * 2.0 ** -24 * 127.5
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(m, imgs, "inpaint", mask="center", respacing=SPEC, dpm_solver=True)                  # RePaint
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(m, imgs, "sr", scale=2, respacing=SPEC, dpm_solver=True, ddim=True)
