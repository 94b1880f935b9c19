"""DDNM+ for a noisy measurement on the GPU (DDPM.restore_noisy, DownsampleDDPM.restore_noisy, ddk_sampler_run_restore_noisy,
p_update_restore_kernel<RestoreNoisy>, p_update_restore_point_kernel<RestoreNoisy> and final_tail_kernel<.., StepKind::RestoreNoisy>) against
tests/restore_noisy_ref.py, the method restated around oracle/unet_ref with oracle/philox_ref draws in NHWC order.

Shapes and bars are those of tests/test_restore_masked_gpu.py for the corresponding cases: the lone op bit for bit on [3, c, 16, 16] and
[3, c, 8, 32] with c = 3 (the 3-channel path of rstm_mask4), 4, 8; the tiny DDPM (unet_chan 32, 3x16x16, unfused tail) against the
restatement's chain to 1e-4 and between the Python loop and the native sampler to 1e-5; a 128-channel UNet on 8x32x32 latents at
B = 16 for the fused tail (n = 1, 2 fused, n = 8 not eligible); fused and unfused tails, and chains that share a workspace: the same
bits."""
import numpy as np
import pytest
import torch

import chain_cases as CC
import restore_noisy_ref as RN
from helpers import dddpm_cfg, ddpm_cfg, det_load, to_nhwc
from oracle import diffusion_ref as D
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4                  # chains against the restatement (tests/test_restore_masked_gpu.py)
LOOP_TOL = 1e-5             # the Python loop against the native sampler (the same file)
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SEED = 613
SIGMA_Y = 0.2
KINDS = [dict(), dict(ddim=True, eta=0.5)]
IDS = ["ancestral", "ddim_eta0.5"]


@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


@pytest.fixture(scope="module")
def data():
    """a noisy y and a mask per block, one start state: computed once, never changed"""
    x_T = syn.synthetic_normal(SHAPE, "restore_noisy.xT")
    mks = {n: CC.mask("checker", 2, 16 // n, 16 // n) for n in (1, 2)}
    ys = {}
    for n in (1, 2):
        y0 = CC.pooled_y(SHAPE, n, f"restore_noisy.x{n}") + SIGMA_Y * syn.synthetic_normal((2, 3, 16 // n, 16 // n), f"restore_noisy.n{n}")
        ys[n] = y0
    return ys, mks, x_T


@pytest.fixture(scope="module")
def native(tiny, data):
    """the native chain's results on the tiny model, 8 steps of the "8"-spaced schedule, shared by the tests that compare against them"""
    m, _ = tiny
    ys, mks, x_T = data
    return {(n, i): m.restore_noisy(ys[n].to(DEV), mks[n], n, sigma_y=SIGMA_Y, respacing="8", x_T=x_T, seed=SEED, **kw).cpu()
            for n in (1, 2) for i, kw in zip(IDS, KINDS)}


# ---------------------------------------------------------------- the lone op, bit for bit
@pytest.mark.parametrize("hw", [(16, 16), (8, 32)], ids=["16x16", "8x32"])
@pytest.mark.parametrize("c", [3, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_lone_op_equals_restatement_bit_for_bit(n, c, hw):
    """ops.p_sample_update_restore_noisy_ given eps_hat against restore_noisy_ref.step on the same inputs, for the three masks and, at
    n >= 2, without one.  The draws are the device's own (ddk_randn: the same Philox call and keying), first checked against
    oracle/philox_ref; rows 7 and 3 have lam in (0, 1) and lam = 1, row 0 has no draw.  y is NaN wherever the mask is 0: the result
    must not see it."""
    from ddk import ops
    h, w = hw
    g = torch.Generator().manual_seed(23 * n + c + h)
    B = 3
    shape = (B, c, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    y0 = torch.rand(B, c, h // n, w // n, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3])
    tab = CC.hand_tables(g, noisy=True)
    seed, stream = 24680, 5
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    dtab = {k: v.to(DEV) for k, v in tab.items()}
    row = lambda k: tab[k][t]
    cases = [(kind, CC.mask(kind, B, h // n, w // n)) for kind in ("checker", "one_measured", "one_hidden")] + ([("none", None)] if n > 1 else [])
    for kind, mk in cases:
        y = y0 if mk is None else torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
        want = RN.step(x, e, y, mk, n, row("c_recip"), row("c_recipm1"), row("c1"), row("c2"), sg, row("lam"), row("sgm"), z)
        xs = to_nhwc(x).to(DEV)
        ops.p_sample_update_restore_noisy_(xs, to_nhwc(e).to(DEV), to_nhwc(y).to(DEV), None if mk is None else mk.to(DEV), n, t.to(DEV), **dtab,
                                           seed=seed, stream_id=stream)
        got = xs.cpu().permute(0, 3, 1, 2)
        assert torch.isfinite(got).all(), kind
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))
        # row 0 (lam = 0, no draw, c1 = 1, c2 = 0) returns the model's own clipped x0: the measurement is never pasted
        x0 = (tab["c_recip"][0] * x[0] - tab["c_recipm1"][0] * e[0]).clamp(-1, 1)
        assert torch.equal(got[0], x0)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_lam_one_and_sgm_sigma_is_the_masked_op_bit_for_bit(n):
    """the tie to the merged kernel at n >= 2: 1 * d is exact, so the op equals ddk_p_sample_update_restore_masked, with a mask and without"""
    from ddk import ops
    g = torch.Generator().manual_seed(n)
    B, c, h, w = 3, 4, 16, 16
    x, e = 2 * torch.randn(B, h, w, c, generator=g), torch.randn(B, h, w, c, generator=g)
    y = torch.rand(B, h // n, w // n, c, generator=g) * 2 - 1
    t = torch.tensor([0, 7, 3]).to(DEV)
    tab = {k: (torch.rand(8, generator=g) * s).to(DEV) for k, s in (("c_recip", 3.0), ("c_recipm1", 2.0), ("c1", 1.0), ("c2", 1.0), ("sigma", 0.5))}
    sgm = tab["sigma"].clone()
    sgm[0] = 0.0                      # the kernels apply sigma as (row > 0 ? sigma : 0)
    for mk in (CC.mask("checker", B, h // n, w // n).to(DEV), None):
        a, b = x.to(DEV), x.to(DEV)
        ops.p_sample_update_restore_noisy_(a, e.to(DEV), y.to(DEV), mk, n, t, **tab, lam=torch.ones(8, device=DEV), sgm=sgm, seed=9, stream_id=2)
        ops.p_sample_update_restore_masked_(b, e.to(DEV), y.to(DEV), mk, n, t, **tab, seed=9, stream_id=2)
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("c", [3, 4])
def test_point_op_with_lam_one_returns_y_within_one_rounding(c):
    """n = 1 with a row of lam = 1, c1 = 1, c2 = 0 and no draw: the measured outputs are x0 + (y - x0), within 2^-23 of y for
    |x0|, |y| <= 1, and the others are the clipped x0"""
    from ddk import ops
    g = torch.Generator().manual_seed(c)
    B, h, w = 2, 16, 16
    x, e = 2 * torch.randn(B, h, w, c, generator=g), torch.randn(B, h, w, c, generator=g)
    y = torch.rand(B, h, w, c, generator=g) * 2 - 1
    mk = CC.mask("checker", B, h, w)
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    tab = dict(c_recip=torch.full((1,), 1.7, device=DEV), c_recipm1=torch.full((1,), 0.9, device=DEV), c1=one, c2=zero, sigma=one, lam=one, sgm=zero)
    out = x.to(DEV)
    ops.p_sample_update_restore_noisy_(out, e.to(DEV), y.to(DEV), mk.to(DEV), 1, torch.zeros(B, dtype=torch.long, device=DEV), **tab)
    out = out.cpu()
    sel = (mk != 0).unsqueeze(-1).expand_as(y)
    err = float((out[sel].double() - y[sel].double()).abs().max())
    print(f"n = 1, lam = 1: measured outputs off y by {err:.3g} (bar 2^-23 = {2.0 ** -23:.3g})")
    assert err <= 2.0 ** -23
    x0 = (torch.tensor(1.7) * x - torch.tensor(0.9) * e).clamp(-1, 1)
    assert torch.equal(out[~sel], x0[~sel])


def test_lone_op_rejects_bad_arguments():
    from ddk import lib as L
    from ddk import ops
    x = torch.zeros(1, 8, 8, 3, device=DEV)
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma", "lam", "sgm")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    with pytest.raises(L.DDKError):                                                        # n = 3
        ops.p_sample_update_restore_noisy_(x, x.clone(), torch.zeros(1, 2, 2, 3, device=DEV), torch.ones(1, 2, 2, device=DEV), 3, t, **tab)
    with pytest.raises(L.DDKError):                                                        # n = 1 without a mask
        ops.p_sample_update_restore_noisy_(x, x.clone(), x.clone(), None, 1, t, **tab)
    with pytest.raises(L.DDKError):                                                        # a null table
        ops.p_sample_update_restore_noisy_(x, x.clone(), x.clone(), torch.ones(1, 8, 8, device=DEV), 1, t, **dict(tab, lam=None))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the tiny DDPM, 8 steps of "8"
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, native, kw, n):
    _, eps = tiny
    ys, mks, x_T = data
    got = native[n, IDS[KINDS.index(kw)]]
    want = RN.RestoreNoisy(BETAS, "8").run(eps, x_T, ys[n], mks[n], n, SIGMA_Y, SEED, **kw)
    err = float((got - want).abs().max())
    print(f"DDNM+ n={n} tiny DDPM, 8 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_and_python_loop_is_close(tiny, data, native, kw, n):
    m, _ = tiny
    ys, mks, x_T = data
    graphed = native[n, IDS[KINDS.index(kw)]]
    run = lambda: m.restore_noisy(ys[n].to(DEV), mks[n], n, sigma_y=SIGMA_Y, respacing="8", x_T=x_T, seed=SEED, **kw).cpu()
    with CC.toggled(m, "use_graph", False):
        eager = run()
    assert torch.equal(graphed, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = run()
    err = float((loop - graphed).abs().max())
    print(f"Python loop vs native, DDNM+ n={n} 8 steps {kw}: {err:.3g}")
    assert err < LOOP_TOL


def test_unmeasured_y_reaches_nothing_and_the_measurement_is_not_pasted(tiny, data, native):
    m, _ = tiny
    ys, mks, x_T = data
    out = native[1, "ancestral"]
    s1 = CC.sel(mks[1], ys[1])
    y_nan = torch.where(s1, ys[1], torch.full_like(ys[1], float("nan")))
    from ddk import ops
    tables, use = m._noisy_tables("8", False, 0.0, SIGMA_Y)
    plan = m._eps_model_nhwc().plan()
    x = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    plan.sample_restore_noisy_nhwc(x, ops.nchw_to_nhwc(y_nan.to(DEV)), mks[1].to(DEV), 1, tables, len(use) - 1, seed=SEED,
                                   stream_id=int(m.rng_stream_id), timesteps=use)
    assert torch.equal(ops.nhwc_to_nchw(x).cpu(), out)
    assert not torch.equal(out[s1], ys[1][s1]) and float(out.abs().max()) <= 1.0          # row 0 returns the clipped x0


@pytest.mark.parametrize("n,kw", [(1, dict()), (2, dict(ddim=True, eta=0.0)), (4, dict(respacing="8", ddim=True, eta=0.5))])
def test_sigma_y_zero_is_restore_bit_for_bit(tiny, n, kw):
    m, _ = tiny
    kw = dict(dict(respacing="8"), **kw)
    y = CC.pooled_y(SHAPE, n, f"restore_noisy.zero{n}")
    mk = CC.mask("checker", 2, 16 // n, 16 // n)
    x_T = syn.synthetic_normal(SHAPE, "restore_noisy.zero.xT")
    want = m.restore(y.to(DEV), mk, n, x_T=x_T, seed=SEED, **kw)
    assert torch.equal(m.restore_noisy(y.to(DEV), mk, n, sigma_y=0, x_T=x_T, seed=SEED, **kw), want)
    assert torch.equal(m.restore_noisy(y.to(DEV), mk, n, sigma_y=0.0, x_T=x_T, seed=SEED, **kw), want)


# ---------------------------------------------------------------- the fused tail: 128 channels, 8x32x32 latents, B = 16
@pytest.fixture(scope="module")
def wide():
    from models import DDPM, Unet
    cfg = ddpm_cfg(128, 8, 32)
    return det_load(DDPM(cfg, Unet(cfg), DEV, 8)).to(DEV).eval()       # an 8-channel "image": the cfg4 latent's shape without the codec


@pytest.mark.parametrize("n,masked", [(1, True), (2, True), (2, False), (8, True)], ids=["n1", "n2", "n2_nomask", "n8"])
def test_fused_tail_equals_unfused_bit_for_bit(wide, n, masked):
    """ "6" steps, DDIM eta 0.5: n = 1 and n = 2 (with and without a mask) end in final_tail_kernel<.., RestoreNoisy>, n = 8 (W n = 256 >
    128) in p_update_restore_kernel<RestoreNoisy> whatever the option says; with DDK_OPT_RESTORE_FUSED_TAIL = 0 all end in the unfused kernels,
    with the same bits.  ddk_sampler_restore_noisy_tail_parts says which tail runs."""
    from ddk import ops
    m = wide
    plan = m._eps_model_nhwc().plan()
    before = ops.cluster_timeouts()
    B = 16
    shape = (B, 8, 32, 32)
    assert plan.restore_noisy_tail_parts(B, 32, 32, n) == (0 if n == 8 else 8)
    y0 = CC.pooled_y(shape, n, f"restore_noisy.wide.{n}") + SIGMA_Y * syn.synthetic_normal((B, 8, 32 // n, 32 // n), f"restore_noisy.wide.n{n}")
    mk = CC.mask("checker", B, 32 // n, 32 // n) if masked else None
    y = torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan"))) if masked else y0
    x_T = syn.synthetic_normal(shape, "restore_noisy.wide.xT")
    run = lambda: m.restore_noisy(y.to(DEV), mk, n, sigma_y=SIGMA_Y, respacing="6", ddim=True, eta=0.5, x_T=x_T, seed=SEED).cpu()
    fused = run()
    plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 0)
    try:
        assert plan.restore_noisy_tail_parts(B, 32, 32, n) == 0
        unfused = run()
    finally:
        plan.set_option(plan.OPT_RESTORE_FUSED_TAIL, 1)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, unfused), float((fused - unfused).abs().max())
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- one workspace, three kinds of chain, two noise levels
def test_chains_share_a_workspace_and_each_sigma_y_has_its_own_graph(tiny, data):
    """two noise levels back to back, and a noisy, a masked and a plain ancestral chain on the same workspace, state buffer, base
    tables and t_start, in two orders: each equals its own single run on a fresh workspace bit for bit (the kind, n, the presence of a
    mask and the two table buffers are in the graph key; y and the mask are staged by every call)"""
    from ddk import lib as L
    from ddk import ops
    m, _ = tiny
    ys, mks, x_T = data
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    before = ops.cluster_timeouts()
    tabs = {sy: m._noisy_tables("8", False, 0.0, sy) for sy in (0.1, 0.4)}
    tables, use = m._spaced_tables("8", False, 0.0)
    for tb, _ in tabs.values():
        assert all(torch.equal(tb[k], tables[k]) for k in tables)
    K = len(use)
    nbytes = max(lib.ddk_sampler_restore_noisy_workspace_bytes(plan.handle, 2, 16, 16, K - 1, n) for n in (1, 2))
    assert nbytes == lib.ddk_sampler_restore_masked_workspace_bytes(plan.handle, 2, 16, 16, K - 1, 1)
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    yd = {n: ops.nchw_to_nhwc(ys[n].to(DEV)) for n in (1, 2)}
    md = {n: mks[n].to(DEV) for n in (1, 2)}
    # what -> (sigma_y, n, with a mask); "m1": the masked chain, "anc": the ancestral one
    jobs = {"a1": (0.1, 1, True), "b1": (0.4, 1, True), "a2": (0.1, 2, True), "a2nm": (0.1, 2, False), "m1": None, "anc": None}

    def launch(what, a, tmap, stream):
        if what == "anc":
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        if what == "m1":
            return lib.ddk_sampler_run_restore_masked(a, tmap, L.ptr(yd[1]), L.ptr(md[1]), 1, stream)
        sy, n, masked = jobs[what]
        tb = tabs[sy][0]
        return lib.ddk_sampler_run_restore_noisy(a, tmap, L.ptr(tb["lam"]), L.ptr(tb["sgm"]), L.ptr(yd[n]), L.ptr(md[n]) if masked else None, n,
                                                 stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    x, tmap = sh.x, sh.tmap
    single = {what: sh.alone(what) for what in jobs}
    names = list(jobs)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert not torch.equal(single[p], single[q]), (p, q)
    for order in (("a1", "b1", "a1", "m1", "anc", "a2", "a2nm", "b1"), ("anc", "a2nm", "m1", "b1", "a2", "a1", "anc", "m1")):
        sh.interleaved(order, single)
    # n = 1 without a mask, a bad n, a null table and injected noise are rejected
    tb = tabs[0.1][0]
    with CC.workspace(plan, nbytes) as ws:
        a = CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED)
        call = lambda lam, sgm, y, mk, n: lib.ddk_sampler_run_restore_noisy(a, tmap, lam, sgm, y, mk, n, L.stream())
        assert call(L.ptr(tb["lam"]), L.ptr(tb["sgm"]), L.ptr(yd[1]), None, 1) == -1 and "mask" in L.last_error()
        assert call(L.ptr(tb["lam"]), L.ptr(tb["sgm"]), L.ptr(yd[1]), L.ptr(md[1]), 3) == -1
        assert call(None, L.ptr(tb["sgm"]), L.ptr(yd[1]), L.ptr(md[1]), 1) == -1 and "table" in L.last_error()
        noise = torch.zeros((K, *x.shape), device=DEV)
        a.noise = L.ptr(noise)
        assert call(L.ptr(tb["lam"]), L.ptr(tb["sgm"]), L.ptr(yd[1]), L.ptr(md[1]), 1) == -1 and "noise" in L.last_error()
    assert ops.cluster_timeouts() == before


# ---------------------------------------------------------------- dDDPM
def test_dddpm_restore_noisy_returns_image_and_latent_and_never_pastes():
    from models import DownsampleDDPM, Unet
    cfg = dddpm_cfg(32, 32, 2)
    m = det_load(DownsampleDDPM(cfg, Unet(cfg), DEV, 3)).to(DEV).eval()
    z_T = syn.synthetic_normal((2, 8, 8, 8), "restore_noisy.dd.zT")
    img = (syn.synthetic_normal((2, 3, 32, 32), "restore_noisy.dd.x").clamp(-1, 1) + 0.1 * syn.synthetic_normal((2, 3, 32, 32), "restore_noisy.dd.n"))
    mk = torch.zeros(32, 32)
    mk[:, :14] = 1
    mk[8:12, 24:28] = 1
    x_out, z = m.restore_noisy(img.to(DEV), mk, 1, sigma_y=0.1, respacing="8", ddim=True, eta=0.5, x_T=z_T, seed=SEED)
    assert x_out.shape == (2, 3, 32, 32) and z.shape == (2, 8, 8, 8) and torch.isfinite(x_out).all() and torch.isfinite(z).all()
    sel = (mk != 0).expand(2, 3, 32, 32)
    assert float((x_out.cpu() - img)[sel].abs().min()) > 0                          # no measured pixel was pasted back
    with torch.no_grad():
        assert torch.equal(x_out, m.rescaled_upsample(z))
    # scale 8: a 4 x 4 noisy low-resolution image with holes, latent block 2
    y = CC.pooled_y((2, 3, 32, 32), 8, "restore_noisy.dd.y") + 0.1 * syn.synthetic_normal((2, 3, 4, 4), "restore_noisy.dd.ny")
    x8, z8 = m.restore_noisy(y.to(DEV), CC.mask("checker", 2, 4, 4), 8, sigma_y=0.1, respacing="8", x_T=z_T, seed=SEED)
    assert x8.shape == (2, 3, 32, 32) and z8.shape == (2, 8, 8, 8) and torch.isfinite(x8).all()


# ---------------------------------------------------------------- the evaluator
def test_evaluator_with_and_without_sigma_y(tiny):
    from utils import restoration_metrics as RMx
    m, _ = tiny
    imgs = (np.random.default_rng(2).random((2, 16, 16, 3)) * 255).astype(np.uint8)
    kw = dict(batch_size=2, seed=5, scale=2, sr_mask="half", respacing="5")
    today = RMx.evaluate_restoration(m, imgs, "sr", **kw)
    zero = RMx.evaluate_restoration(m, imgs, "sr", sigma_y=0.0, **kw)
    assert set(zero) == set(today) and zero["method"] == "ddnm" and "sigma_y" not in zero
    for k in ("images", "methods"):
        for name in today[k]:
            a, b = today[k][name], zero[k][name]
            assert np.array_equal(a, b) if k == "images" else all(np.array_equal(a[q], b[q], equal_nan=True) for q in a)
    assert np.array_equal(today["consistency"], zero["consistency"]) and np.array_equal(today["consistency_u8"], zero["consistency_u8"])
    noisy = RMx.evaluate_restoration(m, imgs, "sr", sigma_y=0.1, **kw)
    assert noisy["method"] == "ddnm_plus" and noisy["sigma_y"] == 0.1 and noisy["unet_forwards"] == 5
    assert set(noisy["methods"]) == {"restored", "replicate", "bicubic"} and noisy["images"]["restored"].shape == imgs.shape
    assert noisy["consistency"].shape == (2,) and np.isfinite(noisy["consistency"]).all() and (noisy["consistency"] > 0).all()
    assert not np.array_equal(noisy["images"]["replicate"], today["images"]["replicate"])       # the baselines see the noisy measurement
    again = RMx.evaluate_restoration(m, imgs, "sr", sigma_y=0.1, **kw)
    assert np.array_equal(again["images"]["restored"], noisy["images"]["restored"])             # the noise is seeded
    inp = RMx.evaluate_restoration(m, imgs, "inpaint", batch_size=2, seed=5, mask="center", method="ddnm", respacing="5", sigma_y=0.1)
    assert inp["method"] == "ddnm_plus" and inp["sigma_y"] == 0.1 and inp["consistency"].shape == (2,)
    for bad in (dict(dpm_solver=True), dict(method="repaint")):
        with pytest.raises(ValueError):
            RMx.evaluate_restoration(m, imgs, "inpaint", batch_size=2, seed=5, mask="center", respacing="5", sigma_y=0.1,
                                     **dict(dict(method="ddnm"), **bad))
    with pytest.raises(ValueError):
        RMx.evaluate_restoration(m, imgs, "sr", sigma_y=-1.0, **kw)
