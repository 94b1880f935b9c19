"""The native likelihood sweep (ddk_vlb_sweep_run; DDPM.test_losses(x, seed= / noise=)): test_losses_ of reference
models/diffusion/ddpm.py:392-446 as one graph-replayed chain -- the sampler's step with a q_sample input and a VLB epilogue --
against the reference golden (g9), today's per-step loop, the CPU oracle at every final-tail width, itself (Philox, cache
isolation) and the evaluate_ddpm.py CLI."""
import json
import os
import subprocess
import sys

import pytest
import torch

from helpers import ddpm_cfg, dddpm_cfg, det_load, golden, rel_err
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"vlb_t", "prior", "vlb", "L_simple_t", "L_simple"}
VLB_STREAM_BIT = 1 << 31


def _model(cfg, cls=None):
    from models import DDPM, Unet
    cls = cls or DDPM
    return det_load(cls(cfg, Unet(cfg), DEV, cfg["unet_in"] if cls is DDPM else 3)).to(DEV).eval()


def _g9_x():
    x = syn.synthetic_input((2, 3, 16, 16), "g9.x").clamp(-1, 1)
    x[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, -0.9995, 0.9995])
    return x


def _loop_with_draws(m, x, draws):
    """today's Python loop (no keywords) fed the given draws through torch.randn_like, in the reference's order"""
    it = iter(list(draws))
    orig = torch.randn_like
    torch.randn_like = lambda z: next(it)
    try:
        return m.test_losses(x)
    finally:
        torch.randn_like = orig


def _equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize("loss_type", ["simple", "hybrid"])
def test_sweep_vs_reference_golden_unfused_epilogue(loss_type):
    """g9's model (unet_chan 32, 16x16, T = 50).  Its final conv has 32 output channels, so the plan packs no Winograd form of it
    (has_wu needs cout % 64 == 0): fused_tail_parts() is 0 and every step ends in conv + GroupNorm + 1x1 -> eps_hat, then
    vlb_sweep_terms_kernel.  The 50 injected draws g9.eps{k} reproduce the reference's own output."""
    g = golden("g9_test_losses")
    m = _model(ddpm_cfg(32, 3, 16, T=50, loss_type=loss_type))
    noise = torch.stack([syn.synthetic_normal((2, 3, 16, 16), f"g9.eps{k}") for k in range(50)]).to(DEV)
    res = m.test_losses(_g9_x().to(DEV), noise=noise)
    assert set(res) == KEYS
    assert res["vlb_t"].shape == (2, 50) and res["L_simple_t"].shape == (50,)
    for k, v in res.items():
        assert rel_err(v.cpu(), torch.as_tensor(g[f"{loss_type}_{k}"])) < 5e-5, k


def test_sweep_fused_tail_matches_loop_at_cfg4_shape():
    """unet_chan 128, 8-channel 32x32 latents, B = 32: the final tail runs as final_tail_kernel<32, 1, StepKind::Vlb>, and the steps use
    the in-launch GroupNorm and the level chain (the single forwards of the loop do not: close, not bitwise)."""
    m = _model(ddpm_cfg(128, 8, 32, T=100))
    x = syn.synthetic_input((32, 8, 32, 32), "sweep.cfg4.x").clamp(-1, 1).to(DEV)
    noise = torch.stack([syn.synthetic_normal((32, 8, 32, 32), f"sweep.cfg4.n{k}") for k in range(100)]).to(DEV)
    want = _loop_with_draws(m, x, noise)
    got = m.test_losses(x, noise=noise)
    assert set(got) == KEYS and got["vlb_t"].shape == (32, 100)
    for k in KEYS:
        assert torch.isfinite(got[k]).all(), k
        assert rel_err(got[k].cpu(), want[k].cpu()) < 1e-4, k
    assert m._eps_model_nhwc().plan()._cluster >= 1          # the in-launch path ran and was not switched off


@pytest.mark.parametrize("shape", ["unfused", "fused"])
def test_sweep_philox_deterministic_and_same_draws_as_injected(shape):
    from ddk import ops
    if shape == "unfused":
        m, xs = _model(ddpm_cfg(32, 3, 16, T=50)), (2, 3, 16, 16)
    else:
        m, xs = _model(ddpm_cfg(128, 8, 32, T=40)), (32, 8, 32, 32)
    T = m.timesteps
    x = syn.synthetic_input(xs, f"sweep.philox.{shape}").clamp(-1, 1).to(DEV)
    a = m.test_losses(x, seed=1234)
    b = m.test_losses(x, seed=1234)
    c = m.test_losses(x, seed=1235)
    assert _equal(a, b)
    assert not torch.equal(a["vlb_t"], c["vlb_t"]) and not torch.equal(a["L_simple_t"], c["L_simple_t"])
    # the draws the kernels make for key (1234, stream 0 | 2^31): NHWC [B,H,W,C] at step t, draw k = T-1-t, as NCHW
    bb, cc, hh, ww = xs
    draws = torch.stack([ops.randn((bb, hh, ww, cc), DEV, 1234, T - 1 - k, m.rng_stream_id | VLB_STREAM_BIT).permute(0, 3, 1, 2)
                         for k in range(T)]).contiguous()
    inj = m.test_losses(x, noise=draws)
    assert _equal(a, inj)


def test_sweep_and_sampler_graph_caches_stay_apart():
    """one plan: sweep, sampler chain of the same shape, sweep again -- the sweeps agree bit for bit, and the sampler's result is
    the one a fresh plan gives (neither kind of chain replays the other's graph)."""
    cfg = ddpm_cfg(128, 8, 32, T=40)
    m = _model(cfg)
    x = syn.synthetic_input((32, 8, 32, 32), "sweep.iso.x").clamp(-1, 1).to(DEV)
    x_T = syn.synthetic_normal((32, 8, 32, 32), "sweep.iso.xT").to(DEV)
    s1 = m.test_losses(x, seed=7)
    smp = m.p_sample_loop((32, 8, 32, 32), x_T=x_T, seed=99)
    s2 = m.test_losses(x, seed=7)
    assert _equal(s1, s2)
    fresh = _model(cfg).p_sample_loop((32, 8, 32, 32), x_T=x_T, seed=99)
    assert torch.equal(smp, fresh)


def test_dddpm_test_losses_passes_keywords_through():
    from models import DownsampleDDPM
    m = _model(dddpm_cfg(32, 32, 2, T=50), DownsampleDDPM)
    x = syn.synthetic_input((2, 3, 32, 32), "sweep.dd.x").to(DEV)
    got = m.test_losses(x, seed=5)
    with torch.no_grad():
        want = m.test_losses_(m.rescaled_downsample(x), seed=5)
    assert _equal(got, want)
    assert got["vlb_t"].shape == (2, 50) and all(torch.isfinite(v).all() for v in got.values())


def test_default_test_losses_draws_from_torch_once_per_step():
    m = _model(ddpm_cfg(32, 3, 16, T=50))
    calls = []
    orig = torch.randn_like

    def counting(z):
        calls.append(tuple(z.shape))
        return orig(z)

    torch.randn_like = counting
    try:
        res = m.test_losses(_g9_x().to(DEV))
    finally:
        torch.randn_like = orig
    assert len(calls) == 50 and set(calls) == {(2, 3, 16, 16)}
    assert set(res) == KEYS


def test_evaluate_ddpm_cli_end_to_end(tmp_path):
    # (T = 25, not 20: the linear schedule at T = 20 ends on beta = 1, so alphas_cumprod[19] = 0 and the step coefficients of t = 19 are
    # Inf -- the reference's own VLB is NaN there (oracle.diffusion_ref.test_losses), and the sweep now reports it instead of hiding it)
    cfg = ddpm_cfg(32, 3, 16, T=25)
    cfg.update(model="ddpm", dataset="cifar10", batch_size=2)
    cfg_path = tmp_path / "cfg.json"
    cfg_path.write_text(json.dumps(cfg))
    out = tmp_path / "metrics.json"
    script = os.path.join(ROOT, "downsampled-diffusion_amd", "evaluate_ddpm.py")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "downsampled-diffusion_amd"))
    r = subprocess.run([sys.executable, script, "--synthetic", str(cfg_path), "--max_batches", "2", "--seed", "3", "--json", str(out)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    metrics = json.loads(out.read_text())
    assert set(metrics) == {"vlb", "L_simple", "is", "fid", "sfid", "precision", "recall"}
    assert all(metrics[k] is None for k in ("is", "fid", "sfid", "precision", "recall"))
    assert all(isinstance(metrics[k], float) and metrics[k] == metrics[k] and abs(metrics[k]) < float("inf") for k in ("vlb", "L_simple"))
    assert "out of scope" in r.stdout


# ---------------------------------------------------------------- every final-tail width vs the CPU oracle
# (unet_chan, in_ch, size, B): which epilogue the sweep's steps end in.  fused_tail_parts (csrc/unet_plan.hip) fuses only when the
# final conv has a Winograd form (unet_chan % 64 == 0), runs in one pass (conv_wino_splits == 1: at least 256 workgroups without
# splitting its 32-channel chunks) and final_tail_ok admits the width for StepKind::Vlb (C <= 128).  Confirmed from the kernel names of one
# rocprofv3 --kernel-trace --stats run of these five sweeps.
SWEEP_CASES = {
    "c128_b32_fused": (128, 8, 32, 32),      # final_tail_kernel<32, 1, StepKind::Vlb>: cfg4's shape
    "c64_b32_fused": (64, 8, 32, 32),        # final_tail_kernel<16, 1, StepKind::Vlb>
    "c64_b8_unfused": (64, 8, 32, 8),        # 64 workgroups: the final conv splits its 2 chunks -> conv + GroupNorm + 1x1
    "c256_b32_unfused": (256, 3, 16, 32),    # one-pass final conv (2 tiles per image), but C = 256 > 128: final_tail_ok(.., StepKind::Vlb)
    "c32_b32_unfused": (32, 3, 16, 32),      # no Winograd final conv; vlb_sweep_terms_kernel over 2 slices per image
}
EDGES = torch.tensor([-1.0, 1.0, -0.9995, 0.9995, -0.999, 0.999, -0.9989, 0.9989])
SWEEP_TOL = 5e-5
T0_TOL = 5e-6         # the t = 0 column on its own (the discretised NLL): measured <= 5.7e-7 over the five cases


def edge_x(shape, key):
    """x in [-1, 1) with the discretised NLL's branch edges: -1, 1, +-0.9995, exactly +-0.999 and +-0.9989, as the first 8 NHWC
    elements of image 0 (pixel 0 on), the last 8 of the last image (ending at pixel H*W-1: the last 128-pixel tile), and across
    the last channel of the middle image."""
    b, c, h, w = shape
    v = syn.synthetic_input(shape, key).clamp(-1, 1).permute(0, 2, 3, 1).contiguous()
    v[0].view(-1)[:8] = EDGES
    v[-1].view(-1)[-8:] = EDGES
    x = v.permute(0, 3, 1, 2).contiguous()
    x[b // 2, c - 1].view(-1)[torch.linspace(0, h * w - 1, 8).long()] = EDGES
    return x


def _oracle_sweep(m, cfg, x, noise):
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    T = cfg["T"]
    with torch.no_grad():
        return D.test_losses(D.schedule_buffers("linear", T), lambda a, t: U.unet_forward(sd, cfg, a, t, pre="latent_model."),
                             x, list(noise), T)


def _sweep_errors(got, want):
    errs = {k: rel_err(got[k].cpu(), want[k]) for k in KEYS}
    errs["t0"] = rel_err(got["vlb_t"][:, -1].cpu(), want["vlb_t"][:, -1])
    errs["t>0"] = rel_err(got["vlb_t"][:, :-1].cpu(), want["vlb_t"][:, :-1])
    return errs


@pytest.mark.parametrize("case", list(SWEEP_CASES))
def test_sweep_every_tail_width_vs_oracle(case):
    """ddk_vlb_sweep_run (T = 50, injected draws) vs oracle/diffusion_ref.test_losses: all five keys at 5e-5 relative, the t = 0
    column -- the only one the NLL branches decide -- on its own at 5e-6.  Negative control: image 0's +0.9995 moved to 0.9985
    (the upper branch to the middle one) must move that column past 10x its bar while every t > 0 column still passes.  One
    element of 8192 moves the column by 6e-5 of its max at 8 channels (7e-4 at 3), hence the tighter bar on that column."""
    chan, cin, size, bsz = SWEEP_CASES[case]
    cfg = ddpm_cfg(chan, cin, size, T=50)
    m = _model(cfg)
    shape = (bsz, cin, size, size)
    x = edge_x(shape, f"sweep.edge.{case}")
    noise = torch.stack([syn.synthetic_normal(shape, f"sweep.edge.{case}.n{k}") for k in range(50)])
    want = _oracle_sweep(m, cfg, x, noise)
    got = m.test_losses(x.to(DEV), noise=noise.to(DEV))
    errs = _sweep_errors(got, want)
    print(f"sweep {case}: relative errors {errs}")
    assert all(errs[k] < SWEEP_TOL for k in KEYS), errs
    assert errs["t0"] < T0_TOL, errs
    moved = x.permute(0, 2, 3, 1).contiguous()
    assert float(moved[0].view(-1)[3]) == float(EDGES[3])
    moved[0].view(-1)[3] = 0.9985
    bad = _sweep_errors(m.test_losses(moved.permute(0, 3, 1, 2).contiguous().to(DEV), noise=noise.to(DEV)), want)
    print(f"sweep {case}, x[0] 0.9995 -> 0.9985: relative errors {bad}")
    assert bad["t0"] > 10 * T0_TOL and bad["t>0"] < SWEEP_TOL and bad["L_simple_t"] < SWEEP_TOL, bad


def test_sampler_window_at_256_channels_vs_oracle():
    """the sampler's final_tail_kernel<32, 2, StepKind::Ancestral> (256 channels, 3x16x16, B = 32: two tiles per image, one-pass final conv):
    20 steps t = 19 .. 0 of replayed graphs with the in-kernel Philox draws vs the oracle fed the same draws (ops.randn, NHWC at
    step t).  Bar as for the golden chains: 1e-4 abs (measured 7.5e-6), the same argmax pixel per image."""
    from ddk import ops
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    cfg = ddpm_cfg(256, 3, 16, T=50)
    m = _model(cfg)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    bsz, seed = 32, 321
    x0 = syn.synthetic_normal((bsz, 3, 16, 16), "sampler.c256.x")
    draw = lambda t: ops.randn((bsz, 16, 16, 3), DEV, seed, step=t, stream_id=0).permute(0, 3, 1, 2).cpu()
    before = ops.cluster_timeouts()
    x = ops.nchw_to_nhwc(x0.to(DEV).contiguous())
    with torch.no_grad():
        m._eps_model_nhwc().plan().sample_nhwc(x, m._tables(), 19, 0, seed=seed, stream_id=0, use_graph=True)
    got = ops.nhwc_to_nchw(x).cpu()
    assert ops.cluster_timeouts() == before
    buf = D.schedule_buffers("linear", 50)
    want = x0
    with torch.no_grad():
        for i in range(19, -1, -1):
            t = torch.full((bsz,), i, dtype=torch.long)
            want = D.p_sample_update(buf, want, t, U.unet_forward(sd, cfg, want, t, pre="latent_model."), draw(i))
    err = float((got - want).abs().max())
    print(f"sampler c256 B=32 t=19..0 Philox: max abs error {err:.3g}")
    assert err <= 1e-4
    assert torch.equal(got.reshape(bsz, -1).argmax(dim=1), want.reshape(bsz, -1).argmax(dim=1))
