"""The benchmark's timed path vs the CPU oracle: cfg4's dDDPM-x3 UNet (unet_chan 128, 8x32x32 latents, linear schedule,
T = 1000) at B = 32, called as bench.py calls it -- plan.sample_nhwc(x, m._tables(), t_start, t_end, seed=, stream_id=3,
use_graph=True), default plan options.  At B = 32 the 3x3 convs run one workgroup per CU, the in-launch GroupNorm, the
first-Block GroupNorm and the level chain exchange data inside their launches, and every step ends in
final_tail_kernel<32, 1, StepKind::Ancestral>; no B <= 8 test reaches that occupancy.

Two 40-step windows, each 16 + 16 + 8 steps of replayed graphs: t = 999 .. 960 with the in-kernel Philox draws (the oracle gets
the same draws from ops.randn, NHWC [B,H,W,C] at step t: p_update_kernel's and final_tail_kernel's indexing), and t = 39 .. 0
with injected draws, which includes the noise-free t == 0 step.  The oracle is oracle/diffusion_ref.p_sample_update around
oracle/unet_ref.unet_forward, started at t_start.  Bar, as for the golden chains: max abs difference <= 1e-4 and the same argmax
pixel per image (measured 4.8e-7 and 9.5e-7; the decoder 1.8e-6; a changed draw in image 17 misses by 0.11).  Every call must
have run the in-launch path: a give-up silently reruns without it."""
import numpy as np
import pytest
import torch

from helpers import dddpm_cfg, det_load, unet_cfg
from oracle import diffusion_ref as D
from oracle import resampler_ref as R
from oracle import unet_ref as U
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, C, S = 32, 8, 32
STREAM = 3
TOL = 1e-4
CFG = dddpm_cfg(128, 256, 3)


@pytest.fixture(scope="module")
def cfg4():
    from models import DownsampleDDPM, Unet
    m = det_load(DownsampleDDPM(CFG, Unet(CFG), DEV, 3)).to(DEV).eval()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    return m, sd


def _oracle_window(sd, x, t_start, t_end, draw):
    """oracle reverse steps t_start .. t_end on NCHW x (CPU); draw(t) -> the NCHW noise of step t"""
    buf = D.schedule_buffers("linear", 1000)
    with torch.no_grad():
        for i in range(t_start, t_end - 1, -1):
            t = torch.full((x.shape[0],), i, dtype=torch.long)
            x = D.p_sample_update(buf, x, t, U.unet_forward(sd, unet_cfg(128, C), x, t, pre="latent_model."), draw(i))
    return x


def _gpu_window(m, x_nchw, t_start, t_end, seed, noise=None):
    """the bench's call on a copy of x; asserts the in-launch path ran (no give-up, option still on).  Returns NCHW on the CPU."""
    from ddk import ops
    plan = m._eps_model_nhwc().plan()
    before = ops.cluster_timeouts()
    x = ops.nchw_to_nhwc(x_nchw.to(DEV).contiguous())
    nz = None if noise is None else noise.to(DEV).permute(0, 1, 3, 4, 2).contiguous()     # [k,B,C,H,W] -> [k,B,H,W,C]
    with torch.no_grad():
        plan.sample_nhwc(x, m._tables(), t_start, t_end, noise=nz, seed=seed, stream_id=STREAM, use_graph=True)
    torch.cuda.synchronize()
    assert plan._cluster >= 1, "the in-launch GroupNorm was switched off by a give-up"
    assert ops.cluster_timeouts() == before
    return ops.nhwc_to_nchw(x).cpu()


def _per_image_err(a, b):
    return (a - b).abs().reshape(a.shape[0], -1).max(dim=1).values


def _argmax(x):
    return x.reshape(x.shape[0], -1).argmax(dim=1)


@pytest.fixture(scope="module")
def late_window(cfg4):
    """t = 39 .. 0, injected draws: (x_start, noise, oracle result)"""
    _, sd = cfg4
    x0 = syn.synthetic_normal((B, C, S, S), "timed.late.x")
    noise = torch.stack([syn.synthetic_normal((B, C, S, S), f"timed.late.n{k}") for k in range(40)])
    want = _oracle_window(sd, x0, 39, 0, lambda t: noise[39 - t])
    return x0, noise, want


def test_timed_path_philox_window_999_to_960(cfg4):
    from ddk import ops
    m, sd = cfg4
    seed = 1234
    x0 = ops.randn((B, S, S, C), DEV, seed, step=1000, stream_id=STREAM).permute(0, 3, 1, 2).cpu().contiguous()
    got = _gpu_window(m, x0, 999, 960, seed)
    want = _oracle_window(sd, x0, 999, 960,
                          lambda t: ops.randn((B, S, S, C), DEV, seed, step=t, stream_id=STREAM).permute(0, 3, 1, 2).cpu())
    err = float((got - want).abs().max())
    print(f"cfg4 B=32 t=999..960 Philox: max abs error {err:.3g}")
    assert torch.isfinite(got).all()
    assert err <= TOL
    assert torch.equal(_argmax(got), _argmax(want))


def test_timed_path_injected_window_39_to_0_and_decode(cfg4, late_window):
    """the window that ends in the t == 0 step, then the x3 decoder (tanh(upsample(z))) over the whole batch: images 0, 17 and 31
    vs oracle/resampler_ref on the same z, and their [0, 255] NHWC images (fix_samples)."""
    m, sd = cfg4
    x0, noise, want = late_window
    got = _gpu_window(m, x0, 39, 0, seed=5, noise=noise)
    err = float((got - want).abs().max())
    print(f"cfg4 B=32 t=39..0 injected: max abs error {err:.3g}")
    assert err <= TOL
    assert torch.equal(_argmax(got), _argmax(want))
    with torch.no_grad():
        img = m.rescaled_upsample(got.to(DEV)).cpu()
        assert img.shape == (B, 3, 256, 256)
        pick = [0, 17, 31]
        ref = torch.cat([R.rescaled_upsample(sd, CFG, got[i:i + 1]) for i in pick])
    derr = float((img[pick] - ref).abs().max())
    print(f"cfg4 decode of images {pick}: max abs error {derr:.3g}")
    assert derr <= TOL
    from utils import fix_samples
    fixed, fixed_ref = fix_samples(img)[pick], D.fix_samples(ref)
    assert fixed.shape == (3, 256, 256, 3)
    assert np.abs(fixed - fixed_ref).max() < 2e-2
    assert (np.round(fixed) != np.round(fixed_ref)).mean() < 2e-3      # identical uint8 images (<=1 LSB on <0.2%)


def test_timed_path_detects_one_changed_draw_in_one_image(cfg4, late_window):
    """negative control: image 17's draw at t = 20 replaced -- image 17 misses the oracle by more than 10x the bar, every other
    image still passes it (the batch stays independent through the in-launch exchanges)."""
    m, _ = cfg4
    x0, noise, want = late_window
    bad = noise.clone()
    bad[39 - 20, 17] = syn.synthetic_normal((C, S, S), "timed.late.control")
    got = _gpu_window(m, x0, 39, 0, seed=5, noise=bad)
    err = _per_image_err(got, want)
    print(f"cfg4 B=32 t=39..0, image 17's draw at t=20 changed: image 17 {float(err[17]):.3g}, others <= "
          f"{float(torch.cat([err[:17], err[18:]]).max()):.3g}")
    assert float(err[17]) > 10 * TOL
    assert float(torch.cat([err[:17], err[18:]]).max()) <= TOL
