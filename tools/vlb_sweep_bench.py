#!/usr/bin/env python3
"""Per-step time of the test-loss sweep at the cfg4 shape (unet_chan 128, 8-channel 32x32 latents, B = 32, T = 1000), synthetic
weights, one process, device events around a synchronised window after a warm-up run of each:
  (a) today's per-step Python loop, DDPM.test_losses(x)  (torch draws, q_sample + single forward + vlb_terms per step);
  (b) the native sweep, DDPM.test_losses(x, seed=s)       (ddk_vlb_sweep_run: graph-replayed steps);
  (c) the sampler on the same shape, ddk_sampler_run      (t = T-1 .. 0).
Prints one JSON line.  `trace sweep|sampler [T]` runs only that chain once at a short T (default 48), for a
rocprofv3 --kernel-trace --stats run that counts launches per step.  GPU-box tool."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]
import torch

from ddk import ops
from models import DDPM, Unet
from utils import synthetic as syn

DEV = "cuda"
B, C, S = 32, 8, 32


def make(T):
    c = dict(unet_chan=128, unet_in=C, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=S, T=T, loss_type="simple",
             beta_schedule="linear", loss_flat="sum")
    m = DDPM(c, Unet(c), DEV, C)
    m.load_state_dict(syn.fill_state_dict(m.state_dict(), skip=syn.SCHEDULE_KEYS))
    return m.to(DEV).eval()


def timed(fn):
    """ms of one call of fn, device events around a synchronised window (after one warm-up call)"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    x = syn.synthetic_input((B, C, S, S), "vlb_bench.x").clamp(-1, 1).to(DEV)
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        T = int(sys.argv[3]) if len(sys.argv) > 3 else 48
        m = make(T)
        with torch.no_grad():
            if sys.argv[2] == "sweep":
                m.test_losses(x, seed=1)
            else:
                m.p_sample_loop((B, C, S, S), seed=1)
        torch.cuda.synchronize()
        print(json.dumps({"trace": sys.argv[2], "T": T, "steps": T}))
        return
    T = 1000
    m = make(T)
    plan, tables = m.latent_model.plan(), m._tables()
    x_nhwc = ops.randn((B, S, S, C), DEV, seed=1, step=T, stream_id=0)
    with torch.no_grad():
        loop_ms = timed(lambda: m.test_losses(x))
        sweep_ms = timed(lambda: m.test_losses(x, seed=1))
        smp_ms = timed(lambda: plan.sample_nhwc(x_nhwc, tables, T - 1, 0, seed=1))
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}",
           "python_loop_ms_per_step": round(loop_ms / T, 4), "native_sweep_ms_per_step": round(sweep_ms / T, 4),
           "sampler_ms_per_step": round(smp_ms / T, 4), "loop_over_sweep": round(loop_ms / sweep_ms, 2),
           "sweep_minus_sampler_ms_per_step": round((sweep_ms - smp_ms) / T, 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
