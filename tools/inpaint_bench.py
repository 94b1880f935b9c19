#!/usr/bin/env python3
"""RePaint inpainting at the benchmark's shape: cfg4 (dDDPM-x3, unet_chan 128, 8x32x32 latents, B = 32, T = 1000), synthetic
weights, default plan options, the native graph sampler.

Two chains are timed ALTERNATELY in this process, REPS times each, from the same x_T and bracketed by device synchronisation, after
the clock has been settled by running plain steps for a while (measuring-on-mi355x: warm up by time): a respaced ancestral chain of
K = 250 steps ("250") and the RePaint chain over the same steps with jump_length 10, jump_n_sample 10 (N = 2410 ops, a centre
square hidden).  Both evaluate the UNet once per step / op; they differ in the step's last kernel (the known latent, the mask and
two more Philox draws).  The figure is the median per-op time over the median per-step time.  images/s = B / (N * ms_op +
t_encode + t_decode) with the x3 encoder and decoder timed in the same run.  Writes one JSON line to stdout and to --out
(default profiles/inpaint_bench.json).  GPU-box tool."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]
import torch

import bench
from ddk import ops
from models import DownsampleDDPM, Unet
from utils import synthetic as syn

DEV = "cuda"
B, C, S, T = 32, 8, 32, 1000
SPEC, J, R = "250", 10, 10
REPS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inpaint_bench.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = bench.cfg4()
    model = DownsampleDDPM(cfg, Unet(cfg), DEV, 3)
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    model = model.to(DEV).eval()
    plan = model.latent_model.plan()
    x0 = ops.randn((B, S, S, C), DEV, seed=1234, step=T, stream_id=0)
    x = x0.clone()
    img = syn.synthetic_normal((B, 3, 256, 256), "inpaint_bench.x").clamp(-1, 1).to(DEV)
    mask = torch.ones(B, 1, 256, 256, device=DEV)
    mask[:, :, 64:192, 64:192] = 0
    m_lat = -torch.nn.functional.max_pool2d(-mask, int(model.dim_reduc))
    known = ops.nchw_to_nhwc(model.rescaled_downsample(img * mask))
    mk = ops.nchw_to_nhwc(m_lat.expand(-1, C, -1, -1).contiguous())
    sp, use_sp = model._spaced_tables(SPEC, False, 0.0)
    ip, use_ip = model._inpaint_tables(SPEC, J, R)
    K, N = len(use_sp), len(use_ip)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def chain(kind, n=None):
        x.copy_(x0)
        if kind == "plain":
            return timed(lambda: plan.sample_nhwc(x, model._tables(), T - 1, T - n, seed=1234, stream_id=0))
        if kind == "spaced":
            return timed(lambda: plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use_sp))
        return timed(lambda: plan.sample_inpaint_nhwc(x, known, mk, ip, use_ip, seed=1234, stream_id=0))

    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:
            chain("plain", 96)
        encode_ms = min(timed(lambda: model.rescaled_downsample(img * mask)) for _ in range(3))
        decode_ms = min(timed(lambda: model.rescaled_upsample(ops.nhwc_to_nchw(x))) for _ in range(3))
        chain("spaced")                                   # captures both chains' graphs outside the timed calls
        chain("inpaint")
        spaced, inp = [], []
        for _ in range(REPS):
            spaced.append(chain("spaced") / K)
            inp.append(chain("inpaint") / N)
        assert torch.isfinite(x).all()
    s, i = statistics.median(spaced), statistics.median(inp)
    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}", "reps": REPS,
           "spaced": {"spec": SPEC, "steps": K, "ms_per_step": round(s, 4), "min_max_ms": [round(min(spaced), 4), round(max(spaced), 4)]},
           "inpaint": {"spec": SPEC, "jump_length": J, "jump_n_sample": R, "ops": N, "ms_per_op": round(i, 4),
                       "min_max_ms": [round(min(inp), 4), round(max(inp), 4)]},
           "inpaint_op_over_spaced_step": round(i / s, 4), "encode_ms": round(encode_ms, 3), "decode_ms": round(decode_ms, 3),
           "inpaint_images_per_sec": round(B / ((N * i + encode_ms + decode_ms) / 1e3), 3)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
