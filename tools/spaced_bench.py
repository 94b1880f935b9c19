#!/usr/bin/env python3
"""Respaced / DDIM sampling at the benchmark's shape: cfg4 (dDDPM-x3, unet_chan 128, 8x32x32 latents, B = 32, T = 1000), synthetic
weights, default plan options, the native graph sampler.

For each K in {50, 100, 250} a DDIM chain (respacing "ddimK", eta 0; the step is the same captured graph whatever the tables) and a
plain chain of the same K steps (t = 999 .. 1000 - K, the benchmark's own call) are timed ALTERNATELY in this process, REPS times
each, every chain from the same x_T and bracketed by device synchronisation; the per-step figure is the median.  The clock is
settled first by running plain steps for a while (measuring-on-mi355x: warm up by time).  images/s = B / (K * ms_step + t_decode),
with the x3 decode (tanh(upsample(z))) timed in the same run; T = 1000 is the plain chain's per-step time x 1000.  One JSON line on
stdout.  GPU-box tool."""
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
KS = (50, 100, 250)
REPS = 5


def main():
    torch.cuda.set_device(0)
    cfg = bench.cfg4()
    model = DownsampleDDPM(cfg, Unet(cfg), DEV, 3)
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    model = model.to(DEV).eval()
    plan = model.latent_model.plan()
    tables = model._tables()
    x0 = ops.randn((B, S, S, C), DEV, seed=1234, step=T, stream_id=0)
    x = x0.clone()

    def chain(kind, K):
        x.copy_(x0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "plain":
            plan.sample_nhwc(x, tables, T - 1, T - K, seed=1234, stream_id=0)
        else:
            sp, use = model._spaced_tables(f"ddim{K}", True, 0.0)
            plan.sample_nhwc(x, sp, K - 1, 0, seed=1234, stream_id=0, timesteps=use)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def decode():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = model.rescaled_upsample(ops.nhwc_to_nchw(x))
        torch.cuda.synchronize()
        assert torch.isfinite(img).all() and img.shape == (B, 3, 256, 256)
        return (time.perf_counter() - t0) * 1e3

    res = {"shape": f"cfg4 unet_chan 128, {C}x{S}x{S} latents, B={B}, T={T}, DDIM eta 0", "reps": REPS, "per_K": {}}
    with torch.no_grad():
        t_settle = time.perf_counter()
        while time.perf_counter() - t_settle < 2.0:          # settle the clock on the step's own load
            chain("plain", 96)
        decode_ms = min(decode() for _ in range(3))
        plain_all = []
        for K in KS:
            chain("plain", K)
            chain("ddim", K)                                 # captures this K's graphs outside the timed calls
            plain, spaced = [], []
            for _ in range(REPS):
                plain.append(chain("plain", K) / K)
                spaced.append(chain("ddim", K) / K)
            assert torch.isfinite(x).all()
            p, s = statistics.median(plain), statistics.median(spaced)
            plain_all += plain
            res["per_K"][str(K)] = {"plain_ms_per_step": round(p, 4), "spaced_ms_per_step": round(s, 4),
                                    "spaced_over_plain": round(s / p, 4), "spaced_min_max_ms": [round(min(spaced), 4), round(max(spaced), 4)],
                                    "plain_min_max_ms": [round(min(plain), 4), round(max(plain), 4)],
                                    "images_per_sec": round(B / ((K * s + decode_ms) / 1e3), 2)}
        p_all = statistics.median(plain_all)
        res["decode_ms"] = round(decode_ms, 3)
        res["T1000_images_per_sec"] = round(B / ((T * p_all + decode_ms) / 1e3), 2)
        res["max_spaced_over_plain"] = max(v["spaced_over_plain"] for v in res["per_K"].values())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
