#!/usr/bin/env python3
"""Time the dDDPM's resamplers in their three modes, and every kernel of csrc/resample.hip on its own.

B = 32 images of 3x256x256, n_downsamples 3 (32x32 latents); unet_in 3 for 'deterministic' (a resize keeps the channels), 8 otherwise.
  * encoder (rescaled_downsample) and decoder (rescaled_upsample) of 'deterministic', 'convolutional' and 'convolutional_res';
  * each new kernel at the shapes those models launch it with, forward and gradients: us per launch and GB/s on ALGORITHMIC bytes
    (every operand read once, every result written once, counted from the shapes below), and that rate as a fraction of the
    contiguous-stream rate from HBM that tools/dma_rate.hip recorded (profiles/r02_dma_rate.txt, 1 GiB source).

Timing: device events around a window of back-to-back calls (>= ~20 ms of work each, up to 2000 calls), replayed from one device
graph so that no per-call host work is in the window; every item warmed up first, then `--repeats` rounds that go through ALL
items in turn (so drift hits them alike), the median per item; one process.  A window of dependent launches on one stream
includes the gap between two kernels (~2 us here), which is what a caller pays as well.

    python tools/resampler_bench.py [--out profiles/resampler_modes_bench.json]
"""
import argparse
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]

import torch  # noqa: E402

B, C_IMG, SIZE, N_DOWN, LATENT = 32, 3, 256, 3, 32


def stream_rate_tb_s():
    """the best contiguous-stream (pattern 0) rate from a 1 GiB source in profiles/r02_dma_rate.txt, and the line it stands on"""
    best, where = 0.0, None
    with open(os.path.join(ROOT, "profiles", "r02_dma_rate.txt")) as f:
        for line in f:
            if not line.startswith("src 1024 MiB pattern 0"):
                continue
            for depth, rate in re.findall(r"(d\d+)\s+([0-9.]+) TB/s", line):
                if float(rate) > best:
                    best, where = float(rate), f"{line.split(':')[0].strip()} {depth}"
    if where is None:
        raise SystemExit("profiles/r02_dma_rate.txt has no 'src 1024 MiB pattern 0' line")
    return best, where


def cfg_for(mode):
    unet_in = 3 if mode == "deterministic" else 8
    return dict(unet_chan=32, unet_in=unet_in, unet_dims=(1, 2, 2, 2), unet_dropout=0.0, image_size=SIZE, T=1000, loss_type="simple",
                beta_schedule="linear", loss_flat="sum", d_mode=mode, u_mode=mode, d_dropout=0, d_chans=64, d_n_blocks=3, u_n_blocks=3,
                ae_loss=True, t_rec_max=100, force_latent=True, n_downsamples=N_DOWN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resampler_modes_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window_ms", type=float, default=20.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resampler_bench needs a ROCm device: a CPU run measures nothing")
    from ddk import ops
    from models import DownsampleDDPM, Unet
    from utils import synthetic as syn
    dev = "cuda"
    f4 = 4
    items = []          # (name, group, fn, algorithmic bytes or None)

    def rnd(*shape):
        return torch.randn(*shape, device=dev)

    # ---- the modules, as the model calls them
    x_img = rnd(B, C_IMG, SIZE, SIZE).clamp(-1, 1)
    for mode in ("deterministic", "convolutional", "convolutional_res"):
        cfg = cfg_for(mode)
        model = DownsampleDDPM(cfg, Unet(cfg), dev, C_IMG)
        model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
        model = model.to(dev).eval()
        z = torch.tanh(rnd(B, cfg["unet_in"], LATENT, LATENT))
        io = f4 * B * (C_IMG * SIZE * SIZE + cfg["unet_in"] * LATENT * LATENT)
        items.append((f"{mode}.encoder", "module", (lambda m=model: m.rescaled_downsample(x_img)), io))
        items.append((f"{mode}.decoder", "module", (lambda m=model, zz=z: m.rescaled_upsample(zz)), io))

    # ---- the kernels
    def plane(c, s):
        return f4 * B * c * s * s
    lat3 = rnd(B, 3, LATENT, LATENT)
    items.append(("bicubic_resize 256->32", "kernel", lambda: ops.bicubic_resize(x_img, (LATENT, LATENT)), plane(3, SIZE) + plane(3, LATENT)))
    items.append(("bicubic_resize 32->256", "kernel", lambda: ops.bicubic_resize(lat3, (SIZE, SIZE)), plane(3, SIZE) + plane(3, LATENT)))
    items.append(("bicubic_resize_grad 256->32", "kernel", lambda: ops.bicubic_resize_grad(lat3, (SIZE, SIZE)), plane(3, SIZE) + plane(3, LATENT)))
    items.append(("bicubic_resize_grad 32->256", "kernel", lambda: ops.bicubic_resize_grad(x_img, (LATENT, LATENT)), plane(3, SIZE) + plane(3, LATENT)))
    for cin, cout, s in ((3, 8, 256), (8, 8, 128), (8, 8, 64)):
        x, w, b, dy = rnd(B, cin, s, s), rnd(cout, cin, 3, 3) * 0.1, rnd(cout), rnd(B, cout, s // 2, s // 2)
        io, wb = plane(cin, s) + plane(cout, s // 2), f4 * w.numel()
        tag = f"{cin}->{cout} {s}->{s // 2}"
        items.append((f"conv_small_s2 {tag}", "kernel", (lambda x=x, w=w, b=b: ops.conv_small_s2(x, w, b)), io + wb))
        items.append((f"conv_small_s2_dgrad {tag}", "kernel", (lambda dy=dy, w=w, s=s: ops.conv_small_s2_dgrad(dy, w, (s, s))), io + wb))
        items.append((f"conv_small_s2_wgrad {tag}", "kernel", (lambda x=x, dy=dy: ops.conv_small_s2_wgrad(x, dy)), io + wb))
    for cin, cout, s in ((8, 8, 32), (8, 8, 64), (8, 3, 128)):
        x, w, b, dy = rnd(B, cin, s, s), rnd(cin, cout, 4, 4) * 0.1, rnd(cout), rnd(B, cout, 2 * s, 2 * s)
        io, wb = plane(cin, s) + plane(cout, 2 * s), f4 * w.numel()
        tag = f"{cin}->{cout} {s}->{2 * s}"
        items.append((f"convt_small_s2 {tag}", "kernel", (lambda x=x, w=w, b=b: ops.convt_small_s2(x, w, b)), io + wb))
        items.append((f"convt_small_s2_dgrad {tag}", "kernel", (lambda dy=dy, w=w: ops.convt_small_s2_dgrad(dy, w)), io + wb))
        items.append((f"convt_small_s2_wgrad {tag}", "kernel", (lambda x=x, dy=dy: ops.convt_small_s2_wgrad(x, dy)), io + wb))

    def timed(run, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n          # ms per call

    def eager(fn, n):
        def run():
            for _ in range(n):
                fn()
        return run

    def graphed(fn, n):
        """n back-to-back calls captured into one device graph: a replay has no per-call host work (allocation, ctypes, Python),
        which at ~10 us per call would otherwise hide a kernel of a few microseconds"""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                fn()
        return g.replay

    counts, runs = {}, {}
    with torch.no_grad():
        for name, group, fn, _ in items:             # warm-up: code objects, tap tables, allocator; then size the window
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            # the ConvResNet modules are dozens of launches of milliseconds in all: eager windows; everything else replays a graph
            make = eager if name.startswith("convolutional_res") else graphed
            one = timed(make(fn, 20), 20)
            n = counts[name] = int(min(2000, max(5, math.ceil(args.window_ms / max(one, 1e-4)))))
            runs[name] = make(fn, n)
            timed(runs[name], n)
        samples = {name: [] for name, *_ in items}
        for _ in range(args.repeats):
            for name, *_ in items:
                samples[name].append(timed(runs[name], counts[name]))
    rate, where = stream_rate_tb_s()
    rows = {"module": {}, "kernel": {}}
    for name, group, _, nbytes in items:
        ms = statistics.median(samples[name])
        gbs = nbytes / (ms * 1e-3) / 1e9
        rows[group][name] = {"us": round(ms * 1e3, 2), "us_min": round(min(samples[name]) * 1e3, 2), "us_max": round(max(samples[name]) * 1e3, 2),
                             "launches_per_window": counts[name], "algorithmic_bytes": nbytes, "GB_s": round(gbs, 1),
                             "fraction_of_stream_rate": round(gbs / (rate * 1e3), 4)}
    result = {"what": "tools/resampler_bench.py: median of %d alternating rounds, device events around windows of back-to-back calls replayed from "
                      "a device graph (the convolutional_res modules: eager); "
                      "module rows are a whole rescaled_downsample / rescaled_upsample (all launches, tanh included) and their bytes are "
                      "the image and the latent only; a kernel row's wgrad is its two launches" % args.repeats,
              "device": torch.cuda.get_device_name(0), "batch": B, "image": [C_IMG, SIZE, SIZE], "latent": LATENT,
              "stream_rate_TB_s": rate, "stream_rate_from": f"profiles/r02_dma_rate.txt: {where}", "modules": rows["module"], "kernels": rows["kernel"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for group in ("module", "kernel"):
        for name, r in rows[group].items():
            print(f"{name:44s} {r['us']:10.1f} us  {r['GB_s']:8.1f} GB/s  {100 * r['fraction_of_stream_rate']:5.1f} % of the stream rate")


if __name__ == "__main__":
    main()
