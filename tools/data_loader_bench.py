#!/usr/bin/env python3
"""What a batch of the native input pipeline costs -> profiles/native_data_bench.json.

  kernel   time per ddk_image_batch launch, device events over >= 200 launches after a warm-up, for 218x178x3 -> 64 (B = 128),
           32x32x3 -> 32 (B = 128), 256^2x3 -> 256 (B = 16) and 1024^2x3 -> 256 (B = 16); the bytes the transform needs (every source
           byte once, every output float once) over that time, as a share of the 8.0 TB/s HBM peak.  The arrays hold 4 x B images, so a
           case's working set (7 - 200 MB) can sit in the 256 MiB Infinity Cache: the share says how close the launch is to the time the
           HBM would need, it is not a measured HBM rate;
  loaders  images/s of the synthetic DataLoader path (SyntheticImages, 4 workers, pinned; host to device copy included) and of
           NativeImageLoader at the same batch sizes;
  step     the optimiser step of tools/train_bench.py's CelebA-64 configuration (dDDPM x2, 2 x 64 images, merged graph replay) fed by
           each loader, alternating in one process.

GPU-box tool: python tools/data_loader_bench.py [--out profiles/native_data_bench.json] [--skip_step]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]
import numpy as np
import torch

from ddk import ops
from utils.data import NativeImageLoader, get_dataloader
from utils.image_batch import Transform

DEV = "cuda"
HBM_PEAK = 8.0e12
CASES = [(218, 178, 3, 64, 128), (32, 32, 3, 32, 128), (256, 256, 3, 256, 16), (1024, 1024, 3, 256, 16)]


def kernel_case(hs, ws, c, s, b, launches=200, warmup=20):
    g = torch.Generator().manual_seed(hs * 31 + s)
    images = torch.randint(0, 256, (4 * b, hs, ws, c), dtype=torch.uint8, generator=g).to(DEV)
    tf = Transform(hs, ws, s)
    tables = tuple(torch.from_numpy(t).to(DEV) for t in (tf.row_start, tf.row_w, tf.col_start, tf.col_w))
    index = [torch.randperm(4 * b, generator=g)[:b].to(DEV) for _ in range(4)]
    for k in range(warmup):
        ops.image_batch(images, index[k % 4], tables, s, True, 1, k)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(launches):
        out = ops.image_batch(images, index[k % 4], tables, s, True, 1, k)
    stop.record()
    torch.cuda.synchronize()
    us = start.elapsed_time(stop) * 1e3 / launches
    nbytes = b * hs * ws * c + b * c * s * s * 4
    r = ops.image_batch_rows_per_group(hs, ws, c, s, tf.row_taps, tf.col_taps)
    return {"case": f"{hs}x{ws}x{c} -> {s}, B = {b}", "us_per_batch": round(us, 2), "images_per_s": round(b / us * 1e6),
            "bytes_read_and_written": nbytes, "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4), "launches": launches,
            "taps": [tf.row_taps, tf.col_taps], "rows_per_group": r, "workgroups": -(-s // r) * b, "finite": bool(torch.isfinite(out).all())}


def loader_rate(loader, batches):
    it = iter(loader)
    next(it)[0].to(DEV)                                   # workers started, first batch through
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    for _ in range(batches):
        n += next(it)[0].to(DEV, non_blocking=True).shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def loaders(tmp):
    rows = []
    for size, bs, shape in ((64, 128, (218, 178)), (32, 128, (32, 32)), (256, 16, (256, 256))):
        cfg = dict(dataset="celeba", image_size=size, batch_size=bs)
        synthetic = get_dataloader(dict(cfg), "cuda", True, os.path.join(tmp, "none"))[0]
        path = os.path.join(tmp, f"bench_{size}.npy")
        np.save(path, np.random.default_rng(size).integers(0, 256, (8 * bs,) + shape + (3,), dtype=np.uint8))
        native = get_dataloader(dict(cfg, data_file=path, rnd_flip=True), "cuda", True, os.path.join(tmp, "none"))[0]
        assert isinstance(native, NativeImageLoader)
        from trainers.train_helpers import cycle
        rows.append({"case": f"{shape[0]}x{shape[1]}x3 -> {size}, B = {bs}",
                     "synthetic_dataloader_images_per_s": round(loader_rate(synthetic, 20)),
                     "native_loader_images_per_s": round(loader_rate(cycle(native), 400))})
        print(rows[-1], flush=True)
    return rows


def step_times(tmp, rounds=3, steps=10):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from train_bench import cfg as bench_cfg
    from models import DownsampleDDPMAutoencoder, Unet
    from trainers.graph_step import GraphedAccumulation
    from trainers.optim import FusedAdam
    from trainers.train_helpers import cycle
    from utils import synthetic as syn
    c = bench_cfg(128, 8, 64, down=2)
    model = DownsampleDDPMAutoencoder(c, Unet(c), DEV, 3).to(DEV).train()
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    opt = FusedAdam(model, lr=2e-4)
    cfg = dict(dataset="celeba", image_size=64, batch_size=64)
    path = os.path.join(tmp, "celeba64.npy")
    np.save(path, np.random.default_rng(0).integers(0, 256, (2048, 218, 178, 3), dtype=np.uint8))
    feeds = {"synthetic_dataloader": cycle(get_dataloader(dict(cfg), "cuda", True, os.path.join(tmp, "none"))[0]),
             "native_loader": cycle(get_dataloader(dict(cfg, data_file=path, rnd_flip=True), "cuda", True, os.path.join(tmp, "none"))[0])}
    graph = GraphedAccumulation(model, 1)
    graph.capture([torch.cat([next(feeds["native_loader"])[0] for _ in range(2)])])
    opt.zero_grad()

    def step(feed):
        x = torch.cat([next(feed)[0].to(DEV, non_blocking=True) for _ in range(2)])
        rows = graph.replay([x])
        opt.step(); opt.zero_grad()
        for m in model.modules():
            if hasattr(m, "invalidate_plan"):
                m.invalidate_plan()
        return rows

    ms = {k: [] for k in feeds}
    for name, feed in feeds.items():
        for _ in range(3):
            step(feed)
    for _ in range(rounds):
        for name, feed in feeds.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(steps):
                rows = step(feed)
            torch.cuda.synchronize()
            ms[name].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
    return {"configuration": "dDDPM x2 64x64, 2 x 64 images per optimiser step, one merged pass replayed as a device graph",
            "ms_per_step": ms, "objective_finite": bool(torch.isfinite(rows).all())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_data_bench.json"))
    ap.add_argument("--skip_step", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "kernel": []}
    for case in CASES:
        res["kernel"].append(kernel_case(*case))
        print(res["kernel"][-1], flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        res["loaders"] = loaders(tmp)
        if not a.skip_step:
            res["step"] = step_times(tmp)
            print(res["step"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")
