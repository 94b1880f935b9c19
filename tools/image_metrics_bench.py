"""Time of one ddk_image_metrics call at 32 x 256 x 256 x 3, a cfg4 batch after the x3 decode, and at
32 x 64 x 64 x 3: device events around single calls (median of 30 after 5 warm-ups), 200 calls back to back behind one
synchronise, and ops.image_metrics with its copy of the results to the host.  Run from the repository root on the GPU box:
python tools/image_metrics_bench.py > profiles/image_metrics_bench.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]

import torch  # noqa: E402

from ddk import lib as L  # noqa: E402
from ddk import ops  # noqa: E402


def main():
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    lib = L.load()
    for shape in [(32, 256, 256, 3), (32, 64, 64, 3)]:
        a = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()
        b = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()
        n, h, w, c = shape
        nbytes = lib.ddk_image_metrics_workspace_bytes(n, h, w, c)
        ws = torch.empty(nbytes // 4 + 4, device="cuda")
        sq = torch.empty((n, 2), dtype=torch.int64, device="cuda")
        ssim = torch.empty(n, device="cuda")

        def call():
            L.check(lib.ddk_image_metrics(L.ptr(a), L.ptr(b), None, n, h, w, c, L.ptr(sq), L.ptr(ssim), L.ptr(ws), nbytes, L.stream()),
                    "image_metrics")

        ev = []
        for i in range(35):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= 5:
                ev.append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = []
        for i in range(15):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ops.image_metrics(a, b)
            host.append((time.perf_counter() - t) * 1e3)
        print(f"{shape}: events median {statistics.median(ev):.4f} ms min {min(ev):.4f} max {max(ev):.4f}; back-to-back "
              f"{(t1 - t0) / 200 * 1e3:.4f} ms/call; ops.image_metrics with host copy median {statistics.median(host[5:]):.4f} ms; "
              f"ssim[0] {float(ssim[0]):.6f} workspace {nbytes} B", flush=True)


if __name__ == "__main__":
    main()
