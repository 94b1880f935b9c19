#!/usr/bin/env python3
"""A/B of two builds of the kernel library on the cfg4 reverse step (batch 32, graph replay), the way tools/fold_ab.py alternates a
plan option:  python tools/lib_ab.py A=path/to/libddk.so B=other/libddk.so [rounds]  -- ms per step, alternating, `rounds` (3) rounds
of 200 steps each, both libraries in this one process (same clocks, same allocator state).  ddk.lib binds one library per import
(DDK_LIB), so each arm imports the Python layer afresh: the project's modules are dropped from sys.modules between the two.
An arm whose library has other entry points than this tree's Python layer binds names its own tree: A=lib.so@path/to/that/checkout
(the Python layer, bench.py and the models are then imported from there)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]
import torch
ROOTS = {ROOT}


def load_arm(path):
    """model, plan and inputs on the library at `path`; returns run(k) = k graph-replayed reverse steps"""
    path, _, root = path.partition("@")
    root = os.path.abspath(root) if root else ROOT
    ROOTS.add(root)
    sys.path[:2] = [os.path.join(root, "downsampled-diffusion_amd"), root]
    os.environ["DDK_LIB"] = os.path.abspath(path)
    for k in [k for k, m in sys.modules.items() if any((getattr(m, "__file__", None) or "").startswith(r + os.sep) for r in ROOTS)]:
        del sys.modules[k]
    from bench import cfg4
    from ddk import lib, ops
    from models import DownsampleDDPM, Unet
    from utils import synthetic as syn
    assert lib.LIB_PATH == os.environ["DDK_LIB"]
    dev = torch.device("cuda", 0)
    cfg = cfg4()
    model = DownsampleDDPM(cfg, Unet(cfg), "cuda", 3)
    model.load_state_dict(syn.fill_state_dict(model.state_dict(), skip=syn.SCHEDULE_KEYS))
    model = model.to(dev).eval()
    plan = model.latent_model.plan()
    tables = model._tables()
    x = ops.randn((32, 32, 32, 8), dev, seed=1, step=1000, stream_id=0)
    return lambda k: plan.sample_nhwc(x, tables, 999, 1000 - k, seed=1, stream_id=0, use_graph=True)


arms = [a.split("=", 1) for a in sys.argv[1:3]]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
runs = [(name, path, load_arm(path)) for name, path in arms]
with torch.no_grad():
    for name, path, run in runs:    # untimed: graphs captured, the shader clock settled under the step's load (bench.py: settle_clock)
        run(200)
    for rnd in range(rounds):
        for name, path, run in runs:
            run(40)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(200)
            torch.cuda.synchronize()
            print(f"round {rnd} {name} ({path}): {(time.perf_counter() - t0) / 200 * 1e3:.4f} ms per step", flush=True)
