"""Time of precision / recall (utils.sample_metrics.compute_prec_recall) at N = 10 000 and N = 50 000 rows
of D = 2048 synthetic non-negative features per set: the three distance passes (radii of both sets, membership) on resident device
tensors between device events (warm-up first, several repetitions, the shader clock probed over the timed region), the whole call
from host arrays with a host clock behind a synchronise, and the numpy float32 path at N = 10 000 on the threads the environment
gives.  Achieved rate = 3 x 2 N^2 D FLOP over the event time, against the fp32 MFMA peak of 256 CUs x 4 SIMDs x 64 FLOP/clk at the
nominal 2.4 GHz (157.3 TFLOP/s) and at the measured clock.  Run from the repository root on the GPU box:
python tools/sample_metrics_bench.py [--out profiles/sample_metrics_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "downsampled-diffusion_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ddk import ops  # noqa: E402
from utils.sample_metrics import compute_prec_recall  # noqa: E402

D = 2048
NOMINAL_PEAK = 256 * 4 * 64 * 2.4e9


def features(seed, n, shift):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D), dtype=np.float32)
    x *= np.float32(0.5)
    x += np.float32(0.3 + shift)
    return np.maximum(x, np.float32(0.0), out=x)


def three_passes(a, b, k=3):
    return ops.manifold_members(a, ops.manifold_radii(a, k), b, ops.manifold_radii(b, k))


def bench(n, warmup, reps):
    ref, smp = features(1, n, 0.0), features(2, n, 0.05)
    a, b = torch.from_numpy(ref).cuda(), torch.from_numpy(smp).cuda()
    for _ in range(warmup):
        three_passes(a, b)
    torch.cuda.synchronize()
    probe = ops.ClockProbe("cuda")
    ms = []
    probe.probe()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ref_in, smp_in = three_passes(a, b)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    probe.probe()
    torch.cuda.synchronize()
    ghz = probe.ghz()
    med = statistics.median(ms)
    flop = 3 * 2.0 * n * n * D
    whole = []
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pr = compute_prec_recall(ref, smp, use_gpu=True)
        whole.append((time.perf_counter() - t) * 1e3)
    rec = dict(N=n, D=D, k=3, warmup=warmup, reps=reps, device_ms=[round(v, 3) for v in ms], device_ms_median=round(med, 3),
               flop=flop, tflops=round(flop / med * 1e-9, 2), fraction_of_nominal_peak=round(flop / (med * 1e-3) / NOMINAL_PEAK, 4),
               shader_clock_ghz=None if ghz is None else round(ghz, 3),
               fraction_of_peak_at_measured_clock=None if ghz is None else round(flop / (med * 1e-3) / (NOMINAL_PEAK * ghz / 2.4), 4),
               radii_column_splits=ops.manifold_radii_splits(n), whole_call_from_host_ms=[round(v, 1) for v in whole],
               precision=pr[0], recall=pr[1])
    print(json.dumps(rec), flush=True)
    return rec, ref, smp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_metrics_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the HIP kernels: it needs a ROCm device"
    torch.cuda.set_device(0)
    result = dict(what="precision / recall: radii(ref), radii(sample), members(ref, sample); synthetic max(0.5 N(0,1) + 0.3 (+ 0.05), 0) features",
                  device=torch.cuda.get_device_name(0), nominal_fp32_mfma_peak_tflops=round(NOMINAL_PEAK * 1e-12, 1), cases=[])
    small, ref, smp = bench(10000, 2, 7)
    t = time.perf_counter()
    host_pr = compute_prec_recall(ref, smp, use_gpu=False)
    host_s = time.perf_counter() - t
    result["cases"].append(small)
    result["numpy_path_N10000"] = dict(seconds=round(host_s, 2), threads_env=os.environ.get("OMP_NUM_THREADS"), cpus_allowed=len(os.sched_getaffinity(0)),
                                       precision=host_pr[0], recall=host_pr[1], equals_kernels=list(host_pr) == [small["precision"], small["recall"]])
    print(json.dumps(result["numpy_path_N10000"]), flush=True)
    del ref, smp
    result["cases"].append(bench(50000, 1, 5)[0])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
