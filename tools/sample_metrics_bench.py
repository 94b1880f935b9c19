"""Time of precision / recall (utils.sample_metrics.compute_prec_recall) at N = 10 000 and N = 50 000 rows
of D = 2048 synthetic non-negative features per set: the three distance passes (radii of both sets, membership) on resident device
tensors between device events (warm-up first, several repetitions, the shader clock probed over the timed region), the whole call
from host arrays with a host clock behind a synchronise, and the numpy float32 path at N = 10 000 on the threads the environment
gives.  Achieved rate = 3 x 2 N^2 D FLOP over the event time, against the fp32 MFMA peak of 256 CUs x 4 SIMDs x 64 FLOP/clk at the
nominal 2.4 GHz (157.3 TFLOP/s) and at the measured clock.  Run from the repository root on the GPU box:
python tools/sample_metrics_bench.py [--out profiles/sample_metrics_bench.json]

With --ext: the three passes again, and in the same process on the same tensors ops.poly_mmd_sums as one
segment, ops.manifold_ball_counts alone and with its radii pass, at N = 10 000 and 50 000; and the hundred subsets of a thousand rows
of KID's conventional form.  Written to profiles/sample_metrics_ext_bench.json (--ext_out)."""
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


def timed(fn, warmup, reps):
    """median and all device-event times of fn() in ms, and the shader clock over the timed region"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    probe = ops.ClockProbe("cuda")
    ms = []
    probe.probe()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    probe.probe()
    torch.cuda.synchronize()
    return statistics.median(ms), ms, probe.ghz()


def rate(flop, med, ghz):
    return dict(flop=flop, tflops=round(flop / med * 1e-9, 2), fraction_of_nominal_peak=round(flop / (med * 1e-3) / NOMINAL_PEAK, 4),
                shader_clock_ghz=None if ghz is None else round(ghz, 3),
                fraction_of_peak_at_measured_clock=None if ghz is None else round(flop / (med * 1e-3) / (NOMINAL_PEAK * ghz / 2.4), 4))


def bench(n, warmup, reps):
    ref, smp = features(1, n, 0.0), features(2, n, 0.05)
    a, b = torch.from_numpy(ref).cuda(), torch.from_numpy(smp).cuda()
    med, ms, ghz = timed(lambda: three_passes(a, b), warmup, reps)
    whole = []
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pr = compute_prec_recall(ref, smp, use_gpu=True)
        whole.append((time.perf_counter() - t) * 1e3)
    rec = dict(N=n, D=D, k=3, warmup=warmup, reps=reps, device_ms=[round(v, 3) for v in ms], device_ms_median=round(med, 3),
               **rate(3 * 2.0 * n * n * D, med, ghz), radii_column_splits=ops.manifold_radii_splits(n),
               whole_call_from_host_ms=[round(v, 1) for v in whole], precision=pr[0], recall=pr[1])
    print(json.dumps(rec), flush=True)
    return rec, ref, smp


def bench_ext(n, warmup, reps):
    """KID's sums and the ball counts beside precision / recall's three passes on the same resident tensors, one after the other"""
    a, b = torch.from_numpy(features(1, n, 0.0)).cuda(), torch.from_numpy(features(2, n, 0.05)).cuda()
    rec = dict(N=n, D=D, warmup=warmup, reps=reps)
    med_pr, ms, ghz = timed(lambda: three_passes(a, b), warmup, reps)
    rec["prec_recall_three_passes"] = dict(device_ms=[round(v, 3) for v in ms], device_ms_median=round(med_pr, 3), **rate(3 * 2.0 * n * n * D, med_pr, ghz))
    med, ms, ghz = timed(lambda: ops.poly_mmd_sums(a, b), warmup, reps)
    tiles = -(-n // ops.MANIFOLD_TILE)
    executed = (tiles * (tiles + 1) + tiles * tiles) * 2.0 * ops.MANIFOLD_TILE ** 2 * D       # upper triangles of the symmetric matrices
    rec["poly_mmd_sums_one_segment"] = dict(device_ms=[round(v, 3) for v in ms], device_ms_median=round(med, 3),
                                            ratio_to_prec_recall=round(med / med_pr, 3), tiles_executed=tiles * (tiles + 1) + tiles * tiles,
                                            nominal=rate(3 * 2.0 * n * n * D, med, ghz), executed=rate(executed, med, ghz))
    radii = ops.manifold_radii(a, 5)
    med, ms, ghz = timed(lambda: ops.manifold_ball_counts(a, radii, b), warmup, reps)
    rec["manifold_ball_counts"] = dict(k=5, device_ms=[round(v, 3) for v in ms], device_ms_median=round(med, 3),
                                       ratio_to_prec_recall=round(med / med_pr, 3), **rate(2.0 * n * n * D, med, ghz))
    med, ms, ghz = timed(lambda: ops.manifold_ball_counts(a, ops.manifold_radii(a, 5), b), warmup, reps)
    rec["density_coverage_two_passes"] = dict(k=5, device_ms=[round(v, 3) for v in ms], device_ms_median=round(med, 3),
                                              ratio_to_prec_recall=round(med / med_pr, 3), **rate(2 * 2.0 * n * n * D, med, ghz))
    print(json.dumps(rec), flush=True)
    return rec, a, b


def bench_subsets(a, b, subsets, m, warmup, reps):
    """the conventional KID form: `subsets` segments of m rows a side, gathered on the device (the gather is timed apart)"""
    from utils.sample_metrics import kid_subset_indices
    ri, si = kid_subset_indices(a.shape[0], b.shape[0], subsets, m, 0)
    ia, ib = torch.from_numpy(ri.reshape(-1)).cuda(), torch.from_numpy(si.reshape(-1)).cuda()
    med_g, ms_g, _ = timed(lambda: (a.index_select(0, ia), b.index_select(0, ib)), warmup, reps)
    ga, gb = a.index_select(0, ia), b.index_select(0, ib)
    med, ms, ghz = timed(lambda: ops.poly_mmd_sums(ga, gb, subsets), warmup, reps)
    tiles = -(-m // ops.MANIFOLD_TILE)
    executed = subsets * (tiles * (tiles + 1) + tiles * tiles) * 2.0 * ops.MANIFOLD_TILE ** 2 * D
    rec = dict(subsets=subsets, subset_size=m, D=D, rows_drawn_from=int(a.shape[0]), gather_ms_median=round(med_g, 3),
               device_ms=[round(v, 3) for v in ms], device_ms_median=round(med, 3), tiles_executed=subsets * (tiles * (tiles + 1) + tiles * tiles),
               nominal=rate(subsets * 3 * 2.0 * m * m * D, med, ghz), executed=rate(executed, med, ghz))
    print(json.dumps(rec), flush=True)
    return rec


def main_ext(out):
    result = dict(what="KID sums (ops.poly_mmd_sums) and ball counts (ops.manifold_ball_counts) beside precision / recall's three passes, "
                       "one process, the same resident tensors; synthetic max(0.5 N(0,1) + 0.3 (+ 0.05), 0) features; `nominal` counts "
                       "3 x 2 N^2 D FLOP, `executed` the tiles the launch runs (upper triangles of the two symmetric matrices, whole 128 x 128 tiles)",
                  device=torch.cuda.get_device_name(0), nominal_fp32_mfma_peak_tflops=round(NOMINAL_PEAK * 1e-12, 1), cases=[])
    small, a, b = bench_ext(10000, 2, 7)
    result["cases"].append(small)
    result["kid_100_subsets_of_1000"] = bench_subsets(a, b, 100, 1000, 1, 5)
    del a, b
    result["cases"].append(bench_ext(50000, 1, 3)[0])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_metrics_bench.json"))
    ap.add_argument("--ext", action="store_true", help="time KID's sums and the ball counts beside the three passes instead (DESIGN.md 3.20)")
    ap.add_argument("--ext_out", default=os.path.join(ROOT, "profiles", "sample_metrics_ext_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the HIP kernels: it needs a ROCm device"
    torch.cuda.set_device(0)
    if args.ext:
        return main_ext(args.ext_out)
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
