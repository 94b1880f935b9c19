"""The host half of ddk_poly_mmd_sums / ddk_manifold_ball_counts under AddressSanitizer + UndefinedBehaviorSanitizer on a machine
without a GPU: tests/host/mmd_walk.cpp, a stand-alone program linked with the `make asan` objects (csrc/host_sanitize.h), calls both
entries over the shapes of test_sample_metrics_ext_gpu.py and the sizes of a real evaluation (one segment of 50 000 rows, a hundred
of a thousand, 65 536 of two) with arenas of exactly the sizes the size queries return; every launch's geometry, pointers and tensor
extents are checked, and every argument error must come back before a launch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downsampled-diffusion_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_mmd_and_ball_count_entries_under_asan_and_ubsan():
    build = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1)), "mmd_walk_asan"], capture_output=True, text=True,
                           timeout=1500)
    assert build.returncode == 0, (build.stdout + build.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([os.path.join(CSRC, "mmd_walk_asan")], capture_output=True, text=True, timeout=300, env=env)
    tail = (run.stdout + run.stderr)[-3000:]
    assert run.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("mmd walk:") and " 0 pointer/geometry errors, 0 failed expectations" in last, last
    assert int(last.split()[2]) == 2 * 10 + 3 * 7           # two launches per accepted sums call, three per ball-count call
