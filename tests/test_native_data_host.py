"""The host half of the image-batch entry under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU:
tests/host/data_walk.cpp, a stand-alone program linked with the `make asan` objects (csrc/host_sanitize.h), calls the band query and the
entry for every shape of the test list (tests/image_batch_ref.py SHAPES, C = 1 and 3) and the larger shapes the kernel must take, with
arenas of exactly the tensors' sizes; the launch's geometry and pointers are checked, and every argument error must come back before a
launch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downsampled-diffusion_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_image_batch_entry_under_asan_and_ubsan():
    build = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1)), "data_walk_asan"], capture_output=True, text=True,
                           timeout=1500)
    assert build.returncode == 0, (build.stdout + build.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([os.path.join(CSRC, "data_walk_asan")], capture_output=True, text=True, timeout=300, env=env)
    tail = (run.stdout + run.stderr)[-3000:]
    assert run.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("data walk: 25 launches,") and " 0 pointer/geometry errors, 0 failed expectations" in last, last
    rows = [ln for ln in run.stdout.splitlines() if "rows per group" in ln]
    assert len(rows) == 25
    bands = {tuple(int(v) for v in ln.replace("x", " ").replace("->", " ").split()[:4]): int(ln.split()[-2]) for ln in rows}
    assert bands[(218, 178, 3, 64)] >= 2 and bands[(64, 64, 3, 16)] >= 2
