"""The host half of the noisy deconvolution entries under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU:
tests/host/fft_noisy_walk.cpp, a stand-alone program linked with the `make asan` objects (csrc/host_sanitize.h), calls the spectrum of
A+ y, the lone step and a three-step eager chain of the new kind, in the plane form and in the multi-launch form, with arenas of
exactly the sizes the size queries return (a short workspace included); every launch's geometry and pointers are checked, and every
argument error must come back before a launch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downsampled-diffusion_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_fft_noisy_entries_under_asan_and_ubsan():
    build = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1)), "fft_noisy_walk_asan"], capture_output=True, text=True,
                           timeout=1500)
    assert build.returncode == 0, (build.stdout + build.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([os.path.join(CSRC, "fft_noisy_walk_asan")], capture_output=True, text=True, timeout=300, env=env)
    tail = (run.stdout + run.stderr)[-3000:]
    assert run.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("fft noisy walk:") and " 0 pointer/geometry errors, 0 failed expectations" in last, last
    chains = [ln for ln in run.stdout.splitlines() if "launches per three-step chain" in ln]
    assert len(chains) == 3 and "multi-launch form" in chains[2]
