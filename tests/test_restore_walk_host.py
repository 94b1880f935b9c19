"""The host half of the block restore entries (ddk_sampler_run_restore, _masked, _multistep, _noisy, _gray) and of the separable ones
(ddk_sampler_run_restore_blur, _sep) under AddressSanitizer + UndefinedBehaviorSanitizer on a machine without a GPU:
tests/host/restore_walk.cpp, a stand-alone program linked with the `make asan` objects (csrc/host_sanitize.h), walks a three-step
eager chain of each entry with arenas of exactly the sizes the size queries return (a workspace 16 bytes short and the plain sampler's
included); every launch's geometry and pointers are checked, and every argument error must come back before a launch.

SIZES is what every sampler size query returned for the walk's shapes before the plane-wide kinds' host path was written once (the
block kinds: one value per n of 1, 2, 4, 3): the layouts behind the queries may be rewritten, the bytes they add up to may not move."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downsampled-diffusion_amd", "csrc")

SIZES = """\
sampler_workspace_bytes 3x16x16 b2 t_start=2: 1963088
sampler_multistep_workspace_bytes 3x16x16 b2 t_start=2: 1969232
sampler_inpaint_workspace_bytes 3x16x16 b2 t_start=2: 1975376
sampler_restore_workspace_bytes 3x16x16 b2 t_start=2: 1964624
sampler_restore_masked_workspace_bytes 3x16x16 b2 t_start=2 n=1,2,4,3: 1971280 1965136 1964624 0
sampler_restore_multistep_workspace_bytes 3x16x16 b2 t_start=2 n=1,2,4,3: 1977424 1971280 1969744 0
sampler_restore_noisy_workspace_bytes 3x16x16 b2 t_start=2 n=1,2,4,3: 1971280 1965136 1964624 0
sampler_restore_gray_workspace_bytes 3x16x16 b2 t_start=2 n=1,2,4,3: 1971280 1965136 1964624 0
sampler_restore_blur_workspace_bytes 3x16x16 b2 t_start=2: 1977424
sampler_restore_cs_workspace_bytes 3x16x16 b2 t_start=2: 1976400
sampler_restore_fft_workspace_bytes 3x16x16 b2 t_start=2: 1982608
sampler_restore_fft_noisy_workspace_bytes 3x16x16 b2 t_start=2: 1995936
sampler_restore_tail_parts 3x16x16 b2 n=1,2,4,3: 0 0 0 0
sampler_restore_masked_tail_parts 3x16x16 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_multistep_tail_parts 3x16x16 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_noisy_tail_parts 3x16x16 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_gray_tail_parts 3x16x16 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_blur_tail_parts 3x16x16 b2: 0
sampler_restore_cs_tail_parts 3x16x16 b2: 0
sampler_restore_fft_tail_parts 3x16x16 b2: 0
sampler_restore_fft_noisy_tail_parts 3x16x16 b2: 0
sampler_workspace_bytes 3x16x16 b2 t_start=999: 5671920
sampler_multistep_workspace_bytes 3x16x16 b2 t_start=999: 5678064
sampler_inpaint_workspace_bytes 3x16x16 b2 t_start=999: 5684208
sampler_restore_workspace_bytes 3x16x16 b2 t_start=999: 5673456
sampler_restore_masked_workspace_bytes 3x16x16 b2 t_start=999 n=1,2,4,3: 5680112 5673968 5673456 0
sampler_restore_multistep_workspace_bytes 3x16x16 b2 t_start=999 n=1,2,4,3: 5686256 5680112 5678576 0
sampler_restore_noisy_workspace_bytes 3x16x16 b2 t_start=999 n=1,2,4,3: 5680112 5673968 5673456 0
sampler_restore_gray_workspace_bytes 3x16x16 b2 t_start=999 n=1,2,4,3: 5680112 5673968 5673456 0
sampler_restore_blur_workspace_bytes 3x16x16 b2 t_start=999: 5686256
sampler_restore_cs_workspace_bytes 3x16x16 b2 t_start=999: 5685232
sampler_restore_fft_workspace_bytes 3x16x16 b2 t_start=999: 5691440
sampler_restore_fft_noisy_workspace_bytes 3x16x16 b2 t_start=999: 5708752
sampler_workspace_bytes 3x80x80 b2 t_start=2: 45742416
sampler_multistep_workspace_bytes 3x80x80 b2 t_start=2: 45896016
sampler_inpaint_workspace_bytes 3x80x80 b2 t_start=2: 46049616
sampler_restore_workspace_bytes 3x80x80 b2 t_start=2: 45780816
sampler_restore_masked_workspace_bytes 3x80x80 b2 t_start=2 n=1,2,4,3: 45947216 45793616 45780816 0
sampler_restore_multistep_workspace_bytes 3x80x80 b2 t_start=2 n=1,2,4,3: 46100816 45947216 45908816 0
sampler_restore_noisy_workspace_bytes 3x80x80 b2 t_start=2 n=1,2,4,3: 45947216 45793616 45780816 0
sampler_restore_gray_workspace_bytes 3x80x80 b2 t_start=2 n=1,2,4,3: 45947216 45793616 45780816 0
sampler_restore_blur_workspace_bytes 3x80x80 b2 t_start=2: 46100816
sampler_restore_cs_workspace_bytes 3x80x80 b2 t_start=2: 0
sampler_restore_fft_workspace_bytes 3x80x80 b2 t_start=2: 0
sampler_restore_fft_noisy_workspace_bytes 3x80x80 b2 t_start=2: 0
sampler_restore_tail_parts 3x80x80 b2 n=1,2,4,3: 0 0 0 0
sampler_restore_masked_tail_parts 3x80x80 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_multistep_tail_parts 3x80x80 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_noisy_tail_parts 3x80x80 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_gray_tail_parts 3x80x80 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_blur_tail_parts 3x80x80 b2: 0
sampler_restore_cs_tail_parts 3x80x80 b2: 0
sampler_restore_fft_tail_parts 3x80x80 b2: 0
sampler_restore_fft_noisy_tail_parts 3x80x80 b2: 0
sampler_workspace_bytes 3x256x256 b1 t_start=2: 224485376
sampler_multistep_workspace_bytes 3x256x256 b1 t_start=2: 225271808
sampler_inpaint_workspace_bytes 3x256x256 b1 t_start=2: 226058240
sampler_restore_workspace_bytes 3x256x256 b1 t_start=2: 224681984
sampler_restore_masked_workspace_bytes 3x256x256 b1 t_start=2 n=1,2,4,3: 225533952 224747520 224681984 0
sampler_restore_multistep_workspace_bytes 3x256x256 b1 t_start=2 n=1,2,4,3: 226320384 225533952 225337344 0
sampler_restore_noisy_workspace_bytes 3x256x256 b1 t_start=2 n=1,2,4,3: 225533952 224747520 224681984 0
sampler_restore_gray_workspace_bytes 3x256x256 b1 t_start=2 n=1,2,4,3: 225533952 224747520 224681984 0
sampler_restore_blur_workspace_bytes 3x256x256 b1 t_start=2: 226582528
sampler_restore_cs_workspace_bytes 3x256x256 b1 t_start=2: 226320384
sampler_restore_fft_workspace_bytes 3x256x256 b1 t_start=2: 227107840
sampler_restore_fft_noisy_workspace_bytes 3x256x256 b1 t_start=2: 230515728
sampler_restore_tail_parts 3x256x256 b1 n=1,2,4,3: 0 0 0 0
sampler_restore_masked_tail_parts 3x256x256 b1 n=1,2,4,3: 0 0 0 -1
sampler_restore_multistep_tail_parts 3x256x256 b1 n=1,2,4,3: 0 0 0 -1
sampler_restore_noisy_tail_parts 3x256x256 b1 n=1,2,4,3: 0 0 0 -1
sampler_restore_gray_tail_parts 3x256x256 b1 n=1,2,4,3: 0 0 0 -1
sampler_restore_blur_tail_parts 3x256x256 b1: 0
sampler_restore_cs_tail_parts 3x256x256 b1: 0
sampler_restore_fft_tail_parts 3x256x256 b1: 0
sampler_restore_fft_noisy_tail_parts 3x256x256 b1: 0
sampler_workspace_bytes 3x16x48 b2 t_start=2: 5545040
sampler_multistep_workspace_bytes 3x16x48 b2 t_start=2: 5563472
sampler_inpaint_workspace_bytes 3x16x48 b2 t_start=2: 5581904
sampler_restore_workspace_bytes 3x16x48 b2 t_start=2: 5549648
sampler_restore_masked_workspace_bytes 3x16x48 b2 t_start=2 n=1,2,4,3: 5569616 5551184 5549648 0
sampler_restore_multistep_workspace_bytes 3x16x48 b2 t_start=2 n=1,2,4,3: 5588048 5569616 5565008 0
sampler_restore_noisy_workspace_bytes 3x16x48 b2 t_start=2 n=1,2,4,3: 5569616 5551184 5549648 0
sampler_restore_gray_workspace_bytes 3x16x48 b2 t_start=2 n=1,2,4,3: 5569616 5551184 5549648 0
sampler_restore_blur_workspace_bytes 3x16x48 b2 t_start=2: 5592144
sampler_restore_cs_workspace_bytes 3x16x48 b2 t_start=2: 0
sampler_restore_fft_workspace_bytes 3x16x48 b2 t_start=2: 0
sampler_restore_fft_noisy_workspace_bytes 3x16x48 b2 t_start=2: 0
sampler_restore_tail_parts 3x16x48 b2 n=1,2,4,3: 0 0 0 0
sampler_restore_masked_tail_parts 3x16x48 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_multistep_tail_parts 3x16x48 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_noisy_tail_parts 3x16x48 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_gray_tail_parts 3x16x48 b2 n=1,2,4,3: 0 0 0 -1
sampler_restore_blur_tail_parts 3x16x48 b2: 0
sampler_restore_cs_tail_parts 3x16x48 b2: 0
sampler_restore_fft_tail_parts 3x16x48 b2: 0
sampler_restore_fft_noisy_tail_parts 3x16x48 b2: 0
"""

# the chains walked, in the walk's order (their launch counts are printed, not pinned: a fused kernel may lower them)
CHAINS = [
    "restore_masked, 3x16x16 b2 n=1 masked",
    "restore_multistep, 3x16x16 b2 n=1 masked",
    "restore_noisy, 3x16x16 b2 n=1 masked",
    "restore_gray, 3x16x16 b2 n=1 masked",
    "restore, 3x16x16 b2 n=2",
    "restore_masked, 3x16x16 b2 n=2",
    "restore_multistep, 3x16x16 b2 n=2",
    "restore_noisy, 3x16x16 b2 n=2",
    "restore_gray, 3x16x16 b2 n=2",
    "restore_blur, 3x16x16 b2",
    "restore_sep, 3x16x16 b2 from 8x12",
    "restore_blur, 3x80x80 b2",
]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_restore_entries_under_asan_and_ubsan():
    build = subprocess.run(["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1)), "restore_walk_asan"], capture_output=True, text=True,
                           timeout=1500)
    assert build.returncode == 0, (build.stdout + build.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([os.path.join(CSRC, "restore_walk_asan")], capture_output=True, text=True, timeout=300, env=env)
    tail = (run.stdout + run.stderr)[-3000:]
    assert run.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
    out = run.stdout.strip().splitlines()
    assert out[-1].startswith("restore walk:") and " 0 pointer/geometry errors, 0 failed expectations" in out[-1], out[-1]
    chains = [ln.split("  ")[0] for ln in out if "launches per three-step chain" in ln]
    assert chains == CHAINS, chains
    sizes = [ln[5:] for ln in out if ln.startswith("size ")]
    want = SIZES.splitlines()
    assert len(sizes) == len(want)
    wrong = [(got, exp) for got, exp in zip(sizes, want) if got != exp]
    assert not wrong, wrong[:5]
