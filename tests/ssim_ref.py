"""PSNR and SSIM restated for the tests of ddk_image_metrics.

``ssim`` is the definition in float64 with the direct two-dimensional 11 x 11 window on the raw 0..255 values: not separable, not
shifted, so it shares no arithmetic with the kernel.  ``sq_err`` is numpy's integer arithmetic.  ``ssim_fp32`` is the kernel's
formula (separable, taps in index order, every product and sum rounded on its own, values shifted by ``shift``) in torch's fp32 on
the CPU: its distance from ``ssim`` on the test inputs is what fp32 costs, and sets the bar the kernel is held to.
``cases`` are those inputs: counter-based uint8 images (utils/synthetic.py), the same on every machine.
"""
import functools

import numpy as np
import torch

from utils import synthetic as syn

WIN, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def window_1d():
    g = np.exp(-((np.arange(WIN) - WIN // 2) ** 2) / (2.0 * SIGMA ** 2))
    return g / g.sum()


def window_2d():
    g = window_1d()
    return np.outer(g, g)


def ssim_map(a, b):
    """uint8 [N, H, W, C] x 2 -> float64 [N, H - 10, W - 10, C], one SSIM value per valid window and channel."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w2 = window_2d()
    view = lambda x: np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN), axis=(1, 2))      # [N, H-10, W-10, C, 11, 11]
    mean = lambda x: (view(x) * w2).sum(axis=(-1, -2))
    mu_a, mu_b = mean(a), mean(b)
    var_a, var_b, cov = mean(a * a) - mu_a ** 2, mean(b * b) - mu_b ** 2, mean(a * b) - mu_a * mu_b
    return ((2 * mu_a * mu_b + C1) * (2 * cov + C2)) / ((mu_a ** 2 + mu_b ** 2 + C1) * (var_a + var_b + C2))


def ssim(a, b):
    """float64 [N]: the mean over windows and channels."""
    return ssim_map(a, b).mean(axis=(1, 2, 3))


def sq_err(a, b, mask=None):
    """(sum (a - b)^2, element count) per image as Python-exact int64 [N]; mask [N, H, W]: pixels where it is nonzero, all channels."""
    d = np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)
    keep = np.ones(d.shape[:3], dtype=np.int64) if mask is None else (np.asarray(mask) != 0).astype(np.int64)
    return (d * d * keep[..., None]).sum(axis=(1, 2, 3)), keep.sum(axis=(1, 2)) * d.shape[3]


def psnr(a, b, mask=None):
    """float64 [N]: 10 log10(255^2 count / sum); inf for sum == 0, nan for count == 0."""
    s, k = sq_err(a, b, mask)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(255.0 ** 2 * k.astype(np.float64) / s.astype(np.float64))


def ssim_fp32(a, b, shift=128.0):
    """float32 [N]: the separable formula in fp32 on (value - shift), horizontal taps then vertical, no fused multiply-add."""
    w = torch.from_numpy(window_1d()).float()
    x, y = torch.tensor(np.asarray(a)).float() - shift, torch.tensor(np.asarray(b)).float() - shift

    def taps(m, dim):
        n = m.shape[dim] - (WIN - 1)
        acc = torch.zeros_like(m.narrow(dim, 0, n))
        for k in range(WIN):
            acc = acc + w[k] * m.narrow(dim, k, n)
        return acc

    mu_a, mu_b, ea2, eb2, eab = (taps(taps(m, 2), 1) for m in (x, y, x * x, y * y, x * y))
    var_a, var_b, cov = ea2 - mu_a * mu_a, eb2 - mu_b * mu_b, eab - mu_a * mu_b
    ma, mb = mu_a + shift, mu_b + shift
    c1, c2 = torch.tensor(C1).float(), torch.tensor(C2).float()
    val = ((2.0 * (ma * mb) + c1) * (2.0 * cov + c2)) / (((ma * ma + mb * mb) + c1) * ((var_a + var_b) + c2))
    return val.sum(dim=(1, 2, 3)) / float(val[0].numel())


# max |ssim_fp32 - ssim| over the cases below (SHAPES x PAIRS): what the kernel's formula costs in fp32, measured with torch on the
# CPU (test_restoration_metrics_cpu.py re-measures it).  The kernel is held to 4 x that: it may add in another, fixed, order.
# Without the shift by 128 the same formula is off by 6.68e-5, 560 x worse: on the flat 255 / 254 pair E[x^2] - mu^2 cancels
# 65025 against 65025.
SSIM_FP32_DEV = 1.20e-7
SSIM_FP32_DEV_UNSHIFTED = 6.68e-5
SSIM_BAR = 4 * SSIM_FP32_DEV


# ------------------------------------------------------------------ test inputs
# 11x11x1: one window; 12x13x3: odd, non-square, halo off by one; 16x16x4; 3 x 45x70x3: crosses the kernel's 32 x 32-window tile
# raggedly both ways (35 x 60 windows); 2 x 64x64x3: several tiles (54 x 54 windows)
SHAPES = [(1, 11, 11, 1), (1, 12, 13, 3), (1, 16, 16, 4), (3, 45, 70, 3), (2, 64, 64, 3)]
PAIRS = ["noise", "near", "flat", "same"]


def u8_image(shape, key):
    u = syn.uniform_pm1(int(np.prod(shape)), "metrics:" + key)
    return np.clip(np.floor((u + 1.0) * 128.0), 0, 255).astype(np.uint8).reshape(shape)


@functools.lru_cache(maxsize=None)
def pair(shape, kind):
    """(a, b) uint8 [N, H, W, C]: independent noise; a and a + noise of up to +-3 levels; flat 255 against flat 254 (E[x^2] - mu^2
    cancels completely, the worst case for fp32); identical images."""
    name = "x".join(map(str, shape))
    a = u8_image(shape, name + ".a")
    if kind == "noise":
        b = u8_image(shape, name + ".b")
    elif kind == "near":
        d = np.round(3.0 * syn.uniform_pm1(a.size, "metrics:" + name + ".d")).astype(np.int64).reshape(shape)
        b = np.clip(a.astype(np.int64) + d, 0, 255).astype(np.uint8)
    elif kind == "flat":
        a, b = np.full(shape, 255, np.uint8), np.full(shape, 254, np.uint8)
    elif kind == "same":
        b = a.copy()
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """float64 SSIM [N] of pair(shape, kind), computed once per process."""
    out = ssim(*pair(shape, kind))
    out.setflags(write=False)
    return out


def mask_for(shape, kind):
    """uint8 [N, H, W]: 'noise' ~half the pixels, 'none' all zero, 'one' a single pixel of the last image."""
    n, h, w, _ = shape
    if kind == "noise":
        return (syn.uniform_pm1(n * h * w, "metrics:mask." + "x".join(map(str, shape))) > 0).astype(np.uint8).reshape(n, h, w) * 7
    m = np.zeros((n, h, w), np.uint8)
    if kind == "one":
        m[n - 1, h - 2, w - 3] = 1
    return m
