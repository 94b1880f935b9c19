"""Diffusion Posterior Sampling (Chung, Kim, Mccann, Klasky, Ye, ICLR 2023): the measurement operators of
DDPM.restore_guided / DownsampleDDPM.restore_guided and the context their chains run in.

An Operator describes y = phi(A x) on NHWC images [B, H, W, C]:
  kind "mean":       A = mask o (n x n block mean), n in {1, 2, 4, 8} (n = 1: plain or masked pixels)
  kind "separable":  A(X) = mask o (A_h X A_w^T) per channel, A_h [h, H], A_w [w, W]
  kind "psf":        A = mask o (circular convolution with a point-spread function, correlation form as psf.psf_spectrum)
and phi the pointwise response: "linear" (phi(u) = u) or "saturate" (phi(u) = clamp(gain u, -1, 1), an over-exposed sensor).
The arrays are kept in float64 as given (what a reference implementation reads) and placed on a device as fp32 at the first use there.
Every transform of the chain's step is a HIP launch (ddk.ops); only measure(), which simulates a sensor for the tools, clamps in torch.
"""
import contextlib

import numpy as np
import torch

from ddk import ops
from . import blur, psf as psf_mod

KINDS = ("mean", "separable", "psf")
RESPONSES = ("linear", "saturate")


class Operator:
    """kind, n, mask [B, h, w] ({0, 1} floats) or None, the matrices A_h / A_w or the spectrum K (numpy float64 / complex128), response
    and gain; in_shape (C, H, W) of the image and out_shape (C, h, w) of the measurement."""

    def __init__(self, kind, in_shape, *, n=1, A_h=None, A_w=None, K=None, mask=None, response="linear", gain=1.0):
        if kind not in KINDS:
            raise ValueError(f"Operator: kind must be one of {KINDS}, got {kind!r}")
        if response not in RESPONSES:
            raise ValueError(f"Operator: response must be one of {RESPONSES}, got {response!r}")
        if isinstance(gain, bool) or not isinstance(gain, (int, float, np.integer, np.floating)) or not np.isfinite(gain) or gain <= 0:
            raise ValueError(f"Operator: gain must be a finite real number > 0, got {gain!r}")
        C, H, W = (int(v) for v in in_shape)
        self.kind, self.response, self.gain = kind, response, float(gain)
        self.in_shape = (C, H, W)
        self.n = 1
        self.A_h = self.A_w = self.K = None
        if kind == "mean":
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n not in ops.MEASURE_BLOCKS:
                raise ValueError(f"Operator: the block n must be an int in {ops.MEASURE_BLOCKS}, got {n!r}")
            if H % n or W % n:
                raise ValueError(f"Operator: n = {n} must divide the image size {H} x {W}")
            self.n = int(n)
            self.out_shape = (C, H // self.n, W // self.n)
        elif kind == "separable":
            mats = []
            for what, A, side in (("A_h", A_h, H), ("A_w", A_w, W)):
                if torch.is_tensor(A):
                    A = A.detach().cpu().numpy()
                try:
                    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
                except (TypeError, ValueError):
                    raise ValueError(f"Operator: {what} must be a real matrix") from None
                if A.ndim != 2 or A.shape[1] != side or not np.all(np.isfinite(A)):
                    raise ValueError(f"Operator: {what} must be a finite [n, {side}] matrix, got shape {A.shape}")
                if A.shape[0] % 4 or not (4 <= A.shape[0] <= 256):
                    raise ValueError(f"Operator: {what} must have a multiple of 4 in [4, 256] rows, got {A.shape[0]}")
                mats.append(A)
            if H % 4 or W % 4 or not (4 <= H <= 256 and 4 <= W <= 256 and 1 <= C <= 8):
                raise ValueError(f"Operator: a separable operator needs an image size of multiples of 4 in [4, 256] with 1 to 8 channels, "
                                 f"got {C} x {H} x {W}")
            self.A_h, self.A_w = mats
            self.out_shape = (C, mats[0].shape[0], mats[1].shape[0])
        else:
            if not psf_mod.size_ok(C, H, W):
                raise ValueError(f"Operator: a point-spread function needs an image size of powers of two in [16, 256] with 1 to 8 channels, "
                                 f"got {C} x {H} x {W}")
            K = np.asarray(K, dtype=np.complex128)
            if K.shape != (H, W) or not np.all(np.isfinite(K)):
                raise ValueError(f"Operator: K must be a finite complex [{H}, {W}] spectrum, got shape {K.shape}")
            self.K = K
            self.out_shape = (C, H, W)
        self.mask = None if mask is None else mask.float().contiguous()
        if self.mask is not None and (self.mask.dim() != 3 or tuple(self.mask.shape[1:]) != self.out_shape[1:]):
            raise ValueError(f"Operator: mask must be [B, {self.out_shape[1]}, {self.out_shape[2]}], got {tuple(self.mask.shape)}")
        self._dev = {}

    # ------------------------------------------------------------------ device operands
    def to(self, device):
        """the operator with its mask on `device` (the matrices follow at their first use)"""
        if self.mask is not None and self.mask.device != torch.device(device):
            self.mask = self.mask.to(device)
        return self

    def _operands(self, device):
        key = str(device)
        hit = self._dev.get(key)
        if hit is None:
            if self.kind == "separable":
                f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
                hit = dict(A_h=f(self.A_h), A_w=f(self.A_w), A_hT=f(self.A_h.T), A_wT=f(self.A_w.T))
            elif self.kind == "psf":
                hit = dict(K=torch.from_numpy(psf_mod.interleave(self.K)).to(device),
                           Kc=torch.from_numpy(psf_mod.interleave(np.conj(self.K))).to(device))
            else:
                hit = {}
            self._dev[key] = hit
        return hit

    # ------------------------------------------------------------------ the linear part, on NHWC fp32 device tensors
    def transform(self, img):
        """the plane-wide transform without the mask: A_h X A_w^T (ops.separable_apply_rect) or the circular convolution
        (ops.circular_conv with K^); the local kind has none (its block mean is part of ops.measure_residual)"""
        m = self._operands(img.device)
        if self.kind == "separable":
            return ops.separable_apply_rect(img.contiguous(), m["A_h"], m["A_w"])
        if self.kind == "psf":
            return ops.circular_conv(img.contiguous(), m["K"])
        raise ValueError("Operator.transform: the local operator has no transform of its own")

    def transform_adjoint(self, r):
        """the transpose of transform: the same launches on the transposed matrices / the conjugate spectrum"""
        m = self._operands(r.device)
        if self.kind == "separable":
            return ops.separable_apply_rect(r.contiguous(), m["A_hT"], m["A_wT"])
        if self.kind == "psf":
            return ops.circular_conv(r.contiguous(), m["Kc"])
        raise ValueError("Operator.transform_adjoint: the local operator has no transform of its own")

    def _zeros_like_measurement(self, img):
        return torch.zeros((img.shape[0], self.out_shape[1], self.out_shape[2], img.shape[3]), device=img.device, dtype=torch.float32)

    def apply(self, img):
        """A img [B, h, w, C] of img [B, H, W, C]: the linear part with its mask (unmeasured elements are 0).  The local kind is the
        residual kernel against y = 0 with the linear response: r = mask (u - 0)."""
        local = self.kind == "mean"
        u = img.contiguous() if local else self.transform(img)
        return ops.measure_residual(u, self._zeros_like_measurement(img), self.mask, self.n if local else 1, "linear", 1.0)[0]

    def adjoint(self, r):
        """A^T r [B, H, W, C] of r [B, h, w, C]"""
        r = r.contiguous()
        if self.mask is not None:        # mask (r - 0), by the residual kernel at n = 1
            r = ops.measure_residual(r, torch.zeros_like(r), self.mask, 1, "linear", 1.0)[0]
        ones = torch.ones((r.shape[0],), device=r.device, dtype=torch.float32)
        v = ops.measure_adjoint(r, ones, ones, self.n if self.kind == "mean" else 1)
        return v if self.kind == "mean" else self.transform_adjoint(v)

    def measure(self, img):
        """y = phi(A img): what the sensor records (unmeasured elements are 0)"""
        u = self.apply(img)
        return u if self.response == "linear" else (self.gain * u).clamp_(-1.0, 1.0)


def make_operator(operator, in_shape, *, mask=None, response="linear", gain=1.0):
    """The Operator of restore_guided's `operator` argument on an image of in_shape (C, H, W): ("mean", n), ("separable", A_h, A_w),
    ("psf", k) with k a preset name or a 2-D array (psf.psf_array), or a name deblur takes ("uniform", "gauss", "aniso": the separable
    blur with zero padding) or deconvolve takes ("diag", "disk").  An Operator passes through.  ValueError for anything else."""
    if isinstance(operator, Operator):
        return operator
    C, H, W = in_shape
    kw = dict(mask=mask, response=response, gain=gain)
    if isinstance(operator, str):
        if operator in blur.PRESETS:
            k_h, k_w = blur.blur_kernel(operator)
            return Operator("separable", in_shape, A_h=blur.blur_matrix(H, k_h), A_w=blur.blur_matrix(W, k_w), **kw)
        if operator in psf_mod.PRESETS:
            operator = ("psf", operator)
        else:
            raise ValueError(f"restore_guided: unknown operator name {operator!r}, one of {blur.PRESETS + psf_mod.PRESETS}")
    if not isinstance(operator, (tuple, list)) or not operator or operator[0] not in KINDS:
        raise ValueError(f"restore_guided: operator must be ('mean', n), ('separable', A_h, A_w), ('psf', k) or a preset name, got {operator!r}")
    kind = operator[0]
    if len(operator) != (3 if kind == "separable" else 2):
        raise ValueError(f"restore_guided: operator {kind!r} takes {'two matrices' if kind == 'separable' else 'one argument'}, got {len(operator) - 1}")
    if kind == "mean":
        return Operator("mean", in_shape, n=operator[1], **kw)
    if kind == "separable":
        return Operator("separable", in_shape, A_h=operator[1], A_w=operator[2], **kw)
    k = psf_mod.psf_array(operator[1])          # its own ValueErrors
    if k.shape[0] > H or k.shape[1] > W:
        raise ValueError(f"restore_guided: a {k.shape[0]} x {k.shape[1]} point-spread function does not fit a {H} x {W} image")
    if not psf_mod.size_ok(C, H, W):
        raise ValueError(f"restore_guided: a point-spread function needs an image size of powers of two in [16, 256] with 1 to 8 channels, "
                         f"got {C} x {H} x {W}")
    return Operator("psf", in_shape, K=psf_mod.psf_spectrum(k, H, W), **kw)


def zeta_table(zeta, rows):
    """zeta as a float64 array of `rows` entries: a real number >= 0 for every row, or a sequence of exactly `rows` such numbers
    (entry k is the step size of the chain's row k).  ValueError otherwise."""
    if isinstance(zeta, bool) or isinstance(zeta, str):
        raise ValueError(f"restore_guided: zeta must be a real number >= 0 or a sequence of {rows} of them, got {zeta!r}")
    if isinstance(zeta, (int, float, np.integer, np.floating)):
        z = np.full(rows, float(zeta), dtype=np.float64)
    else:
        if torch.is_tensor(zeta):
            zeta = zeta.detach().cpu().numpy()
        try:
            z = np.asarray(zeta, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"restore_guided: zeta must be a real number >= 0 or a sequence of {rows} of them") from None
        if z.ndim != 1 or z.shape[0] != rows:
            raise ValueError(f"restore_guided: a zeta sequence needs one entry per step of the chain ({rows}), got shape {z.shape}")
    if not np.all(np.isfinite(z)) or np.any(z < 0):
        raise ValueError("restore_guided: zeta must be finite and >= 0")
    return z


@contextlib.contextmanager
def frozen(module):
    """The context a guided chain runs in: every parameter's requires_grad off and the module in eval mode, so that the autograd path
    serves the INPUT's gradient alone (no weight-gradient launch, no `.grad` touched: ddk.autograd._grad_slot); the flags and `training`
    of every submodule are put back on the way out, also after an exception."""
    flags = [(p, p.requires_grad) for p in module.parameters()]
    modes = [(m, m.training) for m in module.modules()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        module.eval()
        yield module
    finally:
        for p, f in flags:
            p.requires_grad_(f)
        for m, t in modes:
            m.training = t
