"""Independent restatement of DDNM deconvolution for a 2-D point-spread function with periodic boundary, for the deconvolution tests.
Nothing here imports models.diffusion.psf or models.diffusion.respace.

Per channel of an image X [H, W], the PSF k [p, q] (p, q odd), correlation form:

    A(X)[i, j] = sum_{a, b} k[a, b] X[(i + a - p // 2) mod H, (j + b - q // 2) mod W]

In the 2-D Fourier basis A multiplies by K^ = conj(F2(k laid out from index (0, 0))) . phase of the centre; the kept frequencies are
M = |K^| > tol max |K^| together with their mirror images, A+ divides by K^ on M and is zero elsewhere, A+ A = F2^-1 M F2.

Everything is float64 (numpy.fft).  step() forms the clipped x0 in fp32 exactly as restore_ref.step does, then the rest in float64:
it is what the lone op is held to within a derived fp32 bar.  Deconv.run is the chain of restore_ref.Restore with the projection
exchanged; x0' is rounded to fp32 once, where the library's is."""
import numpy as np
import torch

import restore_ref as RR
from repaint_ref import draw


def preset(name):
    """the two presets, restated: "diag" 1/9 on the main diagonal of 9 x 9; "disk" equal weights within radius 3.5 of the centre"""
    k = np.zeros((9, 9))
    for a in range(9):
        for b in range(9):
            if name == "diag":
                k[a, b] = 1.0 if a == b else 0.0
            else:
                k[a, b] = 1.0 if (a - 4) ** 2 + (b - 4) ** 2 <= 12.25 else 0.0
    return k / k.sum()


def blur_direct(X, k):
    """A(X) for one plane by the definition's double loop (slow: small planes only)"""
    H, W = X.shape
    p, q = k.shape
    out = np.zeros((H, W))
    for i in range(H):
        for j in range(W):
            acc = 0.0
            for a in range(p):
                for b in range(q):
                    acc += k[a, b] * X[(i + a - p // 2) % H, (j + b - q // 2) % W]
            out[i, j] = acc
    return out


def spectrum(k, H, W):
    """K^ [H, W] complex128 with F2(A X) = K^ F2(X): a correlation multiplies by the conjugate of the taps' own transform, and the
    centre's offset is a phase"""
    k = np.asarray(k, dtype=np.float64)
    p, q = k.shape
    pad = np.zeros((H, W))
    pad[:p, :q] = k
    u = np.arange(H)[:, None]
    v = np.arange(W)[None, :]
    phase = np.exp(-2j * np.pi * ((p // 2) * u / H + (q // 2) * v / W))
    return np.conj(np.fft.fft2(pad)) * phase


def kept(k, H, W, tol):
    """M [H, W] bool"""
    mag = np.abs(spectrum(k, H, W))
    M = mag > tol * mag.max()
    mirror = M[(-np.arange(H)) % H][:, (-np.arange(W)) % W]
    return M & mirror


def pinv_spectrum(k, H, W, tol):
    K = spectrum(k, H, W)
    M = kept(k, H, W, tol)
    P = np.zeros_like(K)
    P[M] = 1.0 / K[M]
    return P


def planes(x):
    """[B, C, H, W] tensor -> float64 array"""
    return x.detach().double().numpy()


def apply(x, S):
    """Re F2^-1(S F2 x) per plane: [B, C, H, W] (tensor or array) -> float64 array"""
    x = planes(x) if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)
    return np.fft.ifft2(np.asarray(S, dtype=np.complex128) * np.fft.fft2(x, axes=(-2, -1)), axes=(-2, -1)).real


def project(x0, Yp, M):
    """x0' = x0 - A+ A x0 + Yp in float64, as an array"""
    return apply(x0, np.where(M, 0.0, 1.0)) + np.asarray(Yp, dtype=np.float64)


def step(x, eps, M, Yp, cr, crm1, c1, c2, sg, z):
    """One step, per-sample coefficients [B]: x0 in fp32 as restore_ref.step, the rest in float64.  Returns (x_prev, x0, x0')."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    assert x0.dtype == torch.float32
    x0p = torch.from_numpy(project(x0, planes(Yp), M))
    out = (col(c1).double() * x0p + col(c2).double() * x.double()) + col(sg).double() * z.double()
    return out, x0, x0p


class Deconv(RR.Restore):
    def run(self, eps_model, x, y, k, tol, seed, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y [B, C, H, W] the blurred image.  Returns x after steps K-1 .. 0."""
        sd, ex = self.sd, self.sd._extract
        shape = tuple(x.shape)
        H, W = shape[2:]
        M = kept(k, H, W, tol)
        Yp = apply(y, pinv_spectrum(k, H, W, tol))
        with torch.no_grad():
            for kk_ in range(self.K - 1, -1, -1):
                z = draw(shape, seed, kk_, stream)
                x0, kk = sd._pred_xstart(eps_model, x, kk_)
                x0 = torch.from_numpy(project(x0, Yp, M)).float()
                nonzero = float(kk_ != 0)
                if not ddim:
                    mean = ex(sd.posterior_mean_coef1, kk, x) * x0 + ex(sd.posterior_mean_coef2, kk, x) * x
                    x = mean + nonzero * torch.exp(0.5 * ex(sd.posterior_log_variance_clipped, kk, x)) * z
                else:
                    eps = (ex(sd.sqrt_recip_alphas_cumprod, kk, x) * x - x0) / ex(sd.sqrt_recipm1_alphas_cumprod, kk, x)
                    ab, ab_prev = ex(sd.alphas_cumprod, kk, x), ex(sd.alphas_cumprod_prev, kk, x)
                    sigma = eta * torch.sqrt((1 - ab_prev) / (1 - ab)) * torch.sqrt(1 - ab / ab_prev)
                    x = x0 * torch.sqrt(ab_prev) + torch.sqrt(1 - ab_prev - sigma ** 2) * eps + nonzero * sigma * z
        return x
