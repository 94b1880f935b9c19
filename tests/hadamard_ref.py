"""Independent restatement of DDNM compressed sensing with a subsampled, permuted Walsh-Hadamard operator, for the compressed-sensing
tests.  Nothing here imports models.diffusion.hadamard or models.diffusion.respace.

Per channel of an image [B, C, H, W], the plane flattened row-major (N = H W):

    a[j] = X[perm[j]],   v = W a,  W[k][j] = (-1)^popcount(k & j) / sqrt(N),   A(X) = v[0 .. m - 1],   A+ = A^T.

Everything is float64 (fwht: the textbook in-place butterflies on a float64 copy; fwht_int: the same in int64, for the exact cases).
step() forms the clipped x0 in fp32 exactly as restore_ref.step does, then the rest in float64: it is what the lone op is held to
within a derived fp32 bar.  CS.run is the chain of restore_ref.Restore with the projection exchanged; x0' is rounded to fp32 once,
where the library's is."""
import numpy as np
import torch

import restore_ref as RR
from repaint_ref import draw


def sylvester(N):
    """The orthonormal Walsh-Hadamard matrix of order N in natural order, entry by entry from the popcount definition."""
    k = np.arange(N)
    bits = np.zeros((N, N), dtype=np.int64)
    kj = k[:, None] & k[None, :]
    while kj.any():
        bits += kj & 1
        kj >>= 1
    return np.where(bits % 2 == 0, 1.0, -1.0) / np.sqrt(float(N))


def _butterflies(a):
    """unnormalised transform along the last axis of a copy of a (float64 or int64)"""
    a = a.copy()
    N = a.shape[-1]
    h = 1
    while h < N:
        v = a.reshape(*a.shape[:-1], N // (2 * h), 2, h)
        lo, hi = v[..., 0, :].copy(), v[..., 1, :].copy()
        v[..., 0, :] = lo + hi
        v[..., 1, :] = lo - hi
        h *= 2
    return a


def fwht(a):
    """W a along the last axis, float64, orthonormal."""
    a = np.asarray(a, dtype=np.float64)
    return _butterflies(a) / np.sqrt(float(a.shape[-1]))


def fwht_int(a):
    """H a along the last axis in int64, unnormalised: exact."""
    return _butterflies(np.asarray(a, dtype=np.int64))


def planes(x):
    """[B, C, H, W] tensor -> float64 array [B, C, N]"""
    return x.detach().double().reshape(x.shape[0], x.shape[1], -1).numpy()


def measure(x, perm, m):
    """A(x): [B, C, H, W] -> float64 array [B, C, m]"""
    return fwht(planes(x)[..., np.asarray(perm, dtype=np.int64)])[..., :m]


def adjoint(y, perm, shape):
    """A^T y: [B, C, m] -> float64 tensor of `shape` = (B, C, H, W)"""
    y = np.asarray(y, dtype=np.float64)
    N = shape[2] * shape[3]
    w = np.zeros((*y.shape[:2], N))
    w[..., :y.shape[2]] = y
    out = np.zeros_like(w)
    out[..., np.asarray(perm, dtype=np.int64)] = fwht(w)
    return torch.from_numpy(out.reshape(shape))


def project(x0, y, perm):
    """x0' = A^T y + (I - A^T A) x0 in float64: (x0' as a float64 tensor of x0's shape, v = W Pi x0 [B, C, N], w = the selected
    coefficients [B, C, N]); the last two for the caller's error bar."""
    p = np.asarray(perm, dtype=np.int64)
    y = np.asarray(y, dtype=np.float64)
    v = fwht(planes(x0)[..., p])
    w = v.copy()
    w[..., :y.shape[2]] = y
    out = np.zeros_like(w)
    out[..., p] = fwht(w)
    return torch.from_numpy(out.reshape(tuple(x0.shape))), v, w


def step(x, eps, y, perm, cr, crm1, c1, c2, sg, z):
    """One step, per-sample coefficients [B]: x0 in fp32 as restore_ref.step, the rest in float64.  Returns (x_prev, x0, x0', w)."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    assert x0.dtype == torch.float32
    x0p, _, w = project(x0, y, perm)
    out = (col(c1).double() * x0p + col(c2).double() * x.double()) + col(sg).double() * z.double()
    return out, x0, x0p, w


class CS(RR.Restore):
    def run(self, eps_model, x, y, perm, seed, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y [B, C, m] the measurement.  Returns x after steps K-1 .. 0."""
        sd, ex = self.sd, self.sd._extract
        shape = tuple(x.shape)
        yd = y.double().numpy()
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, kk = sd._pred_xstart(eps_model, x, k)
                x0 = project(x0, yd, perm)[0].float()
                nonzero = float(k != 0)
                if not ddim:
                    mean = ex(sd.posterior_mean_coef1, kk, x) * x0 + ex(sd.posterior_mean_coef2, kk, x) * x
                    x = mean + nonzero * torch.exp(0.5 * ex(sd.posterior_log_variance_clipped, kk, x)) * z
                else:
                    eps = (ex(sd.sqrt_recip_alphas_cumprod, kk, x) * x - x0) / ex(sd.sqrt_recipm1_alphas_cumprod, kk, x)
                    ab, ab_prev = ex(sd.alphas_cumprod, kk, x), ex(sd.alphas_cumprod_prev, kk, x)
                    sigma = eta * torch.sqrt((1 - ab_prev) / (1 - ab)) * torch.sqrt(1 - ab / ab_prev)
                    x = x0 * torch.sqrt(ab_prev) + torch.sqrt(1 - ab_prev - sigma ** 2) * eps + nonzero * sigma * z
        return x
