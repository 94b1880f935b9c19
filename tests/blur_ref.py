"""Independent restatement of DDNM deblurring for a separable blur with zero padding, A(X) = A_h X A_w^T per channel, for the
deblurring tests.  Nothing here imports models.diffusion.blur or models.diffusion.respace.

Matrices, the truncated SVD and the projections are float64.  A+ = Q_h (x) Q_w with each axis truncated on its own at tol * s_max, so
A+ A = P_h (x) P_w.  step() forms the clipped x0 in fp32 exactly as restore_ref.step does, then everything else in float64: it is what
the lone op is held to within a derived fp32 bar (the MFMA's summation order is not pinned).  Deblur.run is the chain of
restore_ref.Restore with the projection exchanged; its operands are the float64 matrices rounded to fp32, which is what the library is
handed, and x0' is rounded to fp32 once, where the library's is."""
import numpy as np
import torch

import restore_ref as RR
from repaint_ref import draw


def taps(kernel):
    """(k_h, k_w) float64: "uniform" 9 x 1/9; "gauss" 5 taps sigma 10; "aniso" 9 taps, sigma 20 (rows) and sigma 1 (columns)."""
    def g(length, sigma):
        r = np.arange(length) - (length - 1) / 2
        k = np.exp(-(r * r) / (2.0 * sigma * sigma))
        return k / np.sum(k)
    if isinstance(kernel, str):
        return {"uniform": (np.ones(9) / 9, np.ones(9) / 9), "gauss": (g(5, 10.0), g(5, 10.0)), "aniso": (g(9, 20.0), g(9, 1.0))}[kernel]
    if isinstance(kernel, (tuple, list)) and len(kernel) == 2 and np.ndim(kernel[0]) == 1:
        return np.asarray(kernel[0], dtype=np.float64), np.asarray(kernel[1], dtype=np.float64)
    k = np.asarray(kernel, dtype=np.float64)
    return k, k


def matrix(n, k):
    """A[i, i + j - L // 2] = k[j], built entry by entry."""
    A = np.zeros((n, n))
    L = len(k)
    for i in range(n):
        for j in range(L):
            c = i + j - L // 2
            if 0 <= c < n:
                A[i, c] = k[j]
    return A


def projection(A, tol):
    """(Q, P, rank): Q = sum over s_i > tol s_max of v_i u_i^T / s_i, P = Q A."""
    U, S, Vt = np.linalg.svd(A)
    keep = S > tol * S.max()
    Q = np.zeros_like(A)
    for i in np.nonzero(keep)[0]:
        Q += np.outer(Vt[i], U[:, i]) / S[i]
    return Q, Q @ A, int(keep.sum())


def operands(kernel, H, W, tol=3e-2):
    """dict of float64 torch tensors A_h, A_w, Q_h, Q_w, P_h, P_w."""
    k_h, k_w = taps(kernel)
    A_h, A_w = matrix(H, k_h), matrix(W, k_w)
    Q_h, P_h, _ = projection(A_h, tol)
    Q_w, P_w, _ = projection(A_w, tol)
    return {k: torch.from_numpy(v) for k, v in dict(A_h=A_h, A_w=A_w, Q_h=Q_h, Q_w=Q_w, P_h=P_h, P_w=P_w).items()}


def apply(x, L, R):
    """L . x[b, c] . R^T for every plane of [B, C, H, W], float64."""
    return torch.einsum("ih,bchw,jw->bcij", L.double(), x.double(), R.double())


def step(x, eps, P_h, P_w, Yp, cr, crm1, c1, c2, sg, z):
    """One step, per-sample coefficients [B]: x0 in fp32 as restore_ref.step, the rest in float64.  Returns (x_prev, x0, x0') with the
    last two for the caller's error bar."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    assert x0.dtype == torch.float32
    x0p = (x0.double() - apply(x0, P_h, P_w)) + Yp.double()
    out = (col(c1).double() * x0p + col(c2).double() * x.double()) + col(sg).double() * z.double()
    return out, x0, x0p


class Deblur(RR.Restore):
    def run(self, eps_model, x, y, kernel, seed, tol=3e-2, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y the blurred image, same shape.  Returns x after steps K-1 .. 0."""
        sd, ex = self.sd, self.sd._extract
        shape = tuple(x.shape)
        m = {k: v.float().double() for k, v in operands(kernel, shape[2], shape[3], tol).items()}
        Yp = apply(y, m["Q_h"], m["Q_w"])
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, kk = sd._pred_xstart(eps_model, x, k)
                x0 = ((x0.double() - apply(x0, m["P_h"], m["P_w"])) + Yp).float()
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
