"""Independent restatement of DDNM for a size-changing separable operator A(X) = A_h X A_w^T, A_h [h, H] and A_w [w, W] (DESIGN.md
section 3.15), for the restore_sep tests.  Nothing here imports models.diffusion.blur or models.diffusion.respace.

The matrix of the antialiased bicubic reduction is built entry by entry from its formula; the pseudo-inverse and the projection are
blur_ref.projection's sum over the retained singular triplets, for a rectangular A (Q is [H, h], P = Q A is [H, H]).  The step is
blur_ref.step and the chain is blur_ref.Deblur's with one difference, Yp = Q_h y Q_w^T of a y of its own size."""
import numpy as np
import torch

import blur_ref as BR
from repaint_ref import draw

SIZES = [(16, 2), (16, 4), (32, 2), (32, 4), (32, 8), (48, 4), (64, 4), (80, 2), (256, 2), (256, 4), (256, 8)]      # (H, scale)


def keys(x):
    """Keys' cubic convolution kernel, a = -0.5"""
    x = abs(x)
    if x <= 1:
        return 1.5 * x ** 3 - 2.5 * x ** 2 + 1
    if x < 2:
        return -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2
    return 0.0


def matrix(H, n, kind="bicubic"):
    """A [H / n, H], entry by entry: row i has its centre at c = (i + 0.5) n and the weights k((j - c + 0.5) / n) over
    max(int(c - 2 n + 0.5), 0) <= j < min(int(c + 2 n + 0.5), H), normalised; "mean": 1 / n over block i."""
    A = np.zeros((H // n, H))
    for i in range(H // n):
        if kind == "mean":
            for j in range(i * n, (i + 1) * n):
                A[i, j] = 1.0 / n
            continue
        c = (i + 0.5) * n
        lo, hi = max(int(c - 2 * n + 0.5), 0), min(int(c + 2 * n + 0.5), H)
        row = [keys((j - c + 0.5) / n) for j in range(lo, hi)]
        total = sum(row)
        for j, v in zip(range(lo, hi), row):
            A[i, j] = v / total
    return A


def projection(A, tol=3e-2):
    """(Q [H, h], P [H, H], rank): Q = sum over s_i > tol s_max of v_i u_i^T / s_i, P = Q A."""
    U, S, Vt = np.linalg.svd(A, full_matrices=False)
    keep = S > tol * S.max()
    Q = np.zeros((A.shape[1], A.shape[0]))
    for i in np.nonzero(keep)[0]:
        Q += np.outer(Vt[i], U[:, i]) / S[i]
    return Q, Q @ A, int(keep.sum())


def operands(A_h, A_w, tol=3e-2):
    """dict of float64 torch tensors A_h, A_w, Q_h, Q_w, P_h, P_w of a matrix pair."""
    Q_h, P_h, _ = projection(A_h, tol)
    Q_w, P_w, _ = projection(A_w, tol)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in dict(A_h=A_h, A_w=A_w, Q_h=Q_h, Q_w=Q_w, P_h=P_h, P_w=P_w).items()}


class Separable(BR.Deblur):
    def run(self, eps_model, x, y, A_h, A_w, seed, tol=3e-2, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y [B, C, h, w].  blur_ref.Deblur.run with the fp32-rounded operands of (A_h, A_w) and Yp from the
        small y.  Returns x after steps K-1 .. 0."""
        sd, ex = self.sd, self.sd._extract
        shape = tuple(x.shape)
        m = {k: v.float().double() for k, v in operands(A_h, A_w, tol).items()}
        Yp = BR.apply(y, m["Q_h"], m["Q_w"])
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, kk = sd._pred_xstart(eps_model, x, k)
                x0 = ((x0.double() - BR.apply(x0, m["P_h"], m["P_w"])) + Yp).float()
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
