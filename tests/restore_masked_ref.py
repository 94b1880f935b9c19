"""Independent restatement of DDNM (Wang, Yu, Zhang, ICLR 2023, Algorithm 1) for the operator A = M o pool_n: n x n average pooling
followed by a {0, 1} mask over the pooled pixels, shared by the channels.  A+ = replication of the measured pooled pixels, so
x0' = x0 - A+ A x0 + A+ y moves a measured block by y - mean(block) and leaves every other block alone.  n = 1 is inpainting:
a measured pixel of x0 is replaced by y.

Built on tests/restore_ref.py (the projection for an all-measured mask, whose operation order it keeps) and tests/spaced_ref.py
(the chain).  The unmeasured part is a select (torch.where), never a blend: y there may hold anything, NaN included, and reaches no
result.  At n = 1 the measured part is a select as well, so measured pixels of x0' are y bit for bit."""
import torch

import restore_ref as RR
import spaced_ref as SR
from repaint_ref import draw


def project(x0, y, mk, n):
    """x0' of [B, C, H, W] for y [B, C, H/n, W/n] and mk [B, H/n, W/n] (nonzero = measured) or None (all measured, n >= 2)."""
    if mk is None:
        return RR.project(x0, y, n)
    sel = (mk != 0).unsqueeze(1).expand_as(y)
    if n == 1:
        return torch.where(sel, y, x0)
    moved = RR.project(x0, torch.where(sel, y, torch.zeros_like(y)), n)       # what is not measured is never used
    return torch.where(RR.replicate(sel, n), moved, x0)


def step(x, eps, y, mk, n, cr, crm1, c1, c2, sg, z):
    """One step in the library's linear form, fp32, per-sample coefficients [B]: what the lone op is held to bit for bit."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    x0p = project(x0, y, mk, n)
    return (col(c1) * x0p + col(c2) * x) + col(sg) * z


class RestoreMasked:
    def __init__(self, base_betas, spec):
        T = len(base_betas)
        use = set(range(T)) if spec is None else SR.space_timesteps(T, spec)
        self.sd = SR.SpacedDiffusion(base_betas, use)
        self.K = self.sd.num_timesteps

    def run(self, eps_model, x, y, mk, n, seed, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y [B, C, H/n, W/n]; mk [B, H/n, W/n] or None.  Returns x after steps K-1 .. 0."""
        sd, ex = self.sd, self.sd._extract
        shape = tuple(x.shape)
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, kk = sd._pred_xstart(eps_model, x, k)
                x0 = project(x0, y, mk, n)
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
