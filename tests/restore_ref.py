"""Independent restatement of DDNM super-resolution (Wang, Yu, Zhang, ICLR 2023, Algorithm 1) for the operator A = n x n average
pooling with pseudo-inverse A+ = n x n replication, for the super-resolution tests.

Nothing here imports models.diffusion.respace.  The chain is spaced_ref.SpacedDiffusion's (float64 schedule, coefficients cast to
fp32 per step) with one change: the clipped pred_xstart of every step is replaced by x0' = x0 - A+ A x0 + A+ y before the step's
mean is formed, and x0' is not clipped again.  The ancestral step is q(x_{k-1} | x_k, x0') plus the fixed-small-variance draw; the
DDIM step is its direct form with eps recomputed from x0'.  The draws come from oracle/philox_ref with key (seed, step = k, stream)
in NHWC element order.  The eps model runs at the trained timestep map[k].

project() fixes the order of the fp32 operations (the block summed in row-major order, one rounding per operation), which is what
the library pins, so a single step given the same eps_hat and draw can be compared bit for bit (step())."""
import torch

import spaced_ref as SR
from repaint_ref import draw


def pool(x, n):
    """A: n x n average pooling of [B, C, H, W], in x's dtype."""
    b, c, h, w = x.shape
    return x.reshape(b, c, h // n, n, w // n, n).mean(dim=(3, 5))


def replicate(y, n):
    """A+: every pixel of y becomes an n x n block."""
    return y.repeat_interleave(n, dim=2).repeat_interleave(n, dim=3)


def project(x0, y, n):
    """x0' = x0 + A+ (y - A x0) in fp32: the block sum in row-major order from 0, times 1 / n^2 (exact), y minus that, added to x0."""
    b, c, h, w = x0.shape
    blocks = x0.reshape(b, c, h // n, n, w // n, n)
    s = torch.zeros(b, c, h // n, w // n, dtype=x0.dtype)
    for i in range(n):
        for j in range(n):
            s = s + blocks[:, :, :, i, :, j]
    m = s * x0.new_tensor(1.0 / (n * n))
    return x0 + replicate(y - m, n)


def step(x, eps, y, n, cr, crm1, c1, c2, sg, z):
    """One step in the library's linear form, fp32, per-sample coefficients [B]: what the lone op is held to bit for bit."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    x0p = project(x0, y, n)
    return (col(c1) * x0p + col(c2) * x) + col(sg) * z


class Restore:
    def __init__(self, base_betas, spec):
        T = len(base_betas)
        use = set(range(T)) if spec is None else SR.space_timesteps(T, spec)
        self.sd = SR.SpacedDiffusion(base_betas, use)
        self.K = self.sd.num_timesteps

    def run(self, eps_model, x, y, n, seed, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y [B, C, H/n, W/n].  Returns x after steps K-1 .. 0."""
        sd, ex = self.sd, self.sd._extract
        shape = tuple(x.shape)
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, kk = sd._pred_xstart(eps_model, x, k)
                x0 = project(x0, y, n)
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
