"""Independent restatement of DDNM+ (Wang, Yu, Zhang, ICLR 2023, section 3.3, eqs. 17-19) for a noisy measurement of the operator
A = M o pool_n: y = A x + n, n ~ N(0, sigma_y^2), in y's own [-1, 1] scale.

Built on tests/restore_masked_ref.py (the operator, the select on the mask), tests/restore_ref.py (the block mean's operation order)
and tests/spaced_ref.py (the float64 schedule).  Nothing here imports models.diffusion.respace.  The chain is written in the
library's linear form x_prev = (c1 x0' + c2 x) + s z, whose c1 is the a_t of the paper's eq. 19:

    s_k    = (k > 0 ? sigma[k] : 0)                              the draw's scale, the fp32 value the chain applies
    lam[k] = 1 if s_k >= |c1[k]| sigma_y else s_k / (|c1[k]| sigma_y)            (row 0: 0)
    sgm[k] = sqrt(max(s_k^2 - (c1[k] lam[k] sigma_y)^2, 0))                      (0 where lam < 1)
    x0'    = x0 + lam (y - A x0) on measured blocks (n = 1: x0 + lam (y - x0)), x0 elsewhere
    x_prev = (c1 x0' + c2 x) + (measured ? sgm : s) z

The tables are formed in float64 and cast to fp32 once; step() fixes the order of the fp32 operations, one rounding each, which is
what the library pins, so a single step given the same eps_hat and draw can be compared bit for bit."""
import numpy as np
import torch

import restore_ref as RR
import spaced_ref as SR
from repaint_ref import draw


def block_mean(x0, n):
    """A x0 in fp32 in restore_ref.project's order: the block summed row-major from 0, times 1 / n^2 (exact)."""
    b, c, h, w = x0.shape
    blocks = x0.reshape(b, c, h // n, n, w // n, n)
    s = torch.zeros(b, c, h // n, w // n, dtype=x0.dtype)
    for i in range(n):
        for j in range(n):
            s = s + blocks[:, :, :, i, :, j]
    return s * x0.new_tensor(1.0 / (n * n))


def measured(mk, like, n):
    """bool, like's shape: the elements whose block (n = 1: pixel) is measured; mk None: all"""
    if mk is None:
        return torch.ones_like(like, dtype=torch.bool)
    return RR.replicate((mk != 0).unsqueeze(1), n).expand_as(like)


def project(x0, y, mk, n, lam):
    """x0' of [B, C, H, W] for y [B, C, H/n, W/n], mk [B, H/n, W/n] or None and the per-sample lam [B]"""
    lam = lam.reshape(-1, 1, 1, 1)
    moved = x0 + lam * (y - x0) if n == 1 else x0 + RR.replicate(lam * (y - block_mean(x0, n)), n)
    return torch.where(measured(mk, x0, n), moved, x0)


def step(x, eps, y, mk, n, cr, crm1, c1, c2, sg, lam, sgm, z):
    """One step in the library's linear form, fp32, per-sample coefficients [B] (sg already 0 where the row is 0): what the lone op is
    held to bit for bit."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    x0p = project(x0, y, mk, n, lam)
    scale = torch.where(measured(mk, x, n), col(sgm).expand_as(x), col(sg).expand_as(x))
    return (col(c1) * x0p + col(c2) * x) + scale * z


def noisy_coefficients(c1, s32, sigma_y):
    """float64 (lam, sgm) from the float64 c1 and the fp32 draw scale the chain applies (row 0 counted as 0)"""
    c1 = np.asarray(c1, dtype=np.float64)
    s = np.asarray(s32, dtype=np.float64).copy()
    s[0] = 0.0
    K = len(s)
    lam, sgm = np.zeros(K), np.zeros(K)
    for k in range(1, K):
        a = abs(c1[k]) * sigma_y
        if s[k] >= a:
            lam[k] = 1.0
            sgm[k] = np.sqrt(max(s[k] ** 2 - (c1[k] * sigma_y) ** 2, 0.0))
        else:
            lam[k] = s[k] / a
    return lam, sgm


def linear_tables(sd, ddim=False, eta=0.0):
    """float64 (c1, c2) and the fp32 sigma [K] of spaced_ref.SpacedDiffusion `sd` in the linear form.  DDIM: the direct form
    x0 sqrt(abar_prev) + d eps with eps = (c_recip x - x0) / c_recipm1 gives c1 = sqrt(abar_prev) - d / c_recipm1, c2 = d c_recip /
    c_recipm1, d = sqrt(1 - abar_prev - sigma^2)."""
    if not ddim:
        sigma32 = torch.exp(0.5 * torch.from_numpy(sd.posterior_log_variance_clipped).float())
        return sd.posterior_mean_coef1, sd.posterior_mean_coef2, sigma32
    a, ap = sd.alphas_cumprod, sd.alphas_cumprod_prev
    sigma = eta * np.sqrt((1 - ap) / (1 - a)) * np.sqrt(1 - a / ap)
    d = np.sqrt(np.maximum(1 - ap - sigma ** 2, 0.0))
    return (np.sqrt(ap) - d / sd.sqrt_recipm1_alphas_cumprod, d * sd.sqrt_recip_alphas_cumprod / sd.sqrt_recipm1_alphas_cumprod,
            torch.from_numpy(sigma).float())


class RestoreNoisy:
    def __init__(self, base_betas, spec):
        T = len(base_betas)
        use = set(range(T)) if spec is None else SR.space_timesteps(T, spec)
        self.sd = SR.SpacedDiffusion(base_betas, use)
        self.K = self.sd.num_timesteps

    def tables(self, sigma_y, ddim=False, eta=0.0):
        """fp32 tensors c1, c2, sigma (row 0 zeroed), lam, sgm of K rows"""
        c1, c2, sigma32 = linear_tables(self.sd, ddim, eta)
        lam, sgm = noisy_coefficients(c1, sigma32.double().numpy(), sigma_y)
        s = sigma32.clone()
        s[0] = 0.0
        f32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64)).float()
        return dict(c1=f32(c1), c2=f32(c2), sigma=s, lam=f32(lam), sgm=f32(sgm))

    def run(self, eps_model, x, y, mk, n, sigma_y, seed, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, C, H, W]; y [B, C, H/n, W/n]; mk [B, H/n, W/n] or None.  Returns x after steps K-1 .. 0."""
        tab = self.tables(sigma_y, ddim, eta)
        shape = tuple(x.shape)
        B = shape[0]
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, _ = self.sd._pred_xstart(eps_model, x, k)
                row = lambda name: tab[name][k].expand(B)
                x0p = project(x0, y, mk, n, row("lam"))
                col = lambda name: row(name).reshape(-1, 1, 1, 1)
                scale = torch.where(measured(mk, x, n), col("sgm").expand_as(x), col("sigma").expand_as(x))
                x = (col("c1") * x0p + col("c2") * x) + scale * z
        return x
