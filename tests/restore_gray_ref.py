"""Independent restatement of DDNM / DDNM+ colourisation and grey super-resolution (Wang, Yu, Zhang, ICLR 2023, sections 3.2 and 3.3)
for the operator A = M o pool_n o grey_w on 3-channel images: y [B, 1, H/n, W/n] is the weighted channel sum of x, averaged over
n x n blocks, wherever the mask M [B, H/n, W/n] (None: everywhere) is nonzero.

    "mean": w = (1/3, 1/3, 1/3), A+ replicates d into the three channels;
    "luma": w = (0.299, 0.587, 0.114) (BT.601), A+ multiplies d by a_c = w_c / (w . w).

Built on tests/restore_noisy_ref.py (the step's linear form, the tables lam and sgm, the select on the mask) and tests/spaced_ref.py
(the float64 schedule), with oracle/philox_ref draws.  Nothing here imports models.diffusion.respace.  With d = y - A x0:

    x0'_c  = x0_c + lam a_c d on measured groups, x0_c elsewhere
    x_prev = (c1 x0' + c2 x) + (measured ? sgm : s) z

sigma_y > 0: lam and sgm are restore_noisy_ref's.  sigma_y == 0: lam = 1 in every row, row 0 included, and sgm = the fp32 sigma with
row 0 zero, so row 0 returns x0', whose image under A is y up to rounding.

step() fixes the order of the fp32 operations, one rounding each, which is what the library pins:

    g = 0;  for i, j over the block, row-major:  for c = 0, 1, 2:  g = g + W_c x0_c[i][j]
    m = g NORM;  d = y - m;  x0'_c = x0_c + lam (A_c d)
    mean:  W_c = A_c = 1,  NORM = fp32(1 / (3 n n));   luma:  W_c = fp32(w_c),  NORM = 1 / (n n),  A_c = fp32(w_c / (w . w))"""
import numpy as np
import torch

import restore_noisy_ref as RN
import restore_ref as RR
import spaced_ref as SR
from repaint_ref import draw

LUMA = (0.299, 0.587, 0.114)
EXACT = {"mean": (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0), "luma": LUMA}     # the weights of A as real numbers (float64)


def coefficients(weights, n):
    """fp32 (W [3], A [3], NORM) as 0-dim tensors, the constants of the step"""
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    if weights == "mean":
        one = f(1.0)
        return [one] * 3, [one] * 3, f(np.float32(1.0 / (3 * n * n)))
    if weights != "luma":
        raise ValueError(weights)
    w0, w1, w2 = LUMA
    ww = (w0 * w0 + w1 * w1) + w2 * w2
    return [f(np.float32(w)) for w in LUMA], [f(np.float32(w / ww)) for w in LUMA], f(np.float32(1.0) / np.float32(n * n))


def group_value(x0, n, weights):
    """fp32 A x0 [B, H/n, W/n] of x0 [B, 3, H, W] without the mask, in the pinned order"""
    b, c, h, w = x0.shape
    assert c == 3
    W, _, norm = coefficients(weights, n)
    blocks = x0.reshape(b, 3, h // n, n, w // n, n)
    g = torch.zeros(b, h // n, w // n, dtype=x0.dtype)
    for i in range(n):
        for j in range(n):
            for ch in range(3):
                g = g + W[ch] * blocks[:, ch, :, i, :, j]
    return g * norm


def apply_exact(x, n, weights):
    """float64 A x [B, H/n, W/n] with the exact weights, for the consistency bars"""
    w = torch.tensor(EXACT[weights], dtype=torch.float64).reshape(1, 3, 1, 1)
    return RR.pool((x.double() * w).sum(dim=1, keepdim=True), n)[:, 0]


def measured(mk, like, n):
    """bool, like's shape [B, 3, H, W]: the elements whose block is measured; mk None: all"""
    return RN.measured(mk, like, n)


def project(x0, y, mk, n, lam, weights):
    """x0' of [B, 3, H, W] for y [B, 1, H/n, W/n], mk [B, H/n, W/n] or None and the per-sample lam [B]"""
    _, A, _ = coefficients(weights, n)
    d = y[:, 0] - group_value(x0, n, weights)                       # [B, H/n, W/n]; NaN where y is, selected away below
    lam = lam.reshape(-1, 1, 1)
    moved = torch.stack([x0[:, ch] + RR.replicate((lam * (A[ch] * d)).unsqueeze(1), n)[:, 0] for ch in range(3)], dim=1)
    return torch.where(measured(mk, x0, n), moved, x0)


def step(x, eps, y, mk, n, weights, cr, crm1, c1, c2, sg, lam, sgm, z):
    """One step in the library's linear form, fp32, per-sample coefficients [B] (sg already 0 where the row is 0): what the lone op is
    held to bit for bit."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    x0p = project(x0, y, mk, n, lam, weights)
    scale = torch.where(measured(mk, x, n), col(sgm).expand_as(x), col(sg).expand_as(x))
    return (col(c1) * x0p + col(c2) * x) + scale * z


def exact_coefficients(sigma32):
    """fp32 (lam, sgm) of an exact measurement: lam = 1 everywhere, sgm = sigma with row 0 zero"""
    sgm = sigma32.clone()
    sgm[0] = 0.0
    return torch.ones_like(sgm), sgm


class RestoreGray:
    def __init__(self, base_betas, spec):
        T = len(base_betas)
        use = set(range(T)) if spec is None else SR.space_timesteps(T, spec)
        self.sd = SR.SpacedDiffusion(base_betas, use)
        self.K = self.sd.num_timesteps

    def tables(self, sigma_y, ddim=False, eta=0.0):
        """fp32 tensors c1, c2, sigma (row 0 zeroed), lam, sgm of K rows"""
        c1, c2, sigma32 = RN.linear_tables(self.sd, ddim, eta)
        s = sigma32.clone()
        s[0] = 0.0
        f32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64)).float()
        if sigma_y > 0:
            lam, sgm = (f32(v) for v in RN.noisy_coefficients(c1, sigma32.double().numpy(), sigma_y))
        else:
            lam, sgm = exact_coefficients(sigma32)
        return dict(c1=f32(c1), c2=f32(c2), sigma=s, lam=lam, sgm=sgm)

    def run(self, eps_model, x, y, mk, n, weights, sigma_y, seed, stream=0, ddim=False, eta=0.0):
        """x: x_T [B, 3, H, W]; y [B, 1, H/n, W/n]; mk [B, H/n, W/n] or None.  Returns x after steps K-1 .. 0."""
        tab = self.tables(sigma_y, ddim, eta)
        shape = tuple(x.shape)
        B = shape[0]
        with torch.no_grad():
            for k in range(self.K - 1, -1, -1):
                z = draw(shape, seed, k, stream)
                x0, _ = self.sd._pred_xstart(eps_model, x, k)
                row = lambda name: tab[name][k].expand(B)
                x0p = project(x0, y, mk, n, row("lam"), weights)
                col = lambda name: row(name).reshape(-1, 1, 1, 1)
                scale = torch.where(measured(mk, x, n), col("sgm").expand_as(x), col("sigma").expand_as(x))
                x = (col("c1") * x0p + col("c2") * x) + scale * z
        return x
