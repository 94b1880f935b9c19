"""Independent restatement of DPM-Solver++(2M) (Lu et al. 2022, arXiv:2211.01095, Algorithm 2: data prediction, clipped x0) in
its DIRECT form, and of the log-SNR timestep grid, for the DPM-Solver tests.

Nothing here imports models.diffusion.respace.  The grid is recomputed from the oracle's float64 betas; each step computes its
own lambda, h and r, keeps the list of past clipped x0 predictions and forms D = (1 + 1/(2r)) x0_k - 1/(2r) x0_{k+1}, then
x_prev = (sigma_prev / sigma) x - alpha_prev (exp(-h) - 1) D.  The per-step float64 coefficients are cast to fp32 when gathered,
as spaced_ref does.  The eps model is oracle/unet_ref.unet_forward at the ORIGINAL timestep map[k]."""
import math

import numpy as np
import torch

import spaced_ref as SR


def logsnr_grid(base_betas, n):
    """N trained timesteps nearest (in lambda) to N values evenly spaced from lambda_0 to lambda_{T-1}, walking up from t = 0;
    a collision moves the index one above the previous one."""
    acp = np.cumprod(1.0 - np.asarray(base_betas, dtype=np.float64))
    lam = np.log(np.sqrt(acp / (1.0 - acp)))
    T = len(lam)
    if n < 2 or n > T:
        raise ValueError(f"{n} steps on T = {T}")
    grid = []
    for target in np.linspace(lam[0], lam[T - 1], n):
        i = int(np.argmin(np.abs(lam - target)))
        if grid and i <= grid[-1]:
            i = grid[-1] + 1
        if i > T - 1:
            raise ValueError(f"{n} distinct steps do not fit")
        grid.append(i)
    return grid


def timesteps(base_betas, spec):
    if spec.startswith("logsnr"):
        return logsnr_grid(base_betas, int(spec[len("logsnr"):]))
    return sorted(SR.space_timesteps(len(base_betas), spec))


class DPMSolver:
    """The respaced schedule abar'_k = prod of the respaced alphas (SpacedDiffusion's), abar'_{-1} = 1."""

    def __init__(self, base_betas, spec, order=2):
        self.sd = SR.SpacedDiffusion(base_betas, set(timesteps(base_betas, spec)))
        self.timestep_map = self.sd.timestep_map
        self.K = self.sd.num_timesteps
        self.order = order

    def _ab(self, k):
        return 1.0 if k < 0 else float(self.sd.alphas_cumprod[k])

    def _lam(self, k):
        a = self._ab(k)
        return math.log(math.sqrt(a) / math.sqrt(1.0 - a))

    def step(self, x, x0, hist, k):
        """x_{k-1} from x_k with the clipped x0_k and the past predictions hist (most recent last)."""
        f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()
        a_prev = self._ab(k - 1)
        alpha_prev, sigma_prev = math.sqrt(a_prev), math.sqrt(1.0 - a_prev)
        sigma = math.sqrt(1.0 - self._ab(k))
        if k == 0:                                       # lambda_{-1} = inf: exp(-h) = 0, sigma_prev = 0
            return f32(alpha_prev) * x0
        h = self._lam(k - 1) - self._lam(k)
        second = self.order == 2 and len(hist) > 0
        if second:
            r = (self._lam(k) - self._lam(k + 1)) / h
            D = f32(1.0 + 1.0 / (2.0 * r)) * x0 - f32(1.0 / (2.0 * r)) * hist[-1]
        else:
            D = x0
        return f32(sigma_prev / sigma) * x + f32(-alpha_prev * math.expm1(-h)) * D

    def run(self, eps_model, x, k_start=None, k_end=0):
        k_start = self.K - 1 if k_start is None else k_start
        hist = []
        with torch.no_grad():
            for k in range(k_start, k_end - 1, -1):
                x0, _ = self.sd._pred_xstart(eps_model, x, k)
                x = self.step(x, x0, hist, k)
                hist.append(x0)
        return x
