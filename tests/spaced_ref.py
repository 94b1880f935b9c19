"""Independent restatement of improved-diffusion's respaced sampling (respace.py: space_timesteps, SpacedDiffusion;
gaussian_diffusion.py: p_sample, ddim_sample) in their DIRECT form, for the spaced / DDIM tests.

Nothing here imports models.diffusion.respace: the schedule is recomputed from the oracle's float64 betas, coefficients are
float64 numpy arrays gathered per step and cast to fp32 as improved-diffusion's _extract_into_tensor does, and DDIM recomputes
eps from the clipped pred_xstart and forms mean_pred = pred_xstart * sqrt(abar_prev) + sqrt(1 - abar_prev - sigma^2) * eps, rather
than the library's linear c1 / c2 tables.  The eps model is oracle/unet_ref.unet_forward at the ORIGINAL timestep map[k]
(SpacedDiffusion's _WrappedModel, rescale_timesteps off)."""
import numpy as np
import torch

from oracle import diffusion_ref as D


def space_timesteps(num_timesteps, section_counts):
    """respace.py:space_timesteps (a set, as there)."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            desired_count = int(section_counts[len("ddim"):])
            for i in range(1, num_timesteps):
                if len(range(0, num_timesteps, i)) == desired_count:
                    return set(range(0, num_timesteps, i))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    size_per = num_timesteps // len(section_counts)
    extra = num_timesteps % len(section_counts)
    start_idx = 0
    all_steps = []
    for i, section_count in enumerate(section_counts):
        size = size_per + (1 if i < extra else 0)
        if size < section_count:
            raise ValueError(f"cannot divide section of {size} steps into {section_count}")
        frac_stride = 1 if section_count <= 1 else (size - 1) / (section_count - 1)
        cur_idx = 0.0
        taken_steps = []
        for _ in range(section_count):
            taken_steps.append(start_idx + round(cur_idx))
            cur_idx += frac_stride
        all_steps += taken_steps
        start_idx += size
    return set(all_steps)


class SpacedDiffusion:
    """GaussianDiffusion (fixed-small variance, eps prediction, clipped x_start) over the respaced betas."""

    def __init__(self, base_betas, use_timesteps):
        base_acp = np.cumprod(1.0 - np.asarray(base_betas, dtype=np.float64))
        self.timestep_map = []
        last, new_betas = 1.0, []
        for i, acp in enumerate(base_acp):
            if i in use_timesteps:
                new_betas.append(1 - acp / last)
                last = acp
                self.timestep_map.append(i)
        betas = np.array(new_betas, dtype=np.float64)
        self.num_timesteps = len(betas)
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)

    @staticmethod
    def _extract(arr, k, x):
        return torch.from_numpy(arr)[k].float().reshape(-1, 1, 1, 1).expand_as(x)

    def _pred_xstart(self, eps_model, x, k):
        t = torch.full((x.shape[0],), self.timestep_map[k], dtype=torch.long)
        kk = torch.full((x.shape[0],), k, dtype=torch.long)
        eps = eps_model(x, t)
        x0 = self._extract(self.sqrt_recip_alphas_cumprod, kk, x) * x - self._extract(self.sqrt_recipm1_alphas_cumprod, kk, x) * eps
        return x0.clamp(-1, 1), kk

    def p_sample(self, eps_model, x, k, noise):
        pred_xstart, kk = self._pred_xstart(eps_model, x, k)
        mean = self._extract(self.posterior_mean_coef1, kk, x) * pred_xstart + self._extract(self.posterior_mean_coef2, kk, x) * x
        log_var = self._extract(self.posterior_log_variance_clipped, kk, x)
        nonzero = float(k != 0)
        return mean + nonzero * torch.exp(0.5 * log_var) * noise

    def ddim_sample(self, eps_model, x, k, noise, eta):
        pred_xstart, kk = self._pred_xstart(eps_model, x, k)
        eps = (self._extract(self.sqrt_recip_alphas_cumprod, kk, x) * x - pred_xstart) / self._extract(self.sqrt_recipm1_alphas_cumprod, kk, x)
        alpha_bar = self._extract(self.alphas_cumprod, kk, x)
        alpha_bar_prev = self._extract(self.alphas_cumprod_prev, kk, x)
        sigma = eta * torch.sqrt((1 - alpha_bar_prev) / (1 - alpha_bar)) * torch.sqrt(1 - alpha_bar / alpha_bar_prev)
        mean_pred = pred_xstart * torch.sqrt(alpha_bar_prev) + torch.sqrt(1 - alpha_bar_prev - sigma ** 2) * eps
        nonzero = float(k != 0)
        return mean_pred + nonzero * sigma * noise

    def run(self, eps_model, x, draw, k_start=None, k_end=0, ddim=False, eta=0.0):
        """steps k_start .. k_end; draw(j) is the j-th draw in run order (j = 0 at k_start)."""
        k_start = self.num_timesteps - 1 if k_start is None else k_start
        with torch.no_grad():
            for j, k in enumerate(range(k_start, k_end - 1, -1)):
                z = draw(j)
                x = self.ddim_sample(eps_model, x, k, z, eta) if ddim else self.p_sample(eps_model, x, k, z)
        return x


def linear_betas(T=1000):
    return D.beta_schedule("linear", T)
