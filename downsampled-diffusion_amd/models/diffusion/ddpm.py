"""DDPM with the reference's constructor / method surface (reference models/diffusion/ddpm.py:22-457),
its hot path on HIP kernels.

Hot path (HIP): q_sample, the UNet call, the fused reverse-step update, the T-step sampling loop (one C
call, hipGraph-replayed), the per-sample squared-error loss.
Evaluation path: test_losses_ = T x {q_sample kernel, HIP UNet, one fused VLB kernel
(normal_kl + discretised NLL + flat_bits + L_simple)}, or with seed= / noise= the whole sweep as one native call
(ddk_vlb_sweep_run: the sampler's graph-replayed step with a q_sample input and a VLB epilogue); q_mean_variance / q_posterior / p_mean_variance / calc_prior
stay plain torch expressions on device tensors (a few [B] / [T] gathers, init-time cost).
"""
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from ddk import ops
from ddk.lib import DDKError
from utils import flat_bits, reduce_mean, reduce_sum
from models.utils import discretized_gaussian_log_likelihood, extract, l2_loss, noise_like, normal_kl
from . import blur, hadamard, psf, respace
from .beta_schedule import make_beta_schedule

OBJETIVE_NAMES = ['simple', 'hybrid', 'vlb']
SOLVERS = ('dpm++2m',)


def _once(make):
    """make(*args) at the first call; that first result at every call."""
    made = []

    def get(*args):
        if not made:
            made.append(make(*args))
        return made[0]
    return get


class DDPM(nn.Module):
    def __init__(self, config: dict, latent_model: nn.Module, device: str, color_channels: int = 3):
        super().__init__()
        self.in_channels = color_channels
        self.latent_model = latent_model
        self.device = device
        self.image_size = config['image_size']
        self.timesteps = config['T']
        self.sample_shape = [self.in_channels, self.image_size, self.image_size]
        self.clip_denoised = True
        self.clip_range = (-1., 1.)

        self.L = config['loss_type']
        self.lambda_ = 0.0001
        assert self.L in OBJETIVE_NAMES
        self.get_loss = partial(l2_loss, reduction='none')
        if config['loss_flat'] == 'mean':
            self.flatten_loss = reduce_mean
        elif config['loss_flat'] == 'sum':
            self.flatten_loss = reduce_sum
        else:
            raise ValueError(f'Can only do mean or sum for flatten of loss, but {config["loss_flat"]} was desired..')
        self.loss_flat = config['loss_flat']

        # ---- schedule: float64 on the host, then 12 persistent fp32 buffers (ddpm.py:54-95)
        betas = make_beta_schedule(config['beta_schedule'], self.timesteps)
        assert (betas > 0).all() and (betas <= 1).all(), 'betas must be in (0, 1]'
        self._betas64 = np.asarray(betas, dtype=np.float64)    # source of the respaced / DDIM tables (not a buffer)
        f32_tables = respace.fp32_tables(respace.schedule_arrays(betas))
        for name in respace.SCHEDULE_NAMES:
            self.register_buffer(name, f32_tables[name])
        alphas = 1. - betas

        # L_vlb weights from L_simple (ddpm.py:97-106), non-persistent like the reference
        f32 = partial(torch.tensor, dtype=torch.float32)
        vlb_weights = self.betas ** 2 / (2 * self.posterior_variance * f32(alphas) * (1 - self.alphas_cumprod))
        vlb_weights[0] = vlb_weights[1]
        self.register_buffer('vlb_weights', vlb_weights, persistent=False)
        assert not torch.isnan(self.vlb_weights).all()
        # exp(0.5 * logvar) of ddpm.py:227 evaluated once with the same fp32 torch ops (non-persistent)
        self.register_buffer('posterior_sigma', f32_tables['posterior_sigma'], persistent=False)
        self._spaced = {}      # (chain's key, device) -> (tables, timestep map): see _cached_tables

        # sampler knobs (not in the reference): native hipGraph loop + in-kernel Philox noise by default
        self.native_sampler = True
        self.use_graph = True
        self.rng_stream_id = 0   # set to the rank for batch-sharded sampling

    # ------------------------------------------------------------------ helpers
    def _tables(self):
        return dict(c_recip=self.sqrt_recip_alphas_cumprod, c_recipm1=self.sqrt_recipm1_alphas_cumprod,
                    c1=self.posterior_mean_coef1, c2=self.posterior_mean_coef2, sigma=self.posterior_sigma)

    def _check_device(self, x):
        if not x.is_cuda:
            raise DDKError("DDPM: tensors are on the CPU; the HIP path needs a ROCm device (no CPU fallback)")

    def _eps_model_nhwc(self):
        lm = self.latent_model
        if not hasattr(lm, "plan"):
            raise DDKError("native sampling needs a models.Unet latent_model")
        return lm

    # ------------------------------------------------------------------ q(x_t | x)
    def q_mean_variance(self, x, t):
        """ddpm.py:108-124 (evaluation only)."""
        mean = extract(self.sqrt_alphas_cumprod, t, x.shape) * x
        variance = extract(1. - self.alphas_cumprod, t, x.shape)
        log_variance = extract(self.log_one_minus_alphas_cumprod, t, x.shape)
        return mean, variance, log_variance

    def q_sample(self, x, t, eps):
        """x_t = sqrt(abar_t) x + sqrt(1 - abar_t) eps (ddpm.py:256-273), one fused kernel."""
        assert x.shape == eps.shape
        self._check_device(x)
        if torch.is_grad_enabled() and x.requires_grad:      # only the non-autoencoder dDDPM loss differentiates through z_t
            from ddk import autograd as AG
            return AG.QSampleFn.apply(x.contiguous(), eps.contiguous(), t.contiguous(), self.sqrt_alphas_cumprod,
                                      self.sqrt_one_minus_alphas_cumprod)
        return ops.q_sample(x.contiguous(), eps.contiguous(), t.contiguous(), self.sqrt_alphas_cumprod,
                            self.sqrt_one_minus_alphas_cumprod)

    # ------------------------------------------------------------------ p(x_{t-1} | x_t)
    def predict_x_from_eps(self, x_t, t, eps, clip=True):
        """ddpm.py:149-158 (standalone use is evaluation only; sampling uses the fused update)."""
        assert x_t.shape == eps.shape
        x = (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
             - extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * eps)
        if clip:
            x.clamp_(*self.clip_range)
        return x

    def q_posterior(self, x, x_t, t):
        """ddpm.py:160-185."""
        assert x.shape == x_t.shape
        mean = (extract(self.posterior_mean_coef1, t, x_t.shape) * x
                + extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        variance = extract(self.posterior_variance, t, x_t.shape)
        log_variance = extract(self.posterior_log_variance_clipped, t, x_t.shape)
        return mean, variance, log_variance

    def p_mean_variance(self, x_t, t):
        """ddpm.py:187-201."""
        eps_hat = self.latent_model(x_t, t)
        x_recon = self.predict_x_from_eps(x_t, t, eps_hat, clip=True)
        return self.q_posterior(x_recon, x_t, t)

    @torch.no_grad()
    def p_sample(self, x_t, t, repeat_noise=False):
        """One reverse step (ddpm.py:203-227): UNet, then ONE fused kernel for
        clamp(x0) -> posterior mean -> + [t>0] sigma_t z.  Noise comes from torch's generator exactly as in
        the reference (drawn after the UNet call, also at t == 0)."""
        self._check_device(x_t)
        eps_hat = self.latent_model(x_t, t)
        z = noise_like(x_t.shape, x_t.device, repeat_noise)
        x = x_t.contiguous().clone()
        return ops.p_sample_update_(x, eps_hat.contiguous(), t.contiguous(), noise=z.contiguous(), **self._tables())

    def _cached_tables(self, key, build):
        """build() -> (tables, timestep map), made once per (key, device) and kept with the tables on the model's device:
        repeated calls pass the same table tensors, so they hit the plan's graph cache."""
        device = self.betas.device
        key = (*key, str(device))
        hit = self._spaced.get(key)
        if hit is None:
            tables, use = build()
            hit = self._spaced[key] = ({k: v.to(device) for k, v in tables.items()}, use)
        return hit

    def _spaced_tables(self, respacing, ddim, eta):
        """(tables, timestep map) of a respaced / DDIM chain (respace.spaced_tables); see _cached_tables."""
        return self._cached_tables((respacing, bool(ddim), float(eta)),
                                   lambda: respace.spaced_tables(self._betas64, respacing, ddim, eta))

    def _solver_tables(self, respacing, solver, order=2):
        """(tables c_recip, c_recipm1, c1, c2, c3, timestep map) of a DPM-Solver++(2M) chain (respace.dpm_solver_tables); order 1
        (restore_solver only) is the same chain with c3 = 0 in every row."""
        key = ('solver', respacing, solver) if order == 2 else ('solver', respacing, solver, order)
        return self._cached_tables(key, lambda: respace.dpm_solver_tables(self._betas64, respacing, order=order))

    def _chain_start(self, shape, x_T, early_stop, get_tables):
        """(device, tables, use, start state, k_start, k_end) of a chain with (tables, use) = get_tables(), asked for once the
        device is known to be a GPU.  `use` is the timestep map (None: all T timesteps): the chain runs steps k_start .. k_end of
        its tables, step k at timestep use[k]; early_stop keeps the steps whose timestep is >= early_stop."""
        device = self.betas.device
        if device.type != 'cuda':
            raise DDKError("p_sample_loop: move the model to a ROCm device first (no CPU fallback)")
        tables, use = get_tables()
        if use is None:
            k_start, k_end = self.timesteps - 1, 0 if early_stop is None else early_stop
        else:
            k_start = len(use) - 1
            k_end = 0 if early_stop is None else next((k for k, t in enumerate(use) if t >= early_stop), len(use))
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        return device, tables, use, img, k_start, k_end

    @torch.no_grad()
    def p_sample_loop(self, shape, every=1, early_stop=None, x_T=None, noise=None, seed=None, *, respacing=None, ddim=False,
                      eta=0.0, solver=None):
        """ddpm.py:229-249.  ``every`` is unused (as in the reference).  Extra keyword-only style arguments:
        x_T / noise inject the start state and the per-step draws ([n_steps, *shape]) for parity tests;
        seed fixes the in-kernel Philox stream (default: drawn from torch's generator).

        respacing / ddim / eta (improved-diffusion's timestep_respacing, use_ddim, eta): run K of the T timesteps
        (respace.space_timesteps spec, e.g. "ddim50", "250", "10,10,10"; None keeps all T), as ancestral steps of the respaced
        DDPM or, with ddim=True, as DDIM steps with noise scale eta.  early_stop then runs the spaced steps whose original
        timestep is >= early_stop; noise holds one draw per spaced step run, in run order; the in-kernel Philox draw of spaced
        step k is keyed by k (not by its original timestep).  The defaults run the plain T-step chain.

        solver="dpm++2m": DPM-Solver++(2M) steps over the respacing's timesteps (use "logsnrN").  The
        solver is deterministic: it cannot be combined with ddim, eta or noise (ValueError, before any device work); seed is
        unused.  early_stop cuts the bottom of the chain as for DDIM."""
        if solver is not None:
            if solver not in SOLVERS:
                raise ValueError(f"p_sample_loop: solver must be one of {SOLVERS} or None, got {solver!r}")
            if ddim or eta != 0 or noise is not None:
                raise ValueError(f"p_sample_loop: solver={solver!r} is deterministic and its own update: no ddim, eta or noise")
            return self._solver_loop(shape, early_stop, x_T, respacing, solver)
        spaced = respacing is not None or ddim or eta != 0
        if spaced and (eta < 0 or (eta != 0 and not ddim)):
            raise ValueError(f"p_sample_loop: eta = {eta} needs ddim=True and eta >= 0")
        device, tables, use, img, k_start, k_end = self._chain_start(
            shape, x_T, early_stop, lambda: self._spaced_tables(respacing, ddim, eta) if spaced else (self._tables(), None))
        if k_end > k_start:
            return img
        n_steps = k_start - k_end + 1
        if spaced and noise is not None and tuple(noise.shape) != (n_steps, *shape):
            raise DDKError(f"p_sample_loop: noise must be {(n_steps, *shape)} (one draw per spaced step), got {tuple(noise.shape)}")
        if not self.native_sampler:
            if not spaced:
                for i in reversed(range(k_end, k_start + 1)):      # the reference's own loop shape
                    t = torch.full((shape[0],), i, device=device, dtype=torch.long)
                    img = self.p_sample(img, t)
                return img
            # the same update as a Python loop: UNet at the original timestep, the fused update at the spaced index k
            for j, k in enumerate(range(k_start, k_end - 1, -1)):
                self._check_device(img)
                eps_hat = self.latent_model(img, torch.full((shape[0],), use[k], device=device, dtype=torch.long))
                z = noise_like(img.shape, device) if noise is None else noise[j].to(device).float()
                img = img.contiguous().clone()
                ops.p_sample_update_(img, eps_hat.contiguous(), torch.full((shape[0],), k, device=device, dtype=torch.long),
                                     noise=z.contiguous(), **tables)
            return img
        unet = self._eps_model_nhwc()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        x = ops.nchw_to_nhwc(img.contiguous())
        nz = None
        if noise is not None:
            nz = noise.to(device).float().permute(0, 1, 3, 4, 2).contiguous()   # [k,B,C,H,W] -> [k,B,H,W,C]
        unet.plan().sample_nhwc(x, tables, k_start, k_end, noise=nz, seed=seed, stream_id=self.rng_stream_id,
                                use_graph=self.use_graph, timesteps=use)
        return ops.nhwc_to_nchw(x)

    def _solver_loop(self, shape, early_stop, x_T, respacing, solver):
        """p_sample_loop(solver=...): steps k_start .. k_end of the solver's tables, step k at timestep use[k]; native
        (UnetPlan.sample_multistep_nhwc) or, with native_sampler off, the same update as a Python loop."""
        device, tables, use, img, k_start, k_end = self._chain_start(shape, x_T, early_stop,
                                                                     lambda: self._solver_tables(respacing, solver))
        if k_end > k_start:
            return img
        if not self.native_sampler:
            hist = torch.zeros_like(img).contiguous()
            for k in range(k_start, k_end - 1, -1):
                self._check_device(img)
                eps_hat = self.latent_model(img, torch.full((shape[0],), use[k], device=device, dtype=torch.long))
                img = img.contiguous().clone()
                ops.p_sample_update_multistep_(img, eps_hat.contiguous(), hist, torch.full((shape[0],), k, device=device, dtype=torch.long),
                                               **tables)
            return img
        x = ops.nchw_to_nhwc(img.contiguous())
        self._eps_model_nhwc().plan().sample_multistep_nhwc(x, tables, k_start, k_end, stream_id=self.rng_stream_id,
                                                            use_graph=self.use_graph, timesteps=use)
        return ops.nhwc_to_nchw(x)

    @torch.no_grad()
    def sample(self, batch_size=16, every=1, early_stop=None, *, respacing=None, ddim=False, eta=0.0, solver=None):
        """ddpm.py:251-254 (respacing / ddim / eta / solver: see p_sample_loop)."""
        return self.p_sample_loop((batch_size, *self.sample_shape), every, early_stop, respacing=respacing, ddim=ddim, eta=eta,
                                  solver=solver)

    # ------------------------------------------------------------------ RePaint inpainting (not in the reference)
    INPAINT_UNSUPPORTED = ('ddim', 'solver', 'eta', 'noise', 'early_stop')

    def _inpaint_args(self, x, mask, shape, jump_length, jump_n_sample, unsupported):
        """ValueError for anything inpaint cannot take, before any device work.  Returns (x as float, mask as a float {0, 1}
        tensor broadcast to [B, C, H, W]), both on x's device.  ``shape`` is [C, H, W] of the image."""
        if unsupported:
            raise ValueError(f"inpaint: {sorted(unsupported)} not accepted (RePaint runs ancestral steps with Philox draws over the "
                             f"whole schedule: no {', '.join(self.INPAINT_UNSUPPORTED)})")
        for name, v in (("jump_length", jump_length), ("jump_n_sample", jump_n_sample)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"inpaint: {name} must be an int >= 1, got {v!r}")
        if not (0 <= int(self.rng_stream_id) < 2 ** 29):
            raise ValueError(f"inpaint: rng_stream_id must be < 2^29 (bits 29, 30 key the extra draws), got {self.rng_stream_id}")
        if not torch.is_tensor(x) or x.dim() != 4 or list(x.shape[1:]) != list(shape) or not x.is_floating_point():
            raise ValueError(f"inpaint: x must be a float [B, {', '.join(map(str, shape))}] tensor, got "
                             f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if not torch.is_tensor(mask) or mask.is_complex():
            raise ValueError("inpaint: mask must be a real or bool tensor")
        B, C, H, W = x.shape
        m = mask
        if m.dim() > 4:
            raise ValueError(f"inpaint: mask must broadcast to [B, 1|C, H, W], got {tuple(m.shape)}")
        while m.dim() < 4:
            m = m.unsqueeze(0)
        if m.shape[0] not in (1, B) or m.shape[1] not in (1, C) or tuple(m.shape[2:]) != (H, W):
            raise ValueError(f"inpaint: mask must broadcast to [{B}, 1|{C}, {H}, {W}], got {tuple(mask.shape)}")
        if m.dtype != torch.bool and not bool(((m == 0) | (m == 1)).all()):
            raise ValueError("inpaint: mask values must be 0 or 1 (or bool)")
        m = m.to(device=x.device, dtype=torch.float32).expand(B, C, H, W).contiguous()
        if not bool(torch.isfinite(x[m != 0]).all()):
            raise ValueError("inpaint: the known pixels of x must be finite")
        return x.float(), m

    def _inpaint_tables(self, respacing, jump_length, jump_n_sample):
        """(tables c_recip .. sigma, ka, kb, ja, jb, timestep map) of a RePaint chain (respace.repaint_tables)."""
        j, r = int(jump_length), int(jump_n_sample)
        return self._cached_tables(('repaint', respacing, j, r), lambda: respace.repaint_tables(self._betas64, respacing, j, r))

    def _inpaint_loop(self, z0, m, respacing, jump_length, jump_n_sample, x_T, seed):
        """RePaint over the latent z0 [B, *sample_shape] with mask m (same shape, {0, 1}): native (UnetPlan.sample_inpaint_nhwc) or,
        with native_sampler off, the same op as a Python loop in the same NHWC layout, so both draw the same Philox numbers."""
        device = self.betas.device
        if device.type != 'cuda':
            raise DDKError("inpaint: move the model to a ROCm device first (no CPU fallback)")
        tables, use = self._inpaint_tables(respacing, jump_length, jump_n_sample)
        shape = tuple(z0.shape)
        if x_T is not None and tuple(x_T.shape) != shape:
            raise ValueError(f"inpaint: x_T must be {shape}, got {tuple(x_T.shape)}")
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        z0, m = z0.to(device).float(), m.to(device)
        known = ops.nchw_to_nhwc(torch.where(m != 0, z0, torch.zeros_like(z0)).contiguous())   # nothing hidden reaches the chain
        mk = ops.nchw_to_nhwc(m.contiguous())
        x = ops.nchw_to_nhwc(img.contiguous())
        if not self.native_sampler:
            for k in range(len(use) - 1, -1, -1):
                eps_hat = self.latent_model(ops.nhwc_to_nchw(x), torch.full((shape[0],), use[k], device=device, dtype=torch.long))
                ops.p_sample_update_inpaint_(x, ops.nchw_to_nhwc(eps_hat.contiguous()), known, mk,
                                             torch.full((shape[0],), k, device=device, dtype=torch.long), **tables, seed=seed,
                                             stream_id=int(self.rng_stream_id))
            return ops.nhwc_to_nchw(x)
        self._eps_model_nhwc().plan().sample_inpaint_nhwc(x, known, mk, tables, use, seed=seed, stream_id=int(self.rng_stream_id),
                                                          use_graph=self.use_graph)
        return ops.nhwc_to_nchw(x)

    @torch.no_grad()
    def inpaint(self, x, mask, *, respacing=None, jump_length=10, jump_n_sample=10, x_T=None, seed=None, **unsupported):
        """RePaint inpainting (Lugmayr et al. 2022): fill the pixels of x [B, C, H, W] (in [-1, 1]) where
        mask is 0; mask broadcasts to [B, 1|C, H, W] with values in {0, 1} or bool (1 = known).  Runs the RePaint schedule
        (respace.repaint_schedule) over the respacing's K steps (None: all T) with jumps of jump_length, each resampled
        jump_n_sample times.  x_T: the start state; seed: the Philox key (default: drawn from torch's generator).  The known pixels
        of the result equal x exactly; the hidden pixels of x are never read.  ddim / solver / eta / noise / early_stop raise
        ValueError, as do bad masks, before any device work."""
        x, m = self._inpaint_args(x, mask, self.sample_shape, jump_length, jump_n_sample, unsupported)
        return self._inpaint_loop(x, m, respacing, jump_length, jump_n_sample, x_T, seed)

    # ------------------------------------------------------------------ what the DDNM entries' argument checks share
    @staticmethod
    def _eta_arg(who, ddim, eta):
        """ValueError unless eta is a real number >= 0, and 0 without ddim."""
        if isinstance(eta, bool) or not isinstance(eta, (int, float, np.integer, np.floating)) or eta < 0 or (eta != 0 and not ddim):
            raise ValueError(f"{who}: eta = {eta!r} needs ddim=True and eta >= 0")

    @staticmethod
    def _tol_arg(who, tol):
        """ValueError unless tol is a real number in [0, 1)."""
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (0 <= tol < 1):
            raise ValueError(f"{who}: tol must be a real number in [0, 1), got {tol!r}")

    @staticmethod
    def _y_arg(who, y, shape, min_batch=0, finite=True):
        """ValueError unless y is a float [B, *shape] tensor (a str in shape: any size, named so in the message) with B >= min_batch
        and, with `finite`, no Inf or NaN.  Returns y as float."""
        if not torch.is_tensor(y) or y.dim() != len(shape) + 1 or y.shape[0] < min_batch or not y.is_floating_point() or \
                any(not isinstance(s, str) and d != s for d, s in zip(y.shape[1:], shape)):
            raise ValueError(f"{who}: y must be a float [B, {', '.join(map(str, shape))}] tensor, got "
                             f"{tuple(y.shape) if torch.is_tensor(y) else type(y).__name__}")
        if finite and not bool(torch.isfinite(y).all()):
            raise ValueError(f"{who}: y must be finite")
        return y.float()

    def _chain_tables(self, respacing, ddim, eta):
        """() -> (tables, timestep map or None) of an ancestral or DDIM chain: the spaced tables, or for the plain chain the model's own."""
        spaced = respacing is not None or ddim or eta != 0
        return lambda: self._spaced_tables(respacing, ddim, eta) if spaced else (self._tables(), None)

    # ------------------------------------------------------------------ DDNM super-resolution (not in the reference)
    RESTORE_UNSUPPORTED = ('solver', 'noise', 'early_stop')
    RESTORE_BLOCKS = (2, 4, 8)

    def _restore_args(self, y, scale, shape, ddim, eta, unsupported, block=1):
        """ValueError for anything super_resolve cannot take, before any device work.  Returns y as float.  ``shape`` is [C, H, W]
        of the full-resolution image; the chain's block is scale / block (the dDDPM runs it in a latent dim_reduc times smaller)."""
        if unsupported:
            raise ValueError(f"super_resolve: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws "
                             f"over the whole schedule: no {', '.join(self.RESTORE_UNSUPPORTED)})")
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale % block or scale // block not in self.RESTORE_BLOCKS:
            raise ValueError(f"super_resolve: scale must be an int in {tuple(block * n for n in self.RESTORE_BLOCKS)}, got {scale!r}")
        if eta < 0 or (eta != 0 and not ddim):
            raise ValueError(f"super_resolve: eta = {eta} needs ddim=True and eta >= 0")
        C, H, W = shape
        if H % scale or W % scale:
            raise ValueError(f"super_resolve: scale = {scale} must divide the image size {H} x {W}")
        return self._y_arg("super_resolve", y, (C, H // scale, W // scale))

    def _ddnm_loop(self, who, y, mask, get_tables, x_T, seed, op, chain):
        """What the DDNM chains share, over the latent measured as y ([B, C, h, w], or the grey [B, h, w]) where mask [B, h, w] (None:
        everywhere) is 1: the device check, (tables, timestep map or None) = get_tables(), x_T, the Philox seed (drawn from torch's
        generator when None), then all the tables' steps, native or -- with native_sampler off -- as a Python loop over the same op in
        the same NHWC layout, so both draw the same Philox numbers.  chain(plan, x, y, mask, tables, k_start, seed, use) runs the
        native chain in place on the NHWC x; op(x, eps_hat, y, mask, t, tables, seed) is one step of it."""
        device = self.betas.device
        if device.type != 'cuda':
            raise DDKError(f"{who}: move the model to a ROCm device first (no CPU fallback)")
        tables, use = get_tables()
        shape = (y.shape[0], *self.sample_shape)
        if x_T is not None and tuple(x_T.shape) != shape:
            raise ValueError(f"{who}: x_T must be {shape}, got {tuple(x_T.shape)}")
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        k_start = (self.timesteps if use is None else len(use)) - 1
        yl = y.to(device).float().contiguous()
        if yl.dim() == 4:
            yl = ops.nchw_to_nhwc(yl)
        mk = None if mask is None else mask.to(device).float().contiguous()
        x = ops.nchw_to_nhwc(img.contiguous())
        plan = self._eps_model_nhwc().plan()
        if self.native_sampler:
            chain(plan, x, yl, mk, tables, k_start, seed, use)
            return ops.nhwc_to_nchw(x)
        # the loop's forwards pick their kernels as the chain's steps do (UnetPlan.forwards_as_in_chain): the two GroupNorm
        # paths sum in another order, and a few 1e-6 of eps_hat per step is more than the loop may differ from the chain
        with plan.forwards_as_in_chain():
            for k in range(k_start, -1, -1):
                t_model = k if use is None else use[k]
                eps_hat = self.latent_model(ops.nhwc_to_nchw(x), torch.full((shape[0],), t_model, device=device, dtype=torch.long))
                op(x, ops.nchw_to_nhwc(eps_hat.contiguous()), yl, mk, torch.full((shape[0],), k, device=device, dtype=torch.long), tables, seed)
        return ops.nhwc_to_nchw(x)

    def _restore_loop(self, y, n, respacing, ddim, eta, x_T, seed, mask=None, who="super_resolve"):
        """DDNM over the latent whose n x n block means are held at y [B, C, H/n, W/n] (UnetPlan.sample_restore_nhwc).  mask
        [B, H/n, W/n] ({0, 1} floats, restore() only): the blocks that are held (n = 1: the pixels that are set to y), by the masked
        op and UnetPlan.sample_restore_masked_nhwc."""
        sid, graph = int(self.rng_stream_id), self.use_graph
        if mask is None:
            def op(x, e, yl, mk, t, tables, seed):
                ops.p_sample_update_restore_(x, e, yl, n, t, **tables, seed=seed, stream_id=sid)

            def chain(plan, x, yl, mk, tables, k_start, seed, use):
                plan.sample_restore_nhwc(x, yl, n, tables, k_start, seed=seed, stream_id=sid, use_graph=graph, timesteps=use)
        else:
            def op(x, e, yl, mk, t, tables, seed):
                ops.p_sample_update_restore_masked_(x, e, yl, mk, n, t, **tables, seed=seed, stream_id=sid)

            def chain(plan, x, yl, mk, tables, k_start, seed, use):
                plan.sample_restore_masked_nhwc(x, yl, mk, n, tables, k_start, seed=seed, stream_id=sid, use_graph=graph, timesteps=use)
        return self._ddnm_loop(who, y, mask, self._chain_tables(respacing, ddim, eta), x_T, seed, op, chain)

    @torch.no_grad()
    def super_resolve(self, y, scale, *, downsample="mean", respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """Zero-shot super-resolution with DDNM (Wang, Yu, Zhang 2023): an image [B, C, H, W] whose
        scale x scale average pooling is y [B, C, H/scale, W/scale] (in [-1, 1]); scale in {2, 4, 8}.  downsample="bicubic": y is
        the antialiased bicubic reduction instead (blur.resize_matrix on both axes, what image libraries and the SR benchmarks
        make), restored by restore_separable: H and W multiples of 16 in [16, 256], H/scale and W/scale
        multiples of 4, and A(x_out) = y up to fp32 rounding.  Every step of the chain
        (all T steps, or respacing's K; ancestral, or DDIM with eta) shifts its clipped x0 so that its block means equal y before the
        update; the block means of the result equal y up to fp32 rounding.  x_T: the start state; seed: the Philox key (default:
        drawn from torch's generator).  solver / noise / early_stop raise ValueError, as do a bad scale, a non-finite or misshapen y
        and eta without ddim, before any device work."""
        if downsample not in ("mean", "bicubic"):
            raise ValueError(f"super_resolve: downsample must be 'mean' or 'bicubic', got {downsample!r}")
        y = self._restore_args(y, scale, self.sample_shape, ddim, eta, unsupported)
        if downsample == "bicubic":
            C, H, W = self.sample_shape
            if H % 16 or W % 16 or not (16 <= H <= 256 and 16 <= W <= 256) or (H // scale) % 4 or (W // scale) % 4:
                raise ValueError(f"super_resolve: downsample='bicubic' needs an image size of multiples of 16 in [16, 256] whose "
                                 f"{scale}-fold reduction is a multiple of 4, this model's is {H} x {W}")
            return self.restore_separable(y, blur.resize_matrix(H, int(scale)), blur.resize_matrix(W, int(scale)), respacing=respacing,
                                          ddim=ddim, eta=eta, x_T=x_T, seed=seed)
        return self._restore_loop(y, int(scale), respacing, ddim, eta, x_T, seed)

    # ------------------------------------------------------------------ DDNM with a mask: inpainting and masked super-resolution
    RESTORE_SCALES = (1, 2, 4, 8)

    def _restore_masked_args(self, y, mask, scale, shape, ddim, eta, unsupported, scales):
        """ValueError for anything restore cannot take, before any device work.  ``shape`` is [C, H, W] of the full-resolution
        image, ``scales`` the scales the caller takes.  Returns (y as float with the pixels that are not measured set to 0, the
        mask as {0, 1} floats [B, H/scale, W/scale] or None), on y's device."""
        if unsupported:
            raise ValueError(f"restore: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws "
                             f"over the whole schedule: no {', '.join(self.RESTORE_UNSUPPORTED)})")
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale not in scales:
            raise ValueError(f"restore: scale must be an int in {tuple(scales)}, got {scale!r}")
        self._eta_arg("restore", ddim, eta)
        if mask is None and scale == 1:
            raise ValueError("restore: scale = 1 needs a mask (nothing would be constrained)")
        C, H, W = shape
        if H % scale or W % scale:
            raise ValueError(f"restore: scale = {scale} must divide the image size {H} x {W}")
        h, w = H // scale, W // scale
        return self._measured_args(self._y_arg("restore", y, (C, h, w), finite=False), mask, h, w, "restore")

    @staticmethod
    def _measured_args(y, mask, h, w, who):
        """The mask's and the measured pixels' ValueErrors of restore (and of colorize, which takes the same masks): returns (y with
        the pixels that are not measured set to 0, the mask as {0, 1} floats [B, h, w] or None), on y's device."""
        B = y.shape[0]
        if mask is None:
            if not bool(torch.isfinite(y).all()):
                raise ValueError(f"{who}: y must be finite")
            return y, None
        if not torch.is_tensor(mask) or mask.is_complex():
            raise ValueError(f"{who}: mask must be a real or bool tensor")
        m = mask
        if m.dim() == 4 and m.shape[1] == 1:
            m = m[:, 0]
        elif m.dim() == 2:
            m = m.unsqueeze(0)
        if m.dim() != 3 or m.shape[0] not in (1, B) or tuple(m.shape[1:]) != (h, w):
            raise ValueError(f"{who}: mask must be [{h}, {w}], [{B}, {h}, {w}] or [{B}, 1, {h}, {w}], got {tuple(mask.shape)}")
        if m.dtype != torch.bool and not bool(((m == 0) | (m == 1)).all()):
            raise ValueError(f"{who}: mask values must be 0 or 1 (or bool)")
        m = m.to(device=y.device, dtype=torch.float32).expand(B, h, w).contiguous()
        if not bool((m.reshape(B, -1).amax(dim=1) > 0).all()):
            raise ValueError(f"{who}: every image needs at least one measured pixel (an all-zero mask constrains nothing)")
        sel = (m != 0).unsqueeze(1).expand_as(y)
        if not bool(torch.isfinite(y[sel]).all()):
            raise ValueError(f"{who}: the measured pixels of y must be finite")
        return torch.where(sel, y, torch.zeros_like(y)), m

    @torch.no_grad()
    def restore(self, y, mask=None, scale=1, *, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """Zero-shot restoration with DDNM for A = mask o (scale x scale average pooling): an image
        [B, C, H, W] whose pooling equals y [B, C, H/scale, W/scale] (in [-1, 1]) wherever mask is 1.  mask is [H/scale, W/scale],
        [B, H/scale, W/scale] or [B, 1, H/scale, W/scale] with values in {0, 1} or bool (1 = measured), shared by the channels.
        scale = 1 is inpainting in K = the respacing's steps (ancestral, or DDIM with eta): the measured pixels of the result equal
        y exactly and the others of y are never read.  scale in {2, 4, 8} with a mask upscales a low-resolution image with holes:
        the measured block means of the result equal y up to fp32 rounding; without a mask it is super_resolve.  x_T: the start
        state; seed: the Philox key (default: drawn from torch's generator).  solver / noise / early_stop raise ValueError, as do
        scale = 1 without a mask, a mask that is not {0, 1} or is all zero in some image, a misshapen y or mask, non-finite measured
        pixels and eta without ddim, before any device work."""
        y, m = self._restore_masked_args(y, mask, scale, self.sample_shape, ddim, eta, unsupported, self.RESTORE_SCALES)
        return self._restore_loop(y, int(scale), respacing, ddim, eta, x_T, seed, mask=m, who="restore")

    # ------------------------------------------------------------------ DDNM on the DPM-Solver++(2M) chain
    RESTORE_SOLVER_UNSUPPORTED = ('ddim', 'eta', 'seed', 'noise', 'early_stop')

    def _restore_solver_args(self, y, mask, scale, shape, solver, order, unsupported, scales):
        """ValueError for anything restore_solver cannot take, before any device work; then _restore_masked_args' checks and
        return value."""
        if unsupported:
            raise ValueError(f"restore_solver: {sorted(unsupported)} not accepted (the solver is deterministic and its own update over "
                             f"the whole grid: no {', '.join(self.RESTORE_SOLVER_UNSUPPORTED)})")
        if solver not in SOLVERS:
            raise ValueError(f"restore_solver: solver must be one of {SOLVERS}, got {solver!r}")
        if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order not in (1, 2):
            raise ValueError(f"restore_solver: order must be 1 or 2, got {order!r}")
        return self._restore_masked_args(y, mask, scale, shape, False, 0.0, {}, scales)

    def _restore_solver_loop(self, y, n, respacing, solver, order, x_T, mask=None):
        """DDNM on the solver's chain over the latent whose n x n block means are held at y [B, C, H/n, W/n] where mask [B, H/n, W/n]
        (None: everywhere) is 1 (UnetPlan.sample_restore_multistep_nhwc).  No draws: the seed is not used."""
        C, H, W = self.sample_shape
        # the Python loop's history, NHWC like x: zeros before its first step
        hist = None if self.native_sampler else torch.zeros(y.shape[0], H, W, C, device=self.betas.device)

        def op(x, e, yl, mk, t, tables, seed):
            ops.p_sample_update_restore_multistep_(x, e, hist, yl, mk, n, t, **tables)
        return self._ddnm_loop(
            "restore_solver", y, mask, lambda: self._solver_tables(respacing, solver, int(order)), x_T, 0, op,
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_multistep_nhwc(
                x, yl, mk, n, tables, k_start, stream_id=int(self.rng_stream_id), use_graph=self.use_graph, timesteps=use))

    @torch.no_grad()
    def restore_solver(self, y, mask=None, scale=1, *, respacing=None, solver="dpm++2m", order=2, x_T=None, **unsupported):
        """restore() in few steps: DDNM for A = mask o (scale x scale average pooling) on the
        DPM-Solver++(2M) chain over the respacing's timesteps (use "logsnrN").  Every step projects its clipped x0 onto
        {A x0 = y} and hands the solver that x0', as its data prediction and as its history.  y, mask, scale and their
        ValueErrors: as restore.  order = 1 drops the history term (DDNM on DDIM eta 0 in the solver's form).  Deterministic
        given x_T: ddim / eta / seed / noise / early_stop raise ValueError, as do an unknown solver and an order not in {1, 2},
        before any device work.  The measured pixels (scale 1) equal y exactly; measured block means equal y up to fp32 rounding."""
        y, m = self._restore_solver_args(y, mask, scale, self.sample_shape, solver, order, unsupported, self.RESTORE_SCALES)
        return self._restore_solver_loop(y, int(scale), respacing, solver, order, x_T, mask=m)

    # ------------------------------------------------------------------ DDNM+ for a noisy measurement
    @staticmethod
    def _sigma_y_arg(sigma_y, who):
        """ValueError unless sigma_y is a finite real number >= 0; returns it as a float."""
        if isinstance(sigma_y, bool) or not isinstance(sigma_y, (int, float, np.integer, np.floating)) or \
                not np.isfinite(sigma_y) or sigma_y < 0:
            raise ValueError(f"{who}: sigma_y must be a finite real number >= 0, got {sigma_y!r}")
        return float(sigma_y)

    def _noisy_tables(self, respacing, ddim, eta, sigma_y):
        """(restore's tables plus the per-row lam and sgm of respace.noisy_coefficients, timestep map or None) for this sigma_y,
        cached like _spaced_tables.  The plain chain keeps the model's own tables, as restore does."""
        if respacing is not None or ddim or eta != 0:
            return self._cached_tables(('noisy', respacing, bool(ddim), float(eta), sigma_y),
                                       lambda: respace.noisy_tables(self._betas64, respacing, ddim, eta, sigma_y))

        def plain():
            lam, sgm = respace.noisy_coefficients(respace.schedule_arrays(self._betas64)['posterior_mean_coef1'],
                                                  self.posterior_sigma.detach().double().cpu().numpy(), sigma_y)
            return dict(self._tables(), lam=torch.tensor(lam, dtype=torch.float32), sgm=torch.tensor(sgm, dtype=torch.float32)), None
        return self._cached_tables(('noisy', None, False, 0.0, sigma_y), plain)

    def _restore_noisy_loop(self, y, n, sigma_y, respacing, ddim, eta, x_T, seed, mask=None):
        """DDNM+ over the latent whose n x n block means are measured as y [B, C, H/n, W/n], with noise of standard deviation
        sigma_y, where mask [B, H/n, W/n] (None: everywhere) is 1 (UnetPlan.sample_restore_noisy_nhwc)."""
        sid = int(self.rng_stream_id)
        return self._ddnm_loop(
            "restore_noisy", y, mask, lambda: self._noisy_tables(respacing, ddim, eta, sigma_y), x_T, seed,
            lambda x, e, yl, mk, t, tables, seed: ops.p_sample_update_restore_noisy_(x, e, yl, mk, n, t, **tables, seed=seed, stream_id=sid),
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_noisy_nhwc(
                x, yl, mk, n, tables, k_start, seed=seed, stream_id=sid, use_graph=self.use_graph, timesteps=use))

    def _restore_noisy_args(self, y, mask, scale, shape, sigma_y, ddim, eta, unsupported, scales):
        """restore's ValueErrors (_restore_masked_args, whose return value this returns), then the chain whose draws are all zero."""
        y, m = self._restore_masked_args(y, mask, scale, shape, ddim, eta, unsupported, scales)
        if ddim and eta == 0:
            raise ValueError("restore_noisy: sigma_y > 0 needs a chain that draws (ancestral steps, or ddim with eta > 0): with eta = 0 "
                             "every row's lam is 0 and nothing would be constrained")
        return y, m

    @torch.no_grad()
    def restore_noisy(self, y, mask=None, scale=1, *, sigma_y, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """restore() for a measurement that is only known to +- sigma_y (DDNM+, Wang, Yu, Zhang 2023, section 3.3; DESIGN.md
        section 3.10): y = A x + noise of standard deviation sigma_y, in y's own [-1, 1] scale.  Every step scales its correction
        of x0 by the row's lam <= 1 and the draw on measured elements by the row's sgm <= sigma, so that the noise entering through
        y and the drawn noise add up to the chain's own variance; the last step returns the model's own x0, so y is never pasted
        into the result.  y, mask, scale, the other keywords and their ValueErrors: as restore.  sigma_y must be a finite real
        number >= 0; sigma_y == 0 is restore itself.  With sigma_y > 0 a chain that draws nothing (ddim=True with eta == 0) raises
        ValueError: lam would be 0 in every row.  All before any device work."""
        sigma_y = self._sigma_y_arg(sigma_y, "restore_noisy")
        if sigma_y == 0:
            return self.restore(y, mask, scale, respacing=respacing, ddim=ddim, eta=eta, x_T=x_T, seed=seed, **unsupported)
        y, m = self._restore_noisy_args(y, mask, scale, self.sample_shape, sigma_y, ddim, eta, unsupported, self.RESTORE_SCALES)
        return self._restore_noisy_loop(y, int(scale), sigma_y, respacing, ddim, eta, x_T, seed, mask=m)

    # ------------------------------------------------------------------ DDNM colourisation and grey super-resolution
    GRAY_WEIGHTS = ("mean", "luma")
    COLORIZE_UNSUPPORTED = ('solver', 'noise', 'early_stop', 'paste')

    def _gray_tables(self, respacing, ddim, eta, sigma_y):
        """(restore's tables plus the per-row lam and sgm of a colourisation chain, timestep map or None), cached like _noisy_tables,
        whose tables these are for sigma_y > 0.  sigma_y == 0: lam = 1 in every row and sgm = the fp32 sigma with row 0 zero
        (respace.exact_coefficients)."""
        if sigma_y > 0:
            return self._noisy_tables(respacing, ddim, eta, sigma_y)
        if respacing is not None or ddim or eta != 0:
            return self._cached_tables(('gray', respacing, bool(ddim), float(eta)),
                                       lambda: respace.gray_tables(self._betas64, respacing, ddim, eta, 0.0))

        def plain():
            lam, sgm = respace.exact_coefficients(self.posterior_sigma)
            return dict(self._tables(), lam=lam, sgm=sgm), None
        return self._cached_tables(('gray', None, False, 0.0), plain)

    def _colorize_args(self, y, mask, scale, weights, sigma_y, ddim, eta, unsupported):
        """ValueError for anything colorize cannot take, before any device work.  Returns (y as float [B, H/scale, W/scale] with the
        pixels that are not measured set to 0, the mask as {0, 1} floats of that shape or None, sigma_y as a float)."""
        if unsupported:
            raise ValueError(f"colorize: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws over "
                             f"the whole schedule and never pastes: no {', '.join(self.COLORIZE_UNSUPPORTED)})")
        C, H, W = self.sample_shape
        if C != 3:
            raise ValueError(f"colorize: needs a 3-channel pixel model, this one has {C} channels")
        if weights not in self.GRAY_WEIGHTS:
            raise ValueError(f"colorize: weights must be one of {self.GRAY_WEIGHTS}, got {weights!r}")
        sigma_y = self._sigma_y_arg(sigma_y, "colorize")
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale not in self.RESTORE_SCALES:
            raise ValueError(f"colorize: scale must be an int in {self.RESTORE_SCALES}, got {scale!r}")
        self._eta_arg("colorize", ddim, eta)
        if sigma_y > 0 and ddim and eta == 0:
            raise ValueError("colorize: sigma_y > 0 needs a chain that draws (ancestral steps, or ddim with eta > 0): with eta = 0 every "
                             "row's lam is 0 and nothing would be constrained")
        if H % scale or W % scale:
            raise ValueError(f"colorize: scale = {scale} must divide the image size {H} x {W}")
        h, w = H // scale, W // scale
        y, m = self._measured_args(self._y_arg("colorize", y, (1, h, w), finite=False), mask, h, w, "colorize")
        return y[:, 0].contiguous(), m, sigma_y

    def _colorize_loop(self, y, mask, n, weights, sigma_y, respacing, ddim, eta, x_T, seed):
        """The colourisation chain on y, mask [B, H/n, W/n] (mask None: everywhere) (UnetPlan.sample_restore_gray_nhwc)."""
        sid = int(self.rng_stream_id)
        return self._ddnm_loop(
            "colorize", y, mask, lambda: self._gray_tables(respacing, ddim, eta, sigma_y), x_T, seed,
            lambda x, e, yl, mk, t, tables, seed: ops.p_sample_update_restore_gray_(x, e, yl, mk, n, weights, t, **tables, seed=seed,
                                                                                   stream_id=sid),
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_gray_nhwc(
                x, yl, mk, n, weights, tables, k_start, seed=seed, stream_id=sid, use_graph=self.use_graph, timesteps=use))

    @torch.no_grad()
    def colorize(self, y, mask=None, scale=1, *, weights="mean", sigma_y=0.0, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None,
                 **unsupported):
        """Zero-shot colourisation and grey super-resolution with DDNM (Wang, Yu, Zhang 2023), for 3-channel
        pixel models: an image [B, 3, H, W] whose grey value, averaged over scale x scale blocks, equals y [B, 1, H/scale, W/scale]
        (in [-1, 1]) wherever mask is 1.  weights: "mean" (the three channels averaged, DDNM's own operator) or "luma" (BT.601,
        0.299 R + 0.587 G + 0.114 B).  scale in {1, 2, 4, 8}; mask as restore's, optional at every scale (None: every pixel of y is
        measured).  sigma_y > 0: y carries noise of that standard deviation and the steps are DDNM+'s (restore_noisy's tables);
        with sigma_y == 0 the grey image of the result equals y up to fp32 rounding.  respacing, ddim, eta, x_T, seed: as restore.
        ValueError, before any device work, for a model that does not have 3 channels, solver / noise / early_stop / paste, unknown
        weights, a bad sigma_y, scale or eta, sigma_y > 0 on a chain without draws (ddim with eta == 0), a misshapen or non-float y,
        non-finite measured pixels and every mask restore rejects."""
        y, m, sigma_y = self._colorize_args(y, mask, scale, weights, sigma_y, ddim, eta, unsupported)
        return self._colorize_loop(y, m, int(scale), weights, sigma_y, respacing, ddim, eta, x_T, seed)

    # ------------------------------------------------------------------ DDNM deblurring (separable blur)
    DEBLUR_UNSUPPORTED = ('solver', 'noise', 'early_stop', 'paste', 'mask', 'sigma_y')

    def _blur_operands(self, kernel, tol):
        """{A_h, A_w, Q_h, Q_w, P_h, P_w} of blur.blur_operands on the model's device, cached per (taps, tol, device) like the spaced
        tables: repeated calls pass the same tensors."""
        C, H, W = self.sample_shape
        names = ("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w")
        return self._cached_tables(('blur', *blur._key(kernel), float(tol)),
                                   lambda: (dict(zip(names, blur.blur_operands(kernel, H, W, tol))), None))[0]

    def _deblur_args(self, y, kernel, tol, ddim, eta, unsupported):
        """ValueError for anything deblur cannot take, before any device work.  Returns y as float."""
        if unsupported:
            raise ValueError(f"deblur: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws over the "
                             f"whole schedule on an exact, unmasked measurement: no {', '.join(self.DEBLUR_UNSUPPORTED)})")
        blur.blur_kernel(kernel)      # its own ValueErrors
        self._tol_arg("deblur", tol)
        self._eta_arg("deblur", ddim, eta)
        C, H, W = self.sample_shape
        if H % 16 or W % 16 or not (16 <= H <= 256 and 16 <= W <= 256 and 1 <= C <= 8):
            raise ValueError(f"deblur: the image size must be multiples of 16 in [16, 256] with 1 to 8 channels, this model's is {C} x {H} x {W}")
        return self._y_arg("deblur", y, (C, H, W))

    @torch.no_grad()
    def deblur(self, y, kernel="gauss", *, tol=blur.DEFAULT_TOL, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """Zero-shot deblurring with DDNM (Wang, Yu, Zhang 2023): an image [B, C, H, W] whose separable blur
        with zero padding, A(X) = A_h X A_w^T per channel, is y [B, C, H, W] (in [-1, 1]).  kernel: "uniform" (9 x 9 box), "gauss"
        (5 x 5, sigma 10), "aniso" (9 taps, sigma 20 down the rows, sigma 1 along them), an odd-length 1-D array or a pair
        (k_h, k_w).  tol: singular values of each axis below tol * s_max are dropped from the pseudo-inverse.  Every step of the chain
        (all T steps, or respacing's K; ancestral, or DDIM with eta) replaces the range-space part of its clipped x0 by A+ y before
        the update, so the result's projection P_h x P_w^T equals A+ y up to fp32 rounding, and A(x) = y as far as the truncation
        allows.  x_T: the start state; seed: the Philox key (default: drawn from torch's generator).  H and W multiples of 16 in
        [16, 256].  solver / noise / early_stop / paste / mask / sigma_y raise ValueError, as do an unknown kernel, a bad tol or eta
        and a non-finite or misshapen y, before any device work."""
        y = self._deblur_args(y, kernel, tol, ddim, eta, unsupported)
        sid = int(self.rng_stream_id)
        m = self._blur_operands(kernel, tol)
        yp = _once(lambda yl: ops.separable_apply(yl, m["Q_h"], m["Q_w"]))      # the Python loop's Yp = A+ y, formed at its first step

        def op(x, e, yl, mk, t, tables, seed):
            ops.p_sample_update_restore_blur_(x, e, m["P_h"], m["P_w"], yp(yl), t, **tables, seed=seed, stream_id=sid)
        return self._ddnm_loop(
            "deblur", y, None, self._chain_tables(respacing, ddim, eta), x_T, seed, op,
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_blur_nhwc(
                x, yl, m["P_h"], m["P_w"], m["Q_h"], m["Q_w"], tables, k_start, seed=seed, stream_id=sid, use_graph=self.use_graph,
                timesteps=use))

    # ------------------------------------------------------------------ DDNM for any separable operator (size-changing included)
    def _sep_operands(self, A_h, A_w, tol):
        """{A_h, A_w, Q_h, Q_w, P_h, P_w} of blur.separable_operands on the model's device, cached like _blur_operands."""
        names = ("A_h", "A_w", "Q_h", "Q_w", "P_h", "P_w")
        return self._cached_tables(('sep', A_h.tobytes(), A_w.tobytes(), A_h.shape, A_w.shape, float(tol)),
                                   lambda: (dict(zip(names, blur.separable_operands(A_h, A_w, tol)[:6])), None))[0]

    def _separable_args(self, y, A_h, A_w, tol, ddim, eta, unsupported):
        """ValueError for anything restore_separable cannot take, before any device work.  Returns (y as float, A_h, A_w as float64
        arrays)."""
        who = "restore_separable"
        if unsupported:
            raise ValueError(f"{who}: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws over the "
                             f"whole schedule on an exact, unmasked measurement: no {', '.join(self.DEBLUR_UNSUPPORTED)})")
        self._tol_arg(who, tol)
        self._eta_arg(who, ddim, eta)
        C, H, W = self.sample_shape
        if H % 16 or W % 16 or not (16 <= H <= 256 and 16 <= W <= 256 and 1 <= C <= 8):
            raise ValueError(f"{who}: the image size must be multiples of 16 in [16, 256] with 1 to 8 channels, this model's is {C} x {H} x {W}")
        mats = []
        for what, A, side in (("A_h", A_h, H), ("A_w", A_w, W)):
            if torch.is_tensor(A):
                A = A.detach().cpu().numpy()
            try:
                A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
            except (TypeError, ValueError):
                raise ValueError(f"{who}: {what} must be a real matrix") from None
            if A.ndim != 2 or A.shape[1] != side or not np.all(np.isfinite(A)):
                raise ValueError(f"{who}: {what} must be a finite [n, {side}] matrix, got shape {A.shape}")
            if A.shape[0] % 4 or not (4 <= A.shape[0] <= side):
                raise ValueError(f"{who}: {what} must have a multiple of 4 in [4, {side}] rows, got {A.shape[0]}")
            mats.append(A)
        h, w = mats[0].shape[0], mats[1].shape[0]
        return self._y_arg(who, y, (C, h, w)), mats[0], mats[1]

    @torch.no_grad()
    def restore_separable(self, y, A_h, A_w, *, tol=blur.DEFAULT_TOL, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None,
                          **unsupported):
        """Zero-shot restoration with DDNM for any separable linear operator: an image [B, C, H, W] with
        A_h x A_w^T = y per channel, y [B, C, h, w] (in [-1, 1]), A_h [h, H] and A_w [w, W] real matrices -- blur.resize_matrix for
        the antialiased bicubic reduction, a decimated blur matrix for blur-then-decimate with a known PSF.  The pseudo-inverse is
        taken per axis with the singular values below tol * s_max dropped (blur.separable_operands); the steps are deblur's.  With
        full row rank (nothing dropped) A(x_out) = y up to fp32 rounding.  h and w multiples of 4 in [4, H] and [4, W]; H and W
        multiples of 16 in [16, 256].  respacing, ddim, eta, x_T, seed: as deblur.  solver / noise / early_stop / paste / mask /
        sigma_y raise ValueError, as do misshapen or non-finite matrices, sizes off that grid, a bad tol or eta and a non-finite or
        misshapen y, before any device work."""
        y, A_h, A_w = self._separable_args(y, A_h, A_w, tol, ddim, eta, unsupported)
        sid = int(self.rng_stream_id)
        m = self._sep_operands(A_h, A_w, tol)
        yp = _once(lambda yl: ops.separable_apply_rect(yl, m["Q_h"], m["Q_w"]))      # the Python loop's Yp = A+ y, formed at its first step

        def op(x, e, yl, mk, t, tables, seed):
            ops.p_sample_update_restore_blur_(x, e, m["P_h"], m["P_w"], yp(yl), t, **tables, seed=seed, stream_id=sid)
        return self._ddnm_loop(
            "restore_separable", y, None, self._chain_tables(respacing, ddim, eta), x_T, seed, op,
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_sep_nhwc(
                x, yl, m["P_h"], m["P_w"], m["Q_h"], m["Q_w"], tables, k_start, seed=seed, stream_id=sid, use_graph=self.use_graph,
                timesteps=use))

    # ------------------------------------------------------------------ DDNM compressed sensing (Walsh-Hadamard)
    def _cs_args(self, y, perm, perm_seed, ddim, eta, unsupported):
        """ValueError for anything restore_cs cannot take, before any device work.  Returns (y as float, perm as an int32 array)."""
        who = "restore_cs"
        if unsupported:
            raise ValueError(f"{who}: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws over the "
                             f"whole schedule on an exact measurement of the first m coefficients: no {', '.join(self.DEBLUR_UNSUPPORTED)})")
        self._eta_arg(who, ddim, eta)
        C, H, W = self.sample_shape
        if not hadamard.size_ok(C, H, W):
            raise ValueError(f"{who}: the image size must be powers of two in [16, 256] with 1 to 8 channels, this model's is {C} x {H} x {W}")
        N = H * W
        if perm is None:
            if isinstance(perm_seed, bool) or not isinstance(perm_seed, (int, np.integer)) or perm_seed < 0:
                raise ValueError(f"{who}: perm_seed must be a non-negative integer, got {perm_seed!r}")
            perm = hadamard.cs_perm(N, perm_seed)
        else:
            perm = hadamard.check_perm(perm, N, who)
        self._y_arg(who, y, (C, "m"), min_batch=1, finite=False)
        m = int(y.shape[2])
        if m % 4 or not (4 <= m <= N):
            raise ValueError(f"{who}: y's m must be a multiple of 4 in [4, {N}], got {m}")
        return self._y_arg(who, y, (C, "m")), perm

    @torch.no_grad()
    def restore_cs(self, y, perm=None, *, perm_seed=0, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """Zero-shot compressed sensing with DDNM (Wang, Yu, Zhang 2023): an image [B, C, H, W] whose
        subsampled, permuted Walsh-Hadamard transform is y [B, C, m].  Per channel the plane is flattened row-major, read through perm
        (an integer array of H W entries, a permutation; default hadamard.cs_perm(H W, perm_seed)) and transformed by the orthonormal
        Walsh-Hadamard matrix in natural order; y holds its first m coefficients (m is read from y: hadamard.cs_rows(ratio, H W) for a
        sampling ratio).  Every step of the chain (all T steps, or respacing's K; ancestral, or DDIM with eta) sets the measured
        coefficients of its clipped x0 to y before the update, so A(x_out) = y up to fp32 rounding and everything else is the
        model's.  x_T: the start state; seed: the Philox key (default: drawn from torch's generator).  H and W powers of two in
        [16, 256], m a multiple of 4 in [4, H W].  solver / noise / early_stop / paste / mask / sigma_y raise ValueError, as do a perm
        that is no permutation, a size off that grid, a bad eta and a non-finite or misshapen y, before any device work."""
        y, perm = self._cs_args(y, perm, perm_seed, ddim, eta, unsupported)
        sid = int(self.rng_stream_id)
        perm_dev = _once(lambda: torch.from_numpy(perm).to(self.betas.device))      # placed at the first use (after _ddnm_loop's device check)

        def op(x, e, yl, mk, t, tables, seed):
            ops.p_sample_update_restore_cs_(x, e, yl, perm_dev(), t, **tables, seed=seed, stream_id=sid)
        return self._ddnm_loop(
            "restore_cs", y, None, self._chain_tables(respacing, ddim, eta), x_T, seed, op,
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_cs_nhwc(
                x, yl, perm_dev(), tables, k_start, seed=seed, stream_id=sid, use_graph=self.use_graph, timesteps=use))

    # ------------------------------------------------------------------ DDNM deconvolution (2-D point-spread function, periodic)
    def _psf_operands(self, k, tol):
        """{K, P, mask} of psf.psf_operands on the model's device (K^ and P^ as fp32 [H, W, 2], the mask as fp32 [H, W]), cached per
        (taps, tol, device) like the spaced tables: repeated calls pass the same tensors."""
        C, H, W = self.sample_shape
        return self._cached_tables(('psf', k.tobytes(), k.shape, float(tol)),
                                   lambda: ({n: torch.from_numpy(v) for n, v in zip(("K", "P", "mask"), psf.psf_operands(k, H, W, tol))}, None))[0]

    def _deconvolve_args(self, y, k, tol, ddim, eta, unsupported, who="deconvolve"):
        """ValueError for anything deconvolve (or, as `who`, deconvolve_noisy) cannot take, before any device work.  Returns (y as float,
        the PSF as a float64 array)."""
        if unsupported:
            raise ValueError(f"{who}: {sorted(unsupported)} not accepted (DDNM runs ancestral or DDIM steps with Philox draws over the "
                             f"whole schedule on an exact, unmasked measurement: no {', '.join(self.DEBLUR_UNSUPPORTED)})")
        k = psf.psf_array(k)      # its own ValueErrors
        self._tol_arg(who, tol)
        self._eta_arg(who, ddim, eta)
        C, H, W = self.sample_shape
        if not psf.size_ok(C, H, W):
            raise ValueError(f"{who}: the image size must be powers of two in [16, 256] with 1 to 8 channels, this model's is {C} x {H} x {W}")
        if k.shape[0] > H or k.shape[1] > W:
            raise ValueError(f"{who}: a {k.shape[0]} x {k.shape[1]} point-spread function does not fit a {H} x {W} image")
        return self._y_arg(who, y, (C, H, W), min_batch=1), k

    @torch.no_grad()
    def deconvolve(self, y, psf, *, tol=blur.DEFAULT_TOL, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """Zero-shot deconvolution with DDNM (Wang, Yu, Zhang 2023): an image [B, C, H, W] whose circular
        convolution with a 2-D point-spread function (periodic boundary, correlation form as blur.blur_matrix) is y [B, C, H, W]
        (in [-1, 1]).  psf: "diag" (9 x 9, a 45 degree motion), "disk" (9 x 9 defocus of radius 3.5) or a 2-D array with odd sides no
        larger than the image.  tol: frequencies whose |K^| is below tol * max |K^| are dropped from the pseudo-inverse.  Every step
        of the chain (all T steps, or respacing's K; ancestral, or DDIM with eta) replaces the range-space part of its clipped x0 by
        A+ y before the update, so the result's projection A+ A x equals A+ y up to fp32 rounding, and A(x) = y as far as the
        truncation allows.  x_T: the start state; seed: the Philox key (default: drawn from torch's generator).  H and W powers of
        two in [16, 256].  solver / noise / early_stop / paste / mask / sigma_y raise ValueError, as do an unknown preset, a bad PSF,
        tol or eta and a non-finite or misshapen y, before any device work."""
        y, k = self._deconvolve_args(y, psf, tol, ddim, eta, unsupported)
        sid = int(self.rng_stream_id)
        # the operands on the model's device and the Python loop's Yp = A+ y, made at the first use
        operands = _once(lambda: self._psf_operands(k, tol))
        yp = _once(lambda yl: ops.circular_conv(yl, operands()["P"]))

        def op(x, e, yl, mk, t, tables, seed):
            ops.p_sample_update_restore_fft_(x, e, operands()["mask"], yp(yl), t, **tables, seed=seed, stream_id=sid)
        return self._ddnm_loop(
            "deconvolve", y, None, self._chain_tables(respacing, ddim, eta), x_T, seed, op,
            lambda plan, x, yl, mk, tables, k_start, seed, use: plan.sample_restore_fft_nhwc(
                x, yl, operands()["mask"], operands()["P"], tables, k_start, seed=seed, stream_id=sid, use_graph=self.use_graph,
                timesteps=use))

    # ------------------------------------------------------------------ DDNM+ deconvolution (a noisy blurred image)
    @torch.no_grad()
    def deconvolve_noisy(self, y, psf, *, sigma_y, tol=blur.DEFAULT_TOL, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """deconvolve() for a blurred image that is only known to +- sigma_y (DDNM+, Wang, Yu, Zhang 2023, section 3.3, per frequency;
        DESIGN.md section 3.19): y = A x + noise of standard deviation sigma_y, in y's own [-1, 1] scale.  Every step moves each kept
        frequency of its clipped x0 towards that of A+ y by lam <= 1 and shapes its draw by phi <= sigma, so that the noise entering
        through y, amplified by 1 / |K^|, and the drawn noise add up to the chain's own variance: a frequency with a small |K^|
        receives a small lam instead of amplified noise.  The last step returns the model's own x0.  y, psf, tol, the other keywords
        and their ValueErrors: as deconvolve.  sigma_y must be a finite real number >= 0; sigma_y == 0 is deconvolve itself.  With
        sigma_y > 0 a chain that draws nothing (ddim=True with eta == 0) raises ValueError.  All before any device work.  Keep tol at or
        above sigma_y (gain sigma_y <= 1 on every kept frequency): y's noise is one fixed draw, and what the steps let in of it below
        that level adds up along the chain."""
        sigma_y = self._sigma_y_arg(sigma_y, "deconvolve_noisy")
        if sigma_y == 0:
            return self.deconvolve(y, psf, tol=tol, respacing=respacing, ddim=ddim, eta=eta, x_T=x_T, seed=seed, **unsupported)
        y, k = self._deconvolve_args(y, psf, tol, ddim, eta, unsupported, who="deconvolve_noisy")
        if ddim and eta == 0:
            raise ValueError("deconvolve_noisy: sigma_y > 0 needs a chain that draws (ancestral steps, or ddim with eta > 0): with eta = 0 "
                             "every row's lam is 0 and nothing would be constrained")
        sid = int(self.rng_stream_id)
        C, H, W = self.sample_shape

        @_once                    # the operands on the model's device, made at the first use
        def operands(tables):
            from . import psf as P_
            noisy = self._cached_tables(
                ('psf_noisy', k.tobytes(), k.shape, float(tol), sigma_y, respacing, bool(ddim), float(eta)),
                lambda: ({n: torch.from_numpy(v) for n, v in zip(("gain", "nsc"), P_.psf_noisy_operands(k, H, W, tol, sigma_y, tables["c1"]))},
                         None))[0]
            return dict(self._psf_operands(k, tol), **noisy)
        yh = _once(lambda yl, o: ops.circular_spectrum(yl, o["P"]))      # the Python loop's spectrum of A+ y, likewise

        def op(x, e, yl, mk, t, tables, seed):
            o = operands(tables)
            ops.p_sample_update_restore_fft_noisy_(x, e, o["mask"], o["gain"], o["nsc"], yh(yl, o), t, **tables, seed=seed, stream_id=sid)

        def chain(plan, x, yl, mk, tables, k_start, seed, use):
            o = operands(tables)
            plan.sample_restore_fft_noisy_nhwc(x, yl, o["mask"], o["P"], o["gain"], o["nsc"], tables, k_start, seed=seed, stream_id=sid,
                                               use_graph=self.use_graph, timesteps=use)
        return self._ddnm_loop("deconvolve_noisy", y, None, self._chain_tables(respacing, ddim, eta), x_T, seed, op, chain)

    # ------------------------------------------------------------------ Diffusion Posterior Sampling (gradient-guided restoration)
    GUIDED_UNSUPPORTED = ('solver', 'early_stop')
    GUIDED_RULE = ("c_recip", "c_recipm1", "c1", "c2", "sigma")

    def _guided_args(self, y, operator, zeta, mask, response, gain, respacing, ddim, eta, unsupported, image_shape):
        """ValueError for anything restore_guided cannot take, before any device work.  ``image_shape`` is [C, H, W] of the image the
        operator acts on.  Returns (y as float with the elements that are not measured set to 0, the guidance.Operator with its mask
        as {0, 1} floats [B, h, w] or None, zeta as a float64 array with one entry per step of the chain)."""
        from . import guidance as G
        who = "restore_guided"
        if unsupported:
            raise ValueError(f"{who}: {sorted(unsupported)} not accepted (DPS runs ancestral or DDIM steps over the whole schedule, each "
                             f"followed by a gradient step: no {', '.join(self.GUIDED_UNSUPPORTED)})")
        self._eta_arg(who, ddim, eta)
        op = G.make_operator(operator, tuple(image_shape), response=response, gain=gain)      # its own ValueErrors
        C, h, w = op.out_shape
        y, m = self._measured_args(self._y_arg(who, y, (C, h, w), min_batch=1, finite=False), mask, h, w, who)
        op.mask = m
        rows = self.timesteps if respacing is None else len(respace.space_timesteps(
            self.timesteps, respacing, respace.schedule_arrays(self._betas64)['alphas_cumprod']))
        return y, op, G.zeta_table(zeta, rows)

    def _guided_tables(self, respacing, ddim, eta, zeta):
        """() -> (the chain's tables plus the step sizes `zeta` as an fp32 row table, timestep map or None), cached per zeta like
        the spaced tables: repeated calls pass the same tensors."""
        base = self._chain_tables(respacing, ddim, eta)

        def build():
            tables, use = base()
            return dict(tables, zeta=torch.tensor(zeta, dtype=torch.float32)), use
        return lambda: self._cached_tables(('guided', respacing, bool(ddim), float(eta), zeta.tobytes()), build)

    def _guided_step(self, x, y, op, t_model, t_row, tables, noise=None, seed=0, decode=None):
        """One DPS step in place on the NHWC state x, inside guidance.frozen(self): the UNet's autograd forward on x as a leaf, the clipped
        x0 (ddk.autograd.PredictX0Fn), img = decode(x0) (None: x0 itself), dist = MeasureDistFn(img, y, op), g = d(sum dist) / dx by
        torch.autograd.grad (HIP backward kernels throughout), then ops.p_sample_update_guided_.  Returns (eps_hat, dist, g)."""
        from ddk import autograd as AG
        xt = x.detach().requires_grad_(True)
        with torch.enable_grad():
            eps_hat = self._eps_model_nhwc().forward_nhwc(xt, t_model)
            x0 = AG.PredictX0Fn.apply(xt, eps_hat, t_row, tables["c_recip"], tables["c_recipm1"], True)
            dist = AG.MeasureDistFn.apply(x0 if decode is None else decode(x0), y, op)
            (g,) = torch.autograd.grad(dist.sum(), xt)
        eps_hat, dist, g = eps_hat.detach(), dist.detach(), g.contiguous()
        ops.p_sample_update_guided_(x, eps_hat.contiguous(), g, t_row, **{k: tables[k] for k in self.GUIDED_RULE}, zeta=tables["zeta"],
                                    noise=noise, seed=seed, stream_id=int(self.rng_stream_id))
        return eps_hat, dist, g

    def _guided_loop(self, y, op, get_tables, x_T, seed, noise, decode=None):
        """The DPS chain over the latent [B, *sample_shape] for the measurement y [B, C, h, w] of decode(x0) under op: the device check,
        the tables, x_T, the Philox seed (drawn from torch's generator when None) or the injected draws, then every step of the tables
        as a Python loop of _guided_step with all parameters frozen (guidance.frozen).  Returns the NCHW result."""
        from . import guidance as G
        who = "restore_guided"
        device = self.betas.device
        if device.type != 'cuda':
            raise DDKError(f"{who}: move the model to a ROCm device first (no CPU fallback)")
        tables, use = get_tables()
        shape = (y.shape[0], *self.sample_shape)
        k_start = (self.timesteps if use is None else len(use)) - 1
        if x_T is not None and tuple(x_T.shape) != shape:
            raise ValueError(f"{who}: x_T must be {shape}, got {tuple(x_T.shape)}")
        if noise is not None and tuple(noise.shape) != (k_start + 1, *shape):
            raise ValueError(f"{who}: noise must be {(k_start + 1, *shape)} (one draw per step, in run order), got {tuple(noise.shape)}")
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        yl = ops.nchw_to_nhwc(y.to(device).float().contiguous())
        op.to(device)
        x = ops.nchw_to_nhwc(img.contiguous())
        nz = None if noise is None else noise.to(device).float().permute(0, 1, 3, 4, 2).contiguous()   # [k,B,C,H,W] -> [k,B,H,W,C]
        with G.frozen(self):
            for j, k in enumerate(range(k_start, -1, -1)):
                t_model = torch.full((shape[0],), k if use is None else use[k], device=device, dtype=torch.long)
                t_row = torch.full((shape[0],), k, device=device, dtype=torch.long)
                self._guided_step(x, yl, op, t_model, t_row, tables, noise=None if nz is None else nz[j], seed=seed, decode=decode)
        return ops.nhwc_to_nchw(x)

    def restore_guided(self, y, operator, *, zeta, mask=None, response="linear", gain=1.0, respacing=None, ddim=False, eta=0.0, x_T=None,
                       seed=None, noise=None, **unsupported):
        """Zero-shot restoration with Diffusion Posterior Sampling (Chung et al., ICLR 2023): an image
        [B, C, H, W] whose measurement phi(A x) is close to y.  After every reverse step (all T, or respacing's K; ancestral, or DDIM
        with eta) x moves against the gradient, with respect to x_t and through the UNet, of the distance || phi(A x0) - y ||_2 of the
        step's own clipped x0, taken per image, times zeta: a number >= 0, or one per step of the chain (entry k for row k).
        operator: ("mean", n) with n in {1, 2, 4, 8} (n x n block means; n = 1 with a mask is inpainting), ("separable", A_h, A_w)
        (A_h x A_w^T per channel; sizes multiples of 4 in [4, 256]), ("psf", k) (circular convolution; sizes powers of two in
        [16, 256]) or a name deblur ("uniform", "gauss", "aniso") or deconvolve ("diag", "disk") takes.  mask: as restore's, on the
        measurement's grid.  response="saturate": the sensor clips, phi(u) = clamp(gain u, -1, 1); "linear" ignores gain.  The
        measurement is approached, not held: nothing of y is pasted, and y may carry noise of any level.  x_T: the start state;
        seed: the Philox key (default: drawn from torch's generator); noise: [steps, B, C, H, W] injected draws in run order.
        Every parameter is frozen for the chain (no `.grad` is touched) and its flags are put back afterwards.  solver / early_stop
        raise ValueError, as do a bad operator, response, gain, zeta, mask or eta and a misshapen y, before any device work."""
        y, op, z = self._guided_args(y, operator, zeta, mask, response, gain, respacing, ddim, eta, unsupported, self.sample_shape)
        return self._guided_loop(y, op, self._guided_tables(respacing, ddim, eta, z), x_T, seed, noise)

    @torch.no_grad()
    def reconstruct(self, x, n):
        """ddpm.py:126-147."""
        assert x.shape[0] >= n
        x = x[:n]
        t = torch.linspace(0, self.timesteps - 1, n, device=x.device, dtype=torch.long)
        eps = torch.randn_like(x)
        x_0 = self.q_sample(x, t, eps)
        eps_hat = self.latent_model(x_0, t)
        return self.predict_x_from_eps(x_0, t, eps_hat, clip=False)

    # ------------------------------------------------------------------ training objective
    def _per_sample_sq_err(self, eps, eps_hat):
        """reduce over C,H,W of (eps - eps_hat)^2 (ddpm.py:279 + utils/utils.py:26-40)."""
        if torch.is_grad_enabled() and eps_hat.requires_grad:
            from trainers.autograd_unet import sq_err_sum_autograd
            per = sq_err_sum_autograd(eps, eps_hat)
        else:
            per = ops.sq_err_sum(eps.contiguous(), eps_hat.contiguous())
        if self.loss_flat == 'mean':
            per = per / (eps.numel() // eps.shape[0])
        return per

    def loss_ddpm(self, eps, eps_hat, t):
        """ddpm.py:275-288."""
        loss = self._per_sample_sq_err(eps, eps_hat)
        if self.L == 'simple':
            return loss.mean()
        if self.L == 'vlb':
            return (self.vlb_weights[t] * loss).mean()
        return (loss + self.lambda_ * self.vlb_weights[t] * loss).mean()

    def losses(self, x, t):
        """ddpm.py:290-315."""
        eps = torch.randn_like(x)
        x_t = self.q_sample(x, t, eps)
        eps_hat = self.latent_model(x_t, t)
        return self.loss_ddpm(eps, eps_hat, t)

    # ------------------------------------------------------------------ evaluation-time VLB (ddpm.py:317-446)
    def _vlb_fused(self, x, x_t, t, eps_hat, eps=None):
        """One HIP kernel for q_posterior (x2), predict_x_from_eps(clip), normal_kl, the discretised NLL and flat_bits."""
        return ops.vlb_terms(x.contiguous(), x_t.contiguous(), eps_hat.contiguous(), t.contiguous(),
                             self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.posterior_mean_coef1,
                             self.posterior_mean_coef2, self.posterior_log_variance_clipped,
                             eps=None if eps is None else eps.contiguous())

    def vlb_terms(self, x, x_t, t):
        """ddpm.py:317-366.  Without gradients (evaluation, the only caller in the reference: test_losses_) the UNet's
        eps_hat feeds ONE fused kernel; with gradients enabled the reference's torch expression is kept."""
        if not torch.is_grad_enabled() and x.is_cuda:
            return self._vlb_fused(x, x_t, t, self.latent_model(x_t, t))[0]
        true_mean, _, true_log_var = self.q_posterior(x, x_t, t)
        pred_mean, _, pred_log_var = self.p_mean_variance(x_t, t)
        if self.L == 'hybrid':
            true_mean, pred_mean = true_mean.detach(), pred_mean.detach()
        kl = flat_bits(normal_kl(true_mean, true_log_var, pred_mean, pred_log_var))
        nll = flat_bits(-discretized_gaussian_log_likelihood(x, means=pred_mean, log_scales=0.5 * pred_log_var))
        return torch.where((t == 0), nll, kl)

    @torch.no_grad()
    def calc_prior(self, x):
        """ddpm.py:368-391."""
        t = torch.full((x.shape[0],), self.timesteps - 1, device=x.device, dtype=torch.long)
        mean, _, log_var = self.q_mean_variance(x, t)
        return flat_bits(normal_kl(mean, log_var, 0., 0.))

    @torch.no_grad()
    def test_losses_(self, x, seed=None, noise=None):
        """ddpm.py:393-442: for t = T-1 .. 0: eps ~ N(0,1) (torch's generator, one draw per step like the reference),
        x_t = q_sample, then the VLB term and L_simple of that step.  The reference calls the UNet twice per step on
        identical inputs (vlb_terms, then L_simple); eval-mode forwards are deterministic, so here ONE UNet call feeds one
        fused kernel that returns both the VLB term and sum (eps - eps_hat)^2.  Returns the reference's dict.

        With ``seed`` (in-kernel Philox draws) or ``noise`` (injected draws, NCHW [T, B, C, H, W], draw k at t = T-1-k) the
        whole sweep runs natively instead (UnetPlan.vlb_sweep_nhwc: one C call, graph-replayed steps, the sampler's step
        with a q_sample input and a VLB epilogue).  Without either keyword the loop below runs, with torch's generator."""
        self._check_device(x)
        if seed is not None or noise is not None:
            return self._test_losses_native(x, seed, noise)
        vlb_t, l_simple_t = [], []
        n_el = x.numel()
        for t in reversed(range(self.timesteps)):
            t_batch = torch.full((x.shape[0],), t, device=x.device, dtype=torch.long)
            eps = torch.randn_like(x)
            x_t = self.q_sample(x, t_batch, eps)
            eps_hat = self.latent_model(x_t, t_batch)
            vlb, sq = self._vlb_fused(x, x_t, t_batch, eps_hat, eps)
            vlb_t.append(vlb)
            l_simple_t.append(sq.sum() / n_el)                      # l2_loss(reduction='none').mean()
        vlb_t = torch.stack(vlb_t, dim=1)
        l_simple_t = torch.stack(l_simple_t, dim=0)
        assert l_simple_t.shape[0] == self.timesteps
        prior = self.calc_prior(x)
        return {'vlb_t': vlb_t, 'prior': prior, 'vlb': vlb_t.sum(dim=1) + prior,
                'L_simple_t': l_simple_t, 'L_simple': l_simple_t.sum()}

    def _test_losses_native(self, x, seed, noise):
        b = x.shape[0]
        T = self.timesteps
        nz = None
        if noise is not None:
            if tuple(noise.shape) != (T, *x.shape):
                raise DDKError(f"test_losses: noise must be {(T, *x.shape)}, got {tuple(noise.shape)}")
            nz = noise.to(x.device).float().permute(0, 1, 3, 4, 2).contiguous()   # [T,B,C,H,W] -> [T,B,H,W,C]
        tables = dict(sqrt_acp=self.sqrt_alphas_cumprod, sqrt_1m_acp=self.sqrt_one_minus_alphas_cumprod,
                      c_recip=self.sqrt_recip_alphas_cumprod, c_recipm1=self.sqrt_recipm1_alphas_cumprod,
                      c1=self.posterior_mean_coef1, c2=self.posterior_mean_coef2, post_logvar=self.posterior_log_variance_clipped)
        plan = self._eps_model_nhwc().plan()
        vlb_t, l_simple_t = plan.vlb_sweep_nhwc(ops.nchw_to_nhwc(x.float().contiguous()), tables, T, noise=nz,
                                                seed=0 if seed is None else int(seed), stream_id=self.rng_stream_id,
                                                use_graph=self.use_graph)
        assert vlb_t.shape == (b, T)
        prior = self.calc_prior(x)
        return {'vlb_t': vlb_t, 'prior': prior, 'vlb': vlb_t.sum(dim=1) + prior,
                'L_simple_t': l_simple_t, 'L_simple': l_simple_t.sum()}

    def test_losses(self, x, **kw):
        """``seed`` / ``noise``: see test_losses_."""
        return self.test_losses_(x, **kw)

    def t_sample(self, n):
        """ddpm.py:448-450."""
        return torch.randint(0, self.timesteps, (n,), device=self.betas.device).long()

    def forward(self, x):
        """ddpm.py:452-457."""
        return self.losses(x, self.t_sample(x.shape[0]))
