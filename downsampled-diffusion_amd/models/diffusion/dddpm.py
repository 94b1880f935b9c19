"""Downsampled DDPM (dDDPM): a DDPM over tanh-squashed latents produced by an encoder and decoded by a decoder, each of
config['d_mode'] / config['u_mode']: a learned ConvResNet, a plain stack of stride-2 convs, or a bicubic resize (reference
models/diffusion/dddpm.py:11-177, models/downsampled/wrapper.py).  Same constructor and
return conventions: ``sample`` -> (x, z), ``forward`` -> (objective, {'latent', 'recon'}).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from ddk import ops
from models.downsampled import get_downsampling, get_upsampling
from models.downsampled.convblocks import ConvResNet
from .ddpm import DDPM


class DownsampleDDPM(DDPM):
    def __init__(self, config: dict, denoise_model: nn.Module, device: str, color_channels: int = 3):
        super().__init__(config, denoise_model, device, color_channels)
        self.t_rec_max = int(self.timesteps - 1) if config['t_rec_max'] == -1 else config['t_rec_max']
        self.x_shape = [self.in_channels, self.image_size, self.image_size]
        self.force_latent = config['force_latent']
        unet_in = config['unet_in']
        self.dim_reduc = np.power(2, config['n_downsamples']).astype(int)
        z_size = int(self.image_size / self.dim_reduc)
        self.sample_shape = [unet_in, z_size, z_size]
        assert unet_in >= self.in_channels, (f'Input channels to DDPM-Unet {unet_in} should be equal or larger to '
                                             f'data color channels {self.in_channels}.')
        self.downsample = get_downsampling(config, self.x_shape)
        self.upsample = get_upsampling(config, self.x_shape)

    # ------------------------------------------------------------------ encoder / decoder (dddpm.py:92-112)
    def _resample_nchw(self, net, x):
        """Interpolate / SimpleDownConv / SimpleUpConv on the NCHW tensor as it stands (no channel padding, no layout change), then
        the tanh.  Differentiable when gradients are enabled and a parameter OR the input wants one: an Interpolate decoder has no
        parameters, yet the non-autoencoder loss needs d(loss) / d(z_hat) through it."""
        x = x.contiguous().float()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in net.parameters())):
            from ddk import autograd as AG
            y = net.forward_autograd(x)
            return AG.TanhFn.apply(y) if self.force_latent else y
        y = net(x)
        return ops.tanh(y) if self.force_latent else y

    def rescaled_downsample(self, x):
        """z = tanh(downsample(x)) (tanh only when force_latent)."""
        self._check_device(x)
        if not isinstance(self.downsample, ConvResNet):
            z = self._resample_nchw(self.downsample, x)
        elif torch.is_grad_enabled() and any(p.requires_grad for p in self.downsample.parameters()):
            from trainers.autograd_unet import resnet_forward_autograd
            return resnet_forward_autograd(self.downsample, x, self.force_latent)
        else:
            z = ops.nhwc_to_nchw(self.downsample.forward_nhwc(ops.nchw_to_nhwc(x.contiguous().float(), ops.pad32(x.shape[1])),
                                                              final_tanh=self.force_latent))
        assert list(z.shape)[1:] == self.sample_shape, f'mismatch between {list(z.shape)[1:]} and {self.sample_shape}'
        return z

    def rescaled_upsample(self, z):
        """x = tanh(upsample(z))."""
        self._check_device(z)
        if not isinstance(self.upsample, ConvResNet):
            x = self._resample_nchw(self.upsample, z)
        elif torch.is_grad_enabled() and (z.requires_grad or any(p.requires_grad for p in self.upsample.parameters())):
            # (also for the INPUT's gradient alone, as _resample_nchw: restore_guided differentiates the measurement through the decoder)
            from trainers.autograd_unet import resnet_forward_autograd
            return resnet_forward_autograd(self.upsample, z, self.force_latent)
        else:
            x = ops.nhwc_to_nchw(self.upsample.forward_nhwc(ops.nchw_to_nhwc(z.contiguous().float(), ops.pad32(z.shape[1])),
                                                            final_tanh=self.force_latent))
        assert list(x.shape)[1:] == self.x_shape, f'mismatch between {list(x.shape)[1:]} and {self.x_shape}'
        return x

    # ------------------------------------------------------------------ sampling (dddpm.py:76-90)
    @torch.no_grad()
    def sample(self, batch_size=16, every=1, early_stop=None, *, respacing=None, ddim=False, eta=0.0, solver=None):
        z_sample = self.p_sample_loop((batch_size, *self.sample_shape), every, early_stop, respacing=respacing, ddim=ddim, eta=eta,
                                      solver=solver)
        x_sample = self.rescaled_upsample(z_sample)
        assert list(z_sample.shape)[1:] == self.sample_shape
        assert list(x_sample.shape)[1:] == self.x_shape
        return x_sample, z_sample

    @torch.no_grad()
    def inpaint(self, x, mask, *, respacing=None, jump_length=10, jump_n_sample=10, x_T=None, seed=None, paste=True, **unsupported):
        """RePaint in the latent (DDPM.inpaint).  The hidden pixels are zeroed before the encoder, so
        z0 = rescaled_downsample(x * m) carries nothing of them.  A latent pixel is known only if its whole dim_reduc x dim_reduc
        block is known in every channel (a min-pool of the mask), and all latent channels share that mask.  The decoded result
        gets the known pixels of x put back when paste is set.  Returns (x_out, z) like sample; x_T is a latent start state."""
        x, m = self._inpaint_args(x, mask, self.x_shape, jump_length, jump_n_sample, unsupported)
        x, m = x.to(self.betas.device), m.to(self.betas.device)
        self._check_device(x)
        z0 = self.rescaled_downsample(torch.where(m != 0, x, torch.zeros_like(x)))
        d = int(self.dim_reduc)
        m_lat = -torch.nn.functional.max_pool2d(-m.amin(dim=1, keepdim=True), d)
        m_lat = m_lat.expand(-1, self.sample_shape[0], -1, -1).contiguous()
        z = self._inpaint_loop(z0, m_lat, respacing, jump_length, jump_n_sample, x_T, seed)
        x_out = self.rescaled_upsample(z)
        if paste:
            x_out = torch.where(m != 0, x, x_out)
        return x_out, z

    @torch.no_grad()
    def super_resolve(self, y, scale, *, downsample="mean", respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """DDNM super-resolution in the latent (DDPM.super_resolve) of y [B, C, H/scale, W/scale].  The
        constraint is the latent's: z_ref = rescaled_downsample(y replicated scale x scale), y_lat = the n_lat x n_lat average
        pooling of z_ref with n_lat = scale / dim_reduc in {2, 4, 8}, and the chain keeps the latent's n_lat x n_lat block means
        equal to y_lat.  That is exact in the latent (up to fp32 rounding) and only approximate in pixels: the decoder is not
        linear, so the pooled x_out is close to y, not equal to it.  Returns (x_out, z) like sample; x_T is a latent start state.
        downsample: "mean" only -- a bicubic reduction of the image is no separable operator of the latent (restore_separable):
        anything else is a ValueError."""
        if downsample != "mean":
            raise ValueError(f"super_resolve: a DownsampleDDPM samples in a latent and holds block means there: downsample must be "
                             f"'mean', got {downsample!r} (bicubic super-resolution needs a pixel model, DDPM)")
        d = int(self.dim_reduc)
        y = self._restore_args(y, scale, self.x_shape, ddim, eta, unsupported, block=d)
        y = y.to(self.betas.device)
        self._check_device(y)
        s, n_lat = int(scale), int(scale) // d
        z_ref = self.rescaled_downsample(y.repeat_interleave(s, dim=2).repeat_interleave(s, dim=3))
        y_lat = torch.nn.functional.avg_pool2d(z_ref, n_lat)
        z = self._restore_loop(y_lat, n_lat, respacing, ddim, eta, x_T, seed)
        return self.rescaled_upsample(z), z

    @torch.no_grad()
    def restore(self, y, mask=None, scale=1, *, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, paste=True, **unsupported):
        """DDNM with a mask in the latent (DDPM.restore).  The pixels of y [B, C, H/scale, W/scale] that are
        not measured are zeroed before the encoder, so z_ref = rescaled_downsample(y * m replicated scale x scale) carries nothing
        of them, and the constraint is the latent's, as in inpaint and super_resolve (exact there up to fp32 rounding, approximate
        in pixels: the decoder is not linear).
          scale = 1 (inpainting): a latent pixel is measured only if its whole dim_reduc x dim_reduc footprint is (a min-pool of the
            mask), the block is n_lat = 1 and measured latent pixels are set to z_ref; paste puts the measured pixels of y back.
          scale a multiple of dim_reduc with n_lat = scale / dim_reduc in {1, 2, 4, 8}: a low-resolution pixel is the footprint of
            exactly one n_lat x n_lat latent block, so the mask is the latent's as it stands, and measured blocks keep the mean
            y_lat = avg_pool(z_ref, n_lat).  paste has no meaning here (y is not an image of the output's size) and is ignored.
        scale = 1 needs a mask, and so does scale = dim_reduc (n_lat = 1).  Returns (x_out, z) like sample; x_T is a latent start."""
        d = int(self.dim_reduc)
        scales = (1,) + tuple(d * n for n in (1,) + self.RESTORE_BLOCKS)
        y, m = self._restore_masked_args(y, mask, scale, self.x_shape, ddim, eta, unsupported, scales)
        return self._latent_restore(y, m, int(scale), paste, "restore",
                                    lambda y_lat, n_lat, m_lat: self._restore_loop(y_lat, n_lat, respacing, ddim, eta, x_T, seed, mask=m_lat,
                                                                                   who="restore"))

    def _latent_restore(self, y, m, s, paste, who, loop):
        """What restore, restore_solver and restore_noisy share once their arguments are checked: the latent constraint of y, mask m and scale s
        (see restore), the chain loop(y_lat, n_lat, m_lat) in the latent, the decoder and the paste.  Returns (x_out, z)."""
        d = int(self.dim_reduc)
        if m is None and s == d:
            raise ValueError(f"{who}: scale = {d} is one latent pixel per measurement and needs a mask (nothing would be constrained)")
        m_lat = None
        if s == 1:
            m_lat = -torch.nn.functional.max_pool2d(-m.unsqueeze(1), d)[:, 0]
            if not bool((m_lat.reshape(m_lat.shape[0], -1).amax(dim=1) > 0).all()):
                raise ValueError(f"{who}: no {d} x {d} latent footprint of some image is wholly measured")
        y = y.to(self.betas.device)
        self._check_device(y)
        if s == 1:
            m = m.to(y.device)
            z = loop(self.rescaled_downsample(y), 1, m_lat)               # the argument check zeroed what is not measured
            x_out = self.rescaled_upsample(z)
            if paste:
                x_out = torch.where(m.unsqueeze(1) != 0, y, x_out)
            return x_out, z
        n_lat = s // d
        z_ref = self.rescaled_downsample(y.repeat_interleave(s, dim=2).repeat_interleave(s, dim=3))
        y_lat = torch.nn.functional.avg_pool2d(z_ref, n_lat) if n_lat > 1 else z_ref
        z = loop(y_lat, n_lat, None if m is None else m.to(y.device))
        return self.rescaled_upsample(z), z

    @torch.no_grad()
    def restore_solver(self, y, mask=None, scale=1, *, respacing=None, solver="dpm++2m", order=2, x_T=None, paste=True, **unsupported):
        """DDPM.restore_solver with the constraint held in the latent exactly as restore holds it (same scales, same mask rules, same
        paste).  Returns (x_out, z); x_T is a latent start."""
        d = int(self.dim_reduc)
        scales = (1,) + tuple(d * n for n in (1,) + self.RESTORE_BLOCKS)
        y, m = self._restore_solver_args(y, mask, scale, self.x_shape, solver, order, unsupported, scales)
        return self._latent_restore(y, m, int(scale), paste, "restore_solver",
                                    lambda y_lat, n_lat, m_lat: self._restore_solver_loop(y_lat, n_lat, respacing, solver, order, x_T, mask=m_lat))

    @torch.no_grad()
    def restore_noisy(self, y, mask=None, scale=1, *, sigma_y, respacing=None, ddim=False, eta=0.0, x_T=None, seed=None, **unsupported):
        """DDPM.restore_noisy with the constraint held in the latent as restore holds it (same scales, same mask rules).  There is no
        paste: a noisy measurement is never put back into the result (sigma_y == 0 is restore with paste off).  sigma_y is used as
        the latent's noise level unchanged.  That is an approximation: the encoder is not linear, so noise of standard deviation
        sigma_y on the pixels of y is not noise of exactly that level, nor exactly Gaussian, on z_ref.  Returns (x_out, z); x_T is a
        latent start."""
        sigma_y = self._sigma_y_arg(sigma_y, "restore_noisy")
        if 'paste' in unsupported:
            raise ValueError("restore_noisy: paste is not accepted (a noisy measurement is never put back into the result)")
        if sigma_y == 0:
            return self.restore(y, mask, scale, respacing=respacing, ddim=ddim, eta=eta, x_T=x_T, seed=seed, paste=False, **unsupported)
        d = int(self.dim_reduc)
        scales = (1,) + tuple(d * n for n in (1,) + self.RESTORE_BLOCKS)
        y, m = self._restore_noisy_args(y, mask, scale, self.x_shape, sigma_y, ddim, eta, unsupported, scales)
        return self._latent_restore(y, m, int(scale), False, "restore_noisy",
                                    lambda y_lat, n_lat, m_lat: self._restore_noisy_loop(y_lat, n_lat, sigma_y, respacing, ddim, eta, x_T, seed,
                                                                                         mask=m_lat))

    def colorize(self, y, mask=None, scale=1, **kwargs):
        """Not available: the chain runs in the autoencoder's latent, whose channels are not colours, so the grey operator of
        DDPM.colorize has no meaning there.  A stated limitation, not an approximation: always ValueError."""
        raise ValueError("colorize: a DownsampleDDPM samples in a latent whose channels are not colours; colourisation needs a "
                         "3-channel pixel model (DDPM)")

    def deblur(self, y, kernel="gauss", **kwargs):
        """Not available: the chain runs in the autoencoder's latent, and a blur of the latent is not a blur of the image, so the
        operator of DDPM.deblur has no separable form there.  A stated limitation, not an approximation: always ValueError."""
        raise ValueError("deblur: a DownsampleDDPM samples in a latent, and a blur of the latent is not a blur of the image; deblurring "
                         "needs a pixel model (DDPM)")

    def restore_separable(self, y, A_h, A_w, **kwargs):
        """Not available, for deblur's reason: an operator on the image is not one on the latent.  Always ValueError."""
        raise ValueError("restore_separable: a DownsampleDDPM samples in a latent, and a separable operator on the image has no separable "
                         "form there; it needs a pixel model (DDPM)")

    def restore_cs(self, y, perm=None, **kwargs):
        """Not available, for deblur's reason: a transform of the latent is not a transform of the image.  Always ValueError."""
        raise ValueError("restore_cs: a DownsampleDDPM samples in a latent, and a Walsh-Hadamard transform of the latent is not one of the "
                         "image; compressed sensing needs a pixel model (DDPM)")

    def deconvolve(self, y, psf=None, **kwargs):
        """Not available, for deblur's reason: a convolution of the latent is not one of the image.  Always ValueError."""
        raise ValueError("deconvolve: a DownsampleDDPM samples in a latent, and a point-spread function on the image has no such form there; "
                         "deconvolution needs a pixel model (DDPM)")

    def deconvolve_noisy(self, y, psf=None, **kwargs):
        """Not available, for deconvolve's reason.  Always ValueError."""
        raise ValueError("deconvolve_noisy: a DownsampleDDPM samples in a latent, and a point-spread function on the image has no such form "
                         "there; deconvolution needs a pixel model (DDPM)")

    def restore_guided(self, y, operator, *, zeta, mask=None, response="linear", gain=1.0, respacing=None, ddim=False, eta=0.0, x_T=None,
                       seed=None, noise=None, **unsupported):
        """DDPM.restore_guided with the chain in the latent and the measurement in pixels: every step decodes
        its clipped latent x0, img = rescaled_upsample(x0), measures dist = || phi(A img) - y ||_2 there and takes the gradient back
        through the decoder, the clamp and the UNet to the latent x_t.  So y, operator and mask are the image's -- any operator
        DDPM.restore_guided takes on an image of x_shape, which the DDNM entries of this class refuse or hold only in the latent --
        and all three u_modes work (the learned decoder's parameters are frozen like the UNet's).  Returns (x_out, z) like sample;
        x_T and noise are the latent's."""
        from ddk import autograd as AG
        y, op, zt = self._guided_args(y, operator, zeta, mask, response, gain, respacing, ddim, eta, unsupported, self.x_shape)

        def decode(x0):
            img = self.rescaled_upsample(AG.NhwcToNchwFn.apply(x0, x0.shape[-1]))
            return AG.NchwToNhwcFn.apply(img.contiguous(), img.shape[1])
        z = self._guided_loop(y, op, self._guided_tables(respacing, ddim, eta, zt), x_T, seed, noise, decode=decode)
        with torch.no_grad():
            return self.rescaled_upsample(z), z

    @torch.no_grad()
    def reconstruct(self, x, n):
        """dddpm.py:33-74 (visualisation only)."""
        assert x.shape[0] >= n, f'batch size ({x.shape[0]}) is below {n}'
        x = x[:n]
        t = torch.linspace(0, self.timesteps - 1, n, device=x.device, dtype=torch.long)
        z = self.rescaled_downsample(x)
        eps = torch.randn_like(z)
        z_t = self.q_sample(z, t, eps)
        eps_hat = self.latent_model(z_t, t)
        z_recon = self.predict_x_from_eps(z_t, t, eps_hat, clip=False)
        x_recon = self.rescaled_upsample(z_recon)
        assert list(x_recon.shape)[1:] == self.x_shape
        return x_recon, z_recon

    # ------------------------------------------------------------------ losses (dddpm.py:114-143)
    def loss_recon(self, x, z_hat, t):
        x_hat = self.rescaled_upsample(z_hat)
        assert x_hat.shape == x.shape, f'mismatch between {x_hat.shape} and {x.shape}'
        loss = self._per_sample_sq_err(x, x_hat)
        return torch.where(t < self.t_rec_max, loss, torch.zeros_like(loss))

    def losses(self, x, t):
        z = self.rescaled_downsample(x)
        eps = torch.randn_like(z)
        z_t = self.q_sample(z, t, eps)
        eps_hat = self.latent_model(z_t, t)
        L_ddpm = self.loss_ddpm(eps, eps_hat, t)
        z_hat = self.predict_x_from_eps(z_t, t, eps_hat, clip=False)
        L_rec = self.loss_recon(x, z_hat, t)
        obj = (L_ddpm + L_rec).mean()
        return obj, {'latent': L_ddpm.mean(), 'recon': L_rec.mean()}

    @torch.no_grad()
    def test_losses(self, x, **kw):
        return self.test_losses_(self.rescaled_downsample(x), **kw)


RECON_SIDE_STREAM = True          # see DownsampleDDPMAutoencoder.losses; the tests switch it off to compare
FUSED_OBJECTIVE = True            # idem: the objective of the 'simple' loss in one launch
_recon_streams = {}               # device -> torch.cuda.Stream (module level: a stream must not end up in a deepcopy of the model)


class DownsampleDDPMAutoencoder(DownsampleDDPM):
    """Reconstruction loss taken directly through the autoencoder, latent detached for the DDPM term
    (dddpm.py:151-177; selected by ae_loss=True, train.py:44)."""

    def __init__(self, config: dict, denoise_model: nn.Module, device: str, color_channels: int = 3):
        super().__init__(config, denoise_model, device, color_channels)

    def losses(self, x, t):
        z = self.rescaled_downsample(x)
        # The reconstruction branch (decoder + loss, and with it the backward of both) does not meet the denoiser branch before the two
        # losses are added (the latent is detached): in training on the device it runs on its own stream -- its large memory-bound
        # launches beside the UNet's small latency-bound ones.  autograd runs each backward on the stream of its forward.
        fork = RECON_SIDE_STREAM and x.is_cuda and torch.is_grad_enabled()
        # 'simple' loss in training on the device: objective and the two report values from the per-sample losses in one launch
        # (ddk_ae_objective) instead of where / add / three means and their autograd counterparts
        fused = FUSED_OBJECTIVE and self.L == 'simple' and x.is_cuda and torch.is_grad_enabled()
        recon = (lambda: self._per_sample_sq_err(x, self.rescaled_upsample(z))) if fused else (lambda: self.loss_recon(x, z, t))
        if fork:
            main = torch.cuda.current_stream()
            side = _recon_streams.get(x.device)
            if side is None:
                side = _recon_streams[x.device] = torch.cuda.Stream(device=x.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                L_rec = recon()
        else:
            L_rec = recon()
        z = z.detach()
        eps = torch.randn_like(z)
        z_t = self.q_sample(z, t, eps)
        eps_hat = self.latent_model(z_t, t)
        L_ddpm = self._per_sample_sq_err(eps, eps_hat) if fused else self.loss_ddpm(eps, eps_hat, t)
        if fork:
            main.wait_stream(side)
        if fused:
            from ddk import autograd as AG
            obj, latent, rec = AG.AEObjectiveFn.apply(L_ddpm, L_rec, t.contiguous(), math.ceil(self.t_rec_max))    # t < t_rec_max for integer t, also for a fractional setting
            return obj, {'latent': latent, 'recon': rec}
        obj = (L_ddpm + L_rec).mean()
        return obj, {'latent': L_ddpm.mean(), 'recon': L_rec.mean()}
