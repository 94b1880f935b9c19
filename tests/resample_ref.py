"""Float64 restatement of the dDDPM's 'deterministic' and 'convolutional' resamplers (reference models/downsampled/convblocks.py:8-89,
wrapper.py:22-26,49-55) -- test infrastructure only.

Bicubic (F.interpolate(mode='bicubic', align_corners=True), torch's upsample_bicubic2d) as one dense [n_out, n_in] matrix per
dimension, in numpy float64: A = -0.75, source coordinate o (in-1)/(out-1) (0 when out == 1), i = floor, t = fraction, taps
i-1 .. i+2 with weights c2(t+1), c1(t), c1(1-t), c2(2-t), indices clamped to [0, in-1] -- a clamped tap keeps its weight, so
coinciding taps add.  The two convs run through torch's CPU ops in float64.  tests/test_resampler_modes_cpu.py pins all of it to
the reference's own outputs (tests/golden/g11_resampler_modes.npz).
"""
import numpy as np
import torch
import torch.nn.functional as F

A = -0.75


def _c1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _c2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def bicubic_matrix(n_in, n_out):
    """M [n_out, n_in] float64 with resize(v) = M @ v."""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for o in range(n_out):
        src = o * scale
        i = int(np.floor(src))
        t = src - i
        for k, wk in enumerate((_c2(t + 1.0), _c1(t), _c1(1.0 - t), _c2(2.0 - t))):
            m[o, min(max(i - 1 + k, 0), n_in - 1)] += wk
    return m


def _mats(h_in, w_in, size, dtype=torch.float64):
    return (torch.from_numpy(bicubic_matrix(h_in, int(size[0]))).to(dtype), torch.from_numpy(bicubic_matrix(w_in, int(size[1]))).to(dtype))


def bicubic(x, size, absolute=False):
    """x [B, C, H, W] (any float dtype; computed in x's dtype, float64 for the references) -> [B, C, *size].  absolute: with |M|
    (the sum of |w| |x| the error bound of the tests is built on, when x is already |x|)."""
    mh, mw = _mats(x.shape[2], x.shape[3], size, x.dtype)
    if absolute:
        mh, mw = mh.abs(), mw.abs()
    return torch.einsum("oh,bchw,pw->bcop", mh, x, mw)


def bicubic_grad(dy, in_size, absolute=False):
    """the transpose: dy [B, C, Ho, Wo] -> [B, C, *in_size]"""
    mh, mw = _mats(int(in_size[0]), int(in_size[1]), dy.shape[2:], dy.dtype)
    if absolute:
        mh, mw = mh.abs(), mw.abs()
    return torch.einsum("oh,bcop,pw->bchw", mh, dy, mw)


def conv_down(x, w, b=None):
    """nn.Conv2d(k3, s2, p1)"""
    return F.conv2d(x, w, b, stride=2, padding=1)


def conv_up(x, w, b=None):
    """nn.ConvTranspose2d(k4, s2, p1)"""
    return F.conv_transpose2d(x, w, b, stride=2, padding=1)


def _n_convs(sd, pre):
    n = 0
    while f"{pre}conv.{n}.weight" in sd:
        n += 1
    return n


def _taped(tape, name, x, y):
    """tape (a list, or None): (layer name, its input, its output) of every conv layer; the output keeps its gradient after a
    backward, so a test can form the layer's own sum |dy| |x| for its bound"""
    if tape is not None:
        if y.requires_grad:
            y.retain_grad()
        tape.append((name, x, y))
    return y


def downsample(sd, cfg, x, tape=None):
    """model.downsample(x) for d_mode 'deterministic' / 'convolutional' ('convolutional_res': oracle.resampler_ref)"""
    mode = cfg["d_mode"]
    if mode == "deterministic":
        s = x.shape[2] // 2 ** cfg["n_downsamples"]
        return bicubic(x, (s, s))
    if mode == "convolutional":
        for i in range(_n_convs(sd, "downsample.")):
            x = _taped(tape, f"downsample.conv.{i}", x, conv_down(x, sd[f"downsample.conv.{i}.weight"], sd[f"downsample.conv.{i}.bias"]))
        return x
    from oracle import resampler_ref as R
    return R.conv_res_net(sd, "downsample.", x, cfg["n_downsamples"], cfg["d_n_blocks"], False)


def upsample(sd, cfg, z, tape=None):
    mode = cfg["u_mode"]
    if mode == "deterministic":
        s = cfg["image_size"]
        return bicubic(z, (s, s))
    if mode == "convolutional":
        for i in range(_n_convs(sd, "upsample.")):
            z = _taped(tape, f"upsample.conv.{i}", z, conv_up(z, sd[f"upsample.conv.{i}.weight"], sd[f"upsample.conv.{i}.bias"]))
        return z
    from oracle import resampler_ref as R
    return R.conv_res_net(sd, "upsample.", z, cfg["n_downsamples"], cfg["u_n_blocks"], True)


def rescaled_downsample(sd, cfg, x, tape=None):
    z = downsample(sd, cfg, x, tape)
    return torch.tanh(z) if cfg["force_latent"] else z


def rescaled_upsample(sd, cfg, z, tape=None):
    x = upsample(sd, cfg, z, tape)
    return torch.tanh(x) if cfg["force_latent"] else x


def losses(sd, buf, cfg, x, t, eps, autoencoder, tape=None):
    """DownsampleDDPM.losses / DownsampleDDPMAutoencoder.losses (reference models/diffusion/dddpm.py:122-143,155-177) with injected
    t and eps, the UNet and the schedule arithmetic from oracle/: (objective, {'latent', 'recon'})."""
    from oracle.diffusion_ref import loss_ddpm, predict_x_from_eps, q_sample
    from oracle.unet_ref import unet_forward
    t_rec_max = cfg["T"] - 1 if cfg["t_rec_max"] == -1 else cfg["t_rec_max"]

    def recon(z_in):
        per = ((x - rescaled_upsample(sd, cfg, z_in, tape)) ** 2).flatten(1)
        per = per.sum(dim=1) if cfg["loss_flat"] == "sum" else per.mean(dim=1)
        return torch.where(t < t_rec_max, per, torch.zeros_like(per))

    z = rescaled_downsample(sd, cfg, x, tape)
    l_rec = None
    if autoencoder:
        l_rec = recon(z)
        z = z.detach()
    z_t = q_sample(buf, z, t, eps)
    # the oracle's sinusoidal embedding is fp32 arithmetic on an integer t; a float64 t promotes it to the dtype of a float64 state dict
    eps_hat = unet_forward(sd, cfg, z_t, t.to(z_t.dtype) if z_t.dtype == torch.float64 else t, pre="latent_model.")
    l_ddpm = loss_ddpm(buf, eps, eps_hat, t, cfg["loss_type"], cfg["loss_flat"])
    if not autoencoder:
        l_rec = recon(predict_x_from_eps(buf, z_t, t, eps_hat, clip=False))
    return (l_ddpm + l_rec).mean(), {"latent": l_ddpm.mean(), "recon": l_rec.mean()}
