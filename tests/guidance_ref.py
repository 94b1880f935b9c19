"""Reference of the Diffusion Posterior Sampling step (Chung et al., ICLR 2023) in plain torch on the CPU, in the
dtype of its inputs (float64 for the tests' references, fp32 where a test measures what fp32 arithmetic itself loses):

    eps   = UNet(x_t, t)
    x0    = clamp(c_recip[k] x_t - c_recipm1[k] eps, -1, 1)
    img   = x0 | decode(x0)
    d_b   = || phi(A img_b) - y_b ||_2
    g     = d(sum_b d_b) / d x_t          (torch autograd)
    x_t-1 = (c1[k] x0 + c2[k] x_t) + [k > 0] sigma[k] z - zeta[k] g

The operator is a models.diffusion.guidance.Operator, read through its host fields only (kind, n, mask, A_h, A_w, K, response, gain):
A is written out as avg_pool2d, matrix products and torch.fft.  Tensors are NCHW here.  The UNet is oracle/unet_ref.unet_forward, the
decoders are oracle/resampler_ref and tests/resample_ref.
"""
import torch
import torch.nn.functional as F

from oracle import unet_ref as U


def _cdtype(dtype):
    return torch.complex128 if dtype == torch.float64 else torch.complex64


def linear(op, img):
    """A img without the mask, NCHW, in img's dtype"""
    if op.kind == "mean":
        return F.avg_pool2d(img, op.n) if op.n > 1 else img
    if op.kind == "separable":
        a_h, a_w = torch.from_numpy(op.A_h).to(img.dtype), torch.from_numpy(op.A_w).to(img.dtype)
        return torch.einsum("hH,bcHW,wW->bchw", a_h, img, a_w)
    k = torch.from_numpy(op.K).to(_cdtype(img.dtype))
    return torch.fft.ifft2(k * torch.fft.fft2(img)).real


def response(op, u):
    return u if op.response == "linear" else torch.clamp(op.gain * u, -1.0, 1.0)


def _mask(op, like):
    return None if op.mask is None else op.mask.detach().cpu().to(like.dtype).unsqueeze(1)


def measure(op, img):
    """y = mask phi(A img)"""
    u = response(op, linear(op, img))
    m = _mask(op, u)
    return u if m is None else torch.where(m != 0, u, torch.zeros_like(u))


def measure_dist(op, img, y):
    """dist [B] = sqrt(sum mask (phi(A img) - y)^2) per image"""
    d = response(op, linear(op, img)) - y.to(img.dtype)
    m = _mask(op, d)
    if m is not None:
        d = torch.where(m != 0, d, torch.zeros_like(d))
    return (d * d).flatten(1).sum(dim=1).sqrt()


def dist_and_grad(op, img, y, gout=None):
    """(dist, d(sum_b gout[b] dist[b]) / d img) by torch autograd"""
    x = img.detach().clone().requires_grad_(True)
    dist = measure_dist(op, x, y)
    w = torch.ones_like(dist) if gout is None else gout.to(dist.dtype)
    (v,) = torch.autograd.grad((dist * w).sum(), x)
    return dist.detach(), v


def unet(sd, cfg, x, t, pre=""):
    """oracle unet_forward in x's dtype.  The sinusoidal embedding is fp32 arithmetic on the integer t by the model's definition
    (blocks.py:22-29): a float64 run takes that fp32 embedding widened, so that it differs from the device by the network's rounding
    and not by another sin(t f)."""
    if x.dtype != torch.float64:
        return U.unet_forward(sd, cfg, x, t, pre=pre)
    orig = U.sinusoidal_embedding
    U.sinusoidal_embedding = lambda tt, dim: orig(tt, dim).double()
    try:
        return U.unet_forward(sd, cfg, x, t, pre=pre)
    finally:
        U.sinusoidal_embedding = orig


def decoder(sd, cfg):
    """z -> rescaled_upsample(z) of a dDDPM of any u_mode, on a state dict already in the wanted dtype"""
    import resample_ref as RR
    return lambda z: RR.rescaled_upsample(sd, cfg, z)


def guided_step(eps_model, tables, op, y, x_t, k, noise, decode=None):
    """One step at row k of `tables` (the model's own fp32 tables incl. zeta, widened to x_t's dtype), every image at the same row.
    eps_model(x, k) -> eps_hat.  Returns (eps_hat, dist, g, x_prev), detached."""
    dt = x_t.dtype
    c = {n: float(v[k]) for n, v in tables.items()}
    x = x_t.detach().clone().requires_grad_(True)
    eps = eps_model(x, k)
    x0 = torch.clamp(c["c_recip"] * x - c["c_recipm1"] * eps, -1.0, 1.0)
    dist = measure_dist(op, x0 if decode is None else decode(x0), y.to(dt))
    (g,) = torch.autograd.grad(dist.sum(), x)
    sg = c["sigma"] if k > 0 else 0.0
    with torch.no_grad():
        x_prev = (c["c1"] * x0 + c["c2"] * x) + sg * noise.to(dt) - c["zeta"] * g
    return eps.detach(), dist.detach(), g, x_prev.detach()


def guided_chain(eps_model, tables, op, y, x_T, noises, decode=None):
    """All rows of the tables from the last to row 0; noises[j] is the draw of the j-th step run.  Returns x_0."""
    x = x_T
    rows = len(tables["c1"])
    for j, k in enumerate(range(rows - 1, -1, -1)):
        x = guided_step(eps_model, tables, op, y, x, k, noises[j], decode)[3]
    return x
