"""Independent restatement of DDNM+ (Wang, Yu, Zhang, ICLR 2023, section 3.3 and the SVD form of its appendix) for the circular
convolution with a 2-D point-spread function, whose singular vectors are the 2-D Fourier basis: y = A x + noise of standard deviation
sigma_y.  Built on tests/fft_conv_ref.py (the operator, the kept frequencies) and tests/restore_noisy_ref.py (the linear tables);
nothing here imports models.diffusion.psf or models.diffusion.respace.

Per frequency f of a plane, with s the draw's scale of the row as the kernels apply it (the fp32 sigma, 0 at row 0), nsc = |c1| sigma_y
of the row and gain = 1 / |K^| on the kept frequencies M:

    g = nsc gain[f]
    kept and s >= g:  lam = 1,     phi = sqrt(max(s s - g g, 0))
    kept and s <  g:  lam = s / g, phi = 0
    dropped:          lam = 0,     phi = s
    x0'    = Re F2^-1(X^ + lam (Y^ - X^))        X^ = F2(x0), Y^ = the spectrum of A+ y; a dropped frequency keeps X^ (a select)
    n      = Re F2^-1(phi F2(z))
    x_prev = (c1 x0' + c2 x) + n

multipliers() forms lam and phi in numpy float32, one rounding per operation in the order written, so that the library and this file
read identical multipliers; everything else is float64 (numpy.fft)."""
import numpy as np
import torch

import fft_conv_ref as FR
import restore_noisy_ref as NR
from repaint_ref import draw

f32 = np.float32


def gain(k, H, W, tol):
    """[H, W] float64: 1 / |K^| on the kept frequencies, 0 elsewhere"""
    mag = np.abs(FR.spectrum(k, H, W))
    M = FR.kept(k, H, W, tol)
    g = np.zeros((H, W))
    g[M] = 1.0 / mag[M]
    return g


def multipliers(M, gain32, s, nsc):
    """(lam, phi) float32 [..., H, W] for the kept frequencies M [H, W] bool, gain32 [H, W] float32 and the rows' s and nsc (float32
    scalars or arrays [B]): numpy float32 arithmetic, each operation rounded on its own, division and square root correctly rounded"""
    s = np.asarray(s, dtype=f32).reshape(-1, 1, 1)
    nsc = np.asarray(nsc, dtype=f32).reshape(-1, 1, 1)
    gain32 = np.asarray(gain32, dtype=f32)
    g = (nsc * gain32[None]).astype(f32)
    s_b = np.broadcast_to(s, g.shape).astype(f32)
    full = s_b >= g
    d = ((s_b * s_b).astype(f32) - (g * g).astype(f32)).astype(f32)
    phi_full = np.sqrt(np.maximum(d, f32(0))).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam_part = (s_b / g).astype(f32)
    lam = np.where(full, f32(1), lam_part).astype(f32)
    phi = np.where(full, phi_full, f32(0)).astype(f32)
    Mb = np.broadcast_to(np.asarray(M, dtype=bool)[None], g.shape)
    lam = np.where(Mb, lam, f32(0)).astype(f32)
    phi = np.where(Mb, phi, s_b).astype(f32)
    assert lam.dtype == f32 and phi.dtype == f32
    return lam, phi


def device_index(H, W):
    """[H, W] int: where the device's transform leaves frequency (u, v) of a plane, brev(u) W + brev(v)"""
    def brev(n):
        bits = n.bit_length() - 1
        return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])
    return brev(H)[:, None] * W + brev(W)[None, :]


def to_natural(spec, H, W):
    """the device's spectrum [..., H W] in the transform's order -> [..., H, W] in natural order"""
    return np.asarray(spec)[..., device_index(H, W)]


def to_device(spec, H, W):
    """[..., H, W] in natural order -> [..., H W] in the transform's order"""
    spec = np.asarray(spec)
    out = np.empty(spec.shape[:-2] + (H * W,), dtype=spec.dtype)
    out[..., device_index(H, W).ravel()] = spec.reshape(spec.shape[:-2] + (H * W,))
    return out


def shaped(z, phi):
    """n = Re F2^-1(phi F2(z)) per plane: [B, C, H, W] tensor or array, phi [B, H, W] -> float64 array"""
    z = FR.planes(z) if torch.is_tensor(z) else np.asarray(z, dtype=np.float64)
    return np.fft.ifft2(np.asarray(phi, dtype=np.float64)[:, None] * np.fft.fft2(z, axes=(-2, -1)), axes=(-2, -1)).real


def project(x0, Yhat, M, lam):
    """x0' in float64: x0 [B, C, H, W], Yhat [B, C, H, W] complex128 in natural order (never read where M is false), lam [B, H, W]"""
    x0 = FR.planes(x0) if torch.is_tensor(x0) else np.asarray(x0, dtype=np.float64)
    X = np.fft.fft2(x0, axes=(-2, -1))
    lam = np.asarray(lam, dtype=np.float64)[:, None]
    Y = np.where(M, Yhat, 0.0)
    return np.fft.ifft2(np.where(M, X + lam * (Y - X), X), axes=(-2, -1)).real


def step(x, eps, M, gain32, Yhat, cr, crm1, c1, c2, s, nsc, z, lam_phi=None):
    """One step, per-sample coefficients [B] (s already 0 where the row is 0): x0 in fp32 as restore_ref.step, lam and phi in fp32,
    the rest in float64.  lam_phi: (lam, phi) [B, H, W] in the multipliers' place.  Returns (x_prev, x0, x0', n, lam, phi)."""
    col = lambda v: v.reshape(-1, 1, 1, 1)
    x0 = (col(cr) * x - col(crm1) * eps).clamp(-1, 1)
    assert x0.dtype == torch.float32
    lam, phi = multipliers(M, gain32, s.numpy(), nsc.numpy()) if lam_phi is None else lam_phi
    x0p = torch.from_numpy(project(x0, Yhat, M, lam))
    n = torch.from_numpy(shaped(z, phi))
    out = (col(c1).double() * x0p + col(c2).double() * x.double()) + n
    return out, x0, x0p, n, lam, phi


class DeconvNoisy(NR.RestoreNoisy):
    def rows(self, sigma_y, ddim=False, eta=0.0):
        """float32 arrays [K]: c1, c2, s (sigma with row 0 zeroed) and nsc = |c1| sigma_y, formed in float64"""
        c1, c2, sigma32 = NR.linear_tables(self.sd, ddim, eta)
        s = sigma32.numpy().astype(f32).copy()
        s[0] = 0.0
        c1 = np.asarray(c1, dtype=np.float64)
        return dict(c1=c1.astype(f32), c2=np.asarray(c2, dtype=np.float64).astype(f32), s=s, nsc=(np.abs(c1) * sigma_y).astype(f32))

    def run(self, eps_model, x, y, k, tol, sigma_y, seed, stream=0, ddim=False, eta=0.0, lam_phi=None):
        """x: x_T [B, C, H, W]; y [B, C, H, W] the noisy blurred image.  Returns x after steps K-1 .. 0.  lam_phi(row, lam, phi) ->
        (lam, phi), when given, replaces the row's multipliers (the tests force lam = 1, phi = s with it)."""
        shape = tuple(x.shape)
        B, _, H, W = shape
        M = FR.kept(k, H, W, tol)
        g32 = gain(k, H, W, tol).astype(f32)
        Yhat = FR.pinv_spectrum(k, H, W, tol) * np.fft.fft2(FR.planes(y), axes=(-2, -1))
        tab = self.rows(sigma_y, ddim, eta)
        with torch.no_grad():
            for kk in range(self.K - 1, -1, -1):
                z = draw(shape, seed, kk, stream) if kk > 0 else torch.zeros(shape)
                x0, _ = self.sd._pred_xstart(eps_model, x, kk)
                lam, phi = multipliers(M, g32, np.full(B, tab["s"][kk]), np.full(B, tab["nsc"][kk]))
                if lam_phi is not None:
                    lam, phi = lam_phi(kk, lam, phi)
                x0p = torch.from_numpy(project(x0, Yhat, M, lam)).float()
                n = torch.from_numpy(shaped(z, phi)).float()
                x = (float(tab["c1"][kk]) * x0p + float(tab["c2"][kk]) * x) + n
        return x
