"""The host side of DDNM deconvolution for a 2-D point-spread function with periodic boundary: the PSF, its
spectrum and the truncated pseudo-inverse in the 2-D Fourier basis.  All float64 numpy.

Per channel of an image X [H, W], the PSF k [p, q] (p, q odd):

    A(X)[i, j] = sum_{a, b} k[a, b] X[(i + a - p // 2) mod H, (j + b - q // 2) mod W]       (correlation form, as blur.blur_matrix)

A is diagonal in the 2-D Fourier basis: F2(A X) = K^ . F2(X) with K^ = F2 of k embedded in an H x W plane with its centre at (0, 0)
and flipped (correlation), indices mod H, W.  Its truncated pseudo-inverse divides the spectra on the kept frequencies
M = |K^| > tol max |K^| and is zero elsewhere, so A+ A = F2^-1 M F2 is a projection.  The transforms themselves run on the device
(csrc/fft_conv.hip)."""
import numpy as np

from .blur import DEFAULT_TOL

PRESETS = ("diag", "disk")


def _preset(name):
    if name == "diag":            # a 45 degree motion: 1/9 on the main diagonal of 9 x 9
        return np.eye(9) / 9.0
    d = np.arange(9) - 4          # a defocus disk of radius 3.5
    k = ((d[:, None] ** 2 + d[None, :] ** 2) <= 3.5 ** 2).astype(np.float64)
    return k / k.sum()


def psf_array(psf):
    """The PSF as a float64 array [p, q]: a preset name, or a 2-D array or tensor with odd sides, finite entries and a non-zero sum;
    ValueError otherwise."""
    if isinstance(psf, str):
        if psf not in PRESETS:
            raise ValueError(f"psf: unknown preset {psf!r}, one of {PRESETS}")
        return _preset(psf)
    if hasattr(psf, "detach"):
        psf = psf.detach().cpu().numpy()
    try:
        k = np.array(psf, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("psf: must be a preset name or a 2-D array of numbers") from None
    if k.ndim != 2 or k.shape[0] % 2 == 0 or k.shape[1] % 2 == 0:
        raise ValueError(f"psf: must be a 2-D array with odd sides, got shape {k.shape}")
    if not np.isfinite(k).all():
        raise ValueError("psf: must be finite")
    if k.sum() == 0:
        raise ValueError("psf: the taps must not sum to zero")
    return np.ascontiguousarray(k)


def size_ok(C, H, W):
    """The planes the device transform takes: H and W powers of two in [16, 256], 1 to 8 channels."""
    return all(16 <= v <= 256 and v & (v - 1) == 0 for v in (int(H), int(W))) and 1 <= int(C) <= 8


def psf_spectrum(psf, H, W):
    """K^ [H, W] complex128: F2(A X) = K^ . F2(X).  The taps are laid into an H x W plane so that A is the correlation above: tap
    (a, b) at ((p // 2 - a) mod H, (q // 2 - b) mod W)."""
    k = psf_array(psf)
    p, q = k.shape
    H, W = int(H), int(W)
    if p > H or q > W:
        raise ValueError(f"psf: a {p} x {q} point-spread function does not fit a {H} x {W} plane")
    plane = np.zeros((H, W))
    ia = (p // 2 - np.arange(p)) % H
    ib = (q // 2 - np.arange(q)) % W
    np.add.at(plane, (ia[:, None], ib[None, :]), k)
    return np.fft.fft2(plane)


def psf_projection(psf, H, W, tol=DEFAULT_TOL):
    """(P^, M, kept): the truncated reciprocal spectrum P^ [H, W] complex128 (A+ = F2^-1 P^ F2), the kept frequencies M [H, W] bool,
    Hermitian-symmetric by construction (M[u, v] = M[-u, -v]), and their number."""
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (0 <= tol < 1):
        raise ValueError(f"psf: tol must be a real number in [0, 1), got {tol!r}")
    K = psf_spectrum(psf, H, W)
    mag = np.abs(K)
    M = mag > float(tol) * mag.max()
    M &= np.roll(M[::-1, ::-1], (1, 1), axis=(0, 1))      # (u, v) and (-u, -v) are kept together
    P = np.zeros_like(K)
    P[M] = np.conj(K[M]) / (mag[M] ** 2)
    return P, M, int(M.sum())


def twiddles(L):
    """exp(-2 pi i j / L), j < L / 2, in float64 rounded to fp32: [L / 2, 2] (re, im), the table the device transform reads."""
    j = np.arange(int(L) // 2)
    w = np.exp(-2j * np.pi * j / int(L))
    return np.stack([w.real, w.imag], axis=1).astype(np.float32)


def interleave(S):
    """A complex [H, W] array as fp32 [H, W, 2] (re, im), the layout of the device's multiplier."""
    S = np.asarray(S)
    return np.ascontiguousarray(np.stack([S.real, S.imag], axis=-1).astype(np.float32))


def psf_operands(psf, H, W, tol=DEFAULT_TOL):
    """What the chain takes, as numpy arrays: K^ and P^ interleaved fp32 [H, W, 2], the mask as fp32 [H, W] (1 where kept) and the
    twiddles of max(H, W)."""
    P, M, _ = psf_projection(psf, H, W, tol)
    return interleave(psf_spectrum(psf, H, W)), interleave(P), np.ascontiguousarray(M.astype(np.float32)), twiddles(max(int(H), int(W)))


def psf_noisy_operands(psf, H, W, tol, sigma_y, c1):
    """(gain, nsc) of the DDNM+ deconvolution step, formed in float64 and stored as fp32: gain [H, W] is
    1 / |K^| at the kept frequencies and 0 elsewhere (Hermitian-symmetric like the mask, natural frequency order); nsc [rows] is
    |c1[k]| sigma_y for the chain's table c1 (an array or a tensor, one entry per row)."""
    if isinstance(sigma_y, bool) or not isinstance(sigma_y, (int, float, np.integer, np.floating)) or not np.isfinite(sigma_y) or sigma_y < 0:
        raise ValueError(f"psf: sigma_y must be a finite real number >= 0, got {sigma_y!r}")
    _, M, _ = psf_projection(psf, H, W, tol)
    mag = np.abs(psf_spectrum(psf, H, W))
    mag = 0.5 * (mag + np.roll(mag[::-1, ::-1], (1, 1), axis=(0, 1)))      # |K^(f)| = |K^(-f)| to the last bit
    gain = np.zeros((int(H), int(W)))
    gain[M] = 1.0 / mag[M]
    if hasattr(c1, "detach"):
        c1 = c1.detach().cpu().numpy()
    nsc = np.abs(np.asarray(c1, dtype=np.float64).reshape(-1)) * float(sigma_y)
    return np.ascontiguousarray(gain.astype(np.float32)), np.ascontiguousarray(nsc.astype(np.float32))
