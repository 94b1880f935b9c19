"""Host mathematics of DDNM deblurring for a separable blur with zero padding.

A(X) = A_h X A_w^T per channel of a pixel-space image X [H, W]: A_h is the H x H band matrix of a 1-D kernel k_h of odd length L,
A_h[i, i + j - L // 2] = k_h[j], entries outside the image dropped (zero padding); A_w likewise from k_w.  The pseudo-inverse is
taken per axis, in float64: with A = U S V^T the singular values above tol * s_max are kept, Q = V_k S_k^-1 U_k^T is the truncated
pseudo-inverse and P = Q A = V_k V_k^T the symmetric projection onto the retained right singular vectors.  A+ = Q_h (x) Q_w and
A+ A = P_h (x) P_w stay separable.  (The DDRM / DDNM code thresholds the PRODUCTS of the two axes' singular values instead, which keeps
a non-separable set of directions; the per-axis rule is what lets the step be two small matrix products.)
"""
import functools

import numpy as np
import torch

PRESETS = ("uniform", "gauss", "aniso")
DEFAULT_TOL = 3e-2


def _gauss_taps(length, sigma):
    r = np.arange(length, dtype=np.float64) - length // 2
    k = np.exp(-0.5 * (r / sigma) ** 2)
    return k / k.sum()


def _taps(k, what):
    k = np.asarray(k, dtype=np.float64)
    if k.ndim != 1 or k.size % 2 == 0 or not np.all(np.isfinite(k)):
        raise ValueError(f"blur_kernel: {what} must be a finite 1-D array of odd length, got shape {k.shape}")
    return k


def blur_kernel(kernel):
    """(k_h, k_w), float64 1-D arrays of odd length: a preset's taps ("uniform": 9 of 1/9; "gauss": 5 taps of exp(-(r / 10)^2 / 2),
    normalised; "aniso": 9 normalised Gaussian taps, sigma 20 down the rows and sigma 1 along them), one odd-length 1-D array for both
    axes, or a pair (k_h, k_w) of such arrays."""
    if isinstance(kernel, str):
        if kernel == "uniform":
            k = np.full(9, 1.0 / 9.0)
            return k, k.copy()
        if kernel == "gauss":
            k = _gauss_taps(5, 10.0)
            return k, k.copy()
        if kernel == "aniso":
            return _gauss_taps(9, 20.0), _gauss_taps(9, 1.0)
        raise ValueError(f"blur_kernel: kernel must be one of {PRESETS}, an odd-length 1-D array or a pair of them, got {kernel!r}")
    if isinstance(kernel, (tuple, list)) and len(kernel) == 2 and not np.isscalar(kernel[0]):
        return _taps(kernel[0], "k_h"), _taps(kernel[1], "k_w")
    if torch.is_tensor(kernel):
        kernel = kernel.detach().cpu().numpy()
    k = _taps(kernel, "the kernel")
    return k, k.copy()


def blur_matrix(n, k):
    """The n x n float64 band matrix of the taps k with zero padding: A[i, i + j - L // 2] = k[j]."""
    k = _taps(k, "k")
    A = np.zeros((n, n), dtype=np.float64)
    half = k.size // 2
    for j in range(k.size):
        d = j - half
        i = np.arange(max(0, -d), min(n, n - d))
        A[i, i + d] = k[j]
    return A


def blur_projection(A, tol=DEFAULT_TOL):
    """(Q, P, rank) of a float64 matrix A [h, H], square or not: the pseudo-inverse Q [H, h] truncated at tol * s_max, the projection
    P = Q A [H, H], the number of singular values kept."""
    A = np.asarray(A, dtype=np.float64)
    if not (np.isfinite(tol) and 0 <= tol < 1):
        raise ValueError(f"blur_projection: tol must be in [0, 1), got {tol!r}")
    U, S, Vt = np.linalg.svd(A)
    rank = int(np.count_nonzero(S > tol * S[0]))
    Q = (Vt[:rank].T / S[:rank]) @ U[:, :rank].T
    return Q, Q @ A, rank


def _key(kernel):
    k_h, k_w = blur_kernel(kernel)
    return k_h.tobytes(), k_w.tobytes()


@functools.lru_cache(maxsize=16)
def _operands(kh_bytes, kw_bytes, H, W, tol):
    out = []
    for kb, n in ((kh_bytes, H), (kw_bytes, W)):
        A = blur_matrix(n, np.frombuffer(kb, dtype=np.float64))
        Q, P, rank = blur_projection(A, tol)
        out.append((A, Q, P, rank))
    (A_h, Q_h, P_h, _), (A_w, Q_w, P_w, _) = out
    return tuple(torch.tensor(m, dtype=torch.float32) for m in (A_h, A_w, Q_h, Q_w, P_h, P_w))


def blur_operands(kernel, H, W, tol=DEFAULT_TOL):
    """The fp32 CPU tensors A_h [H, H], A_w [W, W], Q_h, Q_w, P_h, P_w of a kernel (blur_kernel's argument) on an H x W image: formed
    in float64, once per (taps, H, W, tol)."""
    return _operands(*_key(kernel), int(H), int(W), float(tol))


# ---------------------------------------------------------------- size-changing separable operators
RESIZE_KINDS = ("bicubic", "mean")


def _keys_cubic(x):
    """Keys' cubic convolution kernel with a = -0.5."""
    x = np.abs(x)
    return np.where(x <= 1, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2, ((-0.5 * x + 2.5) * x - 4) * x + 2, 0.0))


def resize_matrix(H, scale, kind="bicubic"):
    """A [H / scale, H], float64: one axis of the reduction by an integer scale.  "bicubic": antialiased bicubic downsampling, the
    matrix of torch.nn.functional.interpolate(mode="bicubic", antialias=True, align_corners=False) -- output row i has its centre at
    c = (i + 0.5) scale and the weights k((j - c + 0.5) / scale) over max(int(c - 2 scale + 0.5), 0) <= j < min(int(c + 2 scale + 0.5), H),
    normalised to sum to 1.  "mean": 1 / scale over each block (what super_resolve holds)."""
    if isinstance(H, bool) or isinstance(scale, bool) or not isinstance(H, (int, np.integer)) or not isinstance(scale, (int, np.integer)) \
            or scale < 1 or H < scale or H % scale:
        raise ValueError(f"resize_matrix: scale must be a positive int dividing H, got H = {H!r}, scale = {scale!r}")
    if kind not in RESIZE_KINDS:
        raise ValueError(f"resize_matrix: kind must be one of {RESIZE_KINDS}, got {kind!r}")
    H, n = int(H), int(scale)
    A = np.zeros((H // n, H), dtype=np.float64)
    for i in range(H // n):
        if kind == "mean":
            A[i, i * n:(i + 1) * n] = 1.0 / n
            continue
        c = (i + 0.5) * n
        lo, hi = max(int(c - 2 * n + 0.5), 0), min(int(c + 2 * n + 0.5), H)
        w = _keys_cubic((np.arange(lo, hi, dtype=np.float64) - c + 0.5) / n)
        A[i, lo:hi] = w / w.sum()
    return A


def _matrix(A, what):
    if torch.is_tensor(A):
        A = A.detach().cpu().numpy()
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[0] > A.shape[1] or not np.all(np.isfinite(A)):
        raise ValueError(f"separable_operands: {what} must be a finite [h, H] matrix with h <= H, got shape {A.shape}")
    return A


@functools.lru_cache(maxsize=16)
def _sep_operands(ah_bytes, aw_bytes, h, H, w, W, tol):
    out = []
    for ab, shape in ((ah_bytes, (h, H)), (aw_bytes, (w, W))):
        A = np.frombuffer(ab, dtype=np.float64).reshape(shape)
        Q, P, rank = blur_projection(A, tol)
        out.append((A, Q, P, rank))
    (A_h, Q_h, P_h, r_h), (A_w, Q_w, P_w, r_w) = out
    return tuple(torch.tensor(m, dtype=torch.float32) for m in (A_h, A_w, Q_h, Q_w, P_h, P_w)) + (r_h, r_w)


def separable_operands(A_h, A_w, tol=DEFAULT_TOL):
    """(A_h [h, H], A_w [w, W], Q_h [H, h], Q_w [W, w], P_h [H, H], P_w [W, W], rank_h, rank_w) of any separable operator
    A(X) = A_h X A_w^T given as a float64 matrix pair: the six fp32 CPU tensors of blur_projection per axis and the ranks it kept.
    Formed in float64, once per (matrices, tol); a square band matrix gives exactly blur_operands' tensors."""
    A_h, A_w = _matrix(A_h, "A_h"), _matrix(A_w, "A_w")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (0 <= tol < 1):
        raise ValueError(f"separable_operands: tol must be a real number in [0, 1), got {tol!r}")
    return _sep_operands(A_h.tobytes(), A_w.tobytes(), *A_h.shape, *A_w.shape, float(tol))
