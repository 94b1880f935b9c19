"""The host side of DDNM's compressed-sensing operator: which pixels the transform reads in which order,
and how many of its coefficients are measured.

Per channel, the plane is flattened row-major (j = h W + w, N = H W a power of two), read through a permutation, a[j] = X[perm[j]],
and transformed by the orthonormal Walsh-Hadamard matrix in natural (Sylvester) order; the measurement is the first m coefficients.
The permutation is shared by channels and batch.  The transform itself runs on the device (csrc/hadamard.hip)."""
import numpy as np


def cs_perm(N, seed=0):
    """The pixel permutation of a plane of N pixels: numpy's default_rng(seed).permutation(N), as int32."""
    N = int(N)
    if N <= 0:
        raise ValueError(f"cs_perm: N must be positive, got {N}")
    return np.random.default_rng(int(seed)).permutation(N).astype(np.int32)


def cs_rows(ratio, N):
    """The measured coefficients per plane at a sampling ratio in (0, 1]: 4 round(ratio N / 4), clipped to [4, N]."""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or not (0 < ratio <= 1):
        raise ValueError(f"cs_rows: ratio must be a real number in (0, 1], got {ratio!r}")
    N = int(N)
    return int(min(max(4 * int(round(float(ratio) * N / 4)), 4), N))


def size_ok(C, H, W):
    """The planes the device transform takes: H and W powers of two in [16, 256], 1 to 8 channels."""
    return all(16 <= v <= 256 and v & (v - 1) == 0 for v in (int(H), int(W))) and 1 <= int(C) <= 8


def check_perm(perm, N, who="cs"):
    """perm as a contiguous int32 array after checking that it is a permutation of 0 .. N - 1; ValueError otherwise."""
    if hasattr(perm, "detach"):
        perm = perm.detach().cpu().numpy()
    try:
        p = np.asarray(perm)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: perm must be an integer array") from None
    if p.ndim != 1 or p.shape[0] != N or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"{who}: perm must be an integer array of {N} entries, got shape {p.shape} {p.dtype}")
    if not np.array_equal(np.sort(p.astype(np.int64)), np.arange(N)):
        raise ValueError(f"{who}: perm is not a permutation of 0 .. {N - 1}")
    return np.ascontiguousarray(p.astype(np.int32))
