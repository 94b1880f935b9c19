"""An independent restatement of the input transform for tests/test_native_data_{cpu,gpu}.py: it imports
nothing from utils/image_batch.py.  The resize matrix is built entry by entry in float64 from the formula of ATen's antialiased
bilinear interpolation, the resize / crop arithmetic is torchvision's Resize(int) + CenterCrop, and the flip rule goes through
oracle.philox_ref."""
import numpy as np

from oracle.philox_ref import philox4x32_10

# (Hs, Ws, S); every case runs with C = 1 and C = 3
SHAPES = [(218, 178, 64), (21, 13, 8), (13, 21, 8), (9, 9, 16), (40, 24, 32), (16, 16, 16), (33, 47, 16), (12, 20, 24), (64, 64, 16),
          (7, 5, 4)]


def tri(x):
    return max(1.0 - abs(x), 0.0)


def resize_matrix(n_in, n_out):
    """float64 [n_out, n_in]: F.interpolate(mode="bilinear", antialias=True, align_corners=False) along one axis"""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = min(1.0 / scale, 1.0)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        for j in range(lo, hi):
            m[i, j] = tri((j - c + 0.5) * inv)
        m[i] /= m[i].sum()
    return m


def geometry(Hs, Ws, S):
    """(Ho, Wo, top, left): Resize(S) of the short side, then CenterCrop(S)"""
    if Hs <= Ws:
        Ho, Wo = S, int(S * Ws / Hs)
    else:
        Ho, Wo = int(S * Hs / Ws), S
    return Ho, Wo, int(round((Ho - S) / 2.0)), int(round((Wo - S) / 2.0))


def matrices(Hs, Ws, S):
    """(A_h [S, Hs], A_w [S, Ws]) float64: the rows of the two resize matrices the crop keeps"""
    Ho, Wo, top, left = geometry(Hs, Ws, S)
    return resize_matrix(Hs, Ho)[top:top + S], resize_matrix(Ws, Wo)[left:left + S]


def unit32(u8):
    """u8 / 255 as fp32 computes it (a correctly rounded quotient), as float64"""
    return (u8.astype(np.float32) / np.float32(255.0)).astype(np.float64)


def transform(u8, A_h, A_w, flip=None):
    """float64 [B, C, S, S]: A_h (u8 / 255) A_w^T per channel, * 2 - 1, mirrored along W where flip[b]; u8 [B, Hs, Ws, C]"""
    rows = np.einsum("yh,bhwc->bcyw", np.asarray(A_h, dtype=np.float64), unit32(u8), optimize=True)   # one axis at a time: two matrix products
    x = np.einsum("bcyw,xw->bcyx", rows, np.asarray(A_w, dtype=np.float64), optimize=True) * 2.0 - 1.0
    if flip is not None:
        x = np.where(np.asarray(flip, dtype=bool)[:, None, None, None], x[..., ::-1], x)
    return x


def flips(ids, seed, epoch):
    """bool [n]: bit 0 of word 0 of Philox4x32-10, counter (id lo, id hi, epoch, 0x464c4950), key (seed lo, seed hi)"""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    n = ids.shape[0]
    ctr = np.stack([(ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ids >> np.uint64(32)).astype(np.uint32),
                    np.full(n, epoch, dtype=np.uint32), np.full(n, 0x464C4950, dtype=np.uint32)], axis=-1)
    key = np.stack([np.full(n, seed & 0xFFFFFFFF, dtype=np.uint32), np.full(n, (seed >> 32) & 0xFFFFFFFF, dtype=np.uint32)], axis=-1)
    return (philox4x32_10(ctr, key)[:, 0] & np.uint32(1)).astype(bool)


def bound(row_taps, col_taps):
    """two weighted sums of non-negative terms in fp32, the division and the final * 2 - 1"""
    return 2 * (row_taps + col_taps + 6) * 2.0 ** -24


def images(N, Hs, Ws, C, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(N, Hs, Ws, C), dtype=np.uint8)
