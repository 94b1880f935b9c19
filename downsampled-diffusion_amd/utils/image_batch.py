"""The image transform of the input pipeline, stated once.

The reference's chain (utils/data.py:48-84) is ToTensor (u8 / 255) -> Resize(S) -> CenterCrop(S) -> t * 2 - 1 -> RandomHorizontalFlip
when config['rnd_flip'].  Resize is torchvision's for tensors, F.interpolate(mode="bilinear", antialias=True, align_corners=False):
a separable linear map, so Resize + CenterCrop is S rows of its matrix along H and S rows along W.  This module builds those rows as
tap tables in float64 (rounded to fp32 once) for csrc/image_batch.hip and for the loader's host path, and states the flip rule.
numpy only; nothing here touches a device.
"""
import numpy as np

FLIP_WORD = 0x464C4950       # 'FLIP': counter word 3 of the flip draw
MAX_TAPS = 32                # csrc/image_batch.hip


def resized_shape(Hs: int, Ws: int, S: int) -> tuple:
    """torchvision Resize(S) for an int: the short side becomes S, the long side int(S * long / short)."""
    if Hs <= Ws:
        return S, int(S * Ws / Hs)
    return int(S * Hs / Ws), S


def crop_offset(n: int, S: int) -> int:
    """torchvision CenterCrop: int(round((n - S) / 2.0)) -- Python's round, a half goes to even (53 -> 32 starts at 10)."""
    return int(round((n - S) / 2.0))


def _row(n_in: int, n_out: int, i: int):
    """(lo, float64 weights) of output i of the antialiased bilinear resize n_in -> n_out (ATen's _compute_indices_weights_aa)"""
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = min(1.0 / scale, 1.0)
    c = scale * (i + 0.5)
    lo = max(int(c - support + 0.5), 0)
    hi = min(int(c + support + 0.5), n_in)
    w = np.maximum(1.0 - np.abs((np.arange(lo, hi, dtype=np.float64) - c + 0.5) * inv), 0.0)
    keep = np.flatnonzero(w)                 # a tap at the very edge of the support weighs exactly 0 (n_in == n_out: one weight of 1 is left)
    w = w[keep[0]:keep[-1] + 1]
    return lo + int(keep[0]), w / w.sum()


def resize_tables(n_in: int, n_out: int, off: int, S: int) -> tuple:
    """(start int32 [S], weights float32 [S, taps], taps): rows off .. off+S-1 of the n_in -> n_out resize matrix.  taps is the longest
    row's length; shorter rows are padded with zero weights, their start moved down so that start + taps <= n_in."""
    if not (0 <= off and off + S <= n_out):
        raise ValueError(f"resize_tables: rows {off}..{off + S - 1} are not rows of a {n_in} -> {n_out} resize")
    rows = [_row(n_in, n_out, off + i) for i in range(S)]
    taps = max(len(w) for _, w in rows)
    start = np.zeros(S, dtype=np.int32)
    weights = np.zeros((S, taps), dtype=np.float32)
    for i, (lo, w) in enumerate(rows):
        st = min(lo, n_in - taps)
        start[i] = st
        weights[i, lo - st:lo - st + len(w)] = w.astype(np.float32)
    return start, weights, taps


def dense(start: np.ndarray, weights: np.ndarray, n_in: int) -> np.ndarray:
    """the tables as a matrix [S, n_in] of their own dtype"""
    S, taps = weights.shape
    m = np.zeros((S, n_in), dtype=weights.dtype)
    for i in range(S):
        m[i, start[i]:start[i] + taps] = weights[i]
    return m


class Transform:
    """Resize(S) + CenterCrop(S) of Hs x Ws images as two tap tables (rows: along H, cols: along W)."""

    def __init__(self, Hs: int, Ws: int, S: int):
        if S < 4 or S > 1024 or S % 4:
            raise ValueError(f"image size {S}: the batch kernel takes multiples of 4 in [4, 1024]")
        self.Hs, self.Ws, self.S = int(Hs), int(Ws), int(S)
        self.Ho, self.Wo = resized_shape(Hs, Ws, S)
        self.top, self.left = crop_offset(self.Ho, S), crop_offset(self.Wo, S)
        self.row_start, self.row_w, self.row_taps = resize_tables(Hs, self.Ho, self.top, S)
        self.col_start, self.col_w, self.col_taps = resize_tables(Ws, self.Wo, self.left, S)
        if max(self.row_taps, self.col_taps) > MAX_TAPS:
            raise ValueError(f"{Hs}x{Ws} -> {S}: {max(self.row_taps, self.col_taps)} taps, the batch kernel takes {MAX_TAPS} "
                             f"(a reduction by more than {MAX_TAPS // 2 - 1}x): pack the data set smaller (prepare_dataset.py --size)")

    def matrices(self) -> tuple:
        """(A_h [S, Hs], A_w [S, Ws]) fp32"""
        return dense(self.row_start, self.row_w, self.Hs), dense(self.col_start, self.col_w, self.Ws)


# ---- Philox4x32-10 (Salmon et al., SC'11), the flip draw
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def _philox_word0(c0, c1, c2, c3, k0, k1):
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = (k0 + _W0).astype(np.uint32), (k1 + _W1).astype(np.uint32)
            p0, p1 = c0.astype(np.uint64) * _M0, c2.astype(np.uint64) * _M1
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _LO).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _LO).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0


def flip_bits(ids, seed: int, epoch: int) -> np.ndarray:
    """bool [n]: image id is mirrored iff bit 0 of word 0 of Philox4x32-10 with counter (id lo, id hi, epoch, 'FLIP') and key
    (seed lo, seed hi) is set -- a function of the image, the epoch and the seed, not of the batch, the position or the rank."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64).reshape(-1)
    n = ids.shape[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    full = lambda v: np.full(n, v, dtype=np.uint32)       # noqa: E731
    w0 = _philox_word0((ids & _LO).astype(np.uint32), (ids >> np.uint64(32)).astype(np.uint32), full(int(epoch) & 0xFFFFFFFF),
                       full(FLIP_WORD), full(seed & 0xFFFFFFFF), full(seed >> 32))
    return (w0 & np.uint32(1)).astype(bool)
