"""Where a NaN or an Inf in an op's input may, and must, show in its output: the footprint rules of tests/test_nonfinite_gpu.py,
written once.  Plain torch on the CPU; nothing here touches the library.

A test runs an op twice, on clean seeded inputs and on the same inputs with ONE element replaced by NaN, +Inf or -Inf (plant), and
compares the set of non-finite output elements with that of a reference of the same op on the same planted input (the oracle or a
torch restatement, in fp64 where the restatement allows it; never the kernel):

  exact        the two sets are equal
  exact_kinds  so are the classes (NaN, +Inf, -Inf) element by element
  within       reference set <= output set <= an allowed set derived from the algorithm (the Winograd kernels only: wino_allowed)
  isolated     every image but the planted one is bit-identical to the clean run

`isolated` is the property the finite-valued batch-independence tests cannot see: a kernel that reads a neighbour image's pixel and
multiplies it by an exact zero, or drops it under a mask, is right on finite data and wrong here, because 0 * NaN is NaN."""
import math

import torch

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
VALUES = (NAN, PINF, NINF)
FINITE, K_NAN, K_PINF, K_NINF = 0, 1, 2, 3


def plant(x, where, value):
    """a copy of x with x[where] = value; value is NaN, +Inf or -Inf, where an index tuple naming ONE element"""
    if not (math.isnan(value) or math.isinf(value)):
        raise ValueError(f"plant: {value!r} is finite")
    where = tuple(int(i) for i in where)
    if len(where) != x.dim():
        raise ValueError(f"plant: index {where} does not name one element of a tensor of shape {tuple(x.shape)}")
    out = x.clone()
    out[where] = value
    return out


def nonfinite(t):
    return ~torch.isfinite(t)


def kinds(t):
    """per element: 0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    k = torch.zeros(t.shape, dtype=torch.uint8)
    k[torch.isnan(t)] = K_NAN
    k[torch.isposinf(t)] = K_PINF
    k[torch.isneginf(t)] = K_NINF
    return k


def _shapes(out, ref):
    if tuple(out.shape) != tuple(ref.shape):
        raise ValueError(f"shapes differ: {tuple(out.shape)} vs {tuple(ref.shape)}")


def exact(out, ref):
    _shapes(out, ref)
    return torch.equal(nonfinite(out), nonfinite(ref))


def exact_kinds(out, ref):
    _shapes(out, ref)
    return torch.equal(kinds(out), kinds(ref))


def within(out, ref, allowed):
    """nonfinite(ref) <= nonfinite(out) <= allowed"""
    _shapes(out, ref)
    _shapes(out, allowed)
    o, r = nonfinite(out), nonfinite(ref)
    return not bool((r & ~o).any()) and not bool((o & ~allowed).any())


def isolated(out_planted, out_clean, image):
    """every image (index along dim 0) other than `image` has the same bits in the two runs"""
    _shapes(out_planted, out_clean)
    keep = [b for b in range(out_clean.shape[0]) if b != image]
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    return torch.equal(bits(out_planted[keep]), bits(out_clean[keep]))


def describe(out, ref, allowed=None):
    """one line for an assertion message: how the two non-finite sets differ"""
    o, r = nonfinite(out), nonfinite(ref)
    msg = f"{int(o.sum())} non-finite in the output, {int(r.sum())} in the reference, {int((r & ~o).sum())} missing, {int((o & ~r).sum())} extra"
    d = (kinds(out) != kinds(ref)).reshape(-1)
    if bool(d.any()):
        k = int(d.nonzero()[0])
        msg += f"; first difference at flat index {k}: {out.reshape(-1)[k].item()!r} vs {ref.reshape(-1)[k].item()!r}"
    if allowed is not None:
        msg += f"; {int((o & ~allowed).sum())} outside the allowed set of {int(allowed.sum())}"
    return msg


def wino_allowed(shape, where, tile=2, patch=4, transpose=False):
    """The output elements a Winograd conv may make non-finite when input element `where` = (b, y, x, c) of an NHWC map is: a boolean
    tensor of the NHWC output `shape` (B, Ho, Wo, N).

    Derivation, from the transform and not from a kernel.  F(m x m, r x r) cuts the output into m x m tiles (tile = m) and computes
    tile (ty, tx) as  A^T [ sum_c (G g_c G^T) o (B^T d_c B) ] A  where d_c is the (m + r - 1)^2 input patch (patch = m + r - 1) of
    channel c whose first row and column are  tile * ty - pad,  tile * tx - pad.  B^T d B forms sums and differences over the whole
    patch, so a non-finite d element may reach every one of the patch^2 products; the sum over c carries it to every output
    channel; and A^T M A recovers the m x m outputs by ADDING AND SUBTRACTING those products, which cancels a finite contribution
    and cannot cancel a NaN (Inf - Inf is NaN as well: which is why the rule compares sets and not kinds).  Nothing outside the
    patch enters the tile.  Hence: all channels of every output tile whose patch contains (y, x), in image b only.  Patches of
    neighbouring tiles overlap by r - 1, so up to two tiles per axis qualify.
      3x3, stride 1, padding 1 as F(2x2, 3x3): tile 2, patch 4, pad 1; Ho = H, Wo = W.
      transpose=True: ConvTranspose2d(4, stride 2, padding 1) as F(2x2, 2x2) per output phase (py, px): tile 2, patch 3; phase p reads
      input rows  tile * ty - 1 + p ..  and writes output rows  2 * (tile * ty + a) + p,  a < tile; the same along x.  Ho = 2 H.
    The direct conv's footprint (the reference's set) is a subset of this one; `within` asks for both inclusions."""
    B, Ho, Wo, N = shape
    b, y, x, _ = (int(i) for i in where)
    ok = torch.zeros(shape, dtype=torch.bool)

    def axis(pos, n_out):
        """output coordinates along one axis whose tile's patch holds input coordinate pos"""
        hit = []
        phases = (0, 1) if transpose else (0,)
        n_phase = n_out // 2 if transpose else n_out
        for p in phases:
            for t in range((n_phase + tile - 1) // tile):
                first = tile * t - 1 + p
                if first <= pos < first + patch:
                    hit += [(2 * (tile * t + a) + p) if transpose else (tile * t + a) for a in range(tile) if tile * t + a < n_phase]
        return sorted(set(hit))

    rows, cols = axis(y, Ho), axis(x, Wo)
    for r in rows:
        ok[b, r, cols, :] = True
    return ok
