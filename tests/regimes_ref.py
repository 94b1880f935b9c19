"""Input regimes, plain restatements, deliberately wrong variants and error bars for the norm, attention and optimiser kernels
("Input regimes of the norm, attention and optimiser tests").

Every restatement takes its precision from its inputs: called on ``.double()`` tensors it is the reference, called on the fp32 tensors
it shows what fp32 arithmetic alone costs on that input (``e32``).  A kernel is held to ``bar(existing, e32) = max(existing bar of
the path, 8 x e32)``: 8 for its other summation tree and its Welford / Chan merges.  The ``E32_*`` tables hold the measured ``e32``
(torch on the CPU, maximum over the shapes the GPU tests use); tests/test_regimes_cpu.py measures them again and fails when a stored
value is below the measurement.  The wrong variants (an eps in the wrong place, a one-pass variance, a softmax without its maximum)
are CPU functions only: the CPU test shows that each misses these bars by 10 x in some regime, which is what makes the GPU tests of
the same bars worth running.
"""
import functools
import math

import torch

from oracle import train_ref as TR
from oracle import unet_ref as U

GN_EPS, LN_EPS, GROUPS = U.GN_EPS, U.LN_EPS, U.GROUPS
FACTOR = 8.0
MISH_ABS_BAR = 2e-6                    # test_mish_matches_torch


def err(a, b):
    """max|a - b| / max|b| in fp64; inf when a holds a non-finite value (a miss of any bar)"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    if not bool(torch.isfinite(a).all()):
        return math.inf
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def abs_err(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    if not bool(torch.isfinite(a).all()):
        return math.inf
    return float((a - b).abs().max())


def bar(existing, e32):
    return max(existing, FACTOR * e32)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


# ------------------------------------------------------------------ GroupNorm
GN_REGIMES = ["plain", "tinyvar", "var~eps", "offset", "big", "const", "mixed"]
GN_BWD_REGIMES = ["plain", "tinyvar", "var~eps", "offset", "const"]
# the regime of each of the 8 groups of `mixed`: the six above, then two of them again on other draws
GN_MIXED = ["plain", "tinyvar", "var~eps", "offset", "big", "const", "tinyvar", "offset"]
GN_CONST = 1.75                        # k * 1.75 is exact in fp32 for every k up to a group's size: mean == 1.75, var == 0, exactly


def _gn_fill(regime, shape, g):
    z = torch.randn(shape, generator=g)
    if regime == "plain":
        return 2.0 * z + 0.5
    if regime == "tinyvar":            # var ~ 1e-6 < eps: eps dominates rstd
        return 3.0 + 1e-3 * z
    if regime == "var~eps":            # var ~ 9e-6 ~ eps
        return 0.25 + 3e-3 * z
    if regime == "offset":             # |mean| = 1000 std
        return 1000.0 + z
    if regime == "big":
        return 3e3 * z
    if regime == "const":
        return torch.full(shape, GN_CONST)
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def gn_input(regime, B, C, H, W, seed=0):
    """fp32 NCHW, never modified by its users"""
    g = _gen(1000 + seed)
    if regime != "mixed":
        return _gn_fill(regime, (B, C, H, W), g)
    cpg = C // GROUPS
    return torch.cat([_gn_fill(GN_MIXED[j], (B, cpg, H, W), g) for j in range(GROUPS)], dim=1)


@functools.lru_cache(maxsize=None)
def gn_params(C, B=0, seed=0):
    """gamma, beta [C] and a time shift [B, C]"""
    return 1 + 0.2 * rnd(C, seed=2000 + seed), 0.2 * rnd(C, seed=2001 + seed), rnd(max(B, 1), C, seed=2002 + seed)


def gn_norm(x, gamma, beta, groups=GROUPS, eps=GN_EPS, variant="ref"):
    """GroupNorm of NCHW x as torch.nn.GroupNorm defines it: two-pass variance, eps under the root.  variant: 'eps_outside'
    1 / (sqrt(var) + eps); 'no_eps'; 'onepass' var = E[x^2] - mean^2; 'mean_recip' x - sum * fl(1 / n) in one fused multiply-add, the
    product not rounded -- the wrong forms."""
    B, C = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(dim=-1, keepdim=True)
    xc = xg - mean
    if variant == "mean_recip":        # for an n that is no power of two a constant group then keeps x - mean = -x * (the rounding of 1 / n)
        inv = torch.tensor(1.0 / xg.shape[-1], dtype=x.dtype).double()
        xc = (xg.double() - xg.sum(dim=-1, keepdim=True).double() * inv).to(x.dtype)
    if variant == "onepass":
        var = ((xg * xg).mean(dim=-1, keepdim=True) - mean * mean).clamp_min(0)
    else:
        var = (xc ** 2).mean(dim=-1, keepdim=True)
    if variant == "eps_outside":
        r = 1.0 / (var.sqrt() + eps)
    elif variant == "no_eps":
        r = 1.0 / var.sqrt()
    else:
        r = 1.0 / (var + eps).sqrt()
    y = (xc * r).reshape(x.shape)
    return y * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)


def gn_mish(x, gamma, beta, temb=None, addend=None, groups=GROUPS, eps=GN_EPS, variant="ref"):
    """Block's GroupNorm -> Mish (+ time shift [B, C]) (+ residual)"""
    y = U.mish(gn_norm(x, gamma, beta, groups, eps, variant))
    if temb is not None:
        y = y + temb[:, :, None, None]
    if addend is not None:
        y = y + addend
    return y


def gn_tail(x, gamma, beta, w, b):
    """GroupNorm -> Mish -> 1x1 projection w [n, C], b [n]: the last layers of the network"""
    return torch.einsum("bchw,nc->bnhw", gn_mish(x, gamma, beta), w) + b.view(1, -1, 1, 1)


def gn_grads(x, gamma, beta, dy, groups=GROUPS, eps=GN_EPS):
    """autograd of gn_mish in the precision of its inputs -> (dx, dgamma, dbeta)"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, gamma, beta)]
    return torch.autograd.grad(gn_mish(*leaves, groups=groups, eps=eps), leaves, dy)


def d(*ts):
    out = tuple(None if t is None else t.double() for t in ts)
    return out if len(out) > 1 else out[0]


# the shapes (B, C, H, W) the GPU tests run GroupNorm at, by the bar they share.  e32 is measured over all of them.
GN_SHAPES = [(2, 32, 8, 8), (3, 64, 5, 7), (2, 32, 65, 64), (1, 64, 32, 16), (2, 64, 8, 8), (2, 64, 16, 16), (2, 64, 4, 4), (8, 64, 2, 2),
             (2, 256, 4, 4), (2, 256, 8, 8), (2, 24, 8, 8), (2, 32, 16, 16)]
GN_BWD_SHAPES = [(2, 32, 8, 8), (3, 64, 5, 7), (2, 128, 48, 48), (2, 64, 8, 8), (2, 24, 8, 8)]
CLUSTER_SHAPE = (16, 128, 32, 32)      # smallest entry of test_step_edges_gpu.CLUSTER_CASES
GN_SHAPES_BIG = [CLUSTER_SHAPE]

# e32 of gn_mish (no shift, no residual) per regime, maximum over GN_SHAPES + GN_SHAPES_BIG
E32_GN = {"plain": 2.1e-7, "tinyvar": 1.5e-4, "var~eps": 5.4e-6, "offset": 4.9e-5, "big": 2.4e-7, "mixed": 4.6e-5}
# ... of gn_tail (n = 3) at (2, 32, 16, 16)
E32_GN_TAIL = {"plain": 1.4e-7, "tinyvar": 2.4e-5, "var~eps": 3.2e-6, "offset": 2.5e-5, "big": 1.8e-7, "mixed": 1.4e-5}
# ... of gn_grads (dx, dgamma, dbeta), maximum over GN_BWD_SHAPES
E32_GN_BWD = {"plain": (2.6e-7, 1.7e-7, 1.7e-7), "tinyvar": (8.4e-5, 2.6e-4, 6.0e-5), "var~eps": (5.2e-6, 8.7e-6, 4.4e-6),
              "offset": (9.4e-5, 1.1e-4, 6.7e-5), "const": (1.8e-7, 0.0, 2.3e-7)}       # const: dgamma == 0 exactly


def gn_e32(regime, shape, seed=0):
    x = gn_input(regime, *shape, seed=seed)
    g, b, _ = gn_params(shape[1])
    return err(gn_mish(x, g, b), gn_mish(*d(x, g, b)))


@functools.lru_cache(maxsize=None)
def tail_proj(C, n=3):
    return rnd(n, C, seed=2010, scale=C ** -0.5), rnd(n, seed=2011)


def gn_tail_e32(regime, shape=(2, 32, 16, 16)):
    x = gn_input(regime, *shape)
    g, b, _ = gn_params(shape[1])
    w, bw = tail_proj(shape[1])
    return err(gn_tail(x, g, b, w, bw), gn_tail(*d(x, g, b, w, bw)))


@functools.lru_cache(maxsize=None)
def gn_dy(B, C, H, W):
    return rnd(B, C, H, W, seed=2020)


def gn_bwd_e32(regime, shape):
    x = gn_input(regime, *shape)
    g, b, _ = gn_params(shape[1])
    dy = gn_dy(*shape)
    return tuple(err(a, r) for a, r in zip(gn_grads(x, g, b, dy), gn_grads(*d(x, g, b, dy))))


# ------------------------------------------------------------------ channel LayerNorm (rows = pixels, columns = channels)
LN_REGIMES = ["plain", "tinystd", "std~eps", "offset", "const", "mixed"]
LN_X_REGIMES = ["plain", "tinystd", "std~eps", "offset"]      # what the from-x attention kernels get besides the k regimes
LN_MIXED = ["plain", "tinystd", "std~eps", "offset", "const"]
LN_CONST = 0.75


def _ln_fill(regime, shape, g):
    z = torch.randn(shape, generator=g)
    if regime == "plain":
        return 3.0 * z + 1.0
    if regime == "tinystd":
        return 0.7 + 1e-3 * z
    if regime == "std~eps":            # std ~ 2e-5 against eps = 1e-5 on the std
        return 0.7 + 2e-5 * z
    if regime == "offset":
        return 50.0 + 0.5 * z
    if regime == "const":
        return torch.full(shape, LN_CONST)
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def ln_input(regime, M, C, seed=0):
    """fp32 [M, C]; `mixed`: pixel i in regime LN_MIXED[i % 5]"""
    g = _gen(3000 + seed)
    if regime != "mixed":
        return _ln_fill(regime, (M, C), g)
    out = torch.empty(M, C)
    for j, r in enumerate(LN_MIXED):
        rows = out[j::len(LN_MIXED)]
        rows.copy_(_ln_fill(r, tuple(rows.shape), g))
    return out


@functools.lru_cache(maxsize=None)
def ln_params(C, seed=0):
    return 1 + 0.2 * rnd(C, seed=3100 + seed), 0.2 * rnd(C, seed=3101 + seed)


def chan_layernorm(x, g, b, eps=LN_EPS, variant="ref"):
    """the reference's LayerNorm over channels: (x - mean) / (sqrt(var) + eps) * g + b with the two-pass biased variance.
    variant: 'eps_inside' 1 / sqrt(var + eps); 'onepass' var = E[x^2] - mean^2 -- the wrong forms."""
    mean = x.mean(dim=-1, keepdim=True)
    if variant == "onepass":
        var = ((x * x).mean(dim=-1, keepdim=True) - mean * mean).clamp_min(0)
    else:
        var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    r = 1.0 / (var + eps).sqrt() if variant == "eps_inside" else 1.0 / (var.sqrt() + eps)
    return (x - mean) * r * g + b


def ln_grads(x, g, b, dy, eps=LN_EPS):
    """(dx, dg, db) of chan_layernorm in closed form, in the precision of its inputs.  Autograd gives the same numbers (the CPU test
    checks it) except on a constant pixel, where d sqrt(var) is 0 * inf: there the closed form has its limit, dx = (gy - mean gy) / eps."""
    mean = x.mean(dim=-1, keepdim=True)
    xc = x - mean
    std = (xc * xc).mean(dim=-1, keepdim=True).sqrt()
    r = 1.0 / (std + eps)
    gy = dy * g
    unit = torch.where(std > 0, xc / std.clamp_min(1e-300 if x.dtype == torch.float64 else 1e-37), torch.zeros_like(xc))
    dx = r * (gy - gy.mean(dim=-1, keepdim=True)) - (r * r) * unit * (gy * xc).mean(dim=-1, keepdim=True)
    return dx, (dy * xc * r).sum(dim=0), dy.sum(dim=0)


def ln_grads_autograd(x, g, b, dy):
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, g, b)]
    return torch.autograd.grad(chan_layernorm(*leaves), leaves, dy)


def ln_linear(x, g, b, w, eps=LN_EPS):
    """W LayerNorm(x): x [M, C], w [N, C] -> [M, N]"""
    return chan_layernorm(x, g, b, eps) @ w.t()


def ln_linear_folded(x, g, b, w, eps=LN_EPS):
    """the same in the form the to_qkv kernels use: r (W o g) x - r mean (W g) + W b.  At |mean| >> std its first two terms cancel;
    that loss is the form's own, so the kernels that use it are held to this restatement's e32."""
    mean = x.mean(dim=-1, keepdim=True)
    r = 1.0 / (((x - mean) ** 2).mean(dim=-1, keepdim=True).sqrt() + eps)
    wg = w * g
    return r * (x @ wg.t()) - (r * mean) * wg.sum(dim=1) + w @ b


LN_SHAPES = [(90, 32), (90, 256), (90, 24), (90, 200), (2048, 128)]
E32_LN = {"plain": 1.8e-7, "tinystd": 5.6e-5, "std~eps": 2.3e-3, "offset": 6.3e-6, "mixed": 2.0e-3}
E32_LN_BWD = {"plain": (1.7e-7, 3.0e-7, 2.0e-7), "tinystd": (4.1e-5, 5.2e-5, 2.0e-7), "std~eps": (1.7e-3, 2.5e-3, 2.0e-7),
              "offset": (4.8e-6, 8.4e-6, 2.0e-7), "mixed": (2.8e-4, 1.1e-3, 2.0e-7), "const": (1.5e-7, 0.0, 2.0e-7)}
# e32 of ln_linear_folded against ln_linear in fp64 at (2048, 128) -> 384
# (on a constant pixel r = 1 / eps multiplies the rounding of (W o g) x - mean (W g): the form keeps no digit there)
E32_LN_FOLDED = {"plain": 7.0e-7, "tinystd": 3.8e-4, "std~eps": 2.1e-2, "offset": 5.5e-5, "mixed": 2.0e-2, "const": 1.7e-1}


def ln_e32(regime, shape):
    x = ln_input(regime, *shape)
    g, b = ln_params(shape[1])
    return err(chan_layernorm(x, g, b), chan_layernorm(*d(x, g, b)))


@functools.lru_cache(maxsize=None)
def ln_dy(M, C):
    return rnd(M, C, seed=3200)


def ln_bwd_e32(regime, shape):
    x = ln_input(regime, *shape)
    g, b = ln_params(shape[1])
    return tuple(err(a, r) for a, r in zip(ln_grads(x, g, b, ln_dy(*shape)), ln_grads(*d(x, g, b, ln_dy(*shape)))))


@functools.lru_cache(maxsize=None)
def ln_weight(N, C, seed=0):
    return rnd(N, C, seed=3300 + seed, scale=C ** -0.5)


def ln_folded_e32(regime, shape=(2048, 128), N=384):
    x = ln_input(regime, *shape)
    g, b = ln_params(shape[1])
    w = ln_weight(N, shape[1])
    return err(ln_linear_folded(x, g, b, w), ln_linear(*d(x, g, b, w)))


# ------------------------------------------------------------------ linear attention
HEADS, DH = 4, 32
HC = HEADS * DH
K_REGIMES = ["plain", "k+85", "k-110", "k-equal", "dominant", "kx20"]
# through the weights of the from-x kernels: a shift of W_k ln_b, a scale of W_k, W_k = 0 (every k logit equal, to 0)
K_W_REGIMES = ["plain", "k+85", "k-110", "k-equal", "kx20"]


@functools.lru_cache(maxsize=None)
def qkv_input(regime, B, H, W, seed=0):
    """fp32 [B, 3 * 128, H, W] (q, k, v thirds, 4 heads of 32 channels), 1.5 randn with the k third moved into the regime"""
    t = rnd(B, 3 * HC, H, W, seed=4000 + seed, scale=1.5)
    k = t[:, HC:2 * HC]
    if regime == "k+85":               # exp overflows without the max
        k += 85.0
    elif regime == "k-110":            # every exp underflows to 0 without the max
        k -= 110.0
    elif regime == "k-equal":
        k.fill_(0.25)
    elif regime == "dominant":         # softmax ~ one-hot, and a pixel that vanishes
        k[:, :, H // 2, W // 2] += 60.0
        k[:, :, 0, 0] -= 80.0
    elif regime == "kx20":
        k *= 20.0
    elif regime != "plain":
        raise ValueError(regime)
    return t


def linattn(qkv, variant="ref"):
    """LinearAttention's core: softmax of k over the pixels, ctx = k v^T, out = ctx^T q.  qkv [B, 384, H, W] -> (out [B, 128, H, W],
    ctx [B, 4, 32, 32]).  variant 'nomax': exp(k) / sum exp(k) without the maximum -- the wrong form."""
    B, _, H, W = qkv.shape
    q, k, v = qkv.reshape(B, 3, HEADS, DH, H * W).unbind(1)
    if variant == "nomax":
        e = k.exp()
        ks = e / e.sum(dim=-1, keepdim=True)
    else:
        ks = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", ks, v)
    return torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, HC, H, W), ctx


def linattn_grad(qkv, dout):
    leaf = qkv.detach().clone().requires_grad_(True)
    return torch.autograd.grad(linattn(leaf)[0], leaf, dout)[0]


@functools.lru_cache(maxsize=None)
def attn_weights(regime, C, seed=0):
    """(w_qkv [384, C], ln_g, ln_b) with the k regime written into the k rows: the shift is the multiple of ln_b / |ln_b|^2 that makes
    W_k ln_b equal to it (the rows also pick up that multiple of ln_b . (xn o g), so the logits spread by tens as well)"""
    w = rnd(3 * HC, C, seed=4100 + seed, scale=C ** -0.5)
    g, b = ln_params(C, seed=7)
    wk = w[HC:2 * HC]
    if regime in ("k+85", "k-110"):
        s = 85.0 if regime == "k+85" else -110.0
        wk += (s - wk @ b)[:, None] * (b / (b * b).sum())[None, :]
    elif regime == "k-equal":
        wk.zero_()
    elif regime == "kx20":
        wk *= 20.0
    elif regime != "plain":
        raise ValueError(regime)
    return w, g, b


def attn_from_x(x, w, g, b, folded=False, variant="ref"):
    """PreNorm(LinearAttention) up to to_out: x [B, C, H, W] -> (out, ctx); folded: to_qkv in the kernels' form"""
    B, C, H, W = x.shape
    rows = x.permute(0, 2, 3, 1).reshape(-1, C)
    qkv = ln_linear_folded(rows, g, b, w) if folded else ln_linear(rows, g, b, w)
    return linattn(qkv.reshape(B, H, W, 3 * HC).permute(0, 3, 1, 2), variant)


@functools.lru_cache(maxsize=None)
def attn_x(xreg, B, C, H, W, seed=0):
    return ln_input(xreg, B * H * W, C, seed=50 + seed).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


QKV_SHAPES = [(2, 4, 4), (1, 10, 13), (1, 16, 17)]
# e32 of linattn (out, ctx) and of its gradient: torch's fp32 softmax subtracts the maximum, so every k regime costs the same
E32_ATTN = 6.0e-7
E32_ATTN_BWD = 8.2e-7
# the (k regime, x regime) pairs the from-x kernels run: every k regime on plain x, every x regime on plain k
FROM_X_CASES = [(k, "plain") for k in K_W_REGIMES] + [("plain", xr) for xr in LN_X_REGIMES[1:]]
FROM_X_SHAPES = [(2, 64, 2, 2), (3, 128, 8, 8), (2, 32, 8, 8), (2, 128, 16, 16), (2, 128, 32, 32), (3, 256, 4, 4), (3, 256, 8, 8)]
# e32 (out, ctx) of the folded fp32 form against the plain form in fp64, maximum over FROM_X_SHAPES
E32_FROM_X = {("plain", "plain"): (7.0e-7, 9.5e-7), ("k+85", "plain"): (1.1e-5, 2.1e-5), ("k-110", "plain"): (9.2e-6, 2.2e-5),
              ("k-equal", "plain"): (6.0e-7, 4.7e-7), ("kx20", "plain"): (6.6e-6, 1.3e-5), ("plain", "tinystd"): (5.9e-4, 5.1e-4),
              ("plain", "std~eps"): (1.9e-2, 1.8e-2), ("plain", "offset"): (8.6e-5, 7.2e-5)}


def from_x_e32(kreg, xreg, shape, folded=True):
    B, C, H, W = shape
    x = attn_x(xreg, B, C, H, W)
    w, g, b = attn_weights(kreg, C)
    got = attn_from_x(x, w, g, b, folded=folded)
    ref = attn_from_x(*d(x, w, g, b))
    return err(got[0], ref[0]), err(got[1], ref[1])


@functools.lru_cache(maxsize=None)
def attn_out_proj(C=HC):
    return rnd(C, HC, seed=4200, scale=HC ** -0.5), rnd(C, seed=4201, scale=0.1)


def attn_block(x, w, g, b, w_out, b_out, folded=False):
    """Residual(PreNorm(LinearAttention)): to_out of attn_from_x's output, plus x"""
    out, _ = attn_from_x(x, w, g, b, folded=folded)
    return torch.einsum("bchw,nc->bnhw", out, w_out) + b_out.view(1, -1, 1, 1) + x


BLOCK_SHAPE = (2, 128, 32, 32)
# e32 of attn_block with the folded to_qkv at BLOCK_SHAPE (the residual x raises max|ref|, at `offset` to 50)
E32_ATTN_BLOCK = {("plain", "plain"): 3.9e-7, ("k+85", "plain"): 1.2e-5, ("k-110", "plain"): 3.4e-6, ("k-equal", "plain"): 3.6e-7,
                  ("kx20", "plain"): 3.8e-6, ("plain", "tinystd"): 3.8e-4, ("plain", "std~eps"): 1.4e-2, ("plain", "offset"): 7.5e-6}


def attn_block_e32(kreg, xreg):
    B, C, H, W = BLOCK_SHAPE
    x = attn_x(xreg, B, C, H, W)
    w, g, b = attn_weights(kreg, C)
    wo, bo = attn_out_proj(C)
    return err(attn_block(x, w, g, b, wo, bo, folded=True), attn_block(*d(x, w, g, b, wo, bo)))


# ------------------------------------------------------------------ Adam, gradient clipping, activation gradients
ADAM_N = 4099                          # not a multiple of 256 or of 4
ADAM_LR = 2e-4
ADAM_REGIMES = ["g0", "g1e-9", "g1e-8", "plain"]
ADAM_STEPS = [1, 2, 1000]              # bias corrections near 0 and near 1
ADAM_G_SCALE = {"g0": 0.0, "g1e-9": 1e-9, "g1e-8": 1e-8, "plain": 3.0}


@functools.lru_cache(maxsize=None)
def adam_state(regime):
    """(p, g, m, v): parameters ~ 1e-3 (so that an update of ~ lr is not lost in p's own rounding), moments as they stand after many
    steps on gradients of the regime's scale"""
    s = ADAM_G_SCALE[regime]
    p = rnd(ADAM_N, seed=5000, scale=1e-3)
    g = rnd(ADAM_N, seed=5001, scale=s)
    m = rnd(ADAM_N, seed=5002, scale=0.5 * s)
    v = (rnd(ADAM_N, seed=5003, scale=s) ** 2) * 0.7
    return p, g, m, v


def adam_step(p, g, m, v, step, lr=ADAM_LR, variant="ref"):
    """oracle.train_ref.adam_step; variant 'eps_inside': denom = sqrt(v / bc2 + eps) -- the wrong form"""
    if variant == "ref":
        return TR.adam_step(p, g, m, v, step, lr)
    b1, b2 = TR.ADAM_BETAS
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    denom = (v / (1 - b2 ** step) + TR.ADAM_EPS).sqrt()
    return p - (lr / (1 - b1 ** step)) * m / denom, m, v


def adam_update_err(p_new, p_old, ref_new):
    """relative error of the update p_new - p_old against the reference's: the one quantity a slip of eps changes"""
    return err(p_new.double() - p_old.double(), ref_new.double() - p_old.double())


ADAM_BAR = 1e-5                        # the bar test_optimizer_kernels_match_oracle holds m and v to
# e32 of the update over ADAM_STEPS (g0 has no update: bit-identity is asserted instead)
E32_ADAM = {"g1e-9": 4.7e-6, "g1e-8": 7.9e-7, "plain": 2.1e-7}


def adam_e32(regime, step):
    p, g, m, v = adam_state(regime)
    got = adam_step(p, g, m, v, step)[0]
    return adam_update_err(got, p, adam_step(*d(p, g, m, v), step)[0])


def act_grid():
    """the grid of test_mish_matches_torch and the points where exp, softplus and tanh change regime"""
    return torch.cat([torch.linspace(-30, 30, 4097), torch.tensor([-100.0, 100.0, 0.0, 20.0, -20.0, -88.0, 89.0])])


def act_grads():
    """fp64 autograd of mish and tanh on the grid"""
    x = act_grid().double().requires_grad_(True)
    gm, = torch.autograd.grad(torch.nn.functional.mish(x).sum(), x)
    gt, = torch.autograd.grad(torch.tanh(x).sum(), x)
    return gm.detach(), gt.detach()


# max |fp32 autograd - fp64 autograd| of mish and tanh on the grid (absolute: the gradients are O(1))
E32_ACT_ABS = (1.1e-6, 7.0e-8)              # mish, tanh
