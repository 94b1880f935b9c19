"""Every kernel carries a NaN or an Inf in its data where the reference carries it, and no further: not into another image.

ONE check runs over a table of cases.  A case builds seeded inputs once, runs its op on them, then again with ONE element of one
input replaced by NaN, +Inf or -Inf (tests/nonfinite_ref.py: plant), always in the middle image of a batch of three or more, and
applies the rule of its family to the outputs against a reference of the same op on the same planted input -- the oracle or a
torch-CPU restatement, in fp64 where the restatement allows it, never the kernel:

  exact / exact_kinds / within(wino_allowed)   the set (the classes) of the non-finite output elements, see nonfinite_ref.py
  isolated                                     every other image is bit-identical to the clean run, always
  bitwise_outside (GroupNorm, LayerNorm)       so is every element of the planted image outside the reference's set: a group next
                                               to the planted group stays finite and keeps its bits

Planted positions: a map corner in the last channel of the first 32-channel chunk, the image's last pixel in its last channel (a
channel of the second source where the op concatenates two), and a pixel in the middle; the three values rotate over them.  A
masked read of a neighbour image (a halo row multiplied by 0, a tile of several images summed under a mask) is invisible on finite
data and shows here, because 0 * NaN and 0 * Inf are NaN.  Shapes come from the families' own case tables (test_buffer_contents_gpu.py,
test_kernels_gpu.py, test_step_edges_gpu.py): the smallest at which a workgroup's tile holds more than one image or the planted
pixel's neighbourhood crosses a tile edge; references of per-image ops are evaluated on the planted image alone.

No wait and no address depends on a data value.  Every wait in the library is cl_wait_ge (csrc/cluster_sync.h): it compares an
unsigned arrival counter, read with an atomic load, with `want`, and `want` is a launch parameter at every site -- the tiles per
image (the in-launch GroupNorm of conv_wino.hip, conv_wino2_kernel.inc and conv_first.hip), splits - 1 (the k-split pair counters of
conv_wino2_kernel.inc), 8 * the number of signalling ops so far (chain_wait in level_chain.hip), the constant 2 (the attention split
in attention.hip).  Its bound is wall time.  The records that travel through an exchange ({mean, M2}, partial tiles, softmax
partials) are moved as bit patterns (__float_as_uint) and enter arithmetic only.  No kernel of the table converts a float of its
data to an integer, an index or a loop bound: indices come from the launch geometry, the integer inputs (t, perm) and the
counters.  So a non-finite value cannot stall a wait or move an address; ops.cluster_timeouts() is asserted unchanged by every case
that runs an in-launch exchange.

Which kernel a case takes is asserted with the library's queries where one exists (ddk_conv_splits, ddk_conv_wino_splits,
ddk_convT_wino_splits, ddk_conv_gn_partials, the *_ok and workspace queries).  The halo, 32 -> 32, conv1x1_sm and conv1x1_stream
kernels have no query: conv_forward chooses them by shape alone (choose_halo, choose_c32, conv1x1_sm_ok, conv1x1_stream_ok in csrc/),
and their cases use shapes of test_kernels_gpu.py's and test_buffer_contents_gpu.py's tables for those kernels.

What fails here when it is written with fminf / fmaxf, which return the other operand for a NaN: the clamp of the reverse step
(fminf(fmaxf(x0, -1), 1) is -1 for a NaN x0: a NaN in eps_hat leaves a finite sample), the floor under the VLB's logarithms, the
per-image minimum / maximum of fix_samples, and the clip coefficient of grad_norm_clip (fminf(1, NaN) = 1: one NaN gradient element
clips nothing and spoils one weight where clip_grad_norm_ spoils all).  And mish_grad_f must not return a constant 1 for u = +Inf,
where torch's Mish backward gives NaN (x * 0)."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import nonfinite_ref as NF
import regimes_ref as RG
from helpers import ddpm_cfg, rel_err, to_nchw, to_nhwc
from oracle import diffusion_ref as D
from oracle import train_ref as TR
from oracle import unet_ref as U
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nonzero(w):
    """w with an exact zero (randn gives one now and then) replaced, before anything is packed from it: 0 * Inf is NaN, and the
    conv cases state that one Inf gives Infs with the weights' signs"""
    w[w == 0] = 1e-3
    return w


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


@pytest.fixture(scope="module")
def ops():
    from ddk import lib
    from ddk import ops as o
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


class Case:
    """inputs: name -> CPU tensor (batch first).  run(device inputs) -> tuple of device tensors; ref(CPU fp32 inputs, image) -> tuple
    of CPU tensors of the same shapes (None: that output is not compared with a reference).  plants: (input, index, value).
    rule: 'exact' | 'exact_kinds' | 'within'; allowed(plant) -> tuple of boolean masks for 'within'.  batched[i]: output i has the
    batch as its first axis.  check(): called after every run (counters)."""

    def __init__(self, inputs, run, ref, plants, rule, image, allowed=None, batched=None, bitwise_outside=False, check=None):
        self.inputs, self.run, self.ref, self.plants, self.rule, self.image = inputs, run, ref, plants, rule, image
        self.allowed, self.batched, self.bitwise_outside, self.check = allowed, batched, bitwise_outside, check


CASES = {}


def case(name):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return reg


def spots(shape, image):
    """the planted elements of an NHWC input: (corner, channel 31 or the last below it), (last pixel, last channel), (middle, 0), and
    the last pixel once more with a NaN"""
    _, H, W, C = shape
    return [((image, 0, 0, min(31, C - 1)), NF.NAN), ((image, H - 1, W - 1, C - 1), NF.PINF), ((image, H // 2, W // 2, 0), NF.NINF),
            ((image, H - 1, W - 1, C - 1), NF.NAN)]


def plants_for(inputs, image, names=("x",)):
    """corner / last pixel / middle on the first input; the last pixel, last channel on each further input (a second source)"""
    out = [(names[0], w, v) for w, v in spots(inputs[names[0]].shape, image)]
    for n in names[1:]:
        sp = spots(inputs[n].shape, image)
        out += [(n, sp[3][0], NF.NAN), (n, sp[0][0], NF.PINF)]
    return out


def embed(res, B, image):
    """a per-image result [1, ...] as image `image` of a zero batch of B"""
    out = torch.zeros((B, *res.shape[1:]), dtype=res.dtype)
    out[image] = res[0]
    return out


def d64(t):
    return None if t is None else t.double()


def nchw1(inp, name, image):
    """image `image` of NHWC input `name` as a [1, C, H, W] fp64 tensor"""
    return to_nchw(inp[name][image:image + 1]).double()


def cat_src(inp, image):
    x = nchw1(inp, "x", image)
    return torch.cat([x, nchw1(inp, "x2", image)], dim=1) if "x2" in inp else x


# ================================================================== convs: im2col, 1x1, transpose, halo, c32, stream, small-N
def _conv_case(kind, B, H, W, c0, c1, N, what="", wino=False, image=None, resid=False, seed=1):
    def build(ops):
        lib = ops.L.load()
        cin = c0 + c1
        k = {"s1": 3, "s2": 3, "1x1": 1, "T": 4}[kind]
        img = B // 2 if image is None else image
        x = to_nhwc(rnd(B, cin, H, W, seed=seed))
        bias = rnd(N, seed=seed + 2, scale=0.1)
        if kind == "T":
            w = nonzero(rnd(cin, N, 4, 4, seed=seed + 1, scale=(cin * 4) ** -0.5))
            wp, code = ops.pack_convT_weight(w.to(DEV)), ops.CONVT4X4_S2
            wu = ops.pack_convT_weight_wino(w.to(DEV)) if wino else None
            ho, wo = 2 * H, 2 * W
        else:
            w = nonzero(rnd(N, cin, k, k, seed=seed + 1, scale=(cin * k * k) ** -0.5))
            wp = ops.pack_conv_weight(w.to(DEV))
            code = {"s1": ops.CONV3X3_S1, "s2": ops.CONV3X3_S2, "1x1": ops.CONV1X1}[kind]
            wu = ops.pack_conv_weight_wino(w.to(DEV)) if wino else None
            ho, wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if kind == "s2" else (H, W)
        # which kernel: the library's own queries
        if wino:
            splits = (lib.ddk_convT_wino_splits if kind == "T" else lib.ddk_conv_wino_splits)(B, H, W, cin, N)
            assert splits >= 1, "the case is meant to run on the Winograd kernel"
        else:
            splits = lib.ddk_conv_splits(code, B, H, W, cin, N)
            assert splits >= 1
        if what == "split":
            assert splits > 1, "the case is meant to split k"
        inputs = {"x": x[..., :c0].contiguous()}
        if c1:
            inputs["x2"] = x[..., c0:].contiguous()
        if resid:
            inputs["resid"] = rnd(B, ho, wo, N, seed=seed + 3)
        bd = bias.to(DEV)

        def run(inp):
            return (ops.conv(code, inp["x"], wp, bd, x2=inp.get("x2"), resid=inp.get("resid"), w_wino=wu),)

        def ref(inp):
            xi = cat_src(inp, img)
            if kind == "T":
                y = F.conv_transpose2d(xi, w.double(), bias.double(), stride=2, padding=1)
            else:
                y = F.conv2d(xi, w.double(), bias.double(), stride=2 if kind == "s2" else 1, padding=k // 2)
            y = to_nhwc(y)
            if resid:
                y = y + inp["resid"][img:img + 1].double()
            return (embed(y, B, img),)

        names = ("x", "x2") if c1 else ("x",)
        plants = plants_for(inputs, img, names)
        if resid:
            plants.append(("resid", (img, ho - 1, wo - 1, N - 1), NF.NAN))
        if not wino:
            return Case(inputs, run, ref, plants, "exact_kinds", img)

        def allowed(plant):
            name, where, _ = plant
            if name == "resid":
                m = torch.zeros((B, ho, wo, N), dtype=torch.bool)
                m[where] = True
                return (m,)
            return (NF.wino_allowed((B, ho, wo, N), where, tile=2, patch=3 if kind == "T" else 4, transpose=kind == "T"),)
        return Case(inputs, run, ref, plants, "within", img, allowed=allowed)
    return build


IM2COL_CASES = [  # kind, B, H, W, c0, c1, N, what
    ("s1", 3, 8, 8, 32, 0, 64, ""),              # two images in a 128-row tile of the im2col GEMM
    ("s1", 3, 8, 8, 64, 0, 64, "split"),         # split-K + reduce
    ("s1", 3, 5, 7, 32, 0, 32, ""),              # ragged M, odd map
    ("s1", 3, 4, 4, 32, 32, 64, ""),             # dual source, eight images in a tile
    ("s2", 3, 7, 9, 32, 0, 32, ""),              # stride 2, odd sizes
    ("s2", 3, 8, 8, 64, 0, 64, ""),
    ("1x1", 3, 4, 4, 256, 256, 256, "split"),    # dual source, split-K
    ("1x1", 3, 5, 7, 64, 0, 32, ""),
    ("T", 3, 4, 4, 64, 0, 64, ""),               # 4x4 stride-2 transpose, direct
    ("s1", 69, 8, 8, 256, 0, 384, "split"),      # conv3x3_halo_kernel, odd batch: two images per tile, the last tile half empty
    ("s1", 256, 8, 8, 32, 0, 32, ""),            # conv3x3_c32: two images per tile, the smallest grid the kernel takes (128 tiles)
    ("1x1", 8, 8, 8, 256, 0, 128, ""),           # conv1x1_sm
    ("1x1", 16, 32, 32, 64, 0, 32, ""),          # conv1x1_stream (M = 16384, its minimum)
]
for _c in IM2COL_CASES:
    CASES[f"conv-{'-'.join(map(str, _c[:7]))}"] = _conv_case(*_c)
CASES["conv-s1-3-8-8-64-0-64-resid"] = _conv_case("s1", 3, 8, 8, 64, 0, 64, "split", resid=True)
CASES["conv-1x1-8-8-8-256-0-128-resid"] = _conv_case("1x1", 8, 8, 8, 256, 0, 128, resid=True)
CASES["conv-s1-69-8-8-256-0-384-odd_image"] = _conv_case("s1", 69, 8, 8, 256, 0, 384, "split", image=35)      # the tile's second image
CASES["conv-s1-256-8-8-32-0-32-odd_image"] = _conv_case("s1", 256, 8, 8, 32, 0, 32, image=129)

WINO_CASES = [(3, 4, 4, 64, 0, 64, "split"), (32, 4, 4, 256, 0, 256, "split"), (3, 6, 10, 96, 0, 128, ""), (3, 2, 2, 32, 0, 64, ""),
              (3, 8, 8, 32, 32, 64, "")]
for _c in WINO_CASES:
    CASES[f"wino-{'-'.join(map(str, _c[:6]))}"] = _conv_case("s1", *_c, wino=True, seed=61)
CASES["wino-32-4-4-256-0-256-odd_image"] = _conv_case("s1", 32, 4, 4, 256, 0, 256, "split", wino=True, image=17, seed=61)
CASES["wino-3-4-4-64-0-64-resid"] = _conv_case("s1", 3, 4, 4, 64, 0, 64, "split", wino=True, resid=True, seed=61)
for _c in [(3, 6, 10, 96, 0, 128, ""), (3, 2, 2, 32, 0, 128, ""), (32, 4, 4, 256, 0, 256, "")]:
    CASES[f"convT_wino-{'-'.join(map(str, _c[:6]))}"] = _conv_case("T", *_c, wino=True, seed=11)


@case("conv1x1_small_n")
def _(ops):
    B, H, W = 3, 9, 7
    shapes = ((128, 8), (128, 3), (32, 1), (256, 5))
    inputs = {f"x{i}": to_nhwc(rnd(B, C, H, W, seed=80 + i)) for i, (C, n) in enumerate(shapes)}
    ws = [(rnd(n, C, 1, 1, seed=81 + i, scale=C ** -0.5), rnd(n, seed=82 + i)) for i, (C, n) in enumerate(shapes)]
    wd = [(w.to(DEV), b.to(DEV)) for w, b in ws]
    run = lambda inp: tuple(ops.conv1x1_small_n(inp[f"x{i}"], *wd[i]) for i in range(4))
    ref = lambda inp: tuple(to_nhwc(F.conv2d(to_nchw(inp[f"x{i}"]).double(), ws[i][0].double(), ws[i][1].double())) for i in range(4))
    plants = [(f"x{i}", w, v) for i in range(4) for w, v in spots(inputs[f"x{i}"].shape, 1)[:3]]
    return Case(inputs, run, ref, plants, "exact_kinds", 1)


def _ws_case(B, H, W, N, use_bias, use_resid, use_ln):
    def build(ops):
        K = 128
        assert ops.L.load().ddk_conv1x1_ws_ok(B * H * W, K, N)
        inputs = {"x": to_nhwc(rnd(B, K, H, W, seed=11) * 1.5 + 0.4)}
        w2 = rnd(N, K, seed=12, scale=K ** -0.5)
        g, be = 1 + 0.2 * rnd(K, seed=15), 0.1 * rnd(K, seed=16)
        ln = (dev(w2 @ g), dev(w2 @ be)) if use_ln else None
        wd = dev(w2 * g.view(1, K) if use_ln else w2)
        b = rnd(N, seed=13) if use_bias else None
        if use_resid:
            inputs["resid"] = to_nhwc(rnd(B, N, H, W, seed=14))
        bd = dev(b)
        img = B // 2
        run = lambda inp: (ops.conv1x1_ws(inp["x"], wd, bd, inp.get("resid"), ln),)

        def ref(inp):
            x = inp["x"][img:img + 1].double()
            if use_ln:
                x = RG.chan_layernorm(x, g.double(), be.double())
            y = x @ w2.double().t()
            if use_bias:
                y = y + b.double()
            if use_resid:
                y = y + inp["resid"][img:img + 1].double()
            return (embed(y, B, img),)
        plants = plants_for(inputs, img)
        if use_resid:
            plants.append(("resid", (img, 0, 0, N - 1), NF.NINF))
        # behind a LayerNorm the pixel's channels are all NaN, whatever was planted: sets, not kinds
        return Case(inputs, run, ref, plants, "exact" if use_ln else "exact_kinds", img)
    return build


CASES["conv1x1_ws-3-32-32-128-ln-resid"] = _ws_case(3, 32, 32, 128, False, True, True)
CASES["conv1x1_ws-5-16-32-128-plain"] = _ws_case(5, 16, 32, 128, True, False, False)


# ================================================================== first conv, GroupNorm partials, final tail
def gn_mish64(y, gamma, beta, temb=None, addend=None):
    """Block's GroupNorm -> Mish (+ shift) (+ residual), NCHW fp64"""
    y = F.group_norm(y, 8, gamma.double(), beta.double(), 1e-5)
    y = y * torch.tanh(F.softplus(y))
    if temb is not None:
        y = y + temb.double()[:, :, None, None]
    return y if addend is None else y + addend.double()


def _gn_params(N, B, seed):
    return 1 + rnd(N, seed=seed, scale=0.2), rnd(N, seed=seed + 1, scale=0.2), rnd(B, N, seed=seed + 2)


def _first_case(B, H, W, cin, N, fused, res1x1=True):
    """conv_first plain and with partials; fused: + GroupNorm + Mish from the partials, and the res1x1 form (N <= 256, N / 4 a divisor
    of 256)"""
    def build(ops):
        assert ops.L.load().ddk_conv_first_ok(cin, N, H, W, 8)
        img = B // 2
        inputs = {"x": to_nhwc(rnd(B, cin, H, W, seed=1 + cin) + 0.3)}
        w, b = rnd(N, cin, 3, 3, seed=2 + cin, scale=(cin * 9) ** -0.5), rnd(N, seed=3)
        wf, bd = ops.pack_conv_weight_first(w.to(DEV)), b.to(DEV)
        gamma, beta, temb = _gn_params(N, B, 27)
        gd, bed, td = dev(gamma), dev(beta), dev(temb)
        wr, br = rnd(N, cin, 1, 1, seed=25, scale=cin ** -0.5), rnd(N, seed=26)
        wrd, brd = dev(wr), dev(br)

        def run(inp):
            raw, part, tiles = ops.conv_first(inp["x"], wf, bd, N)
            raw2, none, _ = ops.conv_first(inp["x"], wf, bd, N, partials=False)
            assert none is None and tiles == H * W // 128
            if not fused:
                return raw, raw2
            a = ops.groupnorm_mish_from_partials(raw, part, tiles, gd, bed, temb=td)
            if not res1x1:
                return raw, raw2, a
            return raw, raw2, a, ops.groupnorm_mish_from_partials_res1x1(raw, part, tiles, gd, bed, inp["x"], wrd, brd, temb=td)

        def ref(inp):
            xi = nchw1(inp, "x", img)
            y = F.conv2d(xi, w.double(), b.double(), padding=1)
            res = [embed(to_nhwc(y), B, img)] * 2
            if fused:
                a = gn_mish64(y, gamma, beta, temb[img:img + 1])
                res += [embed(to_nhwc(a), B, img), embed(to_nhwc(a + F.conv2d(xi, wr.double(), br.double())), B, img)]
            return tuple(res if res1x1 else res[:3])
        # raw: every product of the one Inf is an Inf with the weight's sign; behind the GroupNorm everything is NaN: sets there
        return Case(inputs, run, ref, plants_for(inputs, img), "exact", img)
    return build


CASES["conv_first-3-8-16-4-64"] = _first_case(3, 8, 16, 4, 64, False)
CASES["conv_first-3-16-24-5-160-gn"] = _first_case(3, 16, 24, 5, 160, True, res1x1=False)
CASES["conv_first-3-16-16-3-32-gn"] = _first_case(3, 16, 16, 3, 32, True)


def _step_tables():
    buf = D.schedule_buffers("linear", 1000)
    tb = {k: buf[v] for k, v in (("c_recip", "sqrt_recip_alphas_cumprod"), ("c_recipm1", "sqrt_recipm1_alphas_cumprod"),
                                 ("c1", "posterior_mean_coef1"), ("c2", "posterior_mean_coef2"))}
    tb["sigma"] = torch.exp(0.5 * buf["posterior_log_variance_clipped"])
    tb["sigma"][0] = 0.0                       # the t > 0 mask of ddpm.py:227 lives in the table
    return buf, tb, {k: v.to(DEV) for k, v in tb.items()}


def _final_tail_case(B, H, W, C, n_out):
    def build(ops):
        img = B // 2
        assert ops.L.load().ddk_conv_first_ok(8, C, H, W, 8)
        h_in = to_nhwc(rnd(B, 8, H, W, seed=31))
        w3, b3 = rnd(C, 8, 3, 3, seed=32, scale=(8 * 9) ** -0.5), rnd(C, seed=33)
        gamma, beta = 1 + 0.1 * rnd(C, seed=34), 0.1 * rnd(C, seed=35)
        wf, bf = rnd(n_out, C, 1, 1, seed=36, scale=C ** -0.5), rnd(n_out, seed=37)
        buf, tb, tbd = _step_tables()
        t = torch.tensor([0, 500, 999, 1] * 8)[:B]
        inputs = {"h": h_in, "x": rnd(B, H, W, n_out, seed=38, scale=1.5), "z": rnd(B, H, W, n_out, seed=39)}
        w3d, b3d, gd, bed, wfd, bfd, td = (dev(v) for v in (ops.pack_conv_weight_first(w3.to(DEV)), b3, gamma, beta, wf, bf, t))

        def run(inp):
            raw, part, tiles = ops.conv_first(inp["h"], w3d, b3d, C)
            eps = ops.final_tail(raw, part, tiles, gd, bed, wfd, bfd)
            xa = inp["x"].clone()
            eps2 = ops.final_tail(raw, part, tiles, gd, bed, wfd, bfd, x=xa, t=td, tables=tbd, noise=inp["z"])
            xb = inp["x"].clone()
            ops.final_tail(raw, part, tiles, gd, bed, wfd, bfd, x=xb, t=td, tables=tbd, seed=0x1234567887654321, stream_id=3, want_eps=False)
            return eps, eps2, xa, xb

        def ref(inp):
            a = gn_mish64(F.conv2d(nchw1(inp, "h", img), w3.double(), b3.double(), padding=1), gamma, beta)
            eps = F.conv2d(a, wf.double(), bf.double()).float()
            ti = t[img:img + 1]
            x = to_nchw(inp["x"][img:img + 1])
            xn = D.p_sample_update(buf, x, ti, eps, to_nchw(inp["z"][img:img + 1]))
            xp = D.p_sample_update(buf, x, ti, eps, torch.zeros_like(x))       # Philox draws are finite: the set does not depend on them
            e = embed(to_nhwc(eps), B, img)
            return e, e, embed(to_nhwc(xn), B, img), embed(to_nhwc(xp), B, img)
        plants = [("h", w, v) for w, v in spots(h_in.shape, img)[:3]] + [("x", (img, H - 1, W - 1, n_out - 1), NF.NAN), ("x", (img, 0, 0, 0), NF.PINF),
                                                                       ("z", (img, 1, 1, 0), NF.NAN)]
        # classes throughout: behind the GroupNorm every plant in h has become NaN, in the kernel's {mean, M2} merge (Inf - Inf) as in
        # the reference's x - mean; in x the Inf outlives the clamp through c2 * x and must come out an Inf of its sign
        return Case(inputs, run, ref, plants, "exact_kinds", img)
    return build


CASES["final_tail-3-16-16-32-3"] = _final_tail_case(3, 16, 16, 32, 3)
CASES["final_tail-3-16-8-128-4"] = _final_tail_case(3, 16, 8, 128, 4)


def _gn_partials_case(B, H, W, c0, c1, N):
    """Winograd conv that leaves GroupNorm partials: the raw output within the Winograd set, behind the GroupNorm the reference's"""
    def build(ops):
        cin = c0 + c1
        img = B // 2
        assert ops.L.load().ddk_conv_gn_partials(B, H, W, cin, N, 8) == H * W // 128
        x = to_nhwc(rnd(B, cin, H, W, seed=81))
        w, bias = rnd(N, cin, 3, 3, seed=82, scale=(cin * 9) ** -0.5), rnd(N, seed=83, scale=0.1)
        gamma, beta, temb = _gn_params(N, B, 84)
        inputs = {"x": x[..., :c0].contiguous(), "addend": rnd(B, H, W, N, seed=87)}
        if c1:
            inputs["x2"] = x[..., c0:].contiguous()
        wp, wu, bd, gd, bed, td = ops.pack_conv_weight(w.to(DEV)), ops.pack_conv_weight_wino(w.to(DEV)), dev(bias), dev(gamma), dev(beta), dev(temb)

        def run(inp):
            raw, part, np_ = ops.conv_with_gn_partials(inp["x"], wp, bd, wu, x2=inp.get("x2"))
            return raw, ops.groupnorm_mish_from_partials(raw, part, np_, gd, bed, temb=td, addend=inp["addend"])

        def ref(inp):
            y = F.conv2d(cat_src(inp, img), w.double(), bias.double(), padding=1)
            a = gn_mish64(y, gamma, beta, temb[img:img + 1], to_nchw(inp["addend"][img:img + 1]))
            return embed(to_nhwc(y), B, img), embed(to_nhwc(a), B, img)

        def allowed(plant):
            name, where, _ = plant
            whole = torch.zeros((B, H, W, N), dtype=torch.bool)
            if name == "addend":
                one = whole.clone()
                one[where] = True
                return whole, one
            whole[img] = True
            return NF.wino_allowed((B, H, W, N), where), whole
        plants = plants_for(inputs, img, ("x", "x2") if c1 else ("x",)) + [("addend", (img, H - 1, W - 1, N - 1), NF.NAN)]
        return Case(inputs, run, ref, plants, "within", img, allowed=allowed)
    return build


CASES["gn_partials-3-32-16-32-0-64"] = _gn_partials_case(3, 32, 16, 32, 0, 64)
CASES["gn_partials-32-16-16-32-32-256"] = _gn_partials_case(32, 16, 16, 32, 32, 256)       # (a small batch splits the channel chunks and leaves no partials)


def _cluster_case(B, H, W, c0, c1, N, split):
    def build(ops):
        lib = ops.L.load()
        cin = c0 + c1
        if lib.ddk_conv3x3_gn_mish_cluster_ok(B, H, W, cin, N, 8) <= 0:
            pytest.skip("shape / device not eligible for the in-launch GroupNorm")
        assert (lib.ddk_conv3x3_gn_mish_cluster_split_workspace_bytes(B, H, W, cin, N, 8) > 0) == split
        if split:
            assert lib.ddk_conv_wino_splits(B, H, W, cin, N) > 1
        img = B // 2
        x = to_nhwc(rnd(B, cin, H, W, seed=41))
        w, bias = rnd(N, cin, 3, 3, seed=42, scale=(cin * 9) ** -0.5), rnd(N, seed=43)
        gamma, beta, temb = _gn_params(N, B, 44)
        inputs = {"x": x[..., :c0].contiguous(), "addend": rnd(B, H, W, N, seed=47)}
        if c1:
            inputs["x2"] = x[..., c0:].contiguous()
        wu, bd, gd, bed, td = ops.pack_conv_weight_wino(w.to(DEV)), dev(bias), dev(gamma), dev(beta), dev(temb)
        before = ops.cluster_timeouts()
        run = lambda inp: (ops.conv3x3_gn_mish_cluster(inp["x"], wu, bd, gd, bed, x2=inp.get("x2"), temb=td, addend=inp["addend"]),)

        def ref(inp):
            y = F.conv2d(cat_src(inp, img), w.double(), bias.double(), padding=1)
            return (embed(to_nhwc(gn_mish64(y, gamma, beta, temb[img:img + 1], to_nchw(inp["addend"][img:img + 1]))), B, img),)

        def check():
            assert ops.cluster_timeouts() == before, "an in-launch exchange gave up"
        plants = plants_for(inputs, img, ("x", "x2") if c1 else ("x",))[:4] + [("addend", (img, 0, 0, N - 1), NF.NAN)]
        return Case(inputs, run, ref, plants, "exact", img, check=check)
    return build


CASES["gn_cluster-32-16-16-128-0-128-ksplit"] = _cluster_case(32, 16, 16, 128, 0, 128, True)
CASES["gn_cluster-16-32-32-128-0-128"] = _cluster_case(16, 32, 32, 128, 0, 128, False)
CASES["gn_cluster-64-16-16-64-64-128"] = _cluster_case(64, 16, 16, 64, 64, 128, False)


# ================================================================== one-launch Blocks
def _local_case(B, H, W, c0, c1, N, wino):
    def build(ops):
        lib = ops.L.load()
        cin = c0 + c1
        assert (lib.ddk_conv3x3_gn_mish_wino_ok if wino else lib.ddk_conv3x3_gn_mish_ok)(H, W, cin, c0, N, 8)
        img = B // 2
        x = to_nhwc(rnd(B, cin, H, W, seed=71))
        w, bias = rnd(N, cin, 3, 3, seed=72, scale=(cin * 9) ** -0.5), rnd(N, seed=73, scale=0.1)
        gamma, beta, temb = _gn_params(N, B, 74)
        inputs = {"x": x[..., :c0].contiguous(), "addend": rnd(B, H, W, N, seed=77)}
        if c1:
            inputs["x2"] = x[..., c0:].contiguous()
        wl = (ops.pack_conv_weight_wino_local if wino else ops.pack_conv_weight_local)(w.to(DEV))
        bd, gd, bed, td = dev(bias), dev(gamma), dev(beta), dev(temb)
        fn = ops.conv3x3_gn_mish_wino if wino else ops.conv3x3_gn_mish
        run = lambda inp: (fn(inp["x"], wl, bd, gd, bed, x2=inp.get("x2")), fn(inp["x"], wl, bd, gd, bed, temb=td, addend=inp["addend"], x2=inp.get("x2")))

        def ref(inp):
            y = F.conv2d(cat_src(inp, img), w.double(), bias.double(), padding=1)
            return (embed(to_nhwc(gn_mish64(y, gamma, beta)), B, img),
                    embed(to_nhwc(gn_mish64(y, gamma, beta, temb[img:img + 1], to_nchw(inp["addend"][img:img + 1]))), B, img))
        plants = plants_for(inputs, img, ("x", "x2") if c1 else ("x",)) + [("addend", (img, H - 1, W - 1, N - 1), NF.NAN), ("addend", (img, 0, 0, 0), NF.NINF)]
        return Case(inputs, run, ref, plants, "exact", img, bitwise_outside=True)
    return build


CASES["gn_local-3-8-2-32-0-64"] = _local_case(3, 8, 2, 32, 0, 64, False)
CASES["gn_local-3-2-8-64-32-64"] = _local_case(3, 2, 8, 64, 32, 64, False)
CASES["gn_local-5-4-4-256-0-256"] = _local_case(5, 4, 4, 256, 0, 256, False)
CASES["gn_wlocal-3-8-8-32-0-64"] = _local_case(3, 8, 8, 32, 0, 64, True)
CASES["gn_wlocal-3-32-2-32-32-64"] = _local_case(3, 32, 2, 32, 32, 64, True)


def _gn_slabs_case(B, H, S, SA):
    def build(ops):
        C = N = 256
        img = B // 2
        inputs = {"slabs": torch.stack([to_nhwc(rnd(B, C, H, H, seed=300 + k)) for k in range(S)], dim=1),         # [B, S, H, W, C]
                  "a_slabs": torch.stack([to_nhwc(rnd(B, N, H, H, seed=340 + k)) for k in range(SA)], dim=1)}
        sbias, abias, bias = rnd(C, seed=320, scale=0.3), rnd(N, seed=350, scale=0.3), rnd(N, seed=322, scale=0.1)
        w = rnd(N, C, 3, 3, seed=321, scale=(C * 9) ** -0.5)
        wp = (ops.pack_conv_weight_local if H == 4 else ops.pack_conv_weight_wino_local)(w.to(DEV))
        gamma, beta, temb = _gn_params(N, B, 323)
        sbd, abd, bd, gd, bed, td = (dev(v) for v in (sbias, abias, bias, gamma, beta, temb))

        def run(inp):
            sl, asl = inp["slabs"].transpose(0, 1).contiguous(), inp["a_slabs"].transpose(0, 1).contiguous()
            return (ops.conv3x3_gn_mish_slabs(sl, sbd, wp, bd, gd, bed, temb=td, addend_slabs=asl, addend_bias=abd),)

        def ref(inp):
            x = to_nchw(inp["slabs"][img:img + 1].double().sum(1) + sbias.double())
            add = to_nchw(inp["a_slabs"][img:img + 1].double().sum(1) + abias.double())
            y = F.conv2d(x, w.double(), bias.double(), padding=1)
            return (embed(to_nhwc(gn_mish64(y, gamma, beta, temb[img:img + 1], add)), B, img),)
        plants = [("slabs", (img, S - 1, 0, 0, 31), NF.NAN), ("slabs", (img, 0, H - 1, H - 1, C - 1), NF.PINF), ("slabs", (img, S - 1, H - 1, H - 1, C - 1), NF.NINF),
                  ("a_slabs", (img, SA - 1, H - 1, H - 1, N - 1), NF.NAN), ("a_slabs", (img, 0, 0, 0, 0), NF.PINF)]
        return Case(inputs, run, ref, plants, "exact", img, bitwise_outside=True)
    return build


CASES["gn_slabs-5-4-3-2"] = _gn_slabs_case(5, 4, 3, 2)
CASES["gn_slabs-3-8-2-4"] = _gn_slabs_case(3, 8, 2, 4)


# ================================================================== norms
def _gn_case(B, H, W, C, streamed=False):
    def build(ops):
        img = B // 2
        assert (ops.L.load().ddk_groupnorm_workspace_bytes(B, H * W, C, 8) > 0) == streamed
        inputs = {"x": to_nhwc(rnd(B, C, H, W, seed=30, scale=2.0) + 0.5), "addend": to_nhwc(rnd(B, C, H, W, seed=34))}
        gamma, beta, temb = _gn_params(C, B, 31)
        gd, bed, td = dev(gamma), dev(beta), dev(temb)
        run = lambda inp: (ops.groupnorm_mish(inp["x"], gd, bed), ops.groupnorm_mish(inp["x"], gd, bed, temb=td, addend=inp["addend"]))

        def ref(inp):
            x = nchw1(inp, "x", img)
            return (embed(to_nhwc(gn_mish64(x, gamma, beta)), B, img),
                    embed(to_nhwc(gn_mish64(x, gamma, beta, temb[img:img + 1], to_nchw(inp["addend"][img:img + 1]))), B, img))
        cpg = C // 8
        plants = [("x", (img, 0, 0, cpg - 1), NF.NAN), ("x", (img, H - 1, W - 1, C - 1), NF.PINF), ("x", (img, H // 2, W // 2, cpg), NF.NINF),
                  ("x", (img, H - 1, W - 1, 3 * cpg), NF.NAN), ("addend", (img, H - 1, W - 1, C - 1), NF.NAN)]
        return Case(inputs, run, ref, plants, "exact", img, bitwise_outside=True)
    return build


CASES["groupnorm_mish-3-5-7-64"] = _gn_case(3, 5, 7, 64)
CASES["groupnorm_mish-3-4-4-256"] = _gn_case(3, 4, 4, 256)
CASES["groupnorm_mish-3-100-90-64-streamed"] = _gn_case(3, 100, 90, 64, streamed=True)


@case("groupnorm_mish_generic-3-4-4-40")
def _(ops):
    B, H, W, C = 3, 4, 4, 40
    CP = ops.pad32(C)

    def pad(t):
        out = torch.zeros((*t.shape[:-1], CP))
        out[..., :C] = t
        return out
    inputs = {"x": pad(rnd(B, H, W, C, seed=1) * 1.3 + 0.2), "addend": pad(rnd(B, H, W, C, seed=2))}
    gamma, beta, temb = _gn_params(C, B, 4)
    gd, bed, td = dev(gamma), dev(beta), dev(temb)
    run = lambda inp: (ops.groupnorm_mish_generic_train(inp["x"], gd, bed, temb=td, addend=inp["addend"]),)

    def ref(inp):
        y = gn_mish64(to_nchw(inp["x"][..., :C]).double(), gamma, beta, temb, to_nchw(inp["addend"][..., :C]))
        return (pad(to_nhwc(y).float()),)
    plants = [("x", (1, 0, 0, 4), NF.NAN), ("x", (1, 3, 3, C - 1), NF.PINF), ("x", (1, 2, 2, 5), NF.NINF), ("addend", (1, 3, 3, C - 1), NF.NAN)]
    return Case(inputs, run, ref, plants, "exact", 1, bitwise_outside=True)


def _ln_case(C, generic=False):
    def build(ops):
        B, H, W = 3, 6, 5
        CP = ops.pad32(C) if generic else C
        x = torch.zeros(B, H, W, CP)
        x[..., :C] = rnd(B, H, W, C, seed=40, scale=3.0) + 1.0
        g, b = 1 + 0.1 * rnd(C, seed=41), 0.1 * rnd(C, seed=42)
        gd, bd = dev(g.view(1, C, 1, 1)), dev(b.view(1, C, 1, 1))
        fn = ops.chan_layernorm_generic if generic else ops.chan_layernorm
        run = lambda inp: (fn(inp["x"], gd, bd),)

        def ref(inp):
            out = torch.zeros(B, H, W, CP, dtype=torch.float64)
            out[..., :C] = RG.chan_layernorm(inp["x"][..., :C].double(), g.double(), b.double())
            return (out,)
        plants = [("x", (1, 0, 0, min(31, C - 1)), NF.NAN), ("x", (1, H - 1, W - 1, C - 1), NF.PINF), ("x", (1, 3, 2, 0), NF.NINF)]
        return Case({"x": x}, run, ref, plants, "exact", 1, bitwise_outside=True)
    return build


CASES["chan_layernorm-32"] = _ln_case(32)
CASES["chan_layernorm-512"] = _ln_case(512)
CASES["chan_layernorm_generic-40"] = _ln_case(40, generic=True)


# ================================================================== attention
def _linattn_case(B, H, W, fused_up_to=256):
    def build(ops):
        merged = H * W <= min(fused_up_to, 256)          # ops.linattn's own choice: context + apply in one launch
        if not merged:                                   # context over pixel splits + merge, then apply: the split count shows in the bytes
            nbytes = ops.L.load().ddk_linattn_context_workspace_bytes(B, H * W, 4)
            assert nbytes > 0 and nbytes % (B * 4) == 0, "the case is meant to split the pixels of the context"
        inputs = {"qkv": to_nhwc(rnd(B, 384, H, W, seed=60, scale=1.5))}
        run = lambda inp: ops.linattn(inp["qkv"], 4, fused_up_to=fused_up_to)

        def ref(inp):
            out, ctx = RG.linattn(nchw1(inp, "qkv", 1))
            return embed(to_nhwc(out), B, 1), embed(ctx, B, 1)
        # q (head 0), k (head 1, its last dimension), v (head 3, the last channel of qkv); a +Inf in k: exp(Inf - Inf)
        plants = [("qkv", (1, 0, 0, 31), NF.NAN), ("qkv", (1, H - 1, W - 1, 383), NF.PINF), ("qkv", (1, H // 2, W // 2, 128 + 63), NF.NAN),
                  ("qkv", (1, H - 1, W - 1, 128 + 32), NF.PINF), ("qkv", (1, 0, 0, 5), NF.NINF)]
        return Case(inputs, run, ref, plants, "exact", 1)
    return build


CASES["linattn-3-10-13-merged"] = _linattn_case(3, 10, 13)
CASES["linattn-3-15-17-context_apply"] = _linattn_case(3, 15, 17, fused_up_to=64)
CASES["linattn-3-32-32-pixel_split"] = _linattn_case(3, 32, 32)


def _attn_inputs(B, H, W, C):
    x = to_nhwc(rnd(B, C, H, W, seed=181) * 1.3 + 0.2)
    wq = rnd(384, C, seed=182, scale=C ** -0.5)
    return x, wq, 1 + 0.2 * rnd(C, seed=185), 0.1 * rnd(C, seed=186)


def _from_x_case(which, B, H, W, C):
    def build(ops):
        lib = ops.L.load()
        img = B // 2
        x, wq, g, be = _attn_inputs(B, H, W, C)
        wqd, gd, bed = dev(wq.view(384, C, 1, 1)), dev(g), dev(be)
        before = ops.cluster_timeouts()
        check = None
        if which == "small":
            run = lambda inp: ops.linattn_small_from_x(inp["x"], wqd, gd, bed)
        elif which == "split":
            if not lib.ddk_attention_split_ok(B, H * W, C, 4):
                pytest.skip("shape / device not eligible for the pixel-split attention launch")
            run = lambda inp: ops.attention_split_from_x(inp["x"], wqd, gd, bed)

            def check():
                assert ops.cluster_timeouts() == before, "the in-launch exchange gave up"
        elif which == "kv_context":
            assert lib.ddk_attention_kv_context_ok(B, H * W, C, 4)
            run = lambda inp: (ops.attention_kv_context(inp["x"], wqd, gd, bed),)
        else:
            wo, bo = rnd(128, 128, 1, 1, seed=83, scale=128 ** -0.5), rnd(128, seed=84, scale=0.1)
            wod, bod = dev(wo), dev(bo)
            run = lambda inp: (ops.attention_folded(inp["x"], wqd, gd, bed, wod, bod),)

        def ref(inp):
            xi = nchw1(inp, "x", img)
            if which == "folded":
                return (embed(to_nhwc(RG.attn_block(xi, wq.double(), g.double(), be.double(), wo.reshape(128, 128).double(), bo.double())), B, img),)
            out, ctx = RG.attn_from_x(xi, wq.double(), g.double(), be.double())
            return (embed(ctx, B, img),) if which == "kv_context" else (embed(to_nhwc(out), B, img), embed(ctx, B, img))
        return Case({"x": x}, run, ref, plants_for({"x": x}, img), "exact", img, check=check)
    return build


CASES["linattn_small_from_x-3-6-6-96"] = _from_x_case("small", 3, 6, 6, 96)
CASES["linattn_small_from_x-3-2-2-64"] = _from_x_case("small", 3, 2, 2, 64)
CASES["attention_split_from_x-3-8-8-32"] = _from_x_case("split", 3, 8, 8, 32)
CASES["attention_split_from_x-3-16-16-128"] = _from_x_case("split", 3, 16, 16, 128)
CASES["attention_kv_context-5-16-16"] = _from_x_case("kv_context", 5, 16, 16, 128)
CASES["attention_folded-3-32-32"] = _from_x_case("folded", 3, 32, 32, 128)


@pytest.mark.parametrize("H,W,fused_up_to", [(10, 13, 256), (15, 17, 64), (32, 32, 256)])
def test_linattn_minus_inf_in_k_is_a_zero_weight(ops, H, W, fused_up_to):
    """a -Inf in a k entry: its softmax weight is exp(-Inf) = 0, so the result is finite and equal to the reference at test_linattn's
    bar (test_kernels_gpu.py: 2e-5 on out and ctx) -- and the other images keep their bits"""
    qkv = to_nhwc(rnd(3, 384, H, W, seed=60, scale=1.5))
    clean = [t.cpu() for t in ops.linattn(dev(qkv), 4, fused_up_to=fused_up_to)]
    for where in ((1, 0, 0, 128 + 31), (1, H - 1, W - 1, 255)):
        p = NF.plant(qkv, where, NF.NINF)
        out, ctx = (t.cpu() for t in ops.linattn(dev(p), 4, fused_up_to=fused_up_to))
        r_out, r_ctx = RG.linattn(to_nchw(p).double())
        assert torch.isfinite(r_out).all() and torch.isfinite(out).all() and torch.isfinite(ctx).all()
        e_out, e_ctx = rel_err(to_nchw(out), r_out), rel_err(ctx, r_ctx)
        print(f"linattn -Inf in k at {where}: rel err out {e_out:.3e} ctx {e_ctx:.3e}")
        assert e_out < 2e-5 and e_ctx < 2e-5
        assert NF.isolated(out, clean[0], 1) and NF.isolated(ctx, clean[1], 1)


# ================================================================== the level chain (4x4), through test_level_chain_gpu.py's entry
def _level_chain_case(B):
    def build(ops):
        import test_level_chain_gpu as LC
        from ddk import lib as L
        img = B // 2
        gen = lambda shape, seed, scale=1.0: rnd(*shape, seed=seed, scale=scale)
        ws = [gen((256, 256, 3, 3), 30 + i, (256 * 9) ** -0.5) for i in range(2)]
        bs, gs, bes = ([gen((256,), 40 + i, 0.1) for i in range(2)], [1 + gen((256,), 50 + i, 0.1) for i in range(2)],
                       [gen((256,), 60 + i, 0.1) for i in range(2)])
        temb = gen((B, 256), 70)
        w_qkv = gen((384, 256, 1, 1), 24, 256 ** -0.5)
        g, b = 1 + gen((256,), 25, 0.1), gen((256,), 26, 0.1)
        w_out, b_out = gen((256, 128, 1, 1), 27, 128 ** -0.5), gen((256,), 28, 0.1)
        wq = w_qkv.reshape(384, 256)
        lnw = dev(wq * g[None, :])
        c1, c2 = dev((wq * g[None, :]).sum(dim=1)), dev((wq * b[None, :]).sum(dim=1))
        wop = torch.empty_like(lnw)
        L.check(L.load().ddk_pack_qkv_operand(L.ptr(lnw), L.ptr(wop), 4, 256, L.stream()), "pack_qkv_operand")
        wps = [LC.pack3(dev(w), 16) for w in ws]
        wpo = LC.pack1(dev(w_out))
        bsd, gsd, besd, tembd, b_outd = [dev(v) for v in bs], [dev(v) for v in gs], [dev(v) for v in bes], dev(temb), dev(b_out)
        p = LC._p
        before = ops.cluster_timeouts()

        def run(inp):
            """a ResnetBlock (two conv3x3 + GroupNorm ops, the residual kept) handed to the attention block: four hand-offs"""
            xin = inp["x"]
            h0, r1, heads, out = (torch.empty((B, 4, 4, n), device=DEV) for n in (256, 256, 128, 256))
            LC.run_chain([
                LC.ChainOp(p(xin), None, p(wps[0]), p(bsd[0]), p(gsd[0]), p(besd[0]), p(h0), 256, 0, LC.CONV3, LC.SIGNAL | LC.KEEP_FROM_SRC, 0, 256),
                LC.ChainOp(p(h0), None, p(wps[1]), p(bsd[1]), p(gsd[1]), p(besd[1]), p(r1), 256, 0, LC.CONV3,
                           LC.WAIT | LC.SIGNAL | LC.ADD_KEEP | LC.SAVE_KEEP, -1, 256),
                LC.ChainOp(p(r1), None, p(wop), None, p(c1), p(c2), p(heads), 256, 0, LC.ATTN, LC.WAIT | LC.SIGNAL, -1, 128),
                LC.ChainOp(p(heads), None, p(wpo), p(b_outd), None, None, p(out), 128, 0, LC.CONV1, LC.WAIT | LC.ADD_KEEP, -1, 256)], 16, B, tembd)
            return r1, heads, out

        def ref(inp):
            x = nchw1(inp, "x", img)
            h = LC.block_ref(x, ws[0], bs[0], gs[0], bes[0], temb[img:img + 1])
            r1 = LC.block_ref(h, ws[1], bs[1], gs[1], bes[1]) + x
            o, heads = LC.attn_ref(r1, w_qkv, g, b, w_out, b_out)
            return embed(to_nhwc(r1), B, img), embed(to_nhwc(heads), B, img), embed(to_nhwc(o), B, img)

        def check():
            assert ops.cluster_timeouts() == before, "a chain wait gave up"
        x = to_nhwc(gen((B, 256, 4, 4), 80))
        return Case({"x": x}, run, ref, plants_for({"x": x}, img), "exact", img, check=check)
    return build


CASES["level_chain-4x4-B3"] = _level_chain_case(3)
CASES["level_chain-4x4-B32"] = _level_chain_case(32)


# ================================================================== step rules, one op each
STEP_SHAPE = (3, 8, 8, 4)          # NHWC; t = (0, 500, 999): the planted image runs t = 500


def _step_common():
    buf, tb, tbd = _step_tables()
    t = torch.tensor([0, 500, 999])
    inputs = {"x": rnd(*STEP_SHAPE, seed=1, scale=1.5), "eps": rnd(*STEP_SHAPE, seed=2)}
    B, H, W, C = STEP_SHAPE
    plants = [("eps", (1, 0, 0, C - 1), NF.NAN), ("eps", (1, H - 1, W - 1, C - 1), NF.NAN), ("eps", (1, 3, 4, 0), NF.PINF), ("eps", (1, 3, 4, 1), NF.NINF),
              ("x", (1, 0, 0, C - 1), NF.NAN), ("x", (1, H - 1, W - 1, C - 1), NF.NAN), ("x", (1, 4, 3, 0), NF.PINF), ("x", (1, 4, 3, 1), NF.NINF)]
    co = {k: v[t] for k, v in tb.items()}          # per-sample coefficients [B]
    return buf, tb, tbd, t, inputs, plants, co


def _nchw_step(fn):
    """a tests/*_ref.py step on NCHW fp32 tensors, given and returned NHWC"""
    return lambda *a: to_nhwc(fn(*[to_nchw(v) for v in a]))


@case("step-p_sample_update")
def _(ops):
    buf, tb, tbd, t, inputs, plants, co = _step_common()
    inputs["z"] = rnd(*STEP_SHAPE, seed=3)
    td = dev(t)
    run = lambda inp: (ops.p_sample_update_(inp["x"].clone(), inp["eps"], td, noise=inp["z"], **tbd),
                       ops.p_sample_update_(inp["x"].clone(), inp["eps"], td, seed=9, stream_id=2, **tbd))
    ref = lambda inp: (D.p_sample_update(buf, inp["x"], t, inp["eps"], inp["z"]), D.p_sample_update(buf, inp["x"], t, inp["eps"], torch.zeros(STEP_SHAPE)))
    return Case(inputs, run, ref, plants + [("z", (1, 7, 7, 3), NF.NAN)], "exact_kinds", 1)


@case("step-multistep")
def _(ops):
    buf, tb, tbd, t, inputs, plants, co = _step_common()
    inputs["hist"] = rnd(*STEP_SHAPE, seed=4).clamp(-1, 1)
    c3 = 0.25 * tb["c1"]
    tm = {k: tbd[k] for k in ("c_recip", "c_recipm1", "c1", "c2")}
    td, c3d = dev(t), dev(c3)

    def run(inp):
        x, h = inp["x"].clone(), inp["hist"].clone()
        ops.p_sample_update_multistep_(x, inp["eps"], h, td, c3=c3d, **tm)
        return x, h

    def ref(inp):
        col = lambda v: v.reshape(-1, 1, 1, 1)
        x0 = (col(co["c_recip"]) * inp["x"] - col(co["c_recipm1"]) * inp["eps"]).clamp(-1, 1)
        return (col(co["c1"]) * x0 + col(co["c2"]) * inp["x"]) + col(c3[t]) * inp["hist"], x0
    return Case(inputs, run, ref, plants + [("hist", (1, 7, 7, 3), NF.NAN)], "exact_kinds", 1)


@case("step-inpaint")
def _(ops):
    buf, tb, tbd, t, inputs, plants, co = _step_common()
    inputs["known"] = rnd(*STEP_SHAPE, seed=5).clamp(-1, 1)
    mask = (torch.rand(STEP_SHAPE, generator=torch.Generator().manual_seed(6)) > 0.5).float()
    mask[1, 0, 0, 3], mask[1, 7, 7, 3] = 0.0, 1.0          # one planted corner is unknown, the other known: the select hides it there
    T = 1000
    ka, kb, ja, jb = torch.full((T,), 0.9), torch.full((T,), 0.1), torch.full((T,), 0.95), torch.full((T,), 0.05)
    jb[999] = 0.0                                           # no jump for the last image
    kd = [dev(v) for v in (ka, kb, ja, jb)]
    td, md = dev(t), dev(mask)
    run = lambda inp: (ops.p_sample_update_inpaint_(inp["x"].clone(), inp["eps"], inp["known"], md, td, *[tbd[k] for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")],
                                                    *kd, seed=9, stream_id=2),)

    def ref(inp):
        """the draws are finite and enter by + s * z alone: zeros stand in for them, the classes do not depend on their values"""
        col = lambda v: v[t].reshape(-1, 1, 1, 1)
        unk = D.p_sample_update(buf, inp["x"], t, inp["eps"], torch.zeros(STEP_SHAPE))
        o = torch.where(mask != 0, col(ka) * inp["known"], unk)
        return (torch.where(col(jb) != 0, col(ja) * o, o),)
    return Case(inputs, run, ref, plants + [("known", (1, 7, 7, 3), NF.NAN)], "exact_kinds", 1)


def _restore_case(kind):
    def build(ops):
        import restore_masked_ref as RM
        import restore_noisy_ref as RN
        import restore_ref as RR
        buf, tb, tbd, t, inputs, plants, co = _step_common()
        B, H, W, C = STEP_SHAPE
        n = 2
        inputs["y"] = rnd(B, H // n, W // n, C, seed=7, scale=0.5)
        mk = (torch.rand(B, H // n, W // n, generator=torch.Generator().manual_seed(8)) > 0.4).float()
        mk[1, 0, 0], mk[1, H // n - 1, W // n - 1] = 1.0, 0.0          # the corner block is measured, the last block is not
        lam, sgm = torch.linspace(0.2, 1.0, 1000), 0.5 * tb["sigma"]
        td, mkd, lamd, sgmd = dev(t), dev(mk), dev(lam), dev(sgm)
        z = torch.zeros(B, C, H, W)        # stands in for the (finite) Philox draw: the classes do not depend on its values
        cs = [co[k] for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")]
        if kind == "restore":
            run = lambda inp: (ops.p_sample_update_restore_(inp["x"].clone(), inp["eps"], inp["y"], n, td, seed=9, stream_id=2, **tbd),)
            ref = lambda inp: (_nchw_step(lambda x, e, y: RR.step(x, e, y, n, *cs, z))(inp["x"], inp["eps"], inp["y"]),)
        elif kind == "masked":
            run = lambda inp: (ops.p_sample_update_restore_masked_(inp["x"].clone(), inp["eps"], inp["y"], mkd, n, td, seed=9, stream_id=2, **tbd),)
            ref = lambda inp: (_nchw_step(lambda x, e, y: RM.step(x, e, y, mk, n, *cs, z))(inp["x"], inp["eps"], inp["y"]),)
        else:
            run = lambda inp: (ops.p_sample_update_restore_noisy_(inp["x"].clone(), inp["eps"], inp["y"], mkd, n, td, lam=lamd, sgm=sgmd, seed=9, stream_id=2, **tbd),)
            ref = lambda inp: (_nchw_step(lambda x, e, y: RN.step(x, e, y, mk, n, *cs, lam[t], sgm[t], z))(inp["x"], inp["eps"], inp["y"]),)
        return Case(inputs, run, ref, plants + [("y", (1, 0, 0, C - 1), NF.NAN), ("y", (1, H // n - 1, W // n - 1, 0), NF.NAN)], "exact_kinds", 1)
    return build


CASES["step-restore-n2"] = _restore_case("restore")
CASES["step-restore_masked-n2"] = _restore_case("masked")
CASES["step-restore_noisy-n2"] = _restore_case("noisy")


def _plane_case(kind):
    """the plane-wide DDNM steps on one 16x16 plane per (image, channel): a non-finite x0 spreads over its plane and no further"""
    def build(ops):
        import blur_ref as BR
        import fft_conv_ref as FR
        import hadamard_ref as HR
        B, H, W, C = 3, 16, 16, 3
        buf, tb, tbd = _step_tables()
        t = torch.tensor([0, 500, 999])
        co = [tb[k][t] for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")]
        inputs = {"x": rnd(B, H, W, C, seed=1, scale=1.5), "eps": rnd(B, H, W, C, seed=2)}
        td = dev(t)
        z = torch.zeros(B, C, H, W)
        if kind == "blur":
            P_h, P_w = rnd(H, H, seed=3, scale=H ** -0.5), rnd(W, W, seed=4, scale=W ** -0.5)
            Yp = rnd(B, H, W, C, seed=5, scale=0.3)
            Pd = (dev(P_h), dev(P_w), dev(Yp))
            run = lambda inp: (ops.p_sample_update_restore_blur_(inp["x"].clone(), inp["eps"], *Pd, td, seed=9, stream_id=2, **tbd),)
            ref = lambda inp: (to_nhwc(BR.step(to_nchw(inp["x"]), to_nchw(inp["eps"]), P_h, P_w, to_nchw(Yp), *co, z)[0]),)
        elif kind == "cs":
            m = H * W // 4
            y = rnd(B, C, m, seed=3)
            perm = torch.randperm(H * W, generator=torch.Generator().manual_seed(4)).to(torch.int32)
            yd, pd = dev(y), dev(perm)
            run = lambda inp: (ops.p_sample_update_restore_cs_(inp["x"].clone(), inp["eps"], yd, pd, td, seed=9, stream_id=2, **tbd),)
            ref = lambda inp: (to_nhwc(HR.step(to_nchw(inp["x"]), to_nchw(inp["eps"]), y.numpy(), perm.numpy(), *co, z)[0]),)
        else:
            mask = torch.rand(H, W, generator=torch.Generator().manual_seed(3)) > 0.5
            Yp = rnd(B, H, W, C, seed=5, scale=0.3)
            md, Yd = dev(mask.float()), dev(Yp)
            run = lambda inp: (ops.p_sample_update_restore_fft_(inp["x"].clone(), inp["eps"], md, Yd, td, seed=9, stream_id=2, **tbd),)
            ref = lambda inp: (to_nhwc(FR.step(to_nchw(inp["x"]), to_nchw(inp["eps"]), mask.numpy(), to_nchw(Yp), *co, z)[0]),)
        plants = [("eps", (1, 0, 0, C - 1), NF.NAN), ("eps", (1, H - 1, W - 1, 0), NF.NAN), ("x", (1, H - 1, W - 1, C - 1), NF.NAN), ("x", (1, 0, 0, 1), NF.NAN)]
        return Case(inputs, run, ref, plants, "exact", 1)
    return build


CASES["step-restore_blur-16x16"] = _plane_case("blur")
CASES["step-restore_cs-16x16"] = _plane_case("cs")
CASES["step-restore_fft-16x16"] = _plane_case("fft")


@case("vlb_terms-3")
def _(ops):
    buf = D.schedule_buffers("linear", 1000)
    B = 3
    x = syn.synthetic_input((B, 3, 16, 16), "nonfinite.vlb.x").clamp(-1, 1)
    x[1, 0, 0, 0], x[1, 2, 15, 15] = -1.0, 1.0                 # both edge branches of the discretised likelihood
    eps = syn.synthetic_normal((B, 3, 16, 16), "nonfinite.vlb.eps")
    res = []
    for t in (torch.tensor([17, 0, 999]), torch.tensor([0, 500, 999])):        # the planted image at t = 0 (NLL) and at t > 0 (KL)
        res.append((t, D.q_sample(buf, x, t, eps)))
    inputs = {"x": x, "eps_hat": eps + 0.3 * syn.synthetic_normal((B, 3, 16, 16), "nonfinite.vlb.d"), "eps": eps,
              "xt0": res[0][1], "xt1": res[1][1]}
    dv = {k: v.to(DEV) for k, v in buf.items()}
    tabs = (dv["sqrt_recip_alphas_cumprod"], dv["sqrt_recipm1_alphas_cumprod"], dv["posterior_mean_coef1"], dv["posterior_mean_coef2"],
            dv["posterior_log_variance_clipped"])
    tds = [dev(r[0]) for r in res]
    assert ops.L.load().ddk_vlb_terms_workspace_bytes(B, 3 * 16 * 16) > B * 4

    def run(inp):
        out = []
        for i in range(2):
            out += list(ops.vlb_terms(inp["x"], inp[f"xt{i}"], inp["eps_hat"], tds[i], *tabs, eps=inp["eps"]))
        return tuple(out)

    def ref(inp):
        out = []
        for i in range(2):
            out += [D.vlb_terms(buf, inp["x"], inp[f"xt{i}"], res[i][0], inp["eps_hat"]), ((inp["eps"] - inp["eps_hat"]) ** 2).sum(dim=(1, 2, 3))]
        return tuple(out)
    plants = [("eps_hat", (1, 0, 0, 0), NF.NAN), ("eps_hat", (1, 2, 15, 15), NF.NAN), ("eps_hat", (1, 1, 7, 7), NF.NAN), ("eps_hat", (1, 1, 7, 7), NF.PINF),
              ("x", (1, 2, 15, 15), NF.NAN), ("xt0", (1, 0, 0, 0), NF.NAN), ("xt1", (1, 2, 15, 15), NF.NAN), ("eps", (1, 0, 0, 0), NF.NAN)]
    return Case(inputs, run, ref, plants, "exact_kinds", 1)


@case("q_sample-sq_err_sum")
def _(ops):
    buf = D.schedule_buffers("linear", 1000)
    inputs = {"a": rnd(3, 8, 32, 32, seed=120), "b": rnd(3, 8, 32, 32, seed=121)}
    t = torch.tensor([0, 499, 999])
    td, sa, sb = dev(t), buf["sqrt_alphas_cumprod"].to(DEV), buf["sqrt_one_minus_alphas_cumprod"].to(DEV)
    run = lambda inp: (ops.sq_err_sum(inp["a"], inp["b"]), ops.q_sample(inp["a"], inp["b"], td, sa, sb))
    ref = lambda inp: (((inp["a"] - inp["b"]) ** 2).sum(dim=(1, 2, 3)), D.q_sample(buf, inp["a"], t, inp["b"]))
    plants = [(n, w, v) for n in ("a", "b") for w, v in (((1, 0, 0, 0), NF.NAN), ((1, 7, 31, 31), NF.PINF), ((1, 3, 16, 16), NF.NINF))]
    return Case(inputs, run, ref, plants, "exact_kinds", 1)


# ================================================================== elementwise and layout
@case("elementwise")
def _(ops):
    inputs = {"x": to_nhwc(rnd(3, 64, 8, 12, seed=50)), "y": to_nhwc(rnd(3, 64, 8, 12, seed=51))}

    def run(inp):
        x, y = inp["x"], inp["y"]
        return (ops.mish(x), ops.tanh(x), ops.add(x, y), ops.avgpool2(x), ops.upsample_nearest2(x), ops.mish_bwd(x, y), ops.tanh_bwd(x, y),
                ops.avgpool2_bwd(x), ops.upsample_nearest2_bwd(x))

    def ref(inp):
        x, y = inp["x"], inp["y"]
        xn = to_nchw(x)
        leaf = x.clone().requires_grad_(True)
        dmish = torch.autograd.grad(F.mish(leaf), leaf, y)[0]
        return (F.mish(x), torch.tanh(x), x + y, to_nhwc(F.avg_pool2d(xn, 2)), to_nhwc(F.interpolate(xn, scale_factor=2, mode="nearest")),
                dmish, y * (1 - x * x), to_nhwc(F.interpolate(xn, scale_factor=2, mode="nearest")) * 0.25, to_nhwc(F.avg_pool2d(xn, 2)) * 4.0)
    plants = [(n, w, v) for n in ("x", "y") for w, v in (((1, 0, 0, 31), NF.NAN), ((1, 7, 11, 63), NF.PINF), ((1, 4, 6, 0), NF.NINF))]
    return Case(inputs, run, ref, plants, "exact_kinds", 1)


def _fix_samples_case(B, C, H, W):
    """the sampler's output stage: x.min() / x.max() of an image that holds a NaN are NaN, so the whole image is; a +Inf makes the
    range Inf (the rest 0, the element NaN), a -Inf makes every element (x + Inf) / Inf = NaN"""
    def build(ops):
        inputs = {"s": rnd(B, C, H, W, seed=90)}
        run = lambda inp: (ops.fix_samples(inp["s"]),)
        ref = lambda inp: (torch.from_numpy(D.fix_samples(inp["s"])),)
        img = B // 2
        plants = [("s", (img, 0, 0, 0), NF.NAN), ("s", (img, C - 1, H - 1, W - 1), NF.NAN), ("s", (img, C - 1, H - 1, W - 1), NF.PINF),
                  ("s", (img, C // 2, H // 2, W // 2), NF.NINF)]
        return Case(inputs, run, ref, plants, "exact_kinds", img)
    return build


CASES["fix_samples-3-5-6-7"] = _fix_samples_case(3, 5, 6, 7)
CASES["fix_samples-3-3-40-40"] = _fix_samples_case(3, 3, 40, 40)        # 4800 elements: every thread of the image's workgroup reduces several


def test_mish_at_infinity(ops):
    """F.mish(-inf) is -inf * tanh(softplus(-inf)) = -inf * 0 = NaN, F.mish(+inf) = +inf, and so is the kernels' mish_f: pinned"""
    v = torch.tensor([NF.NINF, NF.PINF, NF.NAN, -200.0, 200.0, 0.0, -0.0, 1.0])
    want = F.mish(v)
    assert torch.isnan(want[0]) and want[1] == NF.PINF and torch.isnan(want[2]) and torch.isfinite(want[3:]).all()
    got = ops.mish(dev(v)).cpu()
    assert NF.exact_kinds(got, want), NF.describe(got, want)
    assert rel_err(got[3:], want[3:].double()) < 1e-6


# ================================================================== the optimiser
@case("grad_norm_clip-adam-ema")
def _(ops):
    n = 100003
    inputs = {"g": rnd(n, seed=81, scale=3.0)}
    p0, e0 = rnd(n, seed=80), rnd(n, seed=82)
    p0d, e0d = dev(p0), dev(e0)

    def run(inp):
        p, m, v, ema = p0d.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), e0d.clone()
        nc = ops.grad_norm_clip(inp["g"], 1.0)
        ops.adam_step_(p, inp["g"], m, v, 2e-4, 1, clip=nc)
        ops.ema_update_(ema, p, 0.995)
        return nc, p, m, v, ema

    def ref(inp):
        clipped, total = TR.clip_grads({"w": inp["g"]}, 1.0)
        coef = torch.clamp(1.0 / (total + 1e-6), max=1.0)
        p, m, v = TR.adam_step(p0, clipped["w"], torch.zeros(n), torch.zeros(n), 1, 2e-4)
        return torch.stack([total, coef]), p, m, v, TR.ema_update({"w": e0}, {"w": p}, 0.995)["w"]
    plants = [("g", (0,), NF.NAN), ("g", (n - 1,), NF.NAN), ("g", (n // 2,), NF.PINF)]
    return Case(inputs, run, ref, plants, "exact", None, batched=(False,) * 5)


# ================================================================== the one check, over the whole table
def _cpu(res):
    torch.cuda.synchronize()
    if torch.is_tensor(res):
        res = (res,)
    return tuple(None if t is None else t.detach().cpu().contiguous() for t in res)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", list(CASES))
def test_nonfinite_footprint(ops, name):
    c = CASES[name](ops)
    dev_in = {k: dev(v) for k, v in c.inputs.items()}
    clean = _cpu(c.run(dev_in))
    if c.check:
        c.check()
    for t in clean:
        assert t is not None and bool(torch.isfinite(t).all()), f"{name}: the clean run is not finite"
    assert torch.equal(torch.cat([_bits(t).reshape(-1) for t in clean]), torch.cat([_bits(t).reshape(-1) for t in _cpu(c.run(dev_in))])), \
        f"{name}: two clean runs differ, so bit-identity of the other images means nothing"
    hit = 0
    for plant in c.plants:
        pname, where, value = plant
        tag = f"{name}: {value} in {pname}{tuple(where)}"
        planted = dict(c.inputs)
        planted[pname] = NF.plant(c.inputs[pname], where, value)
        din = dict(dev_in)
        din[pname] = dev(planted[pname])
        got = _cpu(c.run(din))
        if c.check:
            c.check()
        ref = c.ref(planted)
        allowed = c.allowed(plant) if c.allowed else (None,) * len(got)
        assert len(got) == len(ref) == len(clean)
        for i, (g, r, cl) in enumerate(zip(got, ref, clean)):
            if r is not None:
                r = r.reshape(g.shape)
                if c.rule == "exact":
                    assert NF.exact(g, r), f"{tag}: output {i}: {NF.describe(g, r)}"
                elif c.rule == "exact_kinds":
                    assert NF.exact_kinds(g, r), f"{tag}: output {i}: {NF.describe(g, r)}"
                else:
                    assert NF.within(g, r, allowed[i]), f"{tag}: output {i}: {NF.describe(g, r, allowed[i])}"
                hit += int(NF.nonfinite(r).sum())
                if c.bitwise_outside:
                    keep = ~NF.nonfinite(r)
                    assert torch.equal(_bits(g)[keep], _bits(cl)[keep]), f"{tag}: output {i}: an element outside the reference's set changed"
            if c.batched is None or c.batched[i]:
                assert NF.isolated(g, cl, c.image), f"{tag}: output {i}: another image than {c.image} changed"
    assert hit > 0, f"{name}: no reference carries anything non-finite: the case tests nothing"


# ================================================================== whole chains on the tiny model of the sampler goldens
TINY = ddpm_cfg(32, 3, 16)


def _state(cfg):
    from models import DDPM, Unet
    m = DDPM(cfg, Unet(cfg), "cpu", cfg["unet_in"])
    return {k: (v.clone() if k in syn.SCHEDULE_KEYS else syn.fill_tensor(k, v.shape)) for k, v in m.state_dict().items()}


def _model(cfg, sd):
    from models import DDPM, Unet
    m = DDPM(cfg, Unet(cfg), DEV, cfg["unet_in"])
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def _guarded(ops, m, fn):
    """fn() with the in-launch exchanges watched: no give-up, no warning, the plan's option where it was"""
    before = ops.cluster_timeouts()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = fn()
        torch.cuda.synchronize()
    assert ops.cluster_timeouts() == before, "an in-launch exchange gave up"
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
    assert m.latent_model.plan()._cluster == 1, "the cluster check switched the in-launch GroupNorm off"
    return out


def test_whole_chain_carries_a_nan_to_the_end_of_its_image_only(ops):
    """4 steps of the native graph sampler, default options, B = 3, one NaN in x_T of image 1: image 1 ends entirely NaN, as
    oracle.diffusion_ref.p_sample_loop gives, and images 0 and 2 are bit-identical to the run from the clean x_T"""
    sd = _state(TINY)
    shape = (3, 3, 16, 16)
    x_T = syn.synthetic_normal(shape, "nonfinite.chain.xT")
    noise = torch.stack([syn.synthetic_normal(shape, f"nonfinite.chain.n{k}") for k in range(4)])
    planted = NF.plant(x_T, (1, 2, 15, 15), NF.NAN)
    m = _model(TINY, sd)
    assert m.use_graph and m.native_sampler
    clean = _guarded(ops, m, lambda: m.p_sample_loop(shape, early_stop=996, x_T=x_T, noise=noise)).cpu()
    got = _guarded(ops, m, lambda: m.p_sample_loop(shape, early_stop=996, x_T=planted, noise=noise)).cpu()
    buf = D.schedule_buffers("linear", 1000)
    want, _ = D.p_sample_loop(buf, lambda a, b: U.unet_forward(sd, TINY, a, b, pre="latent_model."), planted, list(noise), 1000, 996)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2]]).all()), "the oracle: image 1 NaN, the others finite"
    assert torch.isfinite(clean).all()
    assert NF.exact_kinds(got, want), NF.describe(got, want)
    assert NF.isolated(got, clean, 1), "a NaN in image 1 moved image 0 or 2"
    assert rel_err(got[[0, 2]], want[[0, 2]]) < 1e-4
    # Philox draws instead of injected ones: the same property
    clean = _guarded(ops, m, lambda: m.p_sample_loop(shape, early_stop=996, x_T=x_T, seed=11)).cpu()
    got = _guarded(ops, m, lambda: m.p_sample_loop(shape, early_stop=996, x_T=planted, seed=11)).cpu()
    assert bool(torch.isnan(got[1]).all()) and NF.isolated(got, clean, 1) and torch.isfinite(clean).all()


def test_dpm_solver_chain_carries_a_nan_to_the_end_of_its_image_only(ops):
    sd = _state(TINY)
    shape = (3, 3, 16, 16)
    x_T = syn.synthetic_normal(shape, "nonfinite.chain.xT")
    planted = NF.plant(x_T, (1, 0, 0, 0), NF.NAN)
    m = _model(TINY, sd)
    clean = _guarded(ops, m, lambda: m.p_sample_loop(shape, x_T=x_T, respacing="logsnr4", solver="dpm++2m")).cpu()
    got = _guarded(ops, m, lambda: m.p_sample_loop(shape, x_T=planted, respacing="logsnr4", solver="dpm++2m")).cpu()
    assert torch.isfinite(clean).all()
    assert bool(torch.isnan(got[1]).all()), f"{int(torch.isfinite(got[1]).sum())} finite elements left in the planted image"
    assert NF.isolated(got, clean, 1), "a NaN in image 1 moved image 0 or 2"


def test_likelihood_sweep_reports_nan_for_its_image_only(ops):
    """the native sweep (T = 3) with one NaN in image 1 of the data: that image's terms are NaN as oracle.diffusion_ref.test_losses
    gives, the other images' terms keep their bits; L_simple_t is a mean over the batch and is NaN in both"""
    cfg = ddpm_cfg(32, 3, 16, T=3, schedule="cosine")
    sd = _state(cfg)
    x = syn.synthetic_input((3, 3, 16, 16), "nonfinite.sweep.x").clamp(-1, 1)
    noise = torch.stack([syn.synthetic_normal((3, 3, 16, 16), f"nonfinite.sweep.n{k}") for k in range(3)])
    planted = NF.plant(x, (1, 1, 7, 9), NF.NAN)
    m = _model(cfg, sd)
    clean = _guarded(ops, m, lambda: m.test_losses(dev(x), noise=noise))
    got = _guarded(ops, m, lambda: m.test_losses(dev(planted), noise=noise))
    buf = D.schedule_buffers("cosine", 3)
    want = D.test_losses(buf, lambda a, b: U.unet_forward(sd, cfg, a, b, pre="latent_model."), planted, list(noise), 3)
    for k in ("vlb_t", "prior", "vlb"):
        g, cl, w = got[k].cpu(), clean[k].cpu(), want[k]
        assert torch.isfinite(cl).all()
        assert NF.exact_kinds(g, w), f"{k}: {NF.describe(g, w)}"
        assert bool(torch.isnan(g[1]).all()) and NF.isolated(g, cl, 1), k
    for k in ("L_simple_t", "L_simple"):
        assert NF.exact_kinds(got[k].cpu().reshape(-1), want[k].reshape(-1)), k
