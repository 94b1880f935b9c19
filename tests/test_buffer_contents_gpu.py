"""No result may depend on what an output or workspace buffer held before the launch.

Every buffer ddk.ops / ddk.autograd / ddk.plan hand to the library comes from torch.empty / torch.empty_like (contract: any contents),
and in the other tests the caching allocator serves those from recycled blocks that hold plausible numbers -- often the same op's
earlier result.  Here ONE check runs over a table of cases: each case builds its inputs once, outside any poison, then is run plainly
(twice) and under each of three poison words (tests/poison.py: fresh allocations and the cached ops._scratch buffers filled with
NaN / 0 / 1.0 bit patterns).  Asserted: (a) the case allocated through the patched paths, (b) all result tuples are bit-identical
(compared as integers, so NaNs compare), (c) every float result is finite.  A slab region that a ragged split never writes but the
reduce reads, a GroupNorm partial of a half-empty tile, a counter word outside the memset, an output corner that is never stored: each
gives different bits under at least two of the words.

Buffers whose documented contract is "zeroed by the caller" (torch.zeros: attention_split_workspace, ClockProbe's records, the packed
arena, lnw) stay zeroed: they are outside the patched functions."""
import contextlib
import warnings

import pytest
import torch

from helpers import ddpm_cfg, dddpm_cfg, rel_err, to_nhwc
from poison import WORDS, poisoned_allocations, repoison
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---------------------------------------------------------------------------------------------------------------------------------
# The audit behind the table (read from ddk/ops.py, ddk/autograd.py, ddk/plan.py and the launchers in csrc/): which torch.empty buffers
# an entry receives, and which launch or memset writes a region before which launch reads it.  "out" is always the entry's result
# tensor, written whole by the last launch named.
#
#  im2col conv (conv_igemm.hip conv_forward)      out; ws = splits x |out| slabs when plan_conv splits k.  Every split z < splits owns
#      >= 1 k-chunk (splits = ceil(kiters / kps)) and stores its whole tile, rows < M only; splitk_reduce_kernel reads exactly splits
#      slabs of |out| and writes out (+ bias, resid, Mish).  defer_reduce / leave_slabs: no reduce, `out` stays unwritten by contract
#      and the consumer (ddk_groupnorm_mish_slabs, ..._train_fwd_slabs, conv3x3_gn_mish_slabs) sums the same `splits` slabs.
#  Winograd conv, conv transpose (conv_wino.hip)  as above with splits = conv_wino_splits / convT_wino_splits channel-chunk slabs;
#      a ragged tile block (fewer than 32 tiles) stores only its real tiles and the reduce reads only |out| per slab.
#  conv + GroupNorm partials, conv_first          raw, part [B * tiles][groups][2]: one {mean, M2} record per (128-pixel tile, group),
#      stored by the tile's workgroup in the conv's epilogue; groupnorm_mish_partials(_res1x1) / final_tail read tiles_per_image
#      records per image.  Eligibility (H * W % 128 == 0) leaves no half-empty tile.
#  one-launch Blocks (conv_local.hip)             out only; statistics live in LDS.
#  in-launch GroupNorm (ddk_conv3x3_gn_mish_cluster)   cached scratch: [B][8 * 16] counters + a 16-word give-up line = cl_front_floats(B),
#      zeroed by hipMemsetAsync at every call; the kernels poll counter (image * n_tiles + tile_n) * 16 with n_tiles <= 8; then the
#      records, each stored by its tile before the counter it is published with is bumped.  k-split shapes: conv_wino_cluster_pair_words
#      pair counters, zeroed by a second memset of exactly that many words, then (splits - 1) slabs, each partial tile stored before
#      its pair counter is bumped.  cluster_check reads the give-up word inside the zeroed front.
#  conv1x1_ws / _sm / _stream / small_n           out only.
#  groupnorm_mish                                 out; ws [B][groups][ns][3] on the streamed path: gn_partial_kernel's grid is
#      (B * groups * ns) and stores every record, gn_apply_kernel reads ns per (image, group).
#  linattn / attention_folded / kv_context        ctx, out, kv, a_mat, a1, a2; ws [B * heads][s] partial contexts, one per workgroup of the
#      context launch, merged by a launch that reads s of them.  attention_split_from_x: workspace zeroed by the caller (torch.zeros).
#  conv backward (conv_wgrad.hip)                 dx like a forward conv; weight gradient: ws = splits x N x (taps * cx (+ 1)) slabs, every
#      split's workgroups store their whole tile, wgrad_reduce_kernel reads splits slabs; deferred: the slab
#      buffer is the call's own torch.empty and ddk_wgrad_reduce_jobs reads the same extent.  bias_grad: parts x N partial rows.
#  GroupNorm / LayerNorm backward                 dx, part [4][B][C] (every (image, channel) stored by the group's workgroup), LayerNorm
#      part [2][512][C] of which the kernel reports how many rows n it stored; only rows < n are summed.  small-N conv backward: the same
#      with max_rows 1024.
#  linattn_train / linattn_bwd                    stats, dctx, dqkv; ws: sp pixel-split partial rows, merged by a launch reading sp.
#  small_gemm                                     ws zs x M x N partial products with zs = ceil(K / kper) <= splits: rows_sum_kernel reads
#      zs slabs, not the requested split count.  grad_norm_clip: `blocks` partial sums stored, `blocks` read.
#  resampler convs                                ws: per-workgroup partial weight gradients, all stored, then summed.
#  vlb_terms                                      ws [B] counters + [B][ns][2] partials; the memset covers B words = the words the kernel
#      bumps (counters + b, b < B); the last slice to arrive sums ns partials and puts the counter back to 0.
#  image_metrics                                  sq [N][2] zeroed by memset (atomic integer adds), ssim [N], ws: per-tile doubles, all stored.
#  manifold                                       radii; a_in / b_in zeroed by memset (the kernel only sets flags); ws: row norms, stored by
#      mf_norms before the distance launch; the column-split partial lists after them, one per (row, split).
#  hadamard / circular_conv / separable_rect / DDNM steps   the scratch image of planes that do not fit in LDS: pass 1 stores it whole,
#      pass 2 reads it.
#  UnetPlan workspaces (unet_plan.hip)            one torch.empty per (kind, size); activations and split-K regions as for the single ops.
#      Counter area at off_cl = [B][8 * 16] GroupNorm counters | give-up line | [B][64] level-chain counters | CL_PAIR_WORDS pair
#      counters | [B][4][32] attention-split counters = cl_counter_floats(B) words, ALL zeroed by one hipMemsetAsync at every
#      ddk_unet_forward (unet_plan.hip:1417) and at every chain / sweep start (:1712), outside the captured graph; every counter
#      re-arms itself.  Chain state {counter, seed, stream}: set_chain_state_kernel at the chain's start; t_cur [B]: stored by the
#      first kernel of every step before any kernel of that step reads it; the time-shift table: rebuilt whenever the workspace
#      pointer, the shape or the weights change; x0 history of the multistep rules: zeroed by memset per chain.
# No integer word of any workspace is used as an address or a loop bound except t_cur (above) and the timestep map t_all (copied or
# written by iota64_kernel before time_mlp reads it): everything else that is an integer is a counter.
# ---------------------------------------------------------------------------------------------------------------------------------

# Entries whose two PLAIN runs already differ in bits.  Each line: the case name -> why, from the kernel's code (float atomics,
# arrival-order merges).  Such a case must carry a reference and its parity test's bar (Case.ref / Case.bar) and is compared with
# that instead.  Empty: every entry below is bit-reproducible run to run.
NOT_BIT_REPRODUCIBLE = []


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(*ts):
    out = tuple(None if t is None else t.to(DEV).contiguous() for t in ts)
    return out if len(out) > 1 else out[0]


def fresh_copy(t):
    """a working copy of t in a buffer that came from torch.empty (in-place ops run on it)"""
    out = torch.empty_like(t)
    out.copy_(t)
    return out


@pytest.fixture(scope="module")
def ops():
    from ddk import lib
    from ddk import ops as o
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


class Case:
    """run() -> tuple of result tensors (None entries allowed).  ref / bar: only for NOT_BIT_REPRODUCIBLE entries."""

    def __init__(self, run, ref=None, bar=None):
        self.run, self.ref, self.bar = run, ref, bar


CASES = {}        # name -> builder(ops) -> Case or run callable; the builder makes the inputs, outside any poison


def case(name):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return reg


def _snap(res):
    torch.cuda.synchronize()
    if torch.is_tensor(res):
        res = (res,)
    return tuple(None if t is None else t.detach().cpu().contiguous().clone() for t in res)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b):
    return len(a) == len(b) and all((p is None and q is None) or (p is not None and q is not None and p.shape == q.shape and p.dtype == q.dtype
                                                                 and torch.equal(_bits(p), _bits(q))) for p, q in zip(a, b))


def _first_difference(a, b):
    for i, (p, q) in enumerate(zip(a, b)):
        if p is None or q is None or p.shape != q.shape:
            return f"result {i}: {None if p is None else tuple(p.shape)} vs {None if q is None else tuple(q.shape)}"
        d = (_bits(p) != _bits(q)).reshape(-1)
        if bool(d.any()):
            k = int(d.nonzero()[0])
            return (f"result {i} {tuple(p.shape)}: {int(d.sum())} of {d.numel()} elements differ, first at flat index {k}: "
                    f"{p.reshape(-1)[k].item()!r} vs {q.reshape(-1)[k].item()!r}")
    return "lengths differ"


# ================================================================== im2col convs (ddk_conv_forward)
def _conv_inputs(ops, kind, B, H, W, c0, c1, N, seed=1):
    cin = c0 + c1
    k = {"s1": 3, "s2": 3, "1x1": 1, "T": 4}[kind]
    x = to_nhwc(rnd(B, cin, H, W, seed=seed))
    bias = rnd(N, seed=seed + 2, scale=0.1)
    if kind == "T":
        w = rnd(cin, N, 4, 4, seed=seed + 1, scale=(cin * 4) ** -0.5)
        wp, code, ho, wo = ops.pack_convT_weight(w.to(DEV)), ops.CONVT4X4_S2, 2 * H, 2 * W
    else:
        w = rnd(N, cin, k, k, seed=seed + 1, scale=(cin * k * k) ** -0.5)
        wp = ops.pack_conv_weight(w.to(DEV))
        code = {"s1": ops.CONV3X3_S1, "s2": ops.CONV3X3_S2, "1x1": ops.CONV1X1}[kind]
        ho, wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if kind == "s2" else (H, W)
    x0 = dev(x[..., :c0])
    x1 = dev(x[..., c0:]) if c1 else None
    resid = dev(rnd(B, ho, wo, N, seed=seed + 3))
    return code, x0, x1, w.to(DEV), wp, bias.to(DEV), resid


CONV_CASES = [  # kind, B, H, W, c0, c1, N, what the case is for
    ("s1", 2, 8, 8, 32, 0, 64, "small"),         # small M, 9 k-chunks (the planner keeps it in one piece: ddk_conv_splits == 1)
    ("s1", 2, 8, 8, 64, 0, 64, "split"),         # split-K: 18 k-chunks over 4 slabs (5, 5, 5, 3: a ragged last split) + reduce
    ("s1", 3, 5, 7, 32, 0, 32, "ragged"),        # ragged M
    ("s2", 2, 7, 9, 32, 0, 32, "odd"),           # odd spatial size
    ("T", 4, 4, 4, 64, 0, 64, "T"),
    ("1x1", 2, 4, 4, 256, 256, 256, "split"),    # dual source, split-K
    ("s1", 69, 8, 8, 256, 0, 384, "split"),      # halo-tile kernel, odd batch: the last tile is half empty; two channel-chunk slabs
]


def _conv_case(kind, B, H, W, c0, c1, N, what, with_resid):
    def build(ops):
        code, x0, x1, _, wp, bias, resid = _conv_inputs(ops, kind, B, H, W, c0, c1, N)
        splits = ops.L.load().ddk_conv_splits(code, B, H, W, c0 + c1, N)
        assert splits >= 1
        if what == "split":
            assert splits > 1, "the case is meant to split k"
        return lambda: (ops.conv(code, x0, wp, bias, x2=x1, resid=resid if with_resid else None),)
    return build


for _c in CONV_CASES:
    CASES[f"conv-{'-'.join(map(str, _c[:7]))}"] = _conv_case(*_c, with_resid=False)
    CASES[f"conv-{'-'.join(map(str, _c[:7]))}-resid"] = _conv_case(*_c, with_resid=True)


@case("conv-s1-2-8-8-64-0-64-leave_slabs")
def _(ops):
    code, x0, _, _, wp, bias, _ = _conv_inputs(ops, "s1", 2, 8, 8, 64, 0, 64)
    nslab = ops.L.load().ddk_conv_splits(code, 2, 8, 8, 64, 64)
    assert nslab > 1

    def run():
        out, slabs = ops.conv(code, x0, wp, bias, leave_slabs=True)
        assert slabs is not None and slabs.shape[0] == nslab          # `out` is unwritten by contract: the slabs are the result
        return (slabs,)
    return run


@case("conv-pre_post_mish-split")
def _(ops):
    x = dev(to_nhwc(rnd(2, 64, 8, 8, seed=9)))
    wp = ops.pack_conv_weight(rnd(32, 64, 3, 3, seed=8, scale=(64 * 9) ** -0.5).to(DEV))
    b = rnd(32, seed=7, scale=0.1).to(DEV)
    assert ops.L.load().ddk_conv_splits(ops.CONV3X3_S1, 2, 8, 8, 64, 32) > 1          # post_mish is applied by the reduce kernel
    return lambda: (ops.conv(ops.CONV3X3_S1, x, wp, b, post_mish=True),)


# ================================================================== Winograd convs
WINO_CASES = [(2, 4, 4, 64, 0, 64, True), (3, 6, 10, 96, 0, 128, False), (32, 4, 4, 256, 0, 256, True), (2, 2, 2, 32, 0, 64, False)]


def _wino_case(B, H, W, c0, c1, N, must_split, epilogue):
    def build(ops):
        code, x0, x1, w, wp, bias, resid = _conv_inputs(ops, "s1", B, H, W, c0, c1, N, seed=61)
        wu = ops.pack_conv_weight_wino(w)
        splits = ops.L.load().ddk_conv_wino_splits(B, H, W, c0 + c1, N)
        assert splits >= 1, "the case is meant to run on the Winograd kernel"
        if must_split:
            assert splits > 1, "the case is meant to split the channel chunks"
        if epilogue:
            return lambda: (ops.conv(code, x0, wp, bias, x2=x1, resid=resid, post_mish=True, w_wino=wu),)
        return lambda: (ops.conv(code, x0, wp, bias, x2=x1, w_wino=wu),)
    return build


for _c in WINO_CASES:
    CASES[f"wino-{'-'.join(map(str, _c[:6]))}"] = _wino_case(*_c, epilogue=False)
CASES["wino-2-4-4-64-0-64-post_mish-resid"] = _wino_case(2, 4, 4, 64, 0, 64, True, epilogue=True)
CASES["wino-3-6-10-96-0-128-post_mish-resid"] = _wino_case(3, 6, 10, 96, 0, 128, False, epilogue=True)


@case("wino-32-4-4-256-0-256-leave_slabs")
def _(ops):
    code, x0, _, w, wp, bias, _ = _conv_inputs(ops, "s1", 32, 4, 4, 256, 0, 256, seed=61)
    wu = ops.pack_conv_weight_wino(w)
    nslab = ops.L.load().ddk_conv_wino_splits(32, 4, 4, 256, 256)
    assert nslab > 1

    def run():
        _, slabs = ops.conv(code, x0, wp, bias, w_wino=wu, leave_slabs=True)
        assert slabs is not None and slabs.shape[0] == nslab
        return (slabs,)
    return run


def _convT_wino_case(B, H, W, C, N, slabs):
    def build(ops):
        x = dev(to_nhwc(rnd(B, C, H, W, seed=11)))
        w = rnd(C, N, 4, 4, seed=12, scale=(C * 4) ** -0.5).to(DEV)
        bias = rnd(N, seed=13, scale=0.1).to(DEV)
        wp, wu = ops.pack_convT_weight(w), ops.pack_convT_weight_wino(w)
        splits = ops.L.load().ddk_convT_wino_splits(B, H, W, C, N)
        assert splits > 0 and (slabs is None or splits == slabs)
        return lambda: (ops.conv(ops.CONVT4X4_S2, x, wp, bias, w_wino=wu),)
    return build


for _c in [(3, 6, 10, 96, 128, None), (1, 2, 2, 32, 128, None), (32, 4, 4, 256, 256, 8)]:
    CASES[f"convT_wino-{'-'.join(map(str, _c[:5]))}"] = _convT_wino_case(*_c)


# ================================================================== conv + GroupNorm partials, first conv, final tail
def _gn_params(N, B, seed):
    return dev(1 + rnd(N, seed=seed, scale=0.2), rnd(N, seed=seed + 1, scale=0.2), rnd(B, N, seed=seed + 2))


def _gn_partials_case(B, H, W, c0, c1, N):
    def build(ops):
        code, x0, x1, w, wp, bias, resid = _conv_inputs(ops, "s1", B, H, W, c0, c1, N, seed=81)
        wu = ops.pack_conv_weight_wino(w)
        gamma, beta, temb = _gn_params(N, B, 84)
        assert ops.L.load().ddk_conv_gn_partials(B, H, W, c0 + c1, N, 8) == H * W // 128

        def run():
            raw, part, np_ = ops.conv_with_gn_partials(x0, wp, bias, wu, x2=x1)
            out = ops.groupnorm_mish_from_partials(raw, part, np_, gamma, beta, temb=temb, addend=resid)
            return raw, part, out
        return run
    return build


CASES["gn_partials-1-32-16-32-0-64"] = _gn_partials_case(1, 32, 16, 32, 0, 64)
CASES["gn_partials-32-16-16-32-32-256"] = _gn_partials_case(32, 16, 16, 32, 32, 256)


def _first_inputs(ops, B, H, W, cin, N, seed):
    x = dev(to_nhwc(rnd(B, cin, H, W, seed=seed) + 0.3))
    wf = ops.pack_conv_weight_first(rnd(N, cin, 3, 3, seed=seed + 1, scale=(cin * 9) ** -0.5).to(DEV))
    assert ops.L.load().ddk_conv_first_ok(cin, N, H, W, 8)
    return x, wf, rnd(N, seed=seed + 2).to(DEV)


@case("gn_partials_res1x1-2-16-32-5-32")
def _(ops):
    B, H, W, cin, N = 2, 16, 32, 5, 32
    h_in, wf, b3 = _first_inputs(ops, B, H, W, 4, N, 22)
    x = dev(to_nhwc(rnd(B, cin, H, W, seed=21)))
    wr, br = dev(rnd(N, cin, 1, 1, seed=25, scale=cin ** -0.5), rnd(N, seed=26))
    gamma, beta, temb = _gn_params(N, B, 27)

    def run():
        raw, part, tiles = ops.conv_first(h_in, wf, b3, N)
        return raw, part, ops.groupnorm_mish_from_partials_res1x1(raw, part, tiles, gamma, beta, x, wr, br, temb=temb)
    return run


def _step_tables():
    from oracle import diffusion_ref as D
    buf = D.schedule_buffers("linear", 1000)
    tb = {k: buf[v].to(DEV) for k, v in (("c_recip", "sqrt_recip_alphas_cumprod"), ("c_recipm1", "sqrt_recipm1_alphas_cumprod"),
                                         ("c1", "posterior_mean_coef1"), ("c2", "posterior_mean_coef2"))}
    tb["sigma"] = torch.exp(0.5 * buf["posterior_log_variance_clipped"]).to(DEV)
    return tb


def _final_tail_case(B, H, W, C, n_out):
    def build(ops):
        h_in, wf, b3 = _first_inputs(ops, B, H, W, 8, C, 31)
        gamma, beta, _ = _gn_params(C, B, 34)
        w, bf = dev(rnd(n_out, C, 1, 1, seed=36, scale=C ** -0.5), rnd(n_out, seed=37))
        tb = _step_tables()
        x0, z = dev(rnd(B, H, W, n_out, seed=38, scale=1.5), rnd(B, H, W, n_out, seed=39))
        t = torch.tensor([0, 1, 500, 999] * 8)[:B].to(DEV)

        def run():
            raw, part, tiles = ops.conv_first(h_in, wf, b3, C)
            eps = ops.final_tail(raw, part, tiles, gamma, beta, w, bf)
            xa = fresh_copy(x0)
            eps2 = ops.final_tail(raw, part, tiles, gamma, beta, w, bf, x=xa, t=t, tables=tb, noise=z)
            xb = fresh_copy(x0)
            ops.final_tail(raw, part, tiles, gamma, beta, w, bf, x=xb, t=t, tables=tb, seed=0x1234567887654321, stream_id=3, want_eps=False)
            return eps, eps2, xa, xb
        return run
    return build


CASES["final_tail-2-16-16-32-3"] = _final_tail_case(2, 16, 16, 32, 3)
CASES["final_tail-3-16-8-128-3"] = _final_tail_case(3, 16, 8, 128, 3)


def _conv_first_case(B, H, W, cin, N):
    def build(ops):
        x, wf, b = _first_inputs(ops, B, H, W, cin, N, 1 + cin)

        def run():
            raw, part, tiles = ops.conv_first(x, wf, b, N)
            raw2, none, _ = ops.conv_first(x, wf, b, N, partials=False)
            assert none is None and tiles == H * W // 128
            return raw, part, raw2
        return run
    return build


CASES["conv_first-1-8-16-4-64"] = _conv_first_case(1, 8, 16, 4, 64)         # the smallest of FIRST_CASES: one tile
CASES["conv_first-1-16-24-5-160"] = _conv_first_case(1, 16, 24, 5, 160)     # three tiles, N not a multiple of 64


# ================================================================== one-launch conv + GroupNorm + Mish
def _local_case(B, H, W, c0, c1, N, wino):
    def build(ops):
        lib = ops.L.load()
        ok = (lib.ddk_conv3x3_gn_mish_wino_ok if wino else lib.ddk_conv3x3_gn_mish_ok)(H, W, c0 + c1, c0, N, 8)
        assert ok, "the case is meant to be eligible for the one-launch kernel"
        _, x0, x1, w, _, bias, resid = _conv_inputs(ops, "s1", B, H, W, c0, c1, N, seed=71)
        wl = (ops.pack_conv_weight_wino_local if wino else ops.pack_conv_weight_local)(w)
        gamma, beta, temb = _gn_params(N, B, 74)
        fn = ops.conv3x3_gn_mish_wino if wino else ops.conv3x3_gn_mish
        return lambda: (fn(x0, wl, bias, gamma, beta, x2=x1), fn(x0, wl, bias, gamma, beta, temb=temb, addend=resid, x2=x1))
    return build


CASES["gn_local-1-8-2-32-0-64"] = _local_case(1, 8, 2, 32, 0, 64, False)
CASES["gn_local-3-2-8-64-32-64"] = _local_case(3, 2, 8, 64, 32, 64, False)
CASES["gn_wlocal-2-8-8-32-0-64"] = _local_case(2, 8, 8, 32, 0, 64, True)
CASES["gn_wlocal-3-32-2-32-32-64"] = _local_case(3, 32, 2, 32, 32, 64, True)


def _gn_slabs_case(B, H, S, SA):
    def build(ops):
        C = N = 256
        slabs = dev(torch.stack([to_nhwc(rnd(B, C, H, H, seed=300 + k)) for k in range(S)]))
        a_sl = dev(torch.stack([to_nhwc(rnd(B, N, H, H, seed=340 + k)) for k in range(SA)]))
        sbias, abias, bias = dev(rnd(C, seed=320, scale=0.3), rnd(N, seed=350, scale=0.3), rnd(N, seed=322, scale=0.1))
        w = rnd(N, C, 3, 3, seed=321, scale=(C * 9) ** -0.5).to(DEV)
        wp = ops.pack_conv_weight_local(w) if H == 4 else ops.pack_conv_weight_wino_local(w)
        gamma, beta, temb = _gn_params(N, B, 323)
        return lambda: (ops.conv3x3_gn_mish_slabs(slabs, sbias, wp, bias, gamma, beta, temb=temb, addend_slabs=a_sl, addend_bias=abias),
                        ops.conv3x3_gn_mish_slabs(slabs, sbias, wp, bias, gamma, beta, addend_slabs=slabs, addend_bias=sbias))
    return build


CASES["gn_slabs-5-4-3-2"] = _gn_slabs_case(5, 4, 3, 2)
CASES["gn_slabs-3-8-2-4"] = _gn_slabs_case(3, 8, 2, 4)


def _cluster_case(B, H, W, c0, c1, N, split):
    def build(ops):
        lib = ops.L.load()
        cin = c0 + c1
        if lib.ddk_conv3x3_gn_mish_cluster_ok(B, H, W, cin, N, 8) <= 0:
            pytest.skip("shape / device not eligible for the in-launch GroupNorm")
        if split:
            assert lib.ddk_conv_wino_splits(B, H, W, cin, N) > 1 and lib.ddk_conv3x3_gn_mish_cluster_split_workspace_bytes(B, H, W, cin, N, 8) > 0
        else:
            assert lib.ddk_conv3x3_gn_mish_cluster_split_workspace_bytes(B, H, W, cin, N, 8) == 0
        _, x0, x1, w, _, bias, resid = _conv_inputs(ops, "s1", B, H, W, c0, c1, N, seed=41)
        wu = ops.pack_conv_weight_wino(w)
        gamma, beta, temb = _gn_params(N, B, 44)
        before = ops.cluster_timeouts()

        def run():
            a = ops.conv3x3_gn_mish_cluster(x0, wu, bias, gamma, beta, x2=x1, temb=temb, addend=resid)
            b = ops.conv3x3_gn_mish_cluster(x0, wu, bias, gamma, beta, x2=x1)          # the counters re-armed themselves
            torch.cuda.synchronize()
            assert ops.cluster_timeouts() == before, "an in-launch exchange gave up"
            return a, b
        return run
    return build


CASES["gn_cluster-32-16-16-128-0-128-ksplit"] = _cluster_case(32, 16, 16, 128, 0, 128, True)
CASES["gn_cluster-16-32-32-128-0-128"] = _cluster_case(16, 32, 32, 128, 0, 128, False)


# ================================================================== 1x1 kernels
def _ws_case(B, H, W, N, use_bias, use_resid, use_ln):
    def build(ops):
        K = 128
        assert ops.L.load().ddk_conv1x1_ws_ok(B * H * W, K, N)
        x = dev(to_nhwc(rnd(B, K, H, W, seed=11) * 1.5 + 0.4))
        w2 = rnd(N, K, seed=12, scale=K ** -0.5)
        g, be = 1 + 0.2 * rnd(K, seed=15), 0.1 * rnd(K, seed=16)
        ln = dev(w2 @ g, w2 @ be) if use_ln else None
        wd = dev(w2 * g.view(1, K) if use_ln else w2)
        b = dev(rnd(N, seed=13)) if use_bias else None
        r = dev(to_nhwc(rnd(B, N, H, W, seed=14))) if use_resid else None
        return lambda: (ops.conv1x1_ws(x, wd, b, r, ln),)
    return build


CASES["conv1x1_ws-2-32-32-128"] = _ws_case(2, 32, 32, 128, False, True, True)
CASES["conv1x1_ws-5-16-32-128"] = _ws_case(5, 16, 32, 128, False, False, False)


@case("conv1x1_sm-8-8-8-256-0-128")
def _(ops):
    code, x0, x1, _, wp, bias, resid = _conv_inputs(ops, "1x1", 8, 8, 8, 256, 0, 128, seed=41)
    return lambda: (ops.conv(code, x0, wp, bias), ops.conv(code, x0, wp, bias, resid=resid), ops.conv(code, x0, wp, None))


@case("conv1x1_stream-16-32-32-64-32")
def _(ops):
    B, H, W, cin, N = 16, 32, 32, 64, 32
    code, x0, _, _, wp, bias, resid = _conv_inputs(ops, "1x1", B, H, W, cin, 0, N, seed=51)
    src = dev(rnd(B, H, W, N, seed=55))

    def run():
        a_out = torch.empty(B, H, W, N, device=DEV)
        h = ops.conv(code, x0, wp, bias, mish_out=a_out)
        return (h, a_out, ops.conv(code, x0, wp, bias, pre_mish=True, post_mish=True), ops.conv(code, x0, wp, bias, dmish_src=src, resid=resid))
    return run


@case("conv1x1_stream-64-16-16-3-64-padded")
def _(ops):
    x = rnd(64, 3, 16, 16, seed=51).to(DEV)
    wp = ops.pack_conv_weight(rnd(64, 3, 1, 1, seed=52, scale=3 ** -0.5).to(DEV))
    bias = rnd(64, seed=53, scale=0.1).to(DEV)

    def run():
        xd = ops.nchw_to_nhwc(x, 32)               # the padding channels are written by the layout kernel
        return xd, ops.conv(ops.CONV1X1, xd, wp, bias)
    return run


@case("conv1x1_small_n")
def _(ops):
    ins = [(dev(to_nhwc(rnd(2, C, 9, 7, seed=80))), dev(rnd(n, C, 1, 1, seed=81, scale=C ** -0.5)), dev(rnd(n, seed=82)))
           for C, n in ((128, 8), (128, 3), (32, 1), (256, 5))]
    return lambda: tuple(ops.conv1x1_small_n(x, w, b) for x, w, b in ins)


# ================================================================== norms
def _gn_case(B, H, W, C):
    def build(ops):
        x = dev(to_nhwc(rnd(B, C, H, W, seed=30, scale=2.0) + 0.5))
        g, b = dev(1 + 0.1 * rnd(C, seed=31), 0.1 * rnd(C, seed=32))
        tb = rnd(B, C + 8, seed=33).to(DEV)
        add = dev(to_nhwc(rnd(B, C, H, W, seed=34)))
        return lambda: (ops.groupnorm_mish(x, g, b), ops.groupnorm_mish(x, g, b, temb=tb[:, 4:4 + C], addend=add))
    return build


CASES["groupnorm_mish-3-5-7-64"] = _gn_case(3, 5, 7, 64)
CASES["groupnorm_mish-4-4-4-256"] = _gn_case(4, 4, 4, 256)


@case("groupnorm_mish-1-100-90-64-streamed")
def _(ops):
    """72000 elements per group: the streamed path with its statistics workspace (4 splits, the last one ragged)"""
    B, H, W, C = 1, 100, 90, 64
    assert ops.L.load().ddk_groupnorm_workspace_bytes(B, H * W, C, 8) > 0
    return _gn_case(B, H, W, C)(ops)


@case("conv3x3_groupnorm_mish-2-8-8-64-64-fused_reduce")
def _(ops):
    """conv -> GroupNorm with the split-K slabs summed by the GroupNorm's load (ddk_groupnorm_mish_slabs)"""
    B, H, W, cin, N = 2, 8, 8, 64, 64
    code, x0, _, _, wp, bias, resid = _conv_inputs(ops, "s1", B, H, W, cin, 0, N, seed=35)
    gamma, beta, temb = _gn_params(N, B, 38)
    lib = ops.L.load()
    assert lib.ddk_conv_splits(code, B, H, W, cin, N) > 1 and lib.ddk_groupnorm_workspace_bytes(B, H * W, N, 8) == 0
    return lambda: (ops.conv3x3_groupnorm_mish(x0, wp, bias, gamma, beta, temb=temb, addend=resid),)


def _ln_case(C):
    def build(ops):
        x = dev(to_nhwc(rnd(3, C, 6, 5, seed=40, scale=3.0) + 1.0))
        g, b = dev(1 + 0.1 * rnd(1, C, 1, 1, seed=41), 0.1 * rnd(1, C, 1, 1, seed=42))
        return lambda: (ops.chan_layernorm(x, g, b),)
    return build


CASES["chan_layernorm-32"] = _ln_case(32)
CASES["chan_layernorm-512"] = _ln_case(512)


# ================================================================== attention
def _linattn_case(B, H, W, fused_up_to=256):
    def build(ops):
        qkv = dev(to_nhwc(rnd(B, 384, H, W, seed=60, scale=1.5)))
        if fused_up_to < H * W:
            assert ops.L.load().ddk_linattn_context_workspace_bytes(B, H * W, 4) > 0 or H * W <= 256
        return lambda: ops.linattn(qkv, 4, fused_up_to=fused_up_to)
    return build


CASES["linattn-1-10-13"] = _linattn_case(1, 10, 13)
CASES["linattn-2-15-17"] = _linattn_case(2, 15, 17)
CASES["linattn-2-15-17-context_apply"] = _linattn_case(2, 15, 17, fused_up_to=64)
CASES["linattn-2-32-32-pixel_split"] = _linattn_case(2, 32, 32)


def _attn_x(B, H, W, C, shift=0.0):
    x = rnd(B, C, H, W, seed=181) * 1.3 + 0.2
    if shift:
        x = x + shift * torch.linspace(0, 1, H * W).reshape(1, 1, H, W) * rnd(1, C, 1, 1, seed=187)
    wq = rnd(384, C, 1, 1, seed=182, scale=C ** -0.5 * (3.0 if shift else 1.0))
    return dev(to_nhwc(x), wq, 1 + 0.2 * rnd(C, seed=185), 0.1 * rnd(C, seed=186))


def _small_from_x_case(B, H, W, C):
    def build(ops):
        x, wq, g, be = _attn_x(B, H, W, C)
        return lambda: ops.linattn_small_from_x(x, wq, g, be)
    return build


CASES["linattn_small_from_x-2-6-6-96"] = _small_from_x_case(2, 6, 6, 96)
CASES["linattn_small_from_x-2-2-2-64"] = _small_from_x_case(2, 2, 2, 64)


@case("attention_folded-2-32-32")
def _(ops):
    x, wq, g, be = _attn_x(2, 32, 32, 128)
    wo, bo = dev(rnd(128, 128, 1, 1, seed=83, scale=128 ** -0.5), rnd(128, seed=84, scale=0.1))
    return lambda: (ops.attention_folded(x, wq, g, be, wo, bo),)


@case("attention_kv_context-5-16-16")
def _(ops):
    x, wq, g, be = _attn_x(5, 16, 16, 128)
    assert ops.L.load().ddk_attention_kv_context_ok(5, 256, 128, 4)
    return lambda: (ops.attention_kv_context(x, wq, g, be),)


@case("attention_split_from_x-2-8-8-32")
def _(ops):
    """its workspace stays zeroed by contract (torch.zeros inside the wrapper); out and ctx are poisoned"""
    B, H, W, C = 2, 8, 8, 32
    if not ops.L.load().ddk_attention_split_ok(B, H * W, C, 4):
        pytest.skip("shape / device not eligible for the pixel-split attention launch")
    x, wq, g, be = _attn_x(B, H, W, C, shift=30.0)
    before = ops.cluster_timeouts()

    def run():
        out, ctx = ops.attention_split_from_x(x, wq, g, be)
        torch.cuda.synchronize()
        assert ops.cluster_timeouts() == before
        return out, ctx
    return run


# ================================================================== backward convs through ddk.autograd
CONV_BWD = [("s1", 3, 5, 7, 32, 0, 32), ("s1", 2, 8, 8, 64, 64, 64), ("s2", 2, 8, 8, 128, 0, 128), ("1x1", 2, 4, 4, 64, 64, 128),
            ("T", 4, 4, 4, 64, 0, 64),
            ("s1", 3, 8, 8, 128, 0, 64), ("s1", 6, 4, 4, 64, 64, 128),        # halo weight gradient
            ("s1", 136, 8, 8, 32, 0, 32)]                                    # narrow halo weight gradient


def _conv_bwd_case(kind, B, H, W, c0, c1, N, deferred=False):
    def build(ops):
        from ddk import autograd as AG
        code, x0, x1, w, _, bias, resid = _conv_inputs(ops, kind, B, H, W, c0, c1, N)
        dy = resid          # the output's shape

        def run():
            a0 = x0.clone().requires_grad_(True)
            a1 = x1.clone().requires_grad_(True) if x1 is not None else None
            wd, bd = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            if deferred:       # the trainers' accumulation block: gradients land in pre-existing `.grad` slots, reduces wait for the end
                wd.grad, bd.grad = torch.ones_like(wd), torch.full_like(bd, 2.0)
            with (ops.deferred_wgrad() if deferred else contextlib.nullcontext()):
                out = AG.conv(code, a0, wd, bd, x2=a1)
                out.backward(dy)
            return out.detach(), a0.grad, None if a1 is None else a1.grad, wd.grad, bd.grad
        return run
    return build


for _c in CONV_BWD:
    CASES[f"conv_bwd-{'-'.join(map(str, _c))}"] = _conv_bwd_case(*_c)
CASES["conv_bwd-s1-3-16-16-64-0-32-deferred_wgrad"] = _conv_bwd_case("s1", 3, 16, 16, 64, 0, 32, deferred=True)
CASES["conv_bwd-s1-2-8-8-64-64-64-deferred_wgrad"] = _conv_bwd_case("s1", 2, 8, 8, 64, 64, 64, deferred=True)


# ================================================================== other backward kernels
def _gn_train_case(B, H, W, C, drop):
    def build(ops):
        x = dev(to_nhwc(rnd(B, C, H, W, seed=10, scale=2.0) + 0.3))
        g, b, temb = _gn_params(C, B, 11)
        add, dy = dev(to_nhwc(rnd(B, C, H, W, seed=14)), to_nhwc(rnd(B, C, H, W, seed=15)))
        assert ops.gn_train_resident(B, H * W, C)

        def run():
            y = ops.groupnorm_mish_train(x, g, b, temb=temb, addend=add, drop_p=drop, seed=7, layer=3)
            dx, dtemb, sums = ops.groupnorm_mish_bwd(x, g, b, dy, drop, 7, 3)
            acc = tuple(torch.full((C,), 0.5, device=DEV) for _ in range(3))
            dx2, dtemb2, none = ops.groupnorm_mish_bwd(x, g, b, dy, drop, 7, 3, acc=acc)
            assert none == [None, None, None]
            return (y, dx, dtemb, *sums, dx2, dtemb2, *acc)
        return run
    return build


CASES["groupnorm_train-3-4-4-256"] = _gn_train_case(3, 4, 4, 256, 0.0)
CASES["groupnorm_train-3-4-4-256-dropout"] = _gn_train_case(3, 4, 4, 256, 0.1)


@case("groupnorm_train-1-100-90-64-streamed")
def _(ops):
    """a group slab too large for registers: the streamed training kernels and their cached statistics workspace"""
    B, H, W, C = 1, 100, 90, 64
    x = dev(to_nhwc(rnd(B, C, H, W, seed=10, scale=2.0) + 0.3))
    g, b, temb = _gn_params(C, B, 11)
    dy = dev(to_nhwc(rnd(B, C, H, W, seed=15)))
    assert not ops.gn_train_resident(B, H * W, C)

    def run():
        y = ops.groupnorm_mish_train(x, g, b, temb=temb, drop_p=0.1, seed=7, layer=3)
        dx, dtemb, sums = ops.groupnorm_mish_bwd(x, g, b, dy, 0.1, 7, 3)
        return (y, dx, dtemb, *sums)
    return run


def _gn_train_slabs_case(B, H, W, C, S):
    def build(ops):
        gen = torch.Generator().manual_seed(5)
        slabs = torch.randn(S, B, H, W, C, generator=gen).to(DEV)
        bias, gamma, beta = (torch.randn(C, generator=gen).to(DEV) for _ in range(3))
        temb = torch.randn(B, C, generator=gen).to(DEV)
        x = (slabs.sum(0) + bias).contiguous()

        def run():
            res = []
            for drop in (0.0, 0.1):
                raw = torch.empty_like(x)
                y = ops.groupnorm_mish_train(raw, gamma, beta, temb=temb, drop_p=drop, seed=7, layer=3, slabs=slabs, conv_bias=bias)
                dx, dt, sums = ops.groupnorm_mish_bwd(x, gamma, beta, slabs[0], drop, 7, 3, dy_slabs=slabs)
                res += [raw, y, dx, dt, *sums]
            return tuple(res)
        return run
    return build


CASES["groupnorm_train_slabs-64-2-2-256-8"] = _gn_train_slabs_case(64, 2, 2, 256, 8)
CASES["groupnorm_train_slabs-3-8-8-256-4"] = _gn_train_slabs_case(3, 8, 8, 256, 4)


def _ln_bwd_case(C):
    def build(ops):
        x = dev(to_nhwc(rnd(3, C, 6, 5, seed=30, scale=2.0) + 0.5))
        g = dev(1 + 0.1 * rnd(1, C, 1, 1, seed=31))
        dy, extra = dev(to_nhwc(rnd(3, C, 6, 5, seed=32)), to_nhwc(rnd(3, C, 6, 5, seed=33)))

        def run():
            dx, dg, db = ops.chan_layernorm_bwd(x, g, dy)
            acc = (torch.full((C,), -1.0, device=DEV), torch.full((C,), 2.0, device=DEV))
            dx2, _, _ = ops.chan_layernorm_bwd(x, g, dy, acc=acc, addend=extra)
            return dx, dg, db, dx2, *acc
        return run
    return build


CASES["chan_layernorm_bwd-32"] = _ln_bwd_case(32)
CASES["chan_layernorm_bwd-256"] = _ln_bwd_case(256)


def _linattn_bwd_case(B, H, W):
    def build(ops):
        qkv = dev(to_nhwc(rnd(B, 384, H, W, seed=40, scale=1.2)))
        dout = dev(to_nhwc(rnd(B, 128, H, W, seed=41)))

        def run():
            out, ctx, stats = ops.linattn_train(qkv, 4)
            return out, ctx, stats, ops.linattn_bwd(qkv, dout, ctx, stats, 4), ops.linattn_bwd(qkv, dout, ctx, None, 4)
        return run
    return build


CASES["linattn_bwd-1-10-13"] = _linattn_bwd_case(1, 10, 13)
CASES["linattn_bwd-1-64-64-pixel_split"] = _linattn_bwd_case(1, 64, 64)


@case("time_embed_fwd_bwd")
def _(ops):
    from ddk import autograd as AG
    from ddk.plan import sinusoidal_freqs
    dim = 32
    t = torch.tensor([0, 3, 250, 731, 999]).to(DEV)
    flat = [rnd(4 * dim, dim, seed=60, scale=dim ** -0.5), rnd(4 * dim, seed=61, scale=0.1), rnd(dim, 4 * dim, seed=62, scale=(4 * dim) ** -0.5),
            rnd(dim, seed=63, scale=0.1)]
    for i, co in enumerate((32, 64, 64)):
        flat += [rnd(co, dim, seed=64 + i, scale=dim ** -0.5), rnd(co, seed=70 + i, scale=0.1)]
    flat = [p.to(DEV) for p in flat]
    freqs = sinusoidal_freqs(dim).to(DEV)
    go = rnd(5, 160, seed=999).to(DEV)

    def run():
        leaves = [p.clone().requires_grad_(True) for p in flat]
        out = torch.cat(AG.TimeEmbedFn.apply(t, freqs, *leaves), dim=1)
        out.backward(go)
        return (out.detach(), *[p.grad for p in leaves])
    return run


def _small_gemm_case(mode, M, N, K):
    def build(ops):
        a = dev(rnd(K, M, seed=51) if mode == 2 else rnd(M, K, seed=51))
        b = dev(rnd(N, K, seed=52) if mode == 1 else rnd(K, N, seed=52))

        def run():
            out = torch.empty(M, N, device=DEV)
            ops.small_gemm(mode, a, b, out, M, N, K, a.shape[1], b.shape[1], N)
            acc = torch.ones(M, N, device=DEV)
            ops.small_gemm(mode, a, b, acc, M, N, K, a.shape[1], b.shape[1], N, accumulate=True)
            return out, acc
        return run
    return build


CASES["small_gemm-0-8-32-1000"] = _small_gemm_case(0, 8, 32, 1000)
CASES["small_gemm-0-64-128-4096"] = _small_gemm_case(0, 64, 128, 4096)
CASES["small_gemm-2-96-64-64"] = _small_gemm_case(2, 96, 64, 64)


def _small_n_bwd_case(C, n_out):
    def build(ops):
        from ddk import autograd as AG
        a, w, b = dev(to_nhwc(rnd(2, C, 9, 7, seed=50)), rnd(n_out, C, 1, 1, seed=51, scale=C ** -0.5), rnd(n_out, seed=52))
        go = dev(to_nhwc(rnd(2, n_out, 9, 7, seed=999)))

        def run():
            ad, wd, bd = (t.clone().requires_grad_(True) for t in (a, w, b))
            out = AG.SmallNConvFn.apply(ad, wd, bd)
            out.backward(go)
            return out.detach(), ad.grad, wd.grad, bd.grad
        return run
    return build


CASES["small_n_conv_bwd-32-1"] = _small_n_bwd_case(32, 1)
CASES["small_n_conv_bwd-128-3"] = _small_n_bwd_case(128, 3)


@case("groupnorm_generic-3-4-4-40")
def _(ops):
    B, H, W, C = 3, 4, 4, 40
    CP = ops.pad32(C)

    def pad(t):
        out = torch.zeros((*t.shape[:-1], CP))
        out[..., :C] = t
        return out.to(DEV)
    x, add, dy = pad(rnd(B, H, W, C, seed=1) * 1.3 + 0.2), pad(rnd(B, H, W, C, seed=2)), pad(rnd(B, H, W, C, seed=3))
    g, b, temb = _gn_params(C, B, 4)

    def run():
        res = []
        for drop in (0.0, 0.25):
            y = ops.groupnorm_mish_generic_train(x, g, b, temb=temb, addend=add, drop_p=drop, seed=1234, layer=7)
            dx, dtemb, sums = ops.groupnorm_mish_generic_bwd(x, g, b, dy, drop, 1234, 7)
            res += [y, dx, dtemb, sums]
        return tuple(res)
    return run


@case("chan_layernorm_generic-33-40")
def _(ops):
    M, C = 33, 40
    CP = ops.pad32(C)
    xp, dyp, exp_ = torch.zeros((1, M, 1, CP)), torch.zeros((1, M, 1, CP)), torch.zeros((1, M, 1, CP))
    xp[..., :C], dyp[..., :C], exp_[..., :C] = rnd(1, M, 1, C, seed=1) * 0.9 + 0.5, rnd(1, M, 1, C, seed=2), rnd(1, M, 1, C, seed=3)
    x, dy, extra = dev(xp, dyp, exp_)
    g, b = dev(1 + 0.2 * rnd(1, C, 1, 1, seed=4), 0.2 * rnd(1, C, 1, 1, seed=5))
    return lambda: (ops.chan_layernorm_generic(x, g, b), *ops.chan_layernorm_generic_bwd(x, g, dy), *ops.chan_layernorm_generic_bwd(x, g, dy, addend=extra))


@case("bias_grad")
def _(ops):
    dys = [dev(rnd(3, 5, 7, 64, seed=1)), dev(rnd(2, 16, 16, 384, seed=2)), dev(rnd(1, 1, 3, 32, seed=3))]

    def run():
        res = [ops.bias_grad(dy) for dy in dys]
        acc = torch.full((64,), 0.5, device=DEV)
        ops.bias_grad(dys[0], accumulate_into=acc)
        return (*res, acc)
    return run


@case("grad_norm_clip_adam-100003")
def _(ops):
    n = 100003
    p0, g = dev(rnd(n, seed=80), rnd(n, seed=81, scale=3.0))

    def run():
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        nc = ops.grad_norm_clip(g, 1.0)
        for step in (1, 2):
            ops.adam_step_(p, g, m, v, 2e-4, step, clip=nc)
        return nc, p, m, v
    return run


@case("elementwise_and_layout")
def _(ops):
    x, y = dev(to_nhwc(rnd(2, 64, 8, 12, seed=50)), to_nhwc(rnd(2, 64, 8, 12, seed=51)))
    small = rnd(3, 5, 6, 7, seed=90).to(DEV)
    scale = rnd(2, seed=52).to(DEV)
    return lambda: (ops.mish(x), ops.tanh(x), ops.add(x, y), ops.avgpool2(x), ops.upsample_nearest2(x), ops.mish_bwd(x, y), ops.tanh_bwd(x, y),
                    ops.avgpool2_bwd(x), ops.upsample_nearest2_bwd(x), ops.nchw_to_nhwc(small, 32), ops.nhwc_to_nchw(ops.nchw_to_nhwc(small, 32), 5),
                    ops.pad_channels(to_nhwc(small).contiguous(), 32), ops.zero_stuff2(x, 16, 24), ops.scale_per_sample(x, scale),
                    ops.sq_err_grad(x, y, scale), ops.fix_samples(small), ops.randn((4099,), DEV, seed=42, step=7, stream_id=1))


# ================================================================== weight packing: the padding of every kernel layout is the pack kernel's to write
@case("pack_weights-ragged_channels")
def _(ops):
    """input-channel counts that are no multiple of 32 (and, for conv_first, an odd 9 * C_in): the operand's padding rows are read by
    the conv kernels against zero-padded activations, so they must be written (as zeros), not left as they were allocated"""
    w3, w5, w40 = dev(rnd(64, 3, 3, 3, seed=1), rnd(32, 5, 3, 3, seed=2), rnd(64, 40, 3, 3, seed=3))
    w1x1, wT, wT3 = dev(rnd(96, 72, 1, 1, seed=4), rnd(40, 128, 4, 4, seed=5), rnd(3, 32, 4, 4, seed=6))
    w7 = dev(rnd(32, 7, 3, 3, seed=7))
    wd = dev(rnd(40, 64, 3, 3, seed=8))
    assert ops.L.load().ddk_conv_wino_splits(2, 4, 4, 64, 64) > 0

    def run():
        return (ops.pack_conv_weight(w3), ops.pack_conv_weight(w40), ops.pack_conv_weight(w1x1), ops.pack_convT_weight(wT), ops.pack_convT_weight(wT3),
                ops.pack_conv_weight_wino(w3), ops.pack_conv_weight_wino(w40), ops.pack_convT_weight_wino(wT), ops.pack_conv_weight_local(w40),
                ops.pack_conv_weight_wino_local(w40), ops.pack_conv_weight_first(w3), ops.pack_conv_weight_first(w5), ops.pack_conv_weight_first(w7),
                ops.pack_conv_weight_dgrad(w3, i_pad=32), ops.pack_conv_weight_dgrad(w40, i_pad=64, o_pad=96),
                ops.wino_weight(wd.clone(), (2, 4, 4, 64), 0, 64, dgrad=True))        # (a clone: the cache keys on the tensor, so it packs again)
    return run


@case("time_embedding_and_objective")
def _(ops):
    from ddk.plan import sinusoidal_freqs
    dim = 32
    t = torch.tensor([0, 1, 17, 500, 999, 3, 3, 250, 731]).to(DEV)
    w1t, b1 = dev(rnd(dim, 4 * dim, seed=70, scale=dim ** -0.5), rnd(4 * dim, seed=71, scale=0.1))
    w2t, b2 = dev(rnd(4 * dim, dim, seed=72, scale=(4 * dim) ** -0.5), rnd(dim, seed=73, scale=0.1))
    wpt, bp = dev(rnd(dim, 200, seed=74, scale=dim ** -0.5), rnd(200, seed=75, scale=0.1))
    freqs = sinusoidal_freqs(dim).to(DEV)
    l1, l2, g = dev(rnd(9, seed=76).abs(), rnd(9, seed=77).abs(), rnd(1, seed=78))
    y0 = dev(rnd(9, 200, seed=79))

    def run():
        act, raw = ops.time_mlp(t, freqs, w1t, b1, w2t, b2)
        y = fresh_copy(y0)
        return (act, raw, ops.time_proj(act, wpt, bp), ops.sincos_embed(t, freqs), ops.bias_act_(y, bp, True), y, ops.ae_objective(l1, l2, t, 100),
                *ops.ae_objective_bwd(g, t, 100), ops.rows_sum(y0, 9, 200, 200))
    return run


# ================================================================== resampler ops
@case("bicubic_resize_and_grad")
def _(ops):
    ins = [(syn.synthetic_normal((B, C, i, i), f"poison.bic.x.{i}.{o}").to(DEV), syn.synthetic_normal((B, C, o, o), f"poison.bic.dy.{i}.{o}").to(DEV), i, o)
           for B, C, i, o in ((2, 3, 24, 6), (5, 3, 4, 32), (1, 1, 2, 1))]
    return lambda: tuple(t for x, dy, i, o in ins for t in (ops.bicubic_resize(x, (o, o)), ops.bicubic_resize_grad(dy, (i, i))))


def _small_conv_case(transpose, H, W):
    def build(ops):
        B, cin, cout = 3, 3, 8
        x = rnd(B, cin, H, W, seed=1).to(DEV)
        b = rnd(cout, seed=3, scale=0.1).to(DEV)
        if transpose:
            w, dy = dev(rnd(cin, cout, 4, 4, seed=2, scale=(4 * cin) ** -0.5), rnd(B, cout, 2 * H, 2 * W, seed=4))
            return lambda: (ops.convt_small_s2(x, w, b), ops.convt_small_s2_dgrad(dy, w), *ops.convt_small_s2_wgrad(x, dy))
        w, dy = dev(rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5), rnd(B, cout, (H + 1) // 2, (W + 1) // 2, seed=4))
        return lambda: (ops.conv_small_s2(x, w, b), ops.conv_small_s2_dgrad(dy, w, (H, W)), *ops.conv_small_s2_wgrad(x, dy))
    return build


for _h, _w in ((7, 5), (1, 1)):
    CASES[f"conv_small_s2-{_h}-{_w}"] = _small_conv_case(False, _h, _w)
    CASES[f"convt_small_s2-{_h}-{_w}"] = _small_conv_case(True, _h, _w)


# ================================================================== losses, metrics, operators
@case("vlb_terms-3")
def _(ops):
    from oracle import diffusion_ref as D
    buf = D.schedule_buffers("linear", 1000)
    B = 3
    x = syn.synthetic_input((B, 3, 16, 16), "poison.vlb.x").clamp(-1, 1)
    eps = syn.synthetic_normal((B, 3, 16, 16), "poison.vlb.eps")
    eps_hat = eps + 0.3 * syn.synthetic_normal((B, 3, 16, 16), "poison.vlb.d")
    t = torch.tensor([0, 17, 999])
    x_t = D.q_sample(buf, x, t, eps)
    dv = {k: v.to(DEV) for k, v in buf.items()}
    tabs = (dv["sqrt_recip_alphas_cumprod"], dv["sqrt_recipm1_alphas_cumprod"], dv["posterior_mean_coef1"], dv["posterior_mean_coef2"],
            dv["posterior_log_variance_clipped"])
    xd, xtd, ehd, ed, td = dev(x, x_t, eps_hat, eps, t)
    assert ops.L.load().ddk_vlb_terms_workspace_bytes(B, 3 * 16 * 16) > B * 4       # counters + partials

    def run():
        vlb, sq = ops.vlb_terms(xd, xtd, ehd, td, *tabs, eps=ed)
        vlb2, none = ops.vlb_terms(xd, xtd, ehd, td, *tabs)             # the counters re-armed themselves
        assert none is None
        return vlb, sq, vlb2
    return run


@case("sq_err_sum_q_sample")
def _(ops):
    from oracle import diffusion_ref as D
    buf = D.schedule_buffers("linear", 1000)
    a, b = dev(rnd(4, 8, 32, 32, seed=120), rnd(4, 8, 32, 32, seed=121))
    t = torch.tensor([0, 1, 499, 999]).to(DEV)
    sa, sb = buf["sqrt_alphas_cumprod"].to(DEV), buf["sqrt_one_minus_alphas_cumprod"].to(DEV)
    return lambda: (ops.sq_err_sum(a, b), ops.q_sample(a, b, t, sa, sb))


@case("image_metrics")
def _(ops):
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 256, (3, 13, 17, 3), generator=g, dtype=torch.uint8).to(DEV)
    b = torch.randint(0, 256, (3, 13, 17, 3), generator=g, dtype=torch.uint8).to(DEV)
    mask = (torch.rand(3, 13, 17, generator=g) > 0.5).to(DEV)
    keys = ("psnr", "ssim", "mse", "sq_sum", "count")

    def run():
        plain, masked = ops.image_metrics(a, b), ops.image_metrics(a, b, mask)
        return tuple(r[k] for r in (plain, masked) for k in keys)
    return run


def _manifold_radii_case(N, D, splits):
    def build(ops):
        x = rnd(N, D, seed=7).to(DEV)
        assert ops.manifold_radii_splits(N) == splits
        return lambda: (ops.manifold_radii(x, 3), ops.manifold_radii(x, 7))
    return build


CASES["manifold_radii-150-24"] = _manifold_radii_case(150, 24, 2)        # two column ranges per row block
CASES["manifold_radii-90-24"] = _manifold_radii_case(90, 24, 1)


@case("manifold_members-150-90")
def _(ops):
    a, b = dev(rnd(150, 24, seed=7), rnd(90, 24, seed=8))
    ra, rb = dev(rnd(150, seed=9).abs() * 10 + 20, rnd(90, seed=10).abs() * 10 + 20)

    def run():
        a_in, b_in = ops.manifold_members(a, ra, b, rb)
        only_a, none = ops.manifold_members(a, None, b, rb)
        assert none is None
        return a_in, b_in, only_a
    return run


def _perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(DEV)


def _hadamard_case(B, H, W, C, m):
    def build(ops):
        x = dev(rnd(B, H, W, C, seed=1))
        perm = _perm(H * W, 2)

        def run():
            y = ops.hadamard_measure(x, perm, m)
            return y, ops.hadamard_adjoint(y, perm, H, W)
        return run
    return build


CASES["hadamard-3-16-16-3-m64"] = _hadamard_case(3, 16, 16, 3, 64)
CASES["hadamard-1-256-256-2-scratch"] = _hadamard_case(1, 256, 256, 2, 1024)      # the plane does not fit in LDS: through the scratch image


def _circular_conv_case(B, H, W, C):
    def build(ops):
        x, S = dev(rnd(B, H, W, C, seed=1), rnd(H, W, 2, seed=2, scale=0.5))
        return lambda: (ops.circular_conv(x, S),)
    return build


CASES["circular_conv-3-16-16-3"] = _circular_conv_case(3, 16, 16, 3)
CASES["circular_conv-2-128-256-1-scratch"] = _circular_conv_case(2, 128, 256, 1)  # above 16384 pixels: the complex scratch


@case("separable_apply")
def _(ops):
    x = dev(rnd(2, 16, 32, 3, seed=1))
    Lm, Rm = dev(rnd(16, 16, seed=2, scale=0.25), rnd(32, 32, seed=3, scale=0.2))
    Lr, Rr = dev(rnd(8, 16, seed=4, scale=0.25), rnd(12, 32, seed=5, scale=0.2))
    Lu, Ru = dev(rnd(40, 16, seed=6, scale=0.25), rnd(36, 32, seed=7, scale=0.2))
    return lambda: (ops.separable_apply(x, Lm, Rm), ops.separable_apply_rect(x, Lr, Rr), ops.separable_apply_rect(x, Lu, Ru))


def _restore_step_case(kind, B, H, W, C):
    """one in-place DDNM step on a working copy that came from torch.empty; the larger shape of each kind goes through the
    wrapper's scratch image"""
    def build(ops):
        tb = _step_tables()
        x0, e = dev(rnd(B, H, W, C, seed=1, scale=1.5), rnd(B, H, W, C, seed=2))
        t = torch.tensor([0, 500, 999])[:B].to(DEV)
        if kind == "blur":
            P_h, P_w, Yp = dev(rnd(H, H, seed=3, scale=H ** -0.5), rnd(W, W, seed=4, scale=W ** -0.5), rnd(B, H, W, C, seed=5, scale=0.3))
            step = lambda x: ops.p_sample_update_restore_blur_(x, e, P_h, P_w, Yp, t, **tb, seed=9, stream_id=2)
        elif kind == "cs":
            m = H * W // 4
            y, perm = dev(rnd(B, C, m, seed=3)), _perm(H * W, 4)
            step = lambda x: ops.p_sample_update_restore_cs_(x, e, y, perm, t, **tb, seed=9, stream_id=2)
        else:
            mask = (torch.rand(H, W, generator=torch.Generator().manual_seed(3)) > 0.5).float().to(DEV)
            Yp = dev(rnd(B, H, W, C, seed=5, scale=0.3))
            step = lambda x: ops.p_sample_update_restore_fft_(x, e, mask, Yp, t, **tb, seed=9, stream_id=2)
        return lambda: (step(fresh_copy(x0)),)
    return build


CASES["restore_blur_step-3-16-16-3"] = _restore_step_case("blur", 3, 16, 16, 3)
CASES["restore_blur_step-2-128-128-3-scratch"] = _restore_step_case("blur", 2, 128, 128, 3)
CASES["restore_cs_step-3-16-16-3"] = _restore_step_case("cs", 3, 16, 16, 3)
CASES["restore_cs_step-1-256-256-3-scratch"] = _restore_step_case("cs", 1, 256, 256, 3)
CASES["restore_fft_step-3-16-16-3"] = _restore_step_case("fft", 3, 16, 16, 3)
CASES["restore_fft_step-2-128-256-1-scratch"] = _restore_step_case("fft", 2, 128, 256, 1)


# ================================================================== whole plans, each built inside the poisoned block
def _state(cfg, cls_name="DDPM"):
    """the deterministic weights of a model of this config, made once on the host"""
    import models
    from models import Unet
    m = getattr(models, cls_name)(cfg, Unet(cfg), "cpu", cfg["unet_in"] if cls_name == "DDPM" else 3)
    return {k: (v.clone() if k in syn.SCHEDULE_KEYS else syn.fill_tensor(k, v.shape)) for k, v in m.state_dict().items()}


def _fresh(cfg, sd, cls_name="DDPM", train=False):
    """a new model, hence a new native plan whose workspaces are allocated by the run that follows"""
    import models
    from models import Unet
    m = getattr(models, cls_name)(cfg, Unet(cfg), DEV, cfg["unet_in"] if cls_name == "DDPM" else 3)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


TINY = ddpm_cfg(32, 3, 16)


def _tiny_forward_case(B):
    def build(ops):
        sd = _state(TINY)
        x = syn.synthetic_normal((B, 3, 16, 16), f"poison.fwd.x{B}").to(DEV)
        t = torch.tensor([10, 900, 0, 999, 431])[:B].to(DEV)

        def run():
            m = _fresh(TINY, sd)
            with torch.no_grad():
                return m.latent_model(x, t), m.latent_model(x, t)        # the second forward reuses the (now written) workspace
        return run
    return build


CASES["plan-tiny-forward-B2"] = _tiny_forward_case(2)
CASES["plan-tiny-forward-B5"] = _tiny_forward_case(5)


def _tiny_chain_case(what, graph=True):
    def build(ops):
        sd = _state(TINY)
        shape = (2, 3, 16, 16)
        x_T = syn.synthetic_normal(shape, "poison.chain.xT")
        img = syn.synthetic_input(shape, "poison.chain.img").clamp(-1, 1)
        mask = (torch.rand(16, 16, generator=torch.Generator().manual_seed(1)) > 0.4).float()
        mask8 = (torch.rand(8, 8, generator=torch.Generator().manual_seed(2)) > 0.3).float()
        y8 = torch.nn.functional.avg_pool2d(img, 2)

        def run():
            m = _fresh(TINY, sd)
            m.use_graph = graph
            if what == "ancestral":
                return (m.p_sample_loop(shape, early_stop=997, x_T=x_T, seed=11), m.p_sample_loop(shape, early_stop=997, x_T=x_T, seed=11))
            if what == "dpm":
                return (m.p_sample_loop(shape, x_T=x_T, respacing="logsnr3", solver="dpm++2m"),)
            if what == "repaint":
                return (m.inpaint(img.to(DEV), mask.to(DEV), respacing="4", jump_length=2, jump_n_sample=2, x_T=x_T, seed=11),)
            if what == "ddnm":
                return (m.restore(y8.to(DEV), mask8, 2, respacing="3", x_T=x_T, seed=11),)
            raise AssertionError(what)
        return run
    return build


CASES["plan-tiny-chain3-graph"] = _tiny_chain_case("ancestral", graph=True)
CASES["plan-tiny-chain3-eager"] = _tiny_chain_case("ancestral", graph=False)
CASES["plan-tiny-dpm_solver-3"] = _tiny_chain_case("dpm")
CASES["plan-tiny-repaint"] = _tiny_chain_case("repaint")
CASES["plan-tiny-ddnm"] = _tiny_chain_case("ddnm")


@case("plan-tiny-likelihood_sweep-T3")
def _(ops):
    cfg = ddpm_cfg(32, 3, 16, T=3, schedule="cosine")       # (the linear schedule's betas leave (0, 1] below T = 20)
    sd = _state(cfg)
    x = syn.synthetic_input((2, 3, 16, 16), "poison.sweep.x").clamp(-1, 1).to(DEV)
    keys = ("vlb_t", "prior", "vlb", "L_simple_t", "L_simple")

    def run():
        res = _fresh(cfg, sd).test_losses(x, seed=5)
        return tuple(res[k] for k in keys)
    return run


@case("plan-cfg4-B32-2steps")
def _(ops):
    """the benchmark's shape: the level chain, the in-launch GroupNorm and the counters inside the sampler workspace.  A poisoned
    counter word that the launch sequence does not re-zero shows up as a give-up and rerun, not as a wrong image: so the option, the
    give-up count and the warnings are asserted as well."""
    cfg = ddpm_cfg(128, 8, 32)
    sd = _state(cfg)
    shape = (32, 8, 32, 32)
    x_T = syn.synthetic_normal(shape, "poison.cfg4.xT")

    def run():
        m = _fresh(cfg, sd)
        before = ops.cluster_timeouts()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = m.p_sample_loop(shape, early_stop=998, x_T=x_T, seed=21)
            torch.cuda.synchronize()
        plan = m.latent_model.plan()
        assert plan._cluster == 1, "the in-launch GroupNorm was switched off (an exchange gave up)"
        assert ops.cluster_timeouts() == before
        assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
        return (out,)
    return run


def _train_case(tag):
    def build(ops):
        cls = "DDPM" if tag == "ddpm" else "DownsampleDDPMAutoencoder"
        cfg = ddpm_cfg(32, 3, 16) if tag == "ddpm" else dddpm_cfg(32, 32, 2)
        xshape, eshape = ((4, 3, 16, 16), (4, 3, 16, 16)) if tag == "ddpm" else ((4, 3, 32, 32), (4, 8, 8, 8))
        sd = _state(cfg, cls)
        x = syn.synthetic_input(xshape, f"poison.train.{tag}.x").to(DEV)
        eps = syn.synthetic_normal(eshape, f"poison.train.{tag}.eps").to(DEV)
        tt = torch.tensor([0, 40, 500, 999], device=DEV)

        def run():
            model = _fresh(cfg, sd, cls, train=True)
            model.t_sample = lambda n: tt
            orig = torch.randn_like
            torch.randn_like = lambda z: eps
            try:
                for p in model.parameters():
                    p.grad = torch.zeros_like(p)
                with ops.deferred_wgrad():           # as the trainers run a step: `.grad` slots, reduces at the end of the pass
                    res = model(x)
                    obj = res[0] if isinstance(res, tuple) else res
                    obj.backward()
                torch.cuda.synchronize()
            finally:
                torch.randn_like = orig
            return (obj.detach(), *[p.grad for p in model.parameters()])
        return run
    return build


CASES["train_step-ddpm"] = _train_case("ddpm")
CASES["train_step-dddpm_ae"] = _train_case("dddpm_ae")


# ================================================================== the one check, over the whole table
@pytest.mark.parametrize("name", list(CASES))
def test_results_do_not_depend_on_buffer_contents(ops, name):
    built = CASES[name](ops)
    c = built if isinstance(built, Case) else Case(built)
    plain, again = _snap(c.run()), _snap(c.run())
    reproducible = _same(plain, again)
    if not reproducible:
        assert name in NOT_BIT_REPRODUCIBLE, f"{name}: two plain runs differ ({_first_difference(plain, again)}) and it is not listed"
        assert c.ref is not None and c.bar is not None, f"{name}: listed as not bit-reproducible but has no reference / bar"
    for t in plain:
        assert t is None or not t.is_floating_point() or bool(torch.isfinite(t).all()), f"{name}: plain run is not finite"
    for word in WORDS:
        repoison(word)
        with poisoned_allocations(word) as p:
            got = _snap(c.run())
        assert p.count > 0, f"{name}: nothing was allocated through torch.empty / empty_like / new_empty"
        for t in got:
            assert t is None or not t.is_floating_point() or bool(torch.isfinite(t).all()), f"{name}: not finite under {word:#010x}"
        if reproducible:
            assert _same(plain, got), f"{name}: result depends on buffer contents (word {word:#010x}): {_first_difference(plain, got)}"
        else:
            for g, r in zip(got, c.ref()):
                assert g is None or rel_err(g, r) < c.bar, f"{name}: off its reference under {word:#010x}"


# ================================================================== the harness itself, on the device
@pytest.mark.parametrize("word", WORDS)
def test_the_check_sees_an_unwritten_buffer(ops, word):
    """conv(leave_slabs=True) leaves `out` unwritten by contract when the launch splits k: under poison it holds the word in every
    element (it was allocated through a patched path, and no kernel stored to it), so a consumer that read it would fail the check
    above; and repoison() reaches the cached scratch of ops._ws."""
    code, x0, _, _, wp, bias, _ = _conv_inputs(ops, "s1", 2, 8, 8, 64, 0, 64)
    with poisoned_allocations(word) as p:
        out, slabs = ops.conv(code, x0, wp, bias, leave_slabs=True)
        torch.cuda.synchronize()
    assert slabs is not None and p.count >= 2 and p.bytes >= out.numel() * 4 + slabs.numel() * 4
    want = word - (1 << 32) if word >> 31 else word
    assert bool((out.view(torch.int32) == want).all())
    assert not bool((slabs.view(torch.int32) == want).all())
    ops.grad_norm_clip(torch.ones(1000, device=DEV), 1.0)          # makes sure a cached scratch exists
    assert repoison(word) >= 1
    assert all(bool((buf.view(torch.int32) == want).all()) for buf in ops._scratch.values())
    with poisoned_allocations(word) as p, torch.cuda.graph(torch.cuda.CUDAGraph()):
        torch.empty(64, device=DEV).fill_(2.0)                     # not poisoned (and not counted) while a stream is capturing
    assert p.count == 0
