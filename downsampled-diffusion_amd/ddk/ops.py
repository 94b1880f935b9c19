"""NHWC functional wrappers over the C ABI: one Python function per HIP kernel family.

Tensors are fp32, contiguous, on a ROCm device; activations are [B, H, W, C].  torch is used
only to allocate outputs / workspaces and to supply the current stream.
"""
import ctypes as C
import math

import torch

from . import lib as L

CONV3X3_S1, CONV3X3_S2, CONV1X1, CONVT4X4_S2 = 0, 1, 2, 3
GN_GROUPS, GN_EPS, LN_EPS = 8, 1e-5, 1e-5


def pad32(c):
    return (c + 31) // 32 * 32


# ---------------------------------------------------------------- kernel-layout copies of weights (training path)
# The autograd Functions need a canonical weight in kernel layout for every conv forward / input-gradient.  Within one optimiser
# step the weights do not change between the accumulation micro-batches, so the copies are cached per live parameter and marked
# with the state they are current for: the parameter's torch version counter + an epoch that every in-place weight update done by
# OUR kernels bumps (FusedAdam.step, EMA, load_state_dict paths call weights_changed(); torch ops bump the version counter).
# A stale copy is not thrown away: its buffer is refreshed in place, and the first stale hit after a weight update refreshes EVERY
# registered copy with one launch (ddk_pack_jobs: 285 single-tensor pack launches per cfg3 optimiser step before).
class _PackEntry:
    __slots__ = ("wref", "out", "job", "fresh", "pooled")


_pack_cache = {}              # (tag, data_ptr, shape) -> _PackEntry
_weights_epoch = [0]
_pack_table = {}              # "keys": tuple of cache keys in table order, "dev": device table (uint8), "n", "blocks"
pack_stats = {"single": 0, "batched_launches": 0, "batched_jobs": 0}
_graph_tables = []            # what captured launches point at when no owner is registered (kept for the process' life)
_graph_keep = [_graph_tables]  # innermost registered owner list last; graph_owner() pushes the capturing object's own list


class graph_owner:
    """`with ops.graph_owner(keep):` around a stream capture: every buffer a captured launch of this module addresses through a
    device-side table -- the job table of ddk_pack_jobs AND the weights / kernel-layout copies its jobs read and write, multi_add
    tables -- is appended to `keep`.  The object that owns the captured graph keeps that list for as long as it may replay, so a
    replay never writes through memory another model (or a replaced cache entry) has given back; when the graph goes, so do they."""

    def __init__(self, keep):
        self.keep = keep

    def __enter__(self):
        _graph_keep.append(self.keep)
        return self.keep

    def __exit__(self, *exc):
        for i in range(len(_graph_keep) - 1, 0, -1):       # by identity (two empty lists compare equal); entry 0 is the process-wide list
            if _graph_keep[i] is self.keep:
                del _graph_keep[i]
                break
        return False


def weights_changed():
    """Every cached kernel-layout copy is stale from here on.  Copies that were allocated while a graph was being captured live in
    that graph's private pool (each replay rewrites them): they are dropped, so no eager call is ever served one."""
    _weights_epoch[0] += 1
    dead = [k for k, e in _pack_cache.items() if e.pooled or e.wref() is None]
    for k in dead:
        del _pack_cache[k]
    if dead:
        _pack_table.clear()


def _pack_job(tag, w):
    """(kind, parameters) of ddk_pack_job for the copy `tag` of weight w, or None when the copy has no batched form"""
    name = tag if isinstance(tag, str) else tag[0]
    if w.dim() != 4:
        return None
    o, i, kh, kw = w.shape
    if name == "fwd":
        return (0, [o, i, kh * kw, pad32(i), i, pad32(i)])
    if name == "fwdT" and (kh, kw) == (4, 4):                 # (I, O, 4, 4)
        return (1, [o, i, o, i])
    if name == "dgrad":
        return (2, [o, i, kh * kw, tag[1], o])
    if name == "wino" and (kh, kw) == (3, 3):
        return (3, [o, i, pad32(i)])
    if name == "wino_dgrad" and (kh, kw) == (3, 3):
        return (4, [o, i, tag[1], tag[2], pad32(o)])
    return None


def _state(w):
    return (w._version, _weights_epoch[0])


def _repack_stale():
    """Refresh every stale registered copy in place with ONE launch.  Returns False when that is not possible right now (a new
    job set while a graph is being captured: building its device table would be a host-to-device copy inside the capture)."""
    keys, live = [], []
    for k, e in _pack_cache.items():
        w = e.wref()
        if w is None or e.job is None or e.fresh == _state(w):
            continue
        keys.append((k, w.data_ptr(), e.out.data_ptr()))     # the cached device table is valid for exactly these buffers
        live.append((e, w))
    if not keys:
        return True
    keys = tuple(keys)
    tab = _pack_table
    if tab.get("keys") != keys:
        if torch.cuda.is_current_stream_capturing():
            return False
        jobs = (L.PackJob * len(keys))()
        for j, (e, w) in zip(jobs, live):
            j.src, j.dst, j.kind = w.data_ptr(), e.out.data_ptr(), e.job[0]
            for q, v in enumerate(e.job[1]):
                j.p[q] = int(v)
        blocks = L.load().ddk_pack_jobs_layout(jobs, len(keys))
        if blocks < 0:
            L.check(-1, "pack_jobs_layout")
        host = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8)
        tab.clear()
        tab.update(keys=keys, dev=host.to(live[0][1].device), n=len(keys), blocks=int(blocks))
    if torch.cuda.is_current_stream_capturing():
        # a captured launch reads this table at every replay and writes through the addresses in it: the graph's owner keeps the
        # table, every source weight and every destination copy alive (the cache may drop or replace its entries meanwhile)
        _graph_keep[-1].append((tab["dev"], [(w, e.out) for e, w in live]))
    L.check(L.load().ddk_pack_jobs(tab["dev"].data_ptr(), tab["n"], tab["blocks"], L.stream()), "pack_jobs")
    pack_stats["batched_launches"] += 1
    pack_stats["batched_jobs"] += len(keys)
    for e, w in live:
        e.fresh = _state(w)
    return True


def cached_pack(tag, w, fn):
    """The kernel-layout copy `tag` of the live parameter `w`, current for its present contents (a weakref guards against a new
    tensor re-using the address).  fn(w.detach()) makes a copy the first time; later refreshes go through ddk_pack_jobs."""
    import weakref
    key = (tag, w.data_ptr(), tuple(w.shape))
    e = _pack_cache.get(key)
    if e is not None and e.wref() is w:
        if e.fresh == _state(w):
            return e.out
        if e.job is not None and w.is_contiguous() and _repack_stale() and e.fresh == _state(w):
            return e.out
    e = _PackEntry()
    e.wref, e.out, e.fresh = weakref.ref(w), fn(w.detach()), _state(w)
    e.job = _pack_job(tag, w) if w.is_contiguous() and w.dtype == torch.float32 else None
    e.pooled = bool(w.is_cuda and torch.cuda.is_current_stream_capturing())
    pack_stats["single"] += 1
    _pack_table.clear()           # a new or replaced copy: the device job table (source / destination addresses) is out of date
    _pack_cache[key] = e
    return e.out


def _f32(t):
    if t.dtype != torch.float32:
        raise L.DDKError(f"expected float32, got {t.dtype}")
    return t


# ------------------------------------------------------------------ layout / packing
def nchw_to_nhwc(x, c_pad=None):
    b, c, h, w = x.shape
    c_pad = c if c_pad is None else c_pad
    out = torch.empty((b, h, w, c_pad), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_nchw_to_nhwc(L.ptr(_f32(x)), L.ptr(out), b, c, h, w, c_pad, L.stream()), "nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, c=None):
    b, h, w, cs = x.shape
    c = cs if c is None else c
    out = torch.empty((b, c, h, w), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_nhwc_to_nchw(L.ptr(_f32(x)), L.ptr(out), b, c, h, w, cs, L.stream()), "nhwc_to_nchw")
    return out


def pad_channels(x, c_pad):
    c = x.shape[-1]
    out = torch.empty((*x.shape[:-1], c_pad), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_pad_channels(L.ptr(_f32(x)), L.ptr(out), x.numel() // c, c, c_pad, L.stream()), "pad_channels")
    return out


def pack_conv_weight(w):
    """OIHW -> [O][KH*KW][pad32(I)]"""
    o, i, kh, kw = w.shape
    out = torch.empty((o, kh * kw, pad32(i)), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_weight(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, kh, kw, pad32(i), L.stream()),
            "pack_conv_weight")
    return out


def pack_convT_weight(w):
    """ConvTranspose2d (I,O,4,4) -> [4 phases][O][4 taps][I]"""
    i, o, kh, kw = w.shape
    if (kh, kw) != (4, 4):
        raise L.DDKError("pack_convT_weight: kernel must be 4x4")
    out = torch.empty((4, o, 4, i), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_convT_weight(L.ptr(_f32(w.contiguous())), L.ptr(out), i, o, L.stream()), "pack_convT_weight")
    return out


def pack_conv_weight_wino(w):
    """OIHW 3x3 -> Winograd-domain filter [pad32(I)/32][16][O][32] (ddk_pack_conv_weight_wino)."""
    o, i, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise L.DDKError("pack_conv_weight_wino: kernel must be 3x3")
    out = torch.empty((pad32(i) // 32, 16, o, 32), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_weight_wino(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, pad32(i), L.stream()), "pack_conv_weight_wino")
    return out


def pack_conv_skip_weight_wino(w):
    """1x1 weight [O, I] (or [O, I, 1, 1]) of a res_conv -> the skip-fold operand of the Winograd kernel, W / 4 in MFMA operand order
    [pad32(I)/32][O/32][4][64][4] (ddk_pack_conv_skip_weight_wino); pass as conv(..., skip_w=...)."""
    o, i = w.shape[0], w.shape[1]
    if w.numel() != o * i or o % 32:
        raise L.DDKError("pack_conv_skip_weight_wino: a 1x1 filter with O % 32 == 0")
    out = torch.empty((pad32(i) // 32, o // 32, 4, 64, 4), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_skip_weight_wino(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, pad32(i), L.stream()),
            "pack_conv_skip_weight_wino")
    return out


def pack_convT_weight_wino(w):
    """ConvTranspose2d weight (I, O, 4, 4) -> Winograd F(2x2, 2x2) filters per output phase [4][pad32(I)/32][9][O][32]
    (ddk_pack_convT_weight_wino); pass as conv(CONVT4X4_S2, ..., w_wino=...)."""
    i, o, kh, kw = w.shape
    if (kh, kw) != (4, 4):
        raise L.DDKError("pack_convT_weight_wino: kernel must be 4x4")
    out = torch.empty((4, pad32(i) // 32, 9, o, 32), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_convT_weight_wino(L.ptr(_f32(w.contiguous())), L.ptr(out), i, o, pad32(i), L.stream()), "pack_convT_weight_wino")
    return out


def pack_conv_weight_local(w):
    """OIHW 3x3 -> the operand order of conv3x3_gn_mish (ddk_pack_conv_weight_local): [O/32][9][pad32(I)/32][1024]."""
    o, i, kh, kw = w.shape
    if (kh, kw) != (3, 3) or o % 32:
        raise L.DDKError("pack_conv_weight_local: kernel must be 3x3 and O % 32 == 0")
    out = torch.empty((o // 32, 9, pad32(i) // 32, 1024), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_weight_local(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, pad32(i), L.stream()), "pack_conv_weight_local")
    return out


def pack_conv_weight_wino_local(w):
    """OIHW 3x3 -> Winograd-domain filter in the operand order of conv3x3_gn_mish_wino: [O/32][pad32(I)/32][16][1024]."""
    o, i, kh, kw = w.shape
    if (kh, kw) != (3, 3) or o % 32:
        raise L.DDKError("pack_conv_weight_wino_local: kernel must be 3x3 and O % 32 == 0")
    out = torch.empty((o // 32, pad32(i) // 32, 16, 1024), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_weight_wino_local(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, pad32(i), L.stream()),
            "pack_conv_weight_wino_local")
    return out


def wino_weight(weight, x_shape, c_lo=None, c_hi=None, dgrad=False):
    """Cached Winograd-domain copy of a canonical OIHW 3x3 filter for a conv on NHWC input shape `x_shape`, or None when the
    shape is not eligible (ddk_conv_wino_splits == 0).  dgrad=True: the filter of the INPUT-gradient conv for input channels
    [c_lo, c_hi) -- g'[ci][n][a][b] = w[n][ci][2-a][2-b] -- which is again a 3x3 stride-1 conv (of dY)."""
    b, h, w_, cin_x = x_shape
    o, i = weight.shape[0], weight.shape[1]
    if tuple(weight.shape[2:]) != (3, 3):
        return None
    if dgrad:
        lo, hi = (0 if c_lo is None else c_lo), (i if c_hi is None else c_hi)
        n_out, cin = hi - lo, o
    else:
        lo, hi, n_out, cin = 0, i, o, pad32(i)
    if L.load().ddk_conv_wino_splits(b, h, w_, pad32(cin), n_out) <= 0:
        return None
    if dgrad:
        def pack(t):       # flip + transpose + Winograd transform in ONE kernel (was three torch kernels + the pack)
            out = torch.empty((pad32(o) // 32, 16, hi - lo, 32), device=t.device, dtype=torch.float32)
            L.check(L.load().ddk_pack_conv_weight_wino_dgrad(L.ptr(_f32(t.contiguous())), L.ptr(out), o, i, lo, hi, pad32(o), L.stream()),
                    "pack_conv_weight_wino_dgrad")
            return out
        return cached_pack(("wino_dgrad", lo, hi), weight, pack)
    return cached_pack("wino", weight, pack_conv_weight_wino)


# ------------------------------------------------------------------ conv family
def conv(kind, x, w_packed, bias=None, n_out=None, x2=None, resid=None, pre_mish=False, post_mish=False, w_wino=None, mish_out=None,
         dmish_src=None, leave_slabs=False, skip_w=None, skip_bias=None, skip_out=None, out=None):
    """Implicit-GEMM conv on NHWC x (optionally channel-concatenated with x2 without materialising it).
    skip_w (pack_conv_skip_weight_wino; shapes with ddk_conv_wino_skip_ok only, with w_wino): the launch also computes the 1x1 conv of
    the same input with that weight (+ skip_bias) -- returns (out, skip); skip_out: the tensor that receives it (else a new one).
    out: the tensor to write into (else a new one).
    w_wino: the same 3x3 filter in the Winograd domain -> the F(2x2,3x3) kernel runs when the shape is eligible.
    mish_out: tensor that also receives Mish(out); dmish_src: out = (conv + bias) * Mish'(dmish_src) (+ resid) (ddk_conv_args).
    leave_slabs (plain convs only: no resid / Mish): returns (out, slabs) -- when the launch splits k, `slabs` [S,B,Ho,Wo,N] holds the
    S >= 2 partial sums WITHOUT the bias and `out` is unwritten (ddk_conv_args.defer_reduce: the GroupNorm that follows sums them
    while it loads, ops.groupnorm_mish_train / groupnorm_mish_bwd); otherwise slabs is None and `out` is complete."""
    b, h, w_, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[-1]
    n = n_out if n_out is not None else (w_packed.shape[1] if kind == CONVT4X4_S2 else w_packed.shape[0])
    if kind == CONV3X3_S2:
        ho, wo = (h - 1) // 2 + 1, (w_ - 1) // 2 + 1
    elif kind == CONVT4X4_S2:
        ho, wo = 2 * h, 2 * w_
    elif kind == 4:   # CONV4X4_S2
        ho, wo = h // 2, w_ // 2
    else:
        ho, wo = h, w_
    if out is None:
        out = torch.empty((b, ho, wo, n), device=x.device, dtype=torch.float32)
    lib = L.load()
    ws_bytes = lib.ddk_conv_workspace_bytes(kind, b, h, w_, c0 + c1, n)
    if mish_out is not None or dmish_src is not None:
        w_wino = None                                   # these epilogues live on the im2col kernels
    wsplits = 0
    if w_wino is not None and kind == CONV3X3_S1 and not pre_mish:
        wsplits = lib.ddk_conv_wino_splits(b, h, w_, c0 + c1, n)
        if wsplits > 0:
            ws_bytes = wsplits * out.numel() * 4 if wsplits > 1 else 0
            if skip_w is not None:
                ws_bytes *= 2                           # the skip conv's slabs follow the conv's
    nslab = 1
    if leave_slabs:
        if resid is not None or pre_mish or post_mish or mish_out is not None or dmish_src is not None:
            raise L.DDKError("conv(leave_slabs): only for a plain conv (bias is the consumer's to add)")
        nslab = wsplits if (w_wino is not None and kind == CONV3X3_S1 and wsplits > 0) else lib.ddk_conv_splits(kind, b, h, w_, c0 + c1, n)
        if nslab > 1 and ws_bytes < nslab * out.numel() * 4:
            raise L.DDKError("conv(leave_slabs): internal: workspace smaller than the slabs")
    ws = torch.empty(max(ws_bytes, 16) // 4, device=x.device, dtype=torch.float32) if ws_bytes else None
    a = L.ConvArgs(kind, L.ptr(_f32(x)), L.ptr(x2), c0, c1, L.ptr(w_packed), L.ptr(bias), L.ptr(resid), L.ptr(out),
                   b, h, w_, n, int(pre_mish), int(post_mish), int(leave_slabs and nslab > 1), L.ptr(ws), ws_bytes, L.ptr(w_wino), None, 0,
                   L.ptr(mish_out), L.ptr(dmish_src))
    if skip_w is not None:
        if skip_out is None:
            skip_out = torch.empty((b, ho, wo, n), device=x.device, dtype=torch.float32)
        a.skip_weight, a.skip_bias, a.skip_out = L.ptr(skip_w), L.ptr(skip_bias), L.ptr(skip_out)
        if wsplits > 1 and leave_slabs:
            raise L.DDKError("conv(skip_w): not with leave_slabs")
    L.check(lib.ddk_conv_forward(C.byref(a), L.stream()), "conv_forward")
    if skip_w is not None:
        return out, skip_out
    if leave_slabs:
        return out, (ws[:nslab * out.numel()].view(nslab, b, ho, wo, n) if nslab > 1 else None)
    return out


def conv_with_gn_partials(x, w_packed, bias, w_wino, x2=None, groups=GN_GROUPS):
    """3x3 conv on the Winograd kernel that also emits GroupNorm partials (ddk_conv_args.gn_partials): -> (raw output, partials
    [B * tiles_per_image][groups][2] = {mean, M2} per 128-pixel tile, tiles_per_image).  Only where ddk_conv_gn_partials() > 0."""
    b, h, w_, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[-1]
    n = w_packed.shape[0]
    lib = L.load()
    np_ = lib.ddk_conv_gn_partials(b, h, w_, c0 + c1, n, groups)
    if np_ <= 0:
        raise L.DDKError(f"conv_with_gn_partials: shape {tuple(x.shape)} (+{c1}) -> {n} cannot emit GroupNorm partials")
    raw = torch.empty((b, h, w_, n), device=x.device, dtype=torch.float32)
    part = torch.empty((b * np_, groups, 2), device=x.device, dtype=torch.float32)
    a = L.ConvArgs(CONV3X3_S1, L.ptr(_f32(x)), L.ptr(x2), c0, c1, L.ptr(w_packed), L.ptr(bias), None, L.ptr(raw), b, h, w_, n, 0, 0, 0,
                   None, 0, L.ptr(w_wino), L.ptr(part), groups)
    L.check(lib.ddk_conv_forward(C.byref(a), L.stream()), "conv_forward(gn_partials)")
    return raw, part, np_


def groupnorm_mish_from_partials(x, part, tiles_per_image, gamma, beta, temb=None, addend=None, groups=GN_GROUPS, eps=GN_EPS):
    """GroupNorm+Mish(+temb)(+addend) of x from the partials of conv_with_gn_partials: one read, one write (ddk_groupnorm_mish_partials)."""
    b, h, w_, n = x.shape
    out = torch.empty_like(x)
    stride = temb.stride(0) if temb is not None else 0
    L.check(L.load().ddk_groupnorm_mish_partials(L.ptr(_f32(x)), L.ptr(part), tiles_per_image, L.ptr(gamma), L.ptr(beta),
                                                 temb.data_ptr() if temb is not None else None, stride, L.ptr(addend), L.ptr(out),
                                                 b, h * w_, n, groups, eps, L.stream()), "groupnorm_mish_partials")
    return out


def pack_conv_weight_first(w):
    """OIHW 3x3 with 1 <= I <= 8 -> conv_first's operand order [O/32][ceil(9 I / 2)][64] (ddk_pack_conv_weight_first)."""
    o, i, kh, kw = w.shape
    if (kh, kw) != (3, 3) or o % 32 or not 1 <= i <= 8:
        raise L.DDKError("pack_conv_weight_first: kernel must be 3x3, O % 32 == 0, 1 <= I <= 8")
    out = torch.empty((o // 32, (9 * i + 1) // 2, 64), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_weight_first(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, L.stream()), "pack_conv_weight_first")
    return out


def conv_first(x, w_first, bias, n_out, groups=GN_GROUPS, partials=True):
    """The network's first 3x3 conv on the unpadded NHWC input (C_in <= 8): -> (raw output, GroupNorm partials or None, tiles per
    image).  ddk_conv_first."""
    b, h, w_, cin = x.shape
    lib = L.load()
    if not lib.ddk_conv_first_ok(cin, n_out, h, w_, groups):
        raise L.DDKError(f"conv_first: shape {tuple(x.shape)} -> {n_out} not eligible")
    raw = torch.empty((b, h, w_, n_out), device=x.device, dtype=torch.float32)
    tiles = h * w_ // 128
    part = torch.empty((b * tiles, groups, 2), device=x.device, dtype=torch.float32) if partials else None
    L.check(lib.ddk_conv_first(L.ptr(_f32(x)), L.ptr(w_first), L.ptr(bias), L.ptr(raw), L.ptr(part), b, h, w_, cin, n_out, groups,
                               L.stream()), "conv_first")
    return raw, part, tiles


def conv1x1_ws(x, w_packed, bias=None, resid=None, ln=None, eps=1e-5):
    """1x1 conv of a 128-channel NHWC tensor by the weights-stationary kernel (ddk_conv1x1_ws); w_packed [N][128].
    ln = (c1, c2): LayerNorm folded in (w_packed then holds W o g)."""
    b, h, w_, k = x.shape
    n = w_packed.shape[0]
    lib = L.load()
    if not lib.ddk_conv1x1_ws_ok(b * h * w_, k, n):
        raise L.DDKError(f"conv1x1_ws: shape {tuple(x.shape)} -> {n} not eligible")
    out = torch.empty((b, h, w_, n), device=x.device, dtype=torch.float32)
    c1, c2 = ln if ln is not None else (None, None)
    L.check(lib.ddk_conv1x1_ws(L.ptr(_f32(x)), L.ptr(w_packed), L.ptr(bias), L.ptr(resid), L.ptr(out), b * h * w_, n, L.ptr(c1), L.ptr(c2),
                               eps, L.stream()), "conv1x1_ws")
    return out


def attention_folded(x, w_qkv, ln_g, ln_b, w_out, b_out, heads=4, eps=LN_EPS):
    """PreNorm(LinearAttention) + Residual (blocks.py:8-14,57-71,116-134) on a map with more than 256 pixels and C = heads * 32 = 128,
    in the folded form: k, v projection -> context -> per-image matrix W_out ctx^T W_q (ddk_attention_fold) -> one per-image 1x1 conv
    of x with the LayerNorm folded in and the residual added (ddk_conv1x1_ws_images).  x [B,H,W,128]; w_qkv [384,128(,1,1)], w_out
    [128,128(,1,1)], b_out [128] canonical; ln_g / ln_b the channel LayerNorm's g, b."""
    b, h, w_, c = x.shape
    hc = heads * 32
    wq = w_qkv.reshape(3 * hc, c).to(torch.float32)
    g, be = ln_g.reshape(-1).to(torch.float32), ln_b.reshape(-1).to(torch.float32)
    wg = (wq * g.view(1, c)).contiguous()                   # W o g
    c1, c2 = (wq @ g).contiguous(), (wq @ be).contiguous()  # W g, W b
    lib = L.load()
    m = b * h * w_
    kv = torch.empty((b, h, w_, 2 * hc), device=x.device, dtype=torch.float32)
    L.check(lib.ddk_conv1x1_ws(L.ptr(_f32(x)), L.ptr(wg[hc:].contiguous()), None, None, L.ptr(kv), m, 2 * hc, L.ptr(c1[hc:].contiguous()),
                               L.ptr(c2[hc:].contiguous()), eps, L.stream()), "conv1x1_ws(kv)")
    ctx = torch.empty((b, heads, 32, 32), device=x.device, dtype=torch.float32)
    nbytes = lib.ddk_linattn_context_workspace_bytes(b, h * w_, heads)
    ws = _ws(x.device, nbytes, "linattn") if nbytes else None
    L.check(lib.ddk_linattn_context_kv(L.ptr(kv), L.ptr(ctx), b, h * w_, heads, L.ptr(ws), nbytes, L.stream()), "linattn_context_kv")
    a_mat = torch.empty((b, c, c), device=x.device, dtype=torch.float32)
    a1 = torch.empty((b, c), device=x.device, dtype=torch.float32)
    a2 = torch.empty((b, c), device=x.device, dtype=torch.float32)
    L.check(lib.ddk_attention_fold(L.ptr(ctx), L.ptr(wg[:hc].contiguous()), L.ptr(c1[:hc].contiguous()), L.ptr(c2[:hc].contiguous()),
                                   L.ptr(w_out.reshape(c, hc).contiguous()), L.ptr(b_out), L.ptr(a_mat), L.ptr(a1), L.ptr(a2), b, c, heads,
                                   L.stream()), "attention_fold")
    out = torch.empty_like(x)
    L.check(lib.ddk_conv1x1_ws_images(L.ptr(x), L.ptr(a_mat), None, L.ptr(x), L.ptr(out), m, c, L.ptr(a1), L.ptr(a2), eps, b, L.stream()),
            "conv1x1_ws_images")
    return out


def attention_kv_context(x, w_qkv, ln_g, ln_b, heads=4, eps=LN_EPS):
    """ctx [B,4,32,32] of PreNorm(LinearAttention) (blocks.py:57-60,123,129-131) from x [B,H,W,128] in ONE launch + the split merge
    (ddk_attention_kv_context): the k and v thirds of to_qkv with the LayerNorm folded in, softmax over the pixels of k, k v^T -- no kv
    tensor.  w_qkv [384,128(,1,1)] canonical; ln_g / ln_b the channel LayerNorm's g, b."""
    b, h, w_, c = x.shape
    hc = heads * 32
    lib = L.load()
    if not lib.ddk_attention_kv_context_ok(b, h * w_, c, heads):
        raise L.DDKError(f"attention_kv_context: shape {tuple(x.shape)} with {heads} heads not eligible (C = 128, 4 heads, H*W % 64 == 0)")
    wq = w_qkv.reshape(3 * hc, c).to(torch.float32)
    g, be = ln_g.reshape(-1).to(torch.float32), ln_b.reshape(-1).to(torch.float32)
    wkv = (wq * g.view(1, c))[hc:].contiguous()
    c1, c2 = (wq @ g)[hc:].contiguous(), (wq @ be)[hc:].contiguous()
    ctx = torch.empty((b, heads, 32, 32), device=x.device, dtype=torch.float32)
    nbytes = lib.ddk_attention_kv_context_workspace_bytes(b, h * w_)
    ws = _ws(x.device, nbytes, "kvctx")
    L.check(lib.ddk_attention_kv_context(L.ptr(_f32(x)), L.ptr(wkv), L.ptr(c1), L.ptr(c2), eps, L.ptr(ctx), b, h * w_, L.ptr(ws), nbytes,
                                         L.stream()), "attention_kv_context")
    return ctx


def attention_kv_partials(x, w_qkv, ln_g, ln_b, heads=4, eps=LN_EPS):
    """attention_kv_context without the merge (ddk_attention_kv_partials): the split records [B,4,splits,1088] = {max[32], den[32],
    unnormalised ctx[32][32]} per (image, head, pixel split), for linattn_merge or attention_fold_partials."""
    b, h, w_, c = x.shape
    hc = heads * 32
    lib = L.load()
    if not lib.ddk_attention_kv_context_ok(b, h * w_, c, heads):
        raise L.DDKError(f"attention_kv_partials: shape {tuple(x.shape)} with {heads} heads not eligible (C = 128, 4 heads, H*W % 64 == 0)")
    wq = w_qkv.reshape(3 * hc, c).to(torch.float32)
    g, be = ln_g.reshape(-1).to(torch.float32), ln_b.reshape(-1).to(torch.float32)
    wkv = (wq * g.view(1, c))[hc:].contiguous()
    c1, c2 = (wq @ g)[hc:].contiguous(), (wq @ be)[hc:].contiguous()
    nbytes = lib.ddk_attention_kv_context_workspace_bytes(b, h * w_)
    part = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    splits = C.c_int(0)
    L.check(lib.ddk_attention_kv_partials(L.ptr(_f32(x)), L.ptr(wkv), L.ptr(c1), L.ptr(c2), eps, b, h * w_, L.ptr(part), nbytes,
                                          C.byref(splits), L.stream()), "attention_kv_partials")
    return part.view(b, heads, splits.value, 2 * 32 + 32 * 32)


def linattn_merge(part):
    """ctx [B,heads,32,32] from split records [B,heads,splits,1088] (ddk_linattn_merge), in split order"""
    b, heads, splits, _ = part.shape
    ctx = torch.empty((b, heads, 32, 32), device=part.device, dtype=torch.float32)
    L.check(L.load().ddk_linattn_merge(L.ptr(_f32(part)), L.ptr(ctx), b, heads, splits, L.stream()), "linattn_merge")
    return ctx


def attention_fold_partials(part, wqg, c1q, c2q, w_out, b_out=None, out=None):
    """(A [B,128,128], a1 [B,128], a2 [B,128]) of ddk_attention_fold straight from the split records [B,4,splits,1088] in one launch
    (ddk_attention_fold_partials); wqg [128,128], c1q / c2q [128], w_out [128,128] packed, b_out [128] or None; out = (A, a1, a2) to
    write into given tensors."""
    b, heads, splits, _ = part.shape
    c = wqg.shape[1]
    lib = L.load()
    if not lib.ddk_attention_fold_partials_ok(c, heads, splits):
        raise L.DDKError(f"attention_fold_partials: C = {c}, {heads} heads, {splits} splits not eligible (C = 128, 4 heads, 1 / 2 / 4 / 8 splits)")
    a_mat, a1, a2 = out if out is not None else (torch.empty((b, c, c), device=part.device, dtype=torch.float32),
                                                 torch.empty((b, c), device=part.device, dtype=torch.float32),
                                                 torch.empty((b, c), device=part.device, dtype=torch.float32))
    L.check(lib.ddk_attention_fold_partials(L.ptr(_f32(part)), splits, L.ptr(wqg), L.ptr(c1q), L.ptr(c2q), L.ptr(w_out), L.ptr(b_out),
                                            L.ptr(a_mat), L.ptr(a1), L.ptr(a2), b, c, heads, L.stream()), "attention_fold_partials")
    return a_mat, a1, a2


def groupnorm_mish_from_partials_res1x1(x, part, tiles_per_image, gamma, beta, res_x, res_w, res_b, temb=None, groups=GN_GROUPS,
                                        eps=GN_EPS):
    """groupnorm_mish_from_partials with the addend res_b + res_x @ res_w^T (a 1x1 conv of a <= 8-channel tensor) computed on the
    fly (ddk_groupnorm_mish_partials_res1x1)."""
    b, h, w_, n = x.shape
    cin = res_x.shape[-1]
    out = torch.empty_like(x)
    stride = temb.stride(0) if temb is not None else 0
    L.check(L.load().ddk_groupnorm_mish_partials_res1x1(
        L.ptr(_f32(x)), L.ptr(part), tiles_per_image, L.ptr(gamma), L.ptr(beta), temb.data_ptr() if temb is not None else None, stride,
        L.ptr(_f32(res_x)), L.ptr(res_w.reshape(n, cin).contiguous()), L.ptr(res_b), cin, L.ptr(out), b, h * w_, n, groups, eps,
        L.stream()), "groupnorm_mish_partials_res1x1")
    return out


def final_tail(raw, part, tiles_per_image, gamma, beta, w, bias, x=None, t=None, tables=None, noise=None, seed=0, stream_id=0,
               want_eps=True, groups=GN_GROUPS, eps=GN_EPS):
    """GroupNorm (from conv partials) + Mish + 1x1 projection to n_out <= 8 channels, and -- with x, t, tables -- the in-place
    reverse-step update of x, in one launch (ddk_final_tail).  Returns eps_hat (or None when want_eps is False)."""
    b, h, w_, c = raw.shape
    n_out = w.shape[0]
    eps_out = torch.empty((b, h, w_, n_out), device=raw.device, dtype=torch.float32) if want_eps else None
    tb = tables or {}
    L.check(L.load().ddk_final_tail(L.ptr(_f32(raw)), L.ptr(part), tiles_per_image, L.ptr(gamma), L.ptr(beta), eps,
                                    L.ptr(w.reshape(n_out, c).contiguous()), L.ptr(bias), n_out, L.ptr(eps_out), L.ptr(x), L.ptr(noise),
                                    L.ptr(t), L.ptr(tb.get("c_recip")), L.ptr(tb.get("c_recipm1")), L.ptr(tb.get("c1")),
                                    L.ptr(tb.get("c2")), L.ptr(tb.get("sigma")), seed, stream_id, b, h * w_, c, groups, L.stream()),
            "final_tail")
    return eps_out


def conv3x3_gn_mish_cluster(x, w_wino, bias, gamma, beta, x2=None, temb=None, addend=None, groups=GN_GROUPS, eps=GN_EPS, check=True,
                            skip_w=None, skip_bias=None, skip_out=None, out=None):
    """Block (conv3x3 + GroupNorm + Mish + shift + residual) in ONE Winograd launch whose workgroups exchange tile statistics
    (ddk_conv3x3_gn_mish_cluster); raises when the shape or the device is not eligible.  check=True (default) waits for the
    stream and raises DDKError when an exchange timed out (shared GPU): the output then holds NaN tiles and must not be used;
    timing loops pass check=False and call cluster_check() once at their end.
    skip_w (pack_conv_skip_weight_wino; ddk_conv_wino_skip_ok shapes): the launch also writes the 1x1 conv of the same input
    (+ skip_bias) -> returns (out, skip).  out / skip_out: tensors to write into (else new ones)."""
    b, h, w_, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[-1]
    n = w_wino.shape[2]
    lib = L.load()
    if lib.ddk_conv3x3_gn_mish_cluster_ok(b, h, w_, c0 + c1, n, groups) <= 0:
        raise L.DDKError(f"conv3x3_gn_mish_cluster: shape {tuple(x.shape)} (+{c1}) -> {n} not eligible")
    nbytes = max(lib.ddk_conv3x3_gn_mish_cluster_workspace_bytes(b, h, w_, n),
                 lib.ddk_conv3x3_gn_mish_cluster_split_workspace_bytes(b, h, w_, c0 + c1, n, groups))      # (the k-split kind of shape)
    if skip_w is not None:
        nbytes += max(lib.ddk_conv_wino_splits(b, h, w_, c0 + c1, n) - 1, 0) * b * h * w_ * n * 4     # the skip fold's partial tiles
    ws = _ws(x.device, nbytes, "cluster")
    if out is None:
        out = torch.empty((b, h, w_, n), device=x.device, dtype=torch.float32)
    stride = temb.stride(0) if temb is not None else 0
    args = (L.ptr(_f32(x)), c0, L.ptr(x2), c1, L.ptr(w_wino), L.ptr(bias), L.ptr(gamma), L.ptr(beta),
            temb.data_ptr() if temb is not None else None, stride, L.ptr(addend), L.ptr(out), b, h, w_, n, groups, eps, L.ptr(ws), nbytes)
    if skip_w is not None:
        if skip_out is None:
            skip_out = torch.empty((b, h, w_, n), device=x.device, dtype=torch.float32)
        L.check(lib.ddk_conv3x3_gn_mish_cluster_skip(*args, L.ptr(skip_w), L.ptr(skip_bias), L.ptr(skip_out), L.stream()),
                "conv3x3_gn_mish_cluster_skip")
    else:
        L.check(lib.ddk_conv3x3_gn_mish_cluster(*args, L.stream()), "conv3x3_gn_mish_cluster")
    if check:
        L.check(lib.ddk_conv3x3_gn_mish_cluster_check(L.ptr(ws), b, L.stream()), "conv3x3_gn_mish_cluster")
    return out if skip_w is None else (out, skip_out)


def cluster_check(device, b):
    """ddk_conv3x3_gn_mish_cluster_check on the scratch the wrapper above used on `device` (a tensor's .device) and the current
    stream: raises DDKError if any launch since the last check gave up, and if no such scratch exists (nothing to check is an
    error in a timing loop, not a pass)."""
    ws = _scratch.get((str(device), "cluster", torch.cuda.current_stream().cuda_stream))
    if ws is None:
        raise L.DDKError(f"cluster_check: no cluster workspace on {device} for the current stream")
    L.check(L.load().ddk_conv3x3_gn_mish_cluster_check(L.ptr(ws), b, L.stream()), "conv3x3_gn_mish_cluster")


class ClockProbe:
    """Shader clock held over a region of a stream: probe() before and after, then ghz().  (ddk_debug_clock_probe: one record per
    workgroup {XCC, s_memtime, s_memrealtime}; records of the same XCC are differenced, the median over XCCs is returned.)"""

    def __init__(self, device, workgroups=64):
        self.n = workgroups
        self.a = torch.zeros((workgroups, 4), device=device, dtype=torch.int64)
        self.b = torch.zeros((workgroups, 4), device=device, dtype=torch.int64)
        self._first = True

    def probe(self):
        buf = self.a if self._first else self.b
        self._first = False
        L.check(L.load().ddk_debug_clock_probe(buf.data_ptr(), self.n, L.stream()), "debug_clock_probe")

    def ghz(self):
        """Median over the workgroups whose two records come from the same XCC (workgroup i of both probe launches: the same dispatch
        slot) of d(s_memtime) / d(s_memrealtime).  Pairing records of different workgroups of an XCC (rounds 4-5 took the first record
        per XCC of each probe) mixes counters that are a constant apart: invisible over a second, 30 % off over 25 ms."""
        a, b = self.a.cpu().numpy(), self.b.cpu().numpy()
        rates = []
        for i in range(min(len(a), len(b))):
            if int(a[i, 3]) == 1 and int(b[i, 3]) == 1 and int(a[i, 0]) == int(b[i, 0]):
                dc, dt = int(b[i, 1]) - int(a[i, 1]), int(b[i, 2]) - int(a[i, 2])
                if dt > 0 and dc > 0:
                    rates.append(dc / dt * 0.1)        # cycles per 10 ns tick -> GHz
        rates.sort()
        return rates[len(rates) // 2] if rates else None


def cluster_timeouts():
    return int(L.load().ddk_debug_cluster_timeouts())


def conv3x3_groupnorm_mish(x, w_packed, bias, gamma, beta, x2=None, temb=None, addend=None, groups=GN_GROUPS, eps=GN_EPS, w_wino=None):
    """conv3x3(pad 1) -> GroupNorm -> Mish (+temb)(+addend), two launches.  When the conv splits k its partial slabs are summed by
    the GroupNorm kernel's load (ddk_groupnorm_mish_slabs) instead of a separate reduce pass.  w_wino: the Winograd-domain filter
    (pack_conv_weight_wino) -- the conv then runs on the Winograd kernel where the shape is eligible."""
    b, h, w_, c0 = x.shape
    c1 = 0 if x2 is None else x2.shape[-1]
    n = w_packed.shape[0]
    lib = L.load()
    wino = w_wino is not None and lib.ddk_conv_wino_splits(b, h, w_, c0 + c1, n) > 0
    if wino and lib.ddk_conv_gn_partials(b, h, w_, c0 + c1, n, groups) > 0:
        # one-pass Winograd conv leaves per-tile {mean, M2}; GroupNorm reads the tensor once
        raw, part, np_ = conv_with_gn_partials(x, w_packed, bias, w_wino, x2=x2, groups=groups)
        return groupnorm_mish_from_partials(raw, part, np_, gamma, beta, temb=temb, addend=addend, groups=groups, eps=eps)
    splits = lib.ddk_conv_wino_splits(b, h, w_, c0 + c1, n) if wino else lib.ddk_conv_splits(CONV3X3_S1, b, h, w_, c0 + c1, n)
    if splits == 1 or lib.ddk_groupnorm_workspace_bytes(b, h * w_, n, groups) != 0:
        return groupnorm_mish(conv(CONV3X3_S1, x, w_packed, bias, x2=x2, w_wino=w_wino), gamma, beta, temb=temb, addend=addend,
                              groups=groups, eps=eps)
    ws_bytes = splits * b * h * w_ * n * 4 if wino else lib.ddk_conv_workspace_bytes(CONV3X3_S1, b, h, w_, c0 + c1, n)
    ws = torch.empty(ws_bytes // 4, device=x.device, dtype=torch.float32)
    out = torch.empty((b, h, w_, n), device=x.device, dtype=torch.float32)
    a = L.ConvArgs(CONV3X3_S1, L.ptr(_f32(x)), L.ptr(x2), c0, c1, L.ptr(w_packed), None, None, L.ptr(out), b, h, w_, n, 0, 0, 1,
                   L.ptr(ws), ws_bytes, L.ptr(w_wino) if wino else None)
    L.check(lib.ddk_conv_forward(C.byref(a), L.stream()), "conv_forward(defer)")
    stride = temb.stride(0) if temb is not None else 0
    L.check(lib.ddk_groupnorm_mish_slabs(L.ptr(ws), splits, b * h * w_ * n, L.ptr(bias), L.ptr(gamma), L.ptr(beta),
                                         temb.data_ptr() if temb is not None else None, stride, L.ptr(addend), L.ptr(out),
                                         b, h * w_, n, groups, eps, L.stream()), "groupnorm_mish_slabs")
    return out


# ------------------------------------------------------------------ norms / activations
def groupnorm_mish(x, gamma, beta, temb=None, addend=None, groups=GN_GROUPS, eps=GN_EPS):
    b, h, w, c = x.shape
    out = torch.empty_like(x)
    lib = L.load()
    ws_bytes = lib.ddk_groupnorm_workspace_bytes(b, h * w, c, groups)
    ws = torch.empty(max(ws_bytes, 16) // 4, device=x.device, dtype=torch.float32) if ws_bytes else None
    stride = temb.stride(0) if temb is not None else 0
    L.check(lib.ddk_groupnorm_mish(L.ptr(_f32(x)), L.ptr(gamma), L.ptr(beta),
                                   temb.data_ptr() if temb is not None else None, stride, L.ptr(addend), L.ptr(out),
                                   b, h * w, c, groups, eps, L.ptr(ws), ws_bytes, L.stream()), "groupnorm_mish")
    return out


def conv3x3_gn_mish(x, w_local, bias, gamma, beta, temb=None, addend=None, x2=None, groups=GN_GROUPS, eps=GN_EPS):
    """Block (blocks.py:75-84) in one launch on a 4x4 / 8x8 map: x [B,H,W,c0] (+ x2 [B,H,W,c1], the concat of unet.py:97),
    w_local = pack_conv_weight_local(weight) -> Mish(GN(conv(x) + bias)) (+ temb[b]) (+ addend)."""
    b, h, w, c0 = x.shape
    c1 = x2.shape[-1] if x2 is not None else 0
    n = w_local.shape[0] * 32
    w_packed = w_local
    if w_local.shape[2] * 32 != c0 + c1:
        raise L.DDKError(f"conv3x3_gn_mish: filter packed for {w_local.shape[2] * 32} input channels, input has {c0 + c1}")
    lib = L.load()
    if not lib.ddk_conv3x3_gn_mish_ok(h, w, c0 + c1, c0, n, groups):
        raise L.DDKError(f"conv3x3_gn_mish: shape {tuple(x.shape)} (+{c1}) -> {n} not eligible")
    out = torch.empty((b, h, w, n), device=x.device, dtype=torch.float32)
    stride = temb.stride(0) if temb is not None else 0
    L.check(lib.ddk_conv3x3_gn_mish(L.ptr(_f32(x)), c0, L.ptr(_f32(x2)) if x2 is not None else None, c1, L.ptr(w_packed), L.ptr(bias),
                                    L.ptr(gamma), L.ptr(beta), temb.data_ptr() if temb is not None else None, stride, L.ptr(addend),
                                    L.ptr(out), b, h, w, n, groups, eps, L.stream()), "conv3x3_gn_mish")
    return out


def conv3x3_gn_mish_wino(x, w_wl, bias, gamma, beta, temb=None, addend=None, x2=None, groups=GN_GROUPS, eps=GN_EPS):
    """Block (blocks.py:75-84) in one launch on a 64-pixel map (8x8), Winograd form; w_wl = pack_conv_weight_wino_local(weight)."""
    b, h, w, c0 = x.shape
    c1 = x2.shape[-1] if x2 is not None else 0
    n = w_wl.shape[0] * 32
    lib = L.load()
    if w_wl.shape[1] * 32 != c0 + c1:
        raise L.DDKError(f"conv3x3_gn_mish_wino: filter packed for {w_wl.shape[1] * 32} input channels, input has {c0 + c1}")
    if not lib.ddk_conv3x3_gn_mish_wino_ok(h, w, c0 + c1, c0, n, groups):
        raise L.DDKError(f"conv3x3_gn_mish_wino: shape {tuple(x.shape)} (+{c1}) -> {n} not eligible")
    out = torch.empty((b, h, w, n), device=x.device, dtype=torch.float32)
    stride = temb.stride(0) if temb is not None else 0
    L.check(lib.ddk_conv3x3_gn_mish_wino(L.ptr(_f32(x)), c0, L.ptr(_f32(x2)) if x2 is not None else None, c1, L.ptr(w_wl), L.ptr(bias),
                                         L.ptr(gamma), L.ptr(beta), temb.data_ptr() if temb is not None else None, stride, L.ptr(addend),
                                         L.ptr(out), b, h, w, n, groups, eps, L.stream()), "conv3x3_gn_mish_wino")
    return out


def conv3x3_gn_mish_slabs(src_slabs, src_bias, w_packed, bias, gamma, beta, temb=None, addend_slabs=None, addend_bias=None, groups=GN_GROUPS,
                          eps=GN_EPS):
    """The one-launch Block of the 4x4 / 8x8 maps on operands still in split-K form (ddk_conv3x3_gn_mish_slabs): src_slabs [S][B][H][W][C]
    partial sums of the input (+ src_bias[c]), addend_slabs [S'][B][H][W][N] of the residual (+ addend_bias[c]) or None.  w_packed:
    pack_conv_weight_local (H*W == 16) / pack_conv_weight_wino_local (H*W == 64)."""
    s_, b, h, w, c0 = src_slabs.shape
    n = w_packed.shape[0] * 32
    out = torch.empty((b, h, w, n), device=src_slabs.device, dtype=torch.float32)
    stride = temb.stride(0) if temb is not None else 0
    a_n, a_stride = (addend_slabs.shape[0], addend_slabs.stride(0)) if addend_slabs is not None else (1, 0)
    L.check(L.load().ddk_conv3x3_gn_mish_slabs(L.ptr(_f32(src_slabs)), s_, src_slabs.stride(0), L.ptr(src_bias), c0, L.ptr(w_packed), L.ptr(bias),
                                               L.ptr(gamma), L.ptr(beta), temb.data_ptr() if temb is not None else None, stride,
                                               L.ptr(addend_slabs), a_n, a_stride, L.ptr(addend_bias), L.ptr(out), b, h, w, n, groups, eps,
                                               L.stream()), "conv3x3_gn_mish_slabs")
    return out


def chan_layernorm(x, g, b, eps=LN_EPS):
    c = x.shape[-1]
    out = torch.empty_like(x)
    L.check(L.load().ddk_chan_layernorm(L.ptr(_f32(x)), L.ptr(g.reshape(-1)), L.ptr(b.reshape(-1)), L.ptr(out),
                                        x.numel() // c, c, eps, L.stream()), "chan_layernorm")
    return out


def mish(x):
    out = torch.empty_like(x)
    L.check(L.load().ddk_mish(L.ptr(_f32(x)), L.ptr(out), x.numel(), L.stream()), "mish")
    return out


def tanh(x):
    out = torch.empty_like(x)
    L.check(L.load().ddk_tanh(L.ptr(_f32(x)), L.ptr(out), x.numel(), L.stream()), "tanh")
    return out


def add(a, b):
    out = torch.empty_like(a)
    L.check(L.load().ddk_add(L.ptr(_f32(a)), L.ptr(_f32(b)), L.ptr(out), a.numel(), L.stream()), "add")
    return out


def avgpool2(x):
    b, h, w, c = x.shape
    out = torch.empty((b, h // 2, w // 2, c), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_avgpool2(L.ptr(_f32(x)), L.ptr(out), b, h, w, c, L.stream()), "avgpool2")
    return out


def upsample_nearest2(x):
    b, h, w, c = x.shape
    out = torch.empty((b, 2 * h, 2 * w, c), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_upsample_nearest2(L.ptr(_f32(x)), L.ptr(out), b, h, w, c, L.stream()), "upsample_nearest2")
    return out


def fix_samples(x):
    """x [B,C,H,W] device fp32 -> [B,H,W,C] device fp32 in [0,255] (per-image min-max, utils/eval_helpers.py:37-41)."""
    b, c, h, w = x.shape
    out = torch.empty((b, h, w, c), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_fix_samples(L.ptr(_f32(x)), L.ptr(out), b, c, h, w, L.stream()), "fix_samples")
    return out


# ------------------------------------------------------------------ linear attention core
def linattn(qkv, heads=4, fused_up_to=256):
    """qkv [B,H,W,3*heads*32] -> attention output [B,H,W,heads*32] (before to_out).  Maps of up to `fused_up_to` pixels (<= 256)
    run context + apply in one launch, as in the UNet plan."""
    b, h, w, c3 = qkv.shape
    ctx = torch.empty((b, heads, 32, 32), device=qkv.device, dtype=torch.float32)
    out = torch.empty((b, h, w, c3 // 3), device=qkv.device, dtype=torch.float32)
    lib = L.load()
    if h * w <= min(fused_up_to, 256):      # small maps: context + apply in one launch
        L.check(lib.ddk_linattn_fused_small(L.ptr(_f32(qkv)), L.ptr(ctx), L.ptr(out), b, h * w, heads, L.stream()), "linattn_fused_small")
        return out, ctx
    nbytes = lib.ddk_linattn_context_workspace_bytes(b, h * w, heads)
    ws = torch.empty(nbytes // 4, device=qkv.device, dtype=torch.float32) if nbytes else None
    L.check(lib.ddk_linattn_context(L.ptr(_f32(qkv)), L.ptr(ctx), b, h * w, heads, L.ptr(ws), nbytes, L.stream()), "linattn_context")
    L.check(lib.ddk_linattn_apply(L.ptr(qkv), L.ptr(ctx), L.ptr(out), b, h * w, heads, L.stream()), "linattn_apply")
    return out, ctx


# ------------------------------------------------------------------ time embedding
def time_mlp(t, freqs, w1t, b1, w2t, b2):
    """t int64 [B] -> (Mish(time_mlp(t)) [B,dim], time_mlp(t) [B,dim])"""
    bsz, dim = t.shape[0], w2t.shape[1]
    act = torch.empty((bsz, dim), device=t.device, dtype=torch.float32)
    raw = torch.empty((bsz, dim), device=t.device, dtype=torch.float32)
    if t.dtype != torch.int64:
        raise L.DDKError("time_mlp: t must be int64")
    L.check(L.load().ddk_time_mlp(L.ptr(t), L.ptr(freqs), L.ptr(w1t), L.ptr(b1), L.ptr(w2t), L.ptr(b2), L.ptr(act),
                                  L.ptr(raw), bsz, dim, L.stream()), "time_mlp")
    return act, raw


def time_proj(act, wt, bias):
    bsz, dim = act.shape
    n_out = wt.shape[1]
    out = torch.empty((bsz, n_out), device=act.device, dtype=torch.float32)
    L.check(L.load().ddk_time_proj(L.ptr(_f32(act)), L.ptr(wt), L.ptr(bias), L.ptr(out), bsz, dim, n_out, L.stream()),
            "time_proj")
    return out


def conv1x1_small_n(x, w, bias):
    c = x.shape[-1]
    n_out = w.shape[0]
    out = torch.empty((*x.shape[:-1], n_out), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_conv1x1_small_n(L.ptr(_f32(x)), L.ptr(w.reshape(n_out, c)), L.ptr(bias), L.ptr(out),
                                         x.numel() // c, c, n_out, L.stream()), "conv1x1_small_n")
    return out


# ------------------------------------------------------------------ noise-schedule arithmetic
def q_sample(x, eps, t, sqrt_acp, sqrt_1m_acp):
    out = torch.empty_like(x)
    b = x.shape[0]
    L.check(L.load().ddk_q_sample(L.ptr(_f32(x)), L.ptr(_f32(eps)), L.ptr(t), L.ptr(sqrt_acp), L.ptr(sqrt_1m_acp),
                                  L.ptr(out), b, x.numel() // b, L.stream()), "q_sample")
    return out


def p_sample_update_(x, eps_hat, t, c_recip, c_recipm1, c1, c2, sigma, noise=None, seed=0, stream_id=0):
    """In-place reverse-step update of x (any layout, as long as x / eps_hat / noise agree)."""
    b = x.shape[0]
    L.check(L.load().ddk_p_sample_update(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(noise), L.ptr(t), L.ptr(c_recip),
                                         L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), b, x.numel() // b,
                                         seed, stream_id, L.stream()), "p_sample_update")
    return x


def p_sample_update_multistep_(x, eps_hat, x0_hist, t, c_recip, c_recipm1, c1, c2, c3):
    """In-place DPM-Solver++(2M) update of x and of the history x0_hist (the previous step's clipped x0; zeros before a chain's
    first step); x / eps_hat / x0_hist share one layout."""
    b = x.shape[0]
    L.check(L.load().ddk_p_sample_update_multistep(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(_f32(x0_hist)), L.ptr(t), L.ptr(c_recip),
                                                   L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(c3), b, x.numel() // b, L.stream()),
            "p_sample_update_multistep")
    return x


def p_sample_update_inpaint_(x, eps_hat, known, mask, t, c_recip, c_recipm1, c1, c2, sigma, ka, kb, ja, jb, seed=0, stream_id=0):
    """In-place RePaint op of x per sample row t[b]: the ancestral update with Philox draws, then
    x = mask != 0 ? ka x_known + kb z2 : x, then the row's forward jump where jb != 0; x / eps_hat / known / mask share one layout."""
    b = x.shape[0]
    L.check(L.load().ddk_p_sample_update_inpaint(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(_f32(known)), L.ptr(_f32(mask)), L.ptr(t),
                                                 L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), L.ptr(ka),
                                                 L.ptr(kb), L.ptr(ja), L.ptr(jb), b, x.numel() // b, seed, stream_id, L.stream()),
            "p_sample_update_inpaint")
    return x


def _restore_operands(who, x, eps_hat, y, mask, n, x0_hist=None, takes_mask=True, y_channels=True):
    """What the DDNM step ops share: the shape check of x [B,H,W,C], eps_hat, (x0_hist,) y [B,H/n,W/n(,C)] and mask [B,H/n,W/n] or None
    with its message, then the pointers every C entry starts with and its shape arguments: (x, eps_hat), (y, mask), n, (b, h, w, c)."""
    b, h, w, c = x.shape
    n = int(n)
    if n < 1 or tuple(y.shape) != ((b, h // n, w // n, c) if y_channels else (b, h // n, w // n)) or tuple(eps_hat.shape) != tuple(x.shape) or \
            (x0_hist is not None and tuple(x0_hist.shape) != tuple(x.shape)) or (mask is not None and tuple(mask.shape) != (b, h // n, w // n)):
        hist = "" if x0_hist is None else f"x0_hist {tuple(x0_hist.shape)}, "
        msk = f"mask {None if mask is None else tuple(mask.shape)}, " if takes_mask else ""
        raise L.DDKError(f"{who}: x {tuple(x.shape)}, eps_hat {tuple(eps_hat.shape)}, {hist}y {tuple(y.shape)}, {msk}n = {n}")
    return (L.ptr(_f32(x)), L.ptr(_f32(eps_hat))), (L.ptr(_f32(y)), L.ptr(None if mask is None else _f32(mask))), n, (b, h, w, c)


def p_sample_update_restore_(x, eps_hat, y, n, t, c_recip, c_recipm1, c1, c2, sigma, seed=0, stream_id=0):
    """In-place DDNM super-resolution step of x [B,H,W,C] (NHWC) per sample row t[b]: the clipped x0 is
    shifted so that its n x n block means equal y [B,H/n,W/n,C], then the ancestral update with Philox draws runs on it."""
    xe, (yp, _), n, shape = _restore_operands("p_sample_update_restore", x, eps_hat, y, None, n, takes_mask=False)
    L.check(L.load().ddk_p_sample_update_restore(*xe, yp, n, L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma),
                                                 *shape, seed, stream_id, L.stream()), "p_sample_update_restore")
    return x


def p_sample_update_restore_masked_(x, eps_hat, y, mask, n, t, c_recip, c_recipm1, c1, c2, sigma, seed=0, stream_id=0):
    """In-place DDNM step for A = mask o (n x n average pooling) of x [B,H,W,C] (NHWC) per sample row t[b]:
    where mask [B,H/n,W/n] is nonzero the clipped x0 is shifted so that its block mean equals y [B,H/n,W/n,C] (n = 1: replaced by
    y), elsewhere it is kept; then the ancestral update with Philox draws.  n in {1, 2, 4, 8}; mask None (n >= 2 only): every
    block is measured, p_sample_update_restore_ bit for bit."""
    xe, ym, n, shape = _restore_operands("p_sample_update_restore_masked", x, eps_hat, y, mask, n)
    L.check(L.load().ddk_p_sample_update_restore_masked(*xe, *ym, n, L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2),
                                                        L.ptr(sigma), *shape, seed, stream_id, L.stream()), "p_sample_update_restore_masked")
    return x


def p_sample_update_restore_multistep_(x, eps_hat, x0_hist, y, mask, n, t, c_recip, c_recipm1, c1, c2, c3):
    """In-place DDNM step on the DPM-Solver++(2M) chain of x [B,H,W,C] (NHWC) and of the history x0_hist
    (same layout; zeros before a chain's first step) per sample row t[b]: p_sample_update_restore_masked_'s x0' for y, mask and n,
    then x = (c1 x0' + c2 x) + c3 x0_hist and x0_hist = x0'.  No draw.  n in {1, 2, 4, 8}; mask None (n >= 2 only): every block is
    measured."""
    xe, ym, n, shape = _restore_operands("p_sample_update_restore_multistep", x, eps_hat, y, mask, n, x0_hist=x0_hist)
    L.check(L.load().ddk_p_sample_update_restore_multistep(*xe, L.ptr(_f32(x0_hist)), *ym, n, L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1),
                                                           L.ptr(c1), L.ptr(c2), L.ptr(c3), *shape, L.stream()),
            "p_sample_update_restore_multistep")
    return x


def p_sample_update_restore_noisy_(x, eps_hat, y, mask, n, t, c_recip, c_recipm1, c1, c2, sigma, lam, sgm, seed=0, stream_id=0):
    """In-place DDNM+ step for a noisy measurement of x [B,H,W,C] (NHWC) per sample row t[b]:
    p_sample_update_restore_masked_'s step with the correction of a measured block (n = 1: pixel) scaled by lam[t] and its draw by
    sgm[t] instead of sigma[t]; what is not measured keeps its clipped x0 and the full draw.  n in {1, 2, 4, 8}; mask None (n >= 2
    only): every block is measured."""
    xe, ym, n, shape = _restore_operands("p_sample_update_restore_noisy", x, eps_hat, y, mask, n)
    L.check(L.load().ddk_p_sample_update_restore_noisy(*xe, *ym, n, L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2),
                                                       L.ptr(sigma), L.ptr(lam), L.ptr(sgm), *shape, seed, stream_id, L.stream()),
            "p_sample_update_restore_noisy")
    return x


def p_sample_update_restore_gray_(x, eps_hat, y, mask, n, weights, t, c_recip, c_recipm1, c1, c2, sigma, lam, sgm, seed=0, stream_id=0):
    """In-place DDNM / DDNM+ step for a grey measurement of x [B,H,W,3] (NHWC) per sample row t[b]:
    p_sample_update_restore_noisy_'s step with the block mean replaced by the weighted mean of the n x n x 3 group and the correction
    spread over the channels by A+.  y and mask are [B,H/n,W/n]; mask None: every block measured.  n in {1, 2, 4, 8}; weights "mean"
    (1/3 each) or "luma" (BT.601)."""
    if weights not in L.GRAY_WEIGHTS:
        raise L.DDKError(f"p_sample_update_restore_gray: weights must be 'mean' or 'luma', got {weights!r}")
    xe, ym, n, shape = _restore_operands("p_sample_update_restore_gray", x, eps_hat, y, mask, n, y_channels=False)
    L.check(L.load().ddk_p_sample_update_restore_gray(*xe, *ym, n, L.GRAY_WEIGHTS[weights], L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1),
                                                      L.ptr(c1), L.ptr(c2), L.ptr(sigma), L.ptr(lam), L.ptr(sgm), *shape, seed, stream_id,
                                                      L.stream()), "p_sample_update_restore_gray")
    return x


def separable_apply(x, L_mat, R_mat, out=None):
    """out[b,:,:,c] = L_mat . x[b,:,:,c] . R_mat^T for every image and channel of x [B,H,W,C] (NHWC): L_mat [H,H], R_mat [W,W] fp32
    (DESIGN.md section 3.14).  With (A_h, A_w) of models/diffusion/blur.py it blurs, with (Q_h, Q_w) it forms A+ y.  H and W multiples
    of 16 in [16, 256], C in 1..8.  out may be x."""
    b, h, w, c = x.shape
    if tuple(L_mat.shape) != (h, h) or tuple(R_mat.shape) != (w, w):
        raise L.DDKError(f"separable_apply: x {tuple(x.shape)} needs L [{h},{h}] and R [{w},{w}], got {tuple(L_mat.shape)} and {tuple(R_mat.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape):
        raise L.DDKError(f"separable_apply: out {tuple(out.shape)} must have x's shape {tuple(x.shape)}")
    L.check(L.load().ddk_separable_apply(L.ptr(_f32(x)), L.ptr(_f32(L_mat)), L.ptr(_f32(R_mat)), L.ptr(_f32(out)), b, h, w, c, L.stream()),
            "separable_apply")
    return out


def separable_apply_rect(x, L_mat, R_mat, out=None):
    """out[b,:,:,c] = L_mat . x[b,:,:,c] . R_mat^T for every image and channel of x [B,Hi,Wi,C] (NHWC) with L_mat [Ho,Hi] and R_mat
    [Wo,Wi] fp32: the size-changing form of separable_apply.  With blur.resize_matrix on both axes it is the
    antialiased bicubic reduction, with (Q_h, Q_w) of blur.separable_operands it forms A+ y.  Every size a multiple of 4 in [4, 256], C
    in 1..8.  Returns out [B,Ho,Wo,C], which must not be x; the scratch [B,Ho,Wi,C] is allocated here."""
    b, hi, wi, c = x.shape
    if L_mat.dim() != 2 or R_mat.dim() != 2 or L_mat.shape[1] != hi or R_mat.shape[1] != wi:
        raise L.DDKError(f"separable_apply_rect: x {tuple(x.shape)} needs L [Ho,{hi}] and R [Wo,{wi}], got {tuple(L_mat.shape)} and "
                         f"{tuple(R_mat.shape)}")
    ho, wo = int(L_mat.shape[0]), int(R_mat.shape[0])
    if out is None:
        out = torch.empty((b, ho, wo, c), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (b, ho, wo, c):
        raise L.DDKError(f"separable_apply_rect: out {tuple(out.shape)} must be {(b, ho, wo, c)}")
    scratch = torch.empty((b, ho, wi, c), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_separable_apply_rect(L.ptr(_f32(x)), L.ptr(_f32(L_mat)), L.ptr(_f32(R_mat)), L.ptr(_f32(out)), L.ptr(scratch),
                                              b, hi, wi, ho, wo, c, L.stream()), "separable_apply_rect")
    return out


def p_sample_update_restore_blur_(x, eps_hat, P_h, P_w, Yp, t, c_recip, c_recipm1, c1, c2, sigma, seed=0, stream_id=0, scratch=None):
    """In-place DDNM deblurring step of x [B,H,W,C] (NHWC) per sample row t[b]: the clipped x0 loses its
    range-space part and gains the measurement's, x0' = (x0 - P_h x0 P_w^T) + Yp per channel, then the ancestral update with Philox
    draws runs on it.  P_h [H,H], P_w [W,W]: the projections A+ A of the two axes; Yp = A+ y in x's layout.  An image above 64 KB takes
    two launches through `scratch` (x's shape; allocated here when None)."""
    b, h, w, c = x.shape
    if tuple(eps_hat.shape) != tuple(x.shape) or Yp is None or tuple(Yp.shape) != tuple(x.shape) or \
            (scratch is not None and tuple(scratch.shape) != tuple(x.shape)):
        raise L.DDKError(f"p_sample_update_restore_blur: x {tuple(x.shape)}, eps_hat {tuple(eps_hat.shape)}, "
                         f"Yp {None if Yp is None else tuple(Yp.shape)}, scratch {None if scratch is None else tuple(scratch.shape)}")
    for what, m, side in (("P_h", P_h, h), ("P_w", P_w, w)):
        if m is not None and tuple(m.shape) != (side, side):
            raise L.DDKError(f"p_sample_update_restore_blur: {what} must be [{side},{side}], got {tuple(m.shape)}")
    if scratch is None and h * w * c * 4 > 65536:
        scratch = torch.empty_like(x)
    mats = [L.ptr(None if m is None else _f32(m)) for m in (P_h, P_w)]
    L.check(L.load().ddk_p_sample_update_restore_blur(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), *mats, L.ptr(_f32(Yp)),
                                                      L.ptr(None if scratch is None else _f32(scratch)), L.ptr(t), L.ptr(c_recip),
                                                      L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), b, h, w, c, seed, stream_id,
                                                      L.stream()), "p_sample_update_restore_blur")
    return x


def _cs_operands(who, shape, perm, y, m, device):
    """The checks the compressed-sensing ops share: NHWC shape [B,H,W,C], perm int32 [H*W], y [B,C,m]."""
    b, h, w, c = shape
    if perm is None or tuple(perm.shape) != (h * w,) or perm.dtype != torch.int32 or not perm.is_contiguous() or perm.device != device:
        raise L.DDKError(f"{who}: perm must be a contiguous int32 [{h * w}] tensor on the image's device")
    if y is not None and (tuple(y.shape) != (b, c, m) or y.dtype != torch.float32 or not y.is_contiguous() or y.device != device):
        raise L.DDKError(f"{who}: y must be a contiguous fp32 [{b},{c},{m}] tensor on the image's device, got {tuple(y.shape)} {y.dtype}")
    # a 256 x 256 plane does not fit in LDS: the transform goes through a scratch of the image's size
    return torch.empty(shape, device=device, dtype=torch.float32) if h * w > 32768 else None


def hadamard_measure(x, perm, m):
    """y [B,C,m] = the first m coefficients of the orthonormal Walsh-Hadamard transform (natural order) of every plane of x
    [B,H,W,C] (NHWC fp32) read through perm: a[j] = plane[perm[j]].  perm: int32 [H*W]; H and W powers of
    two in [16, 256], C in 1..8, m a multiple of 4 in [4, H*W]."""
    b, h, w, c = x.shape
    m = int(m)
    scratch = _cs_operands("hadamard_measure", tuple(x.shape), perm, None, m, x.device)
    y = torch.empty((b, c, max(m, 0)), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_hadamard_measure(L.ptr(_f32(x)), L.ptr(perm), L.ptr(y), L.ptr(scratch), b, h, w, c, m, L.stream()), "hadamard_measure")
    return y


def hadamard_adjoint(y, perm, h, w):
    """A^T y = A+ y as an NHWC image [B,h,w,C]: y [B,C,m] padded with zeros to h*w coefficients, transformed and scattered through
    perm."""
    b, c, m = y.shape
    out = torch.empty((b, int(h), int(w), c), device=y.device, dtype=torch.float32)
    scratch = _cs_operands("hadamard_adjoint", tuple(out.shape), perm, y, m, y.device)
    L.check(L.load().ddk_hadamard_adjoint(L.ptr(y), L.ptr(perm), L.ptr(out), L.ptr(scratch), b, int(h), int(w), c, m, L.stream()),
            "hadamard_adjoint")
    return out


def p_sample_update_restore_cs_(x, eps_hat, y, perm, t, c_recip, c_recipm1, c1, c2, sigma, seed=0, stream_id=0):
    """In-place DDNM compressed-sensing step of x [B,H,W,C] (NHWC) per sample row t[b]: the clipped x0's
    first m Walsh-Hadamard coefficients (of each plane read through perm) are replaced by y [B,C,m], then the ancestral update with
    Philox draws runs on the result."""
    if tuple(eps_hat.shape) != tuple(x.shape) or y is None or y.dim() != 3:
        raise L.DDKError(f"p_sample_update_restore_cs: x {tuple(x.shape)}, eps_hat {tuple(eps_hat.shape)}, "
                         f"y {None if y is None else tuple(y.shape)}")
    b, h, w, c = x.shape
    m = int(y.shape[2])
    scratch = _cs_operands("p_sample_update_restore_cs", tuple(x.shape), perm, y, m, x.device)
    L.check(L.load().ddk_p_sample_update_restore_cs(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(y), L.ptr(perm), L.ptr(scratch), L.ptr(t),
                                                    L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), b, h, w, c, m, seed,
                                                    stream_id, L.stream()), "p_sample_update_restore_cs")
    return x


_FFT_TWIDDLES = {}


def fft_twiddles(L, device):
    """The device transform's twiddle table for a longest axis of L: fp32 [L/2, 2] (models/diffusion/psf.py twiddles), kept per
    (L, device)."""
    key = (int(L), str(device))
    if key not in _FFT_TWIDDLES:
        from models.diffusion.psf import twiddles
        _FFT_TWIDDLES[key] = torch.from_numpy(twiddles(L)).to(device)
    return _FFT_TWIDDLES[key]


def _fft_operands(who, shape, device, **arrays):
    """The checks the FFT ops share: NHWC shape [B,H,W,C]; each named array a contiguous fp32 tensor of the
    given shape on the image's device.  Returns (twiddles, scratch): the scratch is the complex T of twice the image's size for planes
    above 16384 pixels, else None."""
    b, h, w, c = shape
    for what, (v, want) in arrays.items():
        if v is None or tuple(v.shape) != want or v.dtype != torch.float32 or not v.is_contiguous() or v.device != device:
            raise L.DDKError(f"{who}: {what} must be a contiguous fp32 [{','.join(map(str, want))}] tensor on the image's device")
    pow2 = lambda v: 16 <= v <= 256 and v & (v - 1) == 0
    if not (pow2(h) and pow2(w)):
        raise L.DDKError(f"{who}: H and W must be powers of two in [16, 256], got [{h},{w}]")
    return fft_twiddles(max(h, w), device), (torch.empty((2, *shape), device=device, dtype=torch.float32) if h * w > 16384 else None)


def circular_conv(x, S):
    """out [B,H,W,C] = Re F2^-1(S . F2(x)) / (H W) per plane of x [B,H,W,C] (NHWC fp32): circular convolution through a complex FFT in
    LDS.  S: fp32 [H,W,2], the complex multiplier (re, im) in natural frequency order -- psf.psf_spectrum for
    the blur A, psf.psf_projection's P^ for A+.  H and W powers of two in [16, 256], C in 1..8."""
    b, h, w, c = x.shape
    tw, scratch = _fft_operands("circular_conv", tuple(x.shape), x.device, S=(S, (h, w, 2)))
    out = torch.empty_like(x, dtype=torch.float32)
    L.check(L.load().ddk_circular_conv(L.ptr(_f32(x)), L.ptr(S), L.ptr(tw), L.ptr(out), L.ptr(scratch), b, h, w, c, L.stream()), "circular_conv")
    return out


def p_sample_update_restore_fft_(x, eps_hat, mask, Yp, t, c_recip, c_recipm1, c1, c2, sigma, seed=0, stream_id=0):
    """In-place DDNM deconvolution step of x [B,H,W,C] (NHWC) per sample row t[b]: the kept frequencies
    (mask [H,W] fp32, nonzero = kept) of the clipped x0's 2-D spectrum are zeroed, Yp = A+ y [B,H,W,C] is added, then the ancestral
    update with Philox draws runs on the result."""
    if tuple(eps_hat.shape) != tuple(x.shape) or Yp is None or tuple(Yp.shape) != tuple(x.shape):
        raise L.DDKError(f"p_sample_update_restore_fft: x {tuple(x.shape)}, eps_hat {tuple(eps_hat.shape)}, "
                         f"Yp {None if Yp is None else tuple(Yp.shape)}")
    b, h, w, c = x.shape
    tw, scratch = _fft_operands("p_sample_update_restore_fft", tuple(x.shape), x.device, mask=(mask, (h, w)), Yp=(Yp, tuple(x.shape)))
    L.check(L.load().ddk_p_sample_update_restore_fft(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(mask), L.ptr(tw), L.ptr(Yp), L.ptr(scratch),
                                                     L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), b, h, w, c,
                                                     seed, stream_id, L.stream()), "p_sample_update_restore_fft")
    return x


def circular_spectrum(x, S):
    """out [B,C,H W,2] = S . F2(x) per plane of x [B,H,W,C] (NHWC fp32), complex (re, im), left in the device transform's own order:
    frequency (u, v) at index brev(u) W + brev(v), brev reversing log2 H and log2 W bits.  With S =
    psf.psf_projection's P^ it is the spectrum of A+ y that p_sample_update_restore_fft_noisy_ reads.  S, shapes: as circular_conv."""
    b, h, w, c = x.shape
    tw, scratch = _fft_operands("circular_spectrum", tuple(x.shape), x.device, S=(S, (h, w, 2)))
    out = torch.empty((b, c, h * w, 2), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_circular_spectrum(L.ptr(_f32(x)), L.ptr(S), L.ptr(tw), L.ptr(out), L.ptr(scratch), b, h, w, c, L.stream()),
            "circular_spectrum")
    return out


def p_sample_update_restore_fft_noisy_(x, eps_hat, mask, gain, nsc, Yhat, t, c_recip, c_recipm1, c1, c2, sigma, seed=0, stream_id=0):
    """In-place DDNM+ deconvolution step of x [B,H,W,C] (NHWC) per sample row t[b], for a blurred image with
    noise: per frequency the clipped x0's spectrum moves towards Yhat (circular_spectrum of y with P^, [B,C,H W,2]) by lam, and the
    Philox draw is shaped by phi, both from the row's sigma, nsc[t[b]] and gain [H,W] (psf.psf_noisy_operands); mask [H,W] fp32 is
    nonzero at the kept frequencies."""
    b, h, w, c = x.shape
    if tuple(eps_hat.shape) != tuple(x.shape) or Yhat is None or tuple(Yhat.shape) != (b, c, h * w, 2):
        raise L.DDKError(f"p_sample_update_restore_fft_noisy: x {tuple(x.shape)}, eps_hat {tuple(eps_hat.shape)}, "
                         f"Yhat {None if Yhat is None else tuple(Yhat.shape)}")
    if nsc is None or nsc.dim() != 1 or tuple(nsc.shape) != tuple(c1.shape):
        raise L.DDKError("p_sample_update_restore_fft_noisy: nsc must have one entry per row of c1")
    tw, scratch = _fft_operands("p_sample_update_restore_fft_noisy", tuple(x.shape), x.device, mask=(mask, (h, w)), gain=(gain, (h, w)),
                                nsc=(nsc, tuple(nsc.shape)), Yhat=(Yhat, (b, c, h * w, 2)))
    if scratch is not None:       # T and T2
        scratch = torch.empty((4, *x.shape), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_p_sample_update_restore_fft_noisy(
        L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(mask), L.ptr(gain), L.ptr(nsc), L.ptr(tw), L.ptr(Yhat), L.ptr(scratch), L.ptr(t),
        L.ptr(c_recip), L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), b, h, w, c, seed, stream_id, L.stream()),
        "p_sample_update_restore_fft_noisy")
    return x


# ---------------------------------------------------------------- Diffusion Posterior Sampling (csrc/guidance.hip)
RESPONSES = {"linear": 0, "saturate": 1}      # DDK_RESPONSE_LINEAR, DDK_RESPONSE_SATURATE (include/ddk.h)
MEASURE_BLOCKS = (1, 2, 4, 8)


def measure_residual(img, y, mask=None, n=1, response="linear", gain=1.0):
    """(r, dist) of the measurement y [B,H/n,W/n,C] of img [B,H,W,C] (NHWC fp32) under A = mask o (n x n block mean) and the pointwise
    response phi: r = mask phi'(u) (phi(u) - y) with u the block mean, dist [B] = sqrt(sum mask (phi(u) - y)^2) per image, summed in
    double in a fixed order.  mask [B,H/n,W/n] fp32 (nonzero = measured) or None; response "linear" (phi(u) = u) or "saturate"
    (phi(u) = clamp(gain u, -1, 1))."""
    if response not in RESPONSES:
        raise L.DDKError(f"measure_residual: response must be one of {tuple(RESPONSES)}, got {response!r}")
    if img.dim() != 4 or n not in MEASURE_BLOCKS or img.shape[1] % n or img.shape[2] % n:
        raise L.DDKError(f"measure_residual: img {tuple(img.shape)} must be [B,H,W,C] with n = {n!r} in {MEASURE_BLOCKS} dividing H and W")
    b, h, w, c = img.shape
    want = (b, h // n, w // n, c)
    if tuple(y.shape) != want or (mask is not None and tuple(mask.shape) != want[:3]):
        raise L.DDKError(f"measure_residual: img {tuple(img.shape)} at n = {n} needs y {want} and mask {want[:3]} or None, got "
                         f"{tuple(y.shape)} and {None if mask is None else tuple(mask.shape)}")
    r = torch.empty(want, device=img.device, dtype=torch.float32)
    dist = torch.empty((b,), device=img.device, dtype=torch.float32)
    lib = L.load()
    nbytes = lib.ddk_measure_residual_workspace_bytes(b, h, w, c, n)
    ws = _ws(img.device, nbytes, "measure") if nbytes else None
    L.check(lib.ddk_measure_residual(L.ptr(_f32(img)), L.ptr(_f32(y)), None if mask is None else L.ptr(_f32(mask)), n, RESPONSES[response],
                                     float(gain), L.ptr(r), L.ptr(dist), b, h, w, c, L.ptr(ws), nbytes, L.stream()), "measure_residual")
    return r, dist


def measure_adjoint(r, dist, gout, n=1):
    """v [B,H,W,C] = s[b] r[b, i / n, j / n, c] / n^2 with s[b] = gout[b] / dist[b] (0 where dist[b] == 0): the gradient of
    sum_b gout[b] dist[b] with respect to img, from measure_residual's r [B,H/n,W/n,C] and dist [B]; gout [B] stays on the device."""
    if r.dim() != 4 or n not in MEASURE_BLOCKS or tuple(dist.shape) != (r.shape[0],) or tuple(gout.shape) != (r.shape[0],):
        raise L.DDKError(f"measure_adjoint: r {tuple(r.shape)}, dist {tuple(dist.shape)}, gout {tuple(gout.shape)}, n = {n!r}")
    b, h, w, c = r.shape
    v = torch.empty((b, h * n, w * n, c), device=r.device, dtype=torch.float32)
    L.check(L.load().ddk_measure_adjoint(L.ptr(_f32(r)), L.ptr(_f32(dist)), L.ptr(_f32(gout)), n, L.ptr(v), b, h * n, w * n, c, L.stream()),
            "measure_adjoint")
    return v


def x0_from_eps(x, eps, t, c_recip, c_recipm1, clip=True):
    """The x0 estimate of a reverse step per sample row t[b]: c_recip x - c_recipm1 eps, clamped to [-1, 1] with clip -- the clipped x0
    of p_sample_update_, bit for bit (any layout, as long as x and eps agree)."""
    if tuple(eps.shape) != tuple(x.shape):
        raise L.DDKError(f"x0_from_eps: x {tuple(x.shape)} and eps {tuple(eps.shape)} must agree")
    b = x.shape[0]
    out = torch.empty_like(x, memory_format=torch.contiguous_format)
    L.check(L.load().ddk_x0_from_eps(L.ptr(_f32(x)), L.ptr(_f32(eps)), L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1), int(bool(clip)), L.ptr(out),
                                     b, x.numel() // b, L.stream()), "x0_from_eps")
    return out


def x0_from_eps_bwd(x, eps, dx0, t, c_recip, c_recipm1, clip=True):
    """(dx, deps) = (c_recip m dx0, -c_recipm1 m dx0), m = 1 where the unclipped x0 lies in [-1, 1] (everywhere without clip)."""
    if tuple(eps.shape) != tuple(x.shape) or tuple(dx0.shape) != tuple(x.shape):
        raise L.DDKError(f"x0_from_eps_bwd: x {tuple(x.shape)}, eps {tuple(eps.shape)} and dx0 {tuple(dx0.shape)} must agree")
    b = x.shape[0]
    dx = torch.empty_like(x, memory_format=torch.contiguous_format)
    deps = torch.empty_like(x, memory_format=torch.contiguous_format)
    L.check(L.load().ddk_x0_from_eps_bwd(L.ptr(_f32(x)), L.ptr(_f32(eps)), L.ptr(_f32(dx0)), L.ptr(t), L.ptr(c_recip), L.ptr(c_recipm1),
                                         int(bool(clip)), L.ptr(dx), L.ptr(deps), b, x.numel() // b, L.stream()), "x0_from_eps_bwd")
    return dx, deps


def p_sample_update_guided_(x, eps_hat, g, t, c_recip, c_recipm1, c1, c2, sigma, zeta, noise=None, seed=0, stream_id=0):
    """p_sample_update_ (same rule, same Philox key or injected noise), then x <- x - zeta[t[b]] g, in place; g has x's layout and zeta
    is a row table like the others.  A row whose zeta is 0 takes no step: all zero gives p_sample_update_'s bits."""
    if tuple(eps_hat.shape) != tuple(x.shape) or tuple(g.shape) != tuple(x.shape) or (noise is not None and tuple(noise.shape) != tuple(x.shape)):
        raise L.DDKError(f"p_sample_update_guided: x {tuple(x.shape)}, eps_hat {tuple(eps_hat.shape)}, g {tuple(g.shape)}, noise "
                         f"{None if noise is None else tuple(noise.shape)} must agree")
    if zeta is None or zeta.dim() != 1 or tuple(zeta.shape) != tuple(c1.shape):
        raise L.DDKError("p_sample_update_guided: zeta must have one entry per row of c1")
    b = x.shape[0]
    L.check(L.load().ddk_p_sample_update_guided(L.ptr(_f32(x)), L.ptr(_f32(eps_hat)), L.ptr(noise), L.ptr(_f32(g)), L.ptr(t), L.ptr(c_recip),
                                                L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(sigma), L.ptr(_f32(zeta)), b, x.numel() // b,
                                                seed, stream_id, L.stream()), "p_sample_update_guided")
    return x


def randn(shape, device, seed, step, stream_id=0):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    L.check(L.load().ddk_randn(L.ptr(out), out.numel(), seed, step, stream_id, L.stream()), "randn")
    return out


def vlb_terms(x, x_t, eps_hat, t, c_recip, c_recipm1, c1, c2, post_logvar, eps=None):
    """Per-sample VLB term in bits/dim (KL for t > 0, discretised NLL at t == 0) and, with eps, sum (eps - eps_hat)^2."""
    b = x.shape[0]
    vlb = torch.empty((b,), device=x.device, dtype=torch.float32)
    sq = torch.empty((b,), device=x.device, dtype=torch.float32) if eps is not None else None
    lib = L.load()
    nbytes = lib.ddk_vlb_terms_workspace_bytes(b, x.numel() // b)
    ws = _ws(x.device, nbytes, "vlb")
    L.check(lib.ddk_vlb_terms(L.ptr(_f32(x)), L.ptr(_f32(x_t)), L.ptr(_f32(eps_hat)), L.ptr(eps), L.ptr(t), L.ptr(c_recip),
                              L.ptr(c_recipm1), L.ptr(c1), L.ptr(c2), L.ptr(post_logvar), L.ptr(vlb), L.ptr(sq), b,
                              x.numel() // b, L.ptr(ws), nbytes, L.stream()), "vlb_terms")
    return vlb, sq


def sq_err_sum(a, b):
    bsz = a.shape[0]
    out = torch.empty((bsz,), device=a.device, dtype=torch.float32)
    L.check(L.load().ddk_sq_err_sum(L.ptr(_f32(a)), L.ptr(_f32(b)), L.ptr(out), bsz, a.numel() // bsz, L.stream()),
            "sq_err_sum")
    return out


SSIM_WINDOW = 11


def image_metrics(a, b, mask=None):
    """PSNR, SSIM and MSE per image of two uint8 device tensors [N, H, W, C] (C in 1..4, H, W >= 11).
    mask: optional uint8 / bool [N, H, W]; the squared error then covers only the pixels where it is nonzero (all channels);
    SSIM always covers the whole image.  Returns host tensors: psnr [N] float64 (inf for identical images, nan when the mask
    selects nothing), ssim [N] float32, mse [N] float64, and the exact integers behind them, sq_sum and count [N] int64.
    Wrong dtypes, mismatched shapes and images smaller than one SSIM window raise ValueError before any device work."""
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise ValueError(f"image_metrics: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t))}")
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"image_metrics: a and b must share one [N, H, W, C] shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    n, h, w, c = a.shape
    if n < 1 or not 1 <= c <= 4:
        raise ValueError(f"image_metrics: N must be positive and C in 1..4, got {tuple(a.shape)}")
    if h < SSIM_WINDOW or w < SSIM_WINDOW:
        raise ValueError(f"image_metrics: H and W must be at least {SSIM_WINDOW} (one SSIM window), got {h} x {w}")
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"image_metrics: mask must be a uint8 or bool tensor, got {getattr(mask, 'dtype', type(mask))}")
        if tuple(mask.shape) != (n, h, w):
            raise ValueError(f"image_metrics: mask must be [N, H, W] = {(n, h, w)}, got {tuple(mask.shape)}")
    if not (a.is_cuda and b.is_cuda and (mask is None or mask.is_cuda)):
        raise L.DDKError("image_metrics: HIP kernels need ROCm device tensors; there is no CPU fallback")
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
    a, b = a.contiguous(), b.contiguous()
    lib = L.load()
    sq = torch.empty((n, 2), device=a.device, dtype=torch.int64)      # the kernel's unsigned 64-bit pairs; both stay far below 2^63
    ssim = torch.empty((n,), device=a.device, dtype=torch.float32)
    nbytes = lib.ddk_image_metrics_workspace_bytes(n, h, w, c)
    ws = _ws(a.device, nbytes, "image_metrics")
    L.check(lib.ddk_image_metrics(L.ptr(a), L.ptr(b), L.ptr(mask), n, h, w, c, L.ptr(sq), L.ptr(ssim), L.ptr(ws), nbytes, L.stream()),
            "image_metrics")
    sq = sq.cpu()
    sq_sum, count = sq[:, 0].contiguous(), sq[:, 1].contiguous()
    s, k = sq_sum.double(), count.double()
    mse = s / k                                                        # 0 / 0 = nan: an empty mask has no error to report
    psnr = 10.0 * torch.log10(255.0 ** 2 * k / s)                      # k / 0 = inf, 0 / 0 = nan
    return dict(psnr=psnr, ssim=ssim.cpu(), mse=mse, sq_sum=sq_sum, count=count)


MANIFOLD_MAX_K = 7            # csrc/manifold.hip keeps a row's 8 smallest distances: k + 1 <= 8
MANIFOLD_TILE = 128           # rows (and columns) of a workgroup's distance tile


def _manifold_features(what, name, t):
    """The checks every feature matrix passes before any device work; returns it with D zero-padded to a multiple of 4."""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: {name} must be a non-empty [N, D] matrix, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise L.DDKError(f"{what}: HIP kernels need ROCm device tensors; there is no CPU fallback")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{what}: {name} holds non-finite features")
    pad = -t.shape[1] % 4
    if pad:                                        # zero columns change no norm and no dot product (the `spatial` features: D = 2023)
        t = torch.nn.functional.pad(t, (0, pad))
    return t.contiguous()


def _manifold_radii_arg(what, name, r, n, device):
    if r is None:
        return None
    if not torch.is_tensor(r) or r.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be a float32 tensor or None, got {getattr(r, 'dtype', type(r))}")
    if tuple(r.shape) != (n,):
        raise ValueError(f"{what}: {name} must be [{n}], one radius per row, got {tuple(r.shape)}")
    if not r.is_cuda:
        raise L.DDKError(f"{what}: HIP kernels need ROCm device tensors; there is no CPU fallback")
    return r.contiguous()


def manifold_radii_splits(n):
    """How many workgroups share the columns of one 128-row block in manifold_radii at this N (from the entry's workspace size)."""
    nbytes = L.load().ddk_knn_radii_workspace_bytes(n)
    return (nbytes // 4 // n - 1) // (MANIFOLD_MAX_K + 1)


def manifold_radii(x, k=3):
    """Squared distance of every row of the float32 device matrix x [N, D] to its k-th nearest neighbour: element k of the row's
    sorted distances to all N rows, itself included (the reference ManifoldEstimator.manifold_radii with nhood_sizes=(k,)).
    Returns a float32 [N] device tensor.  DESIGN.md section 3.16."""
    if not isinstance(k, int) or not 1 <= k <= MANIFOLD_MAX_K:
        raise ValueError(f"manifold_radii: k must be an integer in 1..{MANIFOLD_MAX_K}, got {k!r}")
    if torch.is_tensor(x) and x.dim() == 2 and x.shape[0] < k + 1:
        raise ValueError(f"manifold_radii: N must be at least k + 1 = {k + 1}, got {x.shape[0]}")
    x = _manifold_features("manifold_radii", "x", x)
    n, d = x.shape
    lib = L.load()
    radii = torch.empty((n,), device=x.device, dtype=torch.float32)
    nbytes = lib.ddk_knn_radii_workspace_bytes(n)
    ws = _ws(x.device, nbytes, "manifold")
    L.check(lib.ddk_knn_radii(L.ptr(x), n, d, k, L.ptr(radii), L.ptr(ws), nbytes, L.stream()), "knn_radii")
    return radii


def manifold_members(a, ra, b, rb):
    """One pass over the distances between the rows of a [Na, D] and b [Nb, D] (float32 device tensors):
    a_in[i] = some row j of b has d(a_i, b_j) <= rb[j], b_in[j] = some row i of a has d(a_i, b_j) <= ra[i].
    ra [Na] / rb [Nb] are float32 device tensors; with ra None b_in is None, with rb None a_in is None.
    Returns (a_in, b_in), bool device tensors.  DESIGN.md section 3.16."""
    what = "manifold_members"
    if ra is None and rb is None:
        raise ValueError(f"{what}: neither ra nor rb given: nothing to compute")
    for name, t in (("a", a), ("b", b)):                                  # dtype and shape of both before either touches the device
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"{what}: a and b must be [Na, D] and [Nb, D] with one D, got {tuple(a.shape)} and {tuple(b.shape)}")
    na, nb = a.shape[0], b.shape[0]
    for name, r, n in (("ra", ra, na), ("rb", rb, nb)):
        if r is not None and (not torch.is_tensor(r) or r.dtype != torch.float32 or tuple(r.shape) != (n,)):
            raise ValueError(f"{what}: {name} must be a float32 [{n}] tensor or None, got "
                             f"{getattr(r, 'dtype', type(r))} {tuple(getattr(r, 'shape', ()))}")
    a, b = _manifold_features(what, "a", a), _manifold_features(what, "b", b)
    ra, rb = _manifold_radii_arg(what, "ra", ra, na, a.device), _manifold_radii_arg(what, "rb", rb, nb, a.device)
    lib = L.load()
    a_in = torch.empty((na,), device=a.device, dtype=torch.uint8) if rb is not None else None
    b_in = torch.empty((nb,), device=a.device, dtype=torch.uint8) if ra is not None else None
    nbytes = lib.ddk_manifold_members_workspace_bytes(na, nb)
    ws = _ws(a.device, nbytes, "manifold")
    L.check(lib.ddk_manifold_members(L.ptr(a), L.ptr(ra), na, L.ptr(b), L.ptr(rb), nb, a.shape[1], L.ptr(a_in), L.ptr(b_in), L.ptr(ws),
                                     nbytes, L.stream()), "manifold_members")
    return (a_in.bool() if a_in is not None else None), (b_in.bool() if b_in is not None else None)


def manifold_ball_counts(a, ra, b):
    """counts[i] = the number of rows j of b [Nb, D] with d(a_i, b_j) <= ra[i], for the rows of a [Na, D] (float32 device tensors,
    ra float32 [Na]): how many samples lie in each reference row's k-NN ball (density / coverage, Naeem et al. 2020).
    Returns an int32 [Na] device tensor.  DESIGN.md section 3.20."""
    what = "manifold_ball_counts"
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"{what}: a and b must be [Na, D] and [Nb, D] with one D, got {tuple(a.shape)} and {tuple(b.shape)}")
    na, nb = a.shape[0], b.shape[0]
    if not torch.is_tensor(ra) or ra.dtype != torch.float32 or tuple(ra.shape) != (na,):
        raise ValueError(f"{what}: ra must be a float32 [{na}] tensor, got {getattr(ra, 'dtype', type(ra))} "
                         f"{tuple(getattr(ra, 'shape', ()))}")
    a, b = _manifold_features(what, "a", a), _manifold_features(what, "b", b)
    ra = _manifold_radii_arg(what, "ra", ra, na, a.device)
    lib = L.load()
    counts = torch.empty((na,), device=a.device, dtype=torch.int32)
    nbytes = lib.ddk_manifold_ball_counts_workspace_bytes(na, nb)
    ws = _ws(a.device, nbytes, "manifold")
    L.check(lib.ddk_manifold_ball_counts(L.ptr(a), L.ptr(ra), na, L.ptr(b), nb, a.shape[1], L.ptr(counts), L.ptr(ws), nbytes, L.stream()),
            "manifold_ball_counts")
    return counts


POLY_MMD_MAX_ROWS = 1 << 24   # csrc/manifold.hip MF_MAX_ROWS: rows of all segments together, per side


def poly_mmd_sums(a, b, segments=1, gamma=None, coef0=1.0):
    """The three kernel-matrix sums of the unbiased MMD^2 with k(x, y) = (gamma x.y + coef0)^3, per segment (KID).
    a [S ma, D] and b [S mb, D] are float32 device tensors holding S = `segments` consecutive groups of ma and of mb rows
    (ma, mb >= 2); gamma None means 1 / D.  Returns a float64 [S, 3] device tensor: sum_{i != j} k(a_i, a_j),
    sum_{i != j} k(b_i, b_j), sum_{i, j} k(a_i, b_j) over the rows of each segment.  fp32 up to k, double sums in a fixed order:
    the same bits from run to run.  DESIGN.md section 3.20."""
    what = "poly_mmd_sums"
    if not isinstance(segments, int) or isinstance(segments, bool) or segments < 1:
        raise ValueError(f"{what}: segments must be a positive integer, got {segments!r}")
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.shape[1] < 1:
        raise ValueError(f"{what}: a and b must be [S ma, D] and [S mb, D] with one D, got {tuple(a.shape)} and {tuple(b.shape)}")
    for name, t in (("a", a), ("b", b)):
        if t.shape[0] % segments or t.shape[0] // segments < 2:
            raise ValueError(f"{what}: {name} must hold {segments} segments of at least 2 rows each, got {t.shape[0]} rows")
        if t.shape[0] > POLY_MMD_MAX_ROWS:
            raise ValueError(f"{what}: {name} has {t.shape[0]} rows, more than {POLY_MMD_MAX_ROWS}")
    d = a.shape[1]
    gamma = 1.0 / d if gamma is None else gamma
    for name, v in (("gamma", gamma), ("coef0", coef0)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    a, b = _manifold_features(what, "a", a), _manifold_features(what, "b", b)
    ma, mb = a.shape[0] // segments, b.shape[0] // segments
    lib = L.load()
    sums = torch.empty((segments, 3), device=a.device, dtype=torch.float64)
    nbytes = lib.ddk_poly_mmd_workspace_bytes(segments, ma, mb)
    ws = _ws(a.device, nbytes, "poly_mmd")
    L.check(lib.ddk_poly_mmd_sums(L.ptr(a), L.ptr(b), segments, ma, mb, a.shape[1], float(gamma), float(coef0), L.ptr(sums), L.ptr(ws), nbytes,
                                  L.stream()), "poly_mmd_sums")
    return sums


# ================================================================== training path (backward kernels)
CONV4X4_S2 = 4
_scratch = {}


def _ws(device, nbytes, tag="ws"):
    """Reusable scratch buffer per (device, tag): backward kernels need short-lived workspaces.

    Under stream capture the buffer comes from the capturing graph's PRIVATE memory pool instead (a plain allocation while
    capturing): the graph then owns every scratch address its kernels were recorded with, for as long as it lives.  Handing
    out the shared buffer would bake its address into the graph while a later, larger eager request replaces (and frees)
    it -- the replay would write into memory that belongs to someone else."""
    n = max(nbytes, 16) // 4 + 4
    if device is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return torch.empty(n, device=device, dtype=torch.float32)
    key = (str(device), tag, torch.cuda.current_stream().cuda_stream)     # per stream: two branches of a step may run side by side
    buf = _scratch.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(n, device=device, dtype=torch.float32)
        _scratch[key] = buf
    return buf


def pack_conv_weight_dgrad(w, i_pad=None, o_pad=None):
    """OIHW -> [I_pad][KH*KW][O_pad] with flipped taps: operand of the input-gradient conv."""
    o, i, kh, kw = w.shape
    i_pad = pad32(i) if i_pad is None else i_pad
    o_pad = o if o_pad is None else o_pad
    out = torch.empty((i_pad, kh * kw, o_pad), device=w.device, dtype=torch.float32)
    L.check(L.load().ddk_pack_conv_weight_dgrad(L.ptr(_f32(w.contiguous())), L.ptr(out), o, i, kh, kw, i_pad, o_pad, L.stream()),
            "pack_conv_weight_dgrad")
    return out


def zero_stuff2(dy, h_out, w_out):
    b, h, w, c = dy.shape
    out = torch.empty((b, h_out, w_out, c), device=dy.device, dtype=torch.float32)
    L.check(L.load().ddk_zero_stuff2(L.ptr(_f32(dy)), L.ptr(out), b, h, w, h_out, w_out, c, L.stream()), "zero_stuff2")
    return out


# The slab reduces of a backward pass in one launch.  Inside `with deferred_wgrad():` every conv_wgrad_ keeps its slabs in a buffer of
# its own and only records the reduce; leaving the block (or flush_wgrad()) runs them all with ddk_wgrad_reduce_jobs -- 232 reduce
# launches of 4-7 us per cfg3 optimiser step before.  Nothing may read the gradients in between (the trainers wrap exactly one
# forward + backward); outside the block every call reduces at once, as before.
_wgrad_pending = None         # None: immediate reduces; list of (job struct, slab tensor) while deferring
_rows_pending = []            # (job struct, rows tensor): the GroupNorm / LayerNorm parameter-gradient row sums deferred alongside


# The deferred weight-gradient launches of a backward pass write only their own slabs, which nothing reads before the reduce at the end of
# the pass: they run on a SIDE stream, forked from the caller's stream after the tensors they read were produced and joined in front
# of the reduce -- beside the input-gradient / GroupNorm chain instead of inside it (a captured step keeps the two branches: most of
# these launches are small and latency-bound, and so is the chain).  The tensors a side launch reads are kept alive until the join.
WGRAD_SIDE_STREAM = True
_wgrad_side = {}              # device index -> torch.cuda.Stream
_wgrad_keep = []              # tensors read by side-stream launches since the last join
_wgrad_forked = None          # the side stream with launches the caller's stream has not waited for yet


def _side_stream(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _wgrad_side.get(idx)
    if st is None:
        st = _wgrad_side[idx] = torch.cuda.Stream(device=device)
    return st


WGRAD_SIDE_BATCH = 16            # 8 .. 64 measure alike (16.2 - 16.6 ms per cfg3 step against 16.7 - 16.8 on the caller's stream)
WGRAD_SIDE_MAX_PIXELS = 65536    # larger maps fill the chip by themselves: nothing to overlap, and the forks cost (cfg5 115.4 -> 117.1 ms)
_wgrad_queue = []             # deferred weight-gradient launches not yet issued


def _launch_side_queue():
    """issue the queued launches on the side stream, behind one fork from the caller's stream"""
    global _wgrad_forked
    if not _wgrad_queue:
        return
    lib = L.load()
    side = _side_stream(_wgrad_queue[0][1].device)
    seen = set()
    for entry in _wgrad_queue:                                 # operands and slab buffers are ready on the stream(s) that queued them
        st = entry[-1]
        if st.cuda_stream not in seen:
            seen.add(st.cuda_stream)
            side.wait_stream(st)
    with torch.cuda.stream(side):
        for kind, x, dy, grad_w, grad_b, dims, slab, nbytes, job, _ in _wgrad_queue:
            L.check(lib.ddk_conv_wgrad_defer(kind, L.ptr(x), L.ptr(dy), L.ptr(grad_w), L.ptr(grad_b), *dims, L.ptr(slab), nbytes,
                                             C.byref(job), L.stream()), "conv_wgrad_defer")
            _wgrad_keep.append((x, dy))
    del _wgrad_queue[:]
    _wgrad_forked = side


def _join_side():
    global _wgrad_forked
    _launch_side_queue()
    if _wgrad_forked is not None:
        torch.cuda.current_stream().wait_stream(_wgrad_forked)
        _wgrad_forked = None


class deferred_wgrad:
    def __enter__(self):
        global _wgrad_pending
        self._outer = _wgrad_pending
        if _wgrad_pending is None:
            _wgrad_pending = []
        return self

    def __exit__(self, exc_type, exc, tb):
        global _wgrad_pending
        if self._outer is None:
            try:
                if exc_type is None:
                    flush_wgrad()
            finally:
                if exc_type is not None:
                    del _wgrad_queue[:]
                _join_side()
                del _wgrad_keep[:]
                _wgrad_pending = None
                del _rows_pending[:]
        return False


def _rows_sum_targets(rows, nbatch, batch_stride, nrows, row_stride, targets, n):
    """targets[k][:n] += sum_r rows[k * batch_stride + r * row_stride + :n] (ddk_rows_sum_targets); inside deferred_wgrad() the sum is
    only recorded (`rows` is kept alive) and runs with the others when the block ends"""
    if _wgrad_pending is not None:
        job = L.RowsSumJob()
        job.rows = rows.data_ptr()
        for k in range(4):
            job.out[k] = targets[k].data_ptr() if k < len(targets) and targets[k] is not None else None
        job.batch_stride, job.row_stride, job.nbatch, job.nrows, job.n = batch_stride, row_stride, nbatch, nrows, n
        _rows_pending.append((job, rows))
        return
    t = [L.ptr(x) for x in (list(targets) + [None] * 4)[:4]]
    L.check(L.load().ddk_rows_sum_targets(L.ptr(rows), nbatch, batch_stride, nrows, row_stride, t[0], t[1], t[2], t[3], n, 1, L.stream()),
            "rows_sum_targets")


def _flush_rows():
    global _rows_pending
    pending, _rows_pending = _rows_pending, []
    lib = L.load()
    while pending:
        seen, batch, rest = set(), [], []
        for job, rows in pending:            # two sums into the same gradient must not share a launch
            keys = [p for p in job.out if p]
            if any(k in seen for k in keys):
                rest.append((job, rows))
            else:
                batch.append((job, rows))
                seen.update(keys)
        jobs = (L.RowsSumJob * len(batch))(*[j for j, _ in batch])
        L.check(lib.ddk_rows_sum_jobs(jobs, len(batch), L.stream()), "rows_sum_jobs")
        pending = rest


def flush_wgrad():
    """run the recorded reduces: one launch per set of jobs with pairwise distinct targets (normally one)"""
    global _wgrad_pending
    if _rows_pending:
        _flush_rows()
    _join_side()
    if not _wgrad_pending:
        del _wgrad_keep[:]
        return 0
    pending, _wgrad_pending = _wgrad_pending, []
    lib = L.load()
    launches = 0
    while pending:
        seen, batch, rest = set(), [], []
        for job, slab in pending:        # two reduces into the same gradient elements must not share a launch (no such pair in this model)
            keys = [(job.grad, job.c_off)] + ([("b", job.grad_b)] if job.grad_b else [])
            if any(k in seen for k in keys):
                rest.append((job, slab))
            else:
                batch.append((job, slab))
                seen.update(keys)
        jobs = (L.WgradReduceJob * len(batch))(*[j for j, _ in batch])
        L.check(lib.ddk_wgrad_reduce_jobs(jobs, len(batch), L.stream()), "wgrad_reduce_jobs")     # records travel as kernel arguments
        launches += 1
        pending = rest
    del _wgrad_keep[:]          # (freed on the caller's stream, which has waited for the side stream)
    return launches


def conv_wgrad_(kind, x, dy, grad_w, c_real, cw, c_off, grad_b=None, persistent=False):
    """grad_w (canonical layout, contiguous) += weight gradient of `kind` for the source x (see csrc/conv_wgrad.hip);
    grad_b [N] += column sums of dy when given (the bias gradient, produced by the same launches).
    persistent: grad_w / grad_b are buffers that outlive the backward pass (the parameters' `.grad` slots) -- only then may the
    reduce be deferred inside deferred_wgrad(); a temporary handed back to autograd is reduced at once."""
    b, h, w, cx = x.shape
    n = dy.shape[-1]
    lib = L.load()
    nbytes = lib.ddk_conv_wgrad_workspace_bytes(kind, b, h, w, cx, n)
    if _wgrad_pending is not None and persistent:
        global _wgrad_forked
        slab = torch.empty(max(nbytes, 16) // 4, device=x.device, dtype=torch.float32)
        job = L.WgradReduceJob()
        x, dy = _f32(x), _f32(dy)
        if WGRAD_SIDE_STREAM and b * h * w <= WGRAD_SIDE_MAX_PIXELS:
            # queued; every WGRAD_SIDE_BATCH of them leave together behind ONE fork (a cross-stream edge per launch cost more than the
            # overlap gave: 16.7 -> 18.2 ms per cfg3 step)
            _wgrad_queue.append((kind, x, dy, grad_w, grad_b, (b, h, w, cx, c_real, cw, c_off, n), slab, nbytes, job,
                                 torch.cuda.current_stream()))
            if len(_wgrad_queue) >= WGRAD_SIDE_BATCH:
                _launch_side_queue()
        else:
            L.check(lib.ddk_conv_wgrad_defer(kind, L.ptr(x), L.ptr(dy), L.ptr(grad_w), L.ptr(grad_b), b, h, w, cx, c_real, cw, c_off, n,
                                             L.ptr(slab), nbytes, C.byref(job), L.stream()), "conv_wgrad_defer")
        _wgrad_pending.append((job, slab))
        return grad_w
    ws = _ws(x.device, nbytes, "wgrad")
    L.check(lib.ddk_conv_wgrad_bias(kind, L.ptr(_f32(x)), L.ptr(_f32(dy)), L.ptr(grad_w), L.ptr(grad_b), b, h, w, cx, c_real, cw, c_off, n,
                                    L.ptr(ws), nbytes, L.stream()), "conv_wgrad")
    return grad_w


def bias_grad(dy, accumulate_into=None):
    n = dy.shape[-1]
    out = accumulate_into if accumulate_into is not None else torch.empty(n, device=dy.device, dtype=torch.float32)
    ws = _ws(dy.device, 256 * n * 4, "bias")
    L.check(L.load().ddk_bias_grad(L.ptr(_f32(dy)), L.ptr(out), dy.numel() // n, n, int(accumulate_into is not None), L.ptr(ws),
                                   256 * n * 4, L.stream()), "bias_grad")
    return out


def gn_train_resident(b, hw, c, groups=GN_GROUPS):
    """the training GroupNorm keeps a (sample, group) slab in registers (and so takes the slab forms) when this holds"""
    return L.load().ddk_groupnorm_train_workspace_bytes(b, hw, c, groups) == 0


def groupnorm_mish_train(x, gamma, beta, temb=None, addend=None, drop_p=0.0, seed=0, layer=0, groups=GN_GROUPS, eps=GN_EPS, slabs=None,
                         conv_bias=None):
    """slabs [S,B,H,W,C] (ops.conv(leave_slabs=True)): x = sum(slabs) + conv_bias is formed while loading and WRITTEN into `x`"""
    b, h, w, c = x.shape
    out = torch.empty_like(x)
    stride = temb.stride(0) if temb is not None else 0
    lib = L.load()
    if slabs is not None:
        L.check(lib.ddk_groupnorm_mish_train_fwd_slabs(L.ptr(slabs), slabs.shape[0], slabs.stride(0), L.ptr(conv_bias), L.ptr(x), L.ptr(gamma),
                                                       L.ptr(beta), temb.data_ptr() if temb is not None else None, stride, L.ptr(addend),
                                                       float(drop_p), seed, layer, L.ptr(out), b, h * w, c, groups, eps, L.stream()),
                "groupnorm_mish_train_fwd_slabs")
        return out
    nbytes = lib.ddk_groupnorm_train_workspace_bytes(b, h * w, c, groups)
    ws = _ws(x.device, nbytes, "gn_train") if nbytes else None
    L.check(lib.ddk_groupnorm_mish_train_fwd(L.ptr(_f32(x)), L.ptr(gamma), L.ptr(beta),
                                             temb.data_ptr() if temb is not None else None, stride, L.ptr(addend),
                                             float(drop_p), seed, layer, L.ptr(out), b, h * w, c, groups, eps, L.ptr(ws), nbytes,
                                             L.stream()),
            "groupnorm_mish_train_fwd")
    return out


def groupnorm_mish_bwd(x, gamma, beta, dy, drop_p=0.0, seed=0, layer=0, groups=GN_GROUPS, eps=GN_EPS, acc=None, dy_slabs=None):
    """-> dx, dtemb [B,C], sums [3][C] = (dgamma, dbeta, sum over all pixels of dx -- the bias gradient of the conv that
    produced x).  `acc`: optional (gamma.grad, beta.grad, conv_bias.grad) accumulated into directly (entries may be None).
    dy_slabs [S,B,H,W,C]: dy = sum(dy_slabs), formed while loading (`dy` itself is not read)."""
    b, h, w, c = x.shape
    dx = torch.empty_like(x)
    part = torch.empty((4, b, c), device=x.device, dtype=torch.float32)
    lib = L.load()
    if dy_slabs is not None:
        L.check(lib.ddk_groupnorm_mish_bwd_slabs(L.ptr(_f32(x)), L.ptr(gamma), L.ptr(beta), float(drop_p), seed, layer, L.ptr(dy_slabs),
                                                 dy_slabs.shape[0], dy_slabs.stride(0), L.ptr(dx), L.ptr(part), b, h * w, c, groups, eps,
                                                 L.stream()), "groupnorm_mish_bwd_slabs")
    else:
        nbytes = lib.ddk_groupnorm_train_workspace_bytes(b, h * w, c, groups)
        ws = _ws(x.device, nbytes, "gn_train") if nbytes else None
        L.check(lib.ddk_groupnorm_mish_bwd(L.ptr(_f32(x)), L.ptr(gamma), L.ptr(beta), float(drop_p), seed, layer, L.ptr(_f32(dy)),
                                           L.ptr(dx), L.ptr(part), b, h * w, c, groups, eps, L.ptr(ws), nbytes, L.stream()),
                "groupnorm_mish_bwd")
    sums = [None, None, None]
    missing = [k for k in range(3) if acc is None or acc[k] is None]
    if acc is not None and any(t is not None for t in acc):
        # straight into the parameters' gradients (fixed-order row sums, then +=), one launch for the three of them
        _rows_sum_targets(part[1], 3, b * c, b, c, [acc[0], acc[1], acc[2]], c)
    if missing:
        out = torch.empty((3, c), device=x.device, dtype=torch.float32)
        L.check(lib.ddk_rows_sum_batched(L.ptr(part[1]), 3, b * c, b, c, L.ptr(out), c, 0, L.stream()), "rows_sum_batched")
        for k in missing:
            sums[k] = out[k]
    return dx, part[0], sums


# ---------------------------------------------------------------- widths that are not multiples of 32 (training)
def groupnorm_mish_generic_train(x, gamma, beta, temb=None, addend=None, drop_p=0.0, seed=0, layer=0, groups=GN_GROUPS, eps=GN_EPS):
    """x [B,H,W,CP] with zero padding behind the C = gamma.numel() real channels -> Dropout(Mish(GN(x)) + temb[b]) + addend, padding zero"""
    b, h, w, cp = x.shape
    c = gamma.numel()
    out = torch.empty_like(x)
    stride = temb.stride(0) if temb is not None else 0
    L.check(L.load().ddk_groupnorm_mish_generic_train_fwd(L.ptr(_f32(x)), L.ptr(gamma), L.ptr(beta), temb.data_ptr() if temb is not None else None,
                                                          stride, L.ptr(addend), float(drop_p), seed, layer, L.ptr(out), b, h * w, cp, c, groups,
                                                          eps, L.stream()), "groupnorm_mish_generic_train_fwd")
    return out


def groupnorm_mish_generic_bwd(x, gamma, beta, dy, drop_p=0.0, seed=0, layer=0, groups=GN_GROUPS, eps=GN_EPS):
    """-> dx [B,H,W,CP], dtemb [B,C], (dgamma, dbeta, sum of dx over batch and pixels) [3][C]"""
    b, h, w, cp = x.shape
    c = gamma.numel()
    dx = torch.empty_like(x)
    part = torch.empty((4, b, c), device=x.device, dtype=torch.float32)
    lib = L.load()
    L.check(lib.ddk_groupnorm_mish_generic_bwd(L.ptr(_f32(x)), L.ptr(gamma), L.ptr(beta), float(drop_p), seed, layer, L.ptr(_f32(dy)), L.ptr(dx),
                                               L.ptr(part), b, h * w, cp, c, groups, eps, L.stream()), "groupnorm_mish_generic_bwd")
    sums = torch.empty((3, c), device=x.device, dtype=torch.float32)
    L.check(lib.ddk_rows_sum_batched(L.ptr(part[1]), 3, b * c, b, c, L.ptr(sums), c, 0, L.stream()), "rows_sum_batched")
    return dx, part[0], sums


def chan_layernorm_generic(x, g, b, eps=LN_EPS):
    """LayerNorm over the C = g.numel() real channels of CP-pitched rows; padding written as zero"""
    cp, c = x.shape[-1], g.numel()
    out = torch.empty_like(x)
    L.check(L.load().ddk_chan_layernorm_generic(L.ptr(_f32(x)), L.ptr(g.reshape(-1)), L.ptr(b.reshape(-1)), L.ptr(out), x.numel() // cp, cp, c,
                                                eps, L.stream()), "chan_layernorm_generic")
    return out


def chan_layernorm_generic_bwd(x, g, dy, eps=LN_EPS, addend=None):
    """-> dx (+ addend), dg [C], db [C]"""
    cp, c = x.shape[-1], g.numel()
    m = x.numel() // cp
    dx = torch.empty_like(x)
    max_parts = 512
    part = torch.empty((2, max_parts, c), device=x.device, dtype=torch.float32)
    n = C.c_int(0)
    lib = L.load()
    L.check(lib.ddk_chan_layernorm_generic_bwd(L.ptr(_f32(x)), L.ptr(g.reshape(-1)), L.ptr(_f32(dy)), L.ptr(addend), L.ptr(dx), L.ptr(part),
                                               max_parts, C.byref(n), m, cp, c, eps, L.stream()), "chan_layernorm_generic_bwd")
    # the kernel wrote rows [0, n) of dg and rows [n, 2n) of db, contiguously
    flat = part.view(-1)
    dg = rows_sum(flat[:n.value * c], n.value, c, c)
    db = rows_sum(flat[n.value * c:2 * n.value * c], n.value, c, c)
    return dx, dg, db


def rows_sum(rows, nrows, row_stride, n, out=None):
    if out is None:
        out = torch.empty(n, device=rows.device, dtype=torch.float32)
    L.check(L.load().ddk_rows_sum(rows.data_ptr(), nrows, row_stride, out.data_ptr(), n, 0, L.stream()), "rows_sum")
    return out


_multi_add_tables = {}


def multi_add_(src, segments):
    """ddk_multi_add: dst_k += src[off_k : off_k + n_k] for segments [(offset, dst tensor), ...] in ONE launch.  The device table is
    cached per (offsets, destination addresses): the destinations are views of the optimiser's flat gradient buffer, stable for its
    lifetime."""
    key = (str(src.device),) + tuple((int(o), d.data_ptr(), d.numel()) for o, d in segments)
    tab = _multi_add_tables.get(key)
    if tab is None:
        if len(_multi_add_tables) > 64:
            _multi_add_tables.clear()
        host = torch.tensor([[int(o), d.data_ptr(), d.numel()] for o, d in segments], dtype=torch.int64)
        tab = _multi_add_tables[key] = host.to(src.device)
    if torch.cuda.is_current_stream_capturing():
        _graph_keep[-1].append((tab, [d for _, d in segments]))
    L.check(L.load().ddk_multi_add(L.ptr(src), tab.data_ptr(), len(segments), max(d.numel() for _, d in segments), L.stream()), "multi_add")


def chan_layernorm_bwd(x, g, dy, eps=LN_EPS, acc=None, addend=None):
    """acc = (g.grad slot, b.grad slot): the row sums are ADDED into them (one launch) and (dx, None, None) is returned;
    addend: added to dx by the same launch"""
    c = x.shape[-1]
    m = x.numel() // c
    dx = torch.empty_like(x)
    max_parts = 512
    part = torch.empty((2, max_parts, c), device=x.device, dtype=torch.float32)
    n = C.c_int(0)
    lib = L.load()
    L.check(lib.ddk_chan_layernorm_bwd_add(L.ptr(_f32(x)), L.ptr(g.reshape(-1)), L.ptr(_f32(dy)), L.ptr(addend), L.ptr(dx), L.ptr(part),
                                           max_parts, C.byref(n), m, c, eps, L.stream()), "chan_layernorm_bwd")
    # the kernel laid the rows out as [2][nparts][C] with nparts = n.value
    if acc is not None and acc[0] is not None and acc[1] is not None:
        _rows_sum_targets(part, 2, n.value * c, n.value, c, [acc[0], acc[1]], c)
        return dx, None, None
    out = torch.empty((2, c), device=x.device, dtype=torch.float32)
    L.check(lib.ddk_rows_sum_batched(L.ptr(part), 2, n.value * c, n.value, c, L.ptr(out), c, 0, L.stream()), "rows_sum_batched")
    return dx, out[0], out[1]


def linattn_small_from_x(x, w_qkv, ln_g, ln_b, heads=4, eps=LN_EPS):
    """PreNorm(LinearAttention) up to (not including) to_out on a small map (H*W <= 64) in ONE launch: x [B,H,W,C]; w_qkv the
    canonical to_qkv weight [3*heads*32, C(,1,1)]; ln_g / ln_b the channel LayerNorm's g, b (blocks.py:57-60, 123-134).
    -> (out [B,H,W,heads*32], ctx [B,heads,32,32]).  The folded weights are derived here (the UNet plan caches them)."""
    b, h, w, c = x.shape
    wq = w_qkv.reshape(w_qkv.shape[0], -1).to(torch.float32)
    g, bb = ln_g.reshape(-1).to(torch.float32), ln_b.reshape(-1).to(torch.float32)
    cp = pad32(c)
    lnw = torch.zeros((wq.shape[0], cp), device=x.device, dtype=torch.float32)
    lnw[:, :c] = wq * g[None, :]
    c1 = (wq * g[None, :]).sum(dim=1).contiguous()
    c2 = (wq * bb[None, :]).sum(dim=1).contiguous()
    wop = torch.empty_like(lnw)
    lib = L.load()
    L.check(lib.ddk_pack_qkv_operand(L.ptr(lnw), L.ptr(wop), heads, cp, L.stream()), "pack_qkv_operand")
    ctx = torch.empty((b, heads, 32, 32), device=x.device, dtype=torch.float32)
    out = torch.empty((b, h, w, heads * 32), device=x.device, dtype=torch.float32)
    L.check(lib.ddk_linattn_small_from_x(L.ptr(_f32(x)), L.ptr(wop), L.ptr(c1), L.ptr(c2), eps, L.ptr(ctx), L.ptr(out), b, h * w, c, heads,
                                         L.stream()), "linattn_small_from_x")
    return out, ctx


def attention_split_workspace(batch, device):
    """a zeroed workspace for attention_split_from_x (its counters re-arm themselves: zero it once, reuse it)"""
    nbytes = L.load().ddk_attention_split_workspace_bytes(batch)
    return torch.zeros(max(nbytes, 128) // 4, device=device, dtype=torch.float32)


def attention_split_from_x(x, w_qkv, ln_g, ln_b, heads=4, eps=LN_EPS, workspace=None):
    """PreNorm(LinearAttention) up to (not including) to_out on a 16x16 or 8x8 map in ONE launch, every (image, head) split over two
    workgroups that exchange their softmax partials in the launch (ddk_attention_split_from_x): x [B,H,W,C]; w_qkv the canonical
    to_qkv weight [3*heads*32, C(,1,1)]; ln_g / ln_b the channel LayerNorm's g, b (blocks.py:57-60, 123-134).
    -> (out [B,H,W,heads*32], ctx [B,heads,32,32]).  The folded weights are derived here (the UNet plan caches them)."""
    b, h, w, c = x.shape
    lib = L.load()
    if not lib.ddk_attention_split_ok(b, h * w, c, heads):
        raise L.DDKError(f"attention_split_from_x: shape {tuple(x.shape)} with {heads} heads not eligible "
                         "(H*W of 64 or 256, C % 32 == 0, C <= 256, 4 heads, 8 * B <= the CU count)")
    wq = w_qkv.reshape(w_qkv.shape[0], -1).to(torch.float32)
    g, bb = ln_g.reshape(-1).to(torch.float32), ln_b.reshape(-1).to(torch.float32)
    lnw = (wq * g[None, :]).contiguous()
    c1 = lnw.sum(dim=1).contiguous()
    c2 = (wq * bb[None, :]).sum(dim=1).contiguous()
    ws = attention_split_workspace(b, x.device) if workspace is None else workspace
    ctx = torch.empty((b, heads, 32, 32), device=x.device, dtype=torch.float32)
    out = torch.empty((b, h, w, heads * 32), device=x.device, dtype=torch.float32)
    L.check(lib.ddk_attention_split_from_x(L.ptr(_f32(x)), L.ptr(lnw), L.ptr(c1), L.ptr(c2), eps, L.ptr(ctx), L.ptr(out), b, h * w, c, heads,
                                           L.ptr(ws), ws.numel() * 4, L.stream()), "attention_split_from_x")
    return out, ctx


def linattn_train(qkv, heads=4):
    out, ctx = linattn(qkv, heads)
    b, h, w, _ = qkv.shape
    stats = torch.empty((b, heads, 2, 32), device=qkv.device, dtype=torch.float32)
    lib = L.load()
    nbytes = lib.ddk_linattn_train_workspace_bytes(b, h * w, heads)
    ws = _ws(qkv.device, nbytes, "linattn_train") if nbytes else None
    L.check(lib.ddk_linattn_stats(L.ptr(qkv), L.ptr(stats), b, h * w, heads, L.ptr(ws), nbytes, L.stream()), "linattn_stats")
    return out, ctx, stats


def linattn_bwd(qkv, dout, ctx, stats, heads=4):
    """stats None: the softmax statistics of k are recomputed from qkv by the backward's own launches (ddk_linattn_bwd_recompute)"""
    b, h, w, _ = qkv.shape
    dctx = torch.empty_like(ctx)
    dqkv = torch.empty_like(qkv)
    lib = L.load()
    nbytes = lib.ddk_linattn_train_workspace_bytes(b, h * w, heads)
    ws = _ws(qkv.device, nbytes, "linattn_train") if nbytes else None
    if stats is None:
        scratch = torch.empty((b, heads, 2, 32), device=qkv.device, dtype=torch.float32)
        L.check(lib.ddk_linattn_bwd_recompute(L.ptr(qkv), L.ptr(_f32(dout)), L.ptr(ctx), L.ptr(scratch), L.ptr(dctx), L.ptr(dqkv), b, h * w,
                                              heads, L.ptr(ws), nbytes, L.stream()), "linattn_bwd_recompute")
        return dqkv
    L.check(lib.ddk_linattn_bwd(L.ptr(qkv), L.ptr(_f32(dout)), L.ptr(ctx), L.ptr(stats), L.ptr(dctx), L.ptr(dqkv), b, h * w,
                                heads, L.ptr(ws), nbytes, L.stream()), "linattn_bwd")
    return dqkv


def ae_objective(l_ddpm, l_rec, t, t_rec_max):
    """-> [3] = (objective, latent, recon) of the dDDPM autoencoder's 'simple' loss from the per-sample losses (ddk_ae_objective)"""
    out = torch.empty(3, device=l_ddpm.device, dtype=torch.float32)
    L.check(L.load().ddk_ae_objective(L.ptr(_f32(l_ddpm)), L.ptr(_f32(l_rec)), t.data_ptr(), int(t_rec_max), l_ddpm.numel(), L.ptr(out),
                                      L.stream()), "ae_objective")
    return out


def ae_objective_bwd(g, t, t_rec_max):
    d1 = torch.empty(t.numel(), device=g.device, dtype=torch.float32)
    d2 = torch.empty_like(d1)
    L.check(L.load().ddk_ae_objective_bwd(L.ptr(_f32(g)), t.data_ptr(), int(t_rec_max), t.numel(), L.ptr(d1), L.ptr(d2), L.stream()),
            "ae_objective_bwd")
    return d1, d2


def mish_bwd(x, dy):
    dx = torch.empty_like(x)
    L.check(L.load().ddk_mish_bwd(L.ptr(_f32(x)), L.ptr(_f32(dy)), L.ptr(dx), x.numel(), L.stream()), "mish_bwd")
    return dx


def tanh_bwd(y, dy):
    dx = torch.empty_like(y)
    L.check(L.load().ddk_tanh_bwd(L.ptr(_f32(y)), L.ptr(_f32(dy)), L.ptr(dx), y.numel(), L.stream()), "tanh_bwd")
    return dx


def avgpool2_bwd(dy):
    b, h2, w2, c = dy.shape
    dx = torch.empty((b, 2 * h2, 2 * w2, c), device=dy.device, dtype=torch.float32)
    L.check(L.load().ddk_avgpool2_bwd(L.ptr(_f32(dy)), L.ptr(dx), b, 2 * h2, 2 * w2, c, L.stream()), "avgpool2_bwd")
    return dx


def upsample_nearest2_bwd(dy):
    b, h2, w2, c = dy.shape
    dx = torch.empty((b, h2 // 2, w2 // 2, c), device=dy.device, dtype=torch.float32)
    L.check(L.load().ddk_upsample_nearest2_bwd(L.ptr(_f32(dy)), L.ptr(dx), b, h2 // 2, w2 // 2, c, L.stream()), "upsample_nearest2_bwd")
    return dx


def sq_err_grad(a, b, scale):
    out = torch.empty_like(b)
    bsz = a.shape[0]
    L.check(L.load().ddk_sq_err_grad(L.ptr(_f32(a)), L.ptr(_f32(b)), L.ptr(_f32(scale)), L.ptr(out), bsz, a.numel() // bsz, L.stream()),
            "sq_err_grad")
    return out


def scale_per_sample(x, scale):
    out = torch.empty_like(x)
    bsz = x.shape[0]
    L.check(L.load().ddk_scale_per_sample(L.ptr(_f32(x)), L.ptr(_f32(scale)), L.ptr(out), bsz, x.numel() // bsz, L.stream()),
            "scale_per_sample")
    return out


def conv1x1_small_n_bwd(a, w, dy, acc=None):
    """-> da, dw [n_out, C], db [n_out].  acc = (weight.grad slot, bias.grad slot): the partial rows are summed straight INTO them
    (two row-sum jobs, deferred with the others inside deferred_wgrad()) and (da, None, None) is returned"""
    c = a.shape[-1]
    n_out = w.shape[0]
    m = a.numel() // c
    da = torch.empty_like(a)
    max_rows = 1024
    rowlen = n_out * c + n_out
    part = torch.empty((max_rows, rowlen), device=a.device, dtype=torch.float32)
    n = C.c_int(0)
    L.check(L.load().ddk_conv1x1_small_n_bwd(L.ptr(_f32(a)), L.ptr(w.reshape(n_out, c).contiguous()), L.ptr(_f32(dy)), L.ptr(da),
                                             L.ptr(part), max_rows, C.byref(n), m, c, n_out, L.stream()), "conv1x1_small_n_bwd")
    if acc is not None and acc[0] is not None and acc[1] is not None:
        flat = part.view(-1)
        _rows_sum_targets(flat, 1, 0, n.value, rowlen, [acc[0]], n_out * c)
        _rows_sum_targets(flat[n_out * c:], 1, 0, n.value, rowlen, [acc[1]], n_out)
        return da, None, None
    tot = rows_sum(part, n.value, rowlen, rowlen)
    return da, tot[:n_out * c].reshape(n_out, c), tot[n_out * c:]


def small_gemm(mode, a, b, out, m, n, k, lda, ldb, ldc, accumulate=False):
    lib = L.load()
    nbytes = lib.ddk_small_gemm_workspace_bytes(m, n, k, ldc)
    ws = _ws(out.device, nbytes, "small_gemm") if nbytes else None
    L.check(lib.ddk_small_gemm(mode, a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, lda, ldb, ldc, int(accumulate), L.ptr(ws), nbytes,
                               L.stream()), "small_gemm")
    return out


def sincos_embed(t, freqs):
    bsz, dim = t.shape[0], freqs.numel() * 2
    e = torch.empty((bsz, dim), device=t.device, dtype=torch.float32)
    L.check(L.load().ddk_sincos_embed(L.ptr(t), L.ptr(freqs), L.ptr(e), bsz, dim, L.stream()), "sincos_embed")
    return e


def bias_act_(y, bias, want_act):
    act = torch.empty_like(y) if want_act else None
    L.check(L.load().ddk_bias_act(L.ptr(y), L.ptr(bias), L.ptr(act), y.shape[0], y.shape[1], L.stream()), "bias_act")
    return act


# ------------------------------------------------------------------ optimiser (flat buffers)
def grad_norm_clip(flat_grad, max_norm):
    """-> device tensor [norm, clip_coef] (no host sync)"""
    out = torch.empty(2, device=flat_grad.device, dtype=torch.float32)
    ws = _ws(flat_grad.device, 4096, "norm")
    L.check(L.load().ddk_grad_norm_clip(L.ptr(flat_grad), flat_grad.numel(), float(max_norm), L.ptr(out), L.ptr(ws), 4096, L.stream()),
            "grad_norm_clip")
    return out


def adam_step_(p, g, m, v, lr, step, clip=None, betas=(0.9, 0.999), eps=1e-8):
    L.check(L.load().ddk_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                                   float(eps), int(step), L.ptr(clip), L.stream()), "adam_step")


def ema_update_(p_ema, p, decay):
    L.check(L.load().ddk_ema_update(L.ptr(p_ema), L.ptr(p), p.numel(), float(decay), L.stream()), "ema_update")


# ================================================================== the 'deterministic' / 'convolutional' resamplers (csrc/resample.hip)
# NCHW tensors throughout: the callers hold NCHW and the channel counts are 1..8, so there is no channel padding and no layout change.
BICUBIC_A = -0.75
_bicubic_cache = {}            # (n_in, n_out, device, transposed) -> tuple of device tensors


def bicubic_taps(n_in, n_out):
    """The 1-D taps of torch's upsample_bicubic2d with align_corners=True, as numpy (idx int32 [n_out, 4], w float32 [n_out, 4]):
    source coordinate o (n_in - 1) / (n_out - 1) (0 when n_out == 1), i = its floor, t = its fraction, taps i-1 .. i+2 with the
    cubic-convolution weights c2(t+1), c1(t), c1(1-t), c2(2-t) for A = -0.75; indices clamped to [0, n_in - 1] -- a clamped tap
    keeps its weight.  Everything in float64, cast once."""
    import numpy as np
    a = BICUBIC_A
    o = np.arange(n_out, dtype=np.float64)
    src = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(1)
    i = np.floor(src)
    t = src - i
    c1 = lambda x: ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0               # |x| <= 1
    c2 = lambda x: ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a         # 1 < |x| < 2
    w = np.stack([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)], axis=1)
    idx = np.clip(i[:, None].astype(np.int64) + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx.astype(np.int32), w.astype(np.float32)


def bicubic_taps_transposed(n_in, n_out):
    """The same taps listed per INPUT index (the gather form of the gradient): (start int32 [n_in + 1], out_idx int32 [nnz],
    w float32 [nnz]); entries start[i] .. start[i+1]-1 are the outputs that tap i, ascending.  Taps of one output that coincide after
    clamping are one entry with their (fp32) weights added in float64."""
    import numpy as np
    idx, w = bicubic_taps(n_in, n_out)
    lists = [dict() for _ in range(n_in)]
    for o in range(n_out):
        for k in range(4):
            d = lists[int(idx[o, k])]
            d[o] = d.get(o, 0.0) + float(w[o, k])
    start, oi, ww = [0], [], []
    for d in lists:
        for o in sorted(d):
            oi.append(o)
            ww.append(d[o])
        start.append(len(oi))
    return np.asarray(start, np.int32), np.asarray(oi, np.int32), np.asarray(ww, np.float32)


def _bicubic_tables(n_in, n_out, device, transposed=False):
    """Device copies of the tap tables, made once per (n_in, n_out, device) (like DDPM._cached_tables: a graph capture finds them
    ready, its warm-up passes made them)."""
    key = (int(n_in), int(n_out), str(device), transposed)
    tabs = _bicubic_cache.get(key)
    if tabs is None:
        host = bicubic_taps_transposed(n_in, n_out) if transposed else bicubic_taps(n_in, n_out)
        tabs = tuple(torch.from_numpy(h).contiguous().to(device) for h in host)
        if transposed:
            tabs += (int((host[0][1:] - host[0][:-1]).max()),)           # the longest list: how the gradient kernel shares its work
        _bicubic_cache[key] = tabs
    return tabs


def _nchw(x, what):
    if x.dim() != 4:
        raise L.DDKError(f"{what}: expected an NCHW tensor, got {x.dim()} dimensions")
    return _f32(x)


def bicubic_resize(x, size):
    """F.interpolate(x, size, mode='bicubic', align_corners=True) of an NCHW tensor; size = (Hout, Wout)."""
    b, c, h, w = _nchw(x, "bicubic_resize").shape
    ho, wo = int(size[0]), int(size[1])
    xp = L.ptr(x)
    ih, wh = _bicubic_tables(h, ho, x.device)
    iw, ww = _bicubic_tables(w, wo, x.device)
    out = torch.empty((b, c, ho, wo), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_bicubic_resize(xp, L.ptr(out), L.ptr(ih), L.ptr(wh), L.ptr(iw), L.ptr(ww), b * c, h, w, ho, wo, L.stream()),
            "bicubic_resize")
    return out


def bicubic_resize_grad(dy, in_size):
    """Gradient of bicubic_resize with respect to its input: dy [B, C, Hout, Wout] -> [B, C, *in_size]."""
    b, c, ho, wo = _nchw(dy, "bicubic_resize_grad").shape
    h, w = int(in_size[0]), int(in_size[1])
    dyp = L.ptr(dy)
    sh, oh, wh, _ = _bicubic_tables(h, ho, dy.device, transposed=True)
    sw, ow, ww, longest_w = _bicubic_tables(w, wo, dy.device, transposed=True)
    dx = torch.empty((b, c, h, w), device=dy.device, dtype=torch.float32)
    L.check(L.load().ddk_bicubic_resize_grad(dyp, L.ptr(dx), L.ptr(sh), L.ptr(oh), L.ptr(wh), L.ptr(sw), L.ptr(ow), L.ptr(ww), longest_w,
                                             b * c, h, w, ho, wo, L.stream()), "bicubic_resize_grad")
    return dx


def _small_conv_shapes(x, w, what, transpose):
    b, c, h, wd = _nchw(x, what).shape
    if w.dim() != 4 or tuple(w.shape[2:]) != ((4, 4) if transpose else (3, 3)):
        raise L.DDKError(f"{what}: the weight must be [{'C_in, C_out, 4, 4' if transpose else 'C_out, C_in, 3, 3'}], got {tuple(w.shape)}")
    cin, cout = (w.shape[0], w.shape[1]) if transpose else (w.shape[1], w.shape[0])
    if not (1 <= cin <= 32 and 1 <= cout <= 32):
        raise L.DDKError(f"{what}: 1 <= channels <= 32 (got {cin} -> {cout})")
    return b, c, h, wd, int(cin), int(cout)


def conv_small_s2(x, w, bias=None):
    """nn.Conv2d(C_in, C_out, 3, stride=2, padding=1) on NCHW, 1 <= C <= 32, any H, W >= 1."""
    b, c, h, wd, cin, cout = _small_conv_shapes(x, w, "conv_small_s2", False)
    if c != cin:
        raise L.DDKError(f"conv_small_s2: the input has {c} channels, the weight takes {cin}")
    out = torch.empty((b, cout, (h + 1) // 2, (wd + 1) // 2), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_conv_small_s2(L.ptr(x), L.ptr(_f32(w)), L.ptr(bias), L.ptr(out), b, cin, cout, h, wd, L.stream()), "conv_small_s2")
    return out


def conv_small_s2_dgrad(dy, w, in_size):
    """Input gradient of conv_small_s2: dy [B, C_out, ceil(H/2), ceil(W/2)] -> [B, C_in, H, W] with (H, W) = in_size."""
    b, c, ho, wo, cin, cout = _small_conv_shapes(dy, w, "conv_small_s2_dgrad", False)
    h, wd = int(in_size[0]), int(in_size[1])
    if c != cout or (ho, wo) != ((h + 1) // 2, (wd + 1) // 2):
        raise L.DDKError(f"conv_small_s2_dgrad: dy {tuple(dy.shape)} is not the output of a [{cin}, {h}, {wd}] input")
    dx = torch.empty((b, cin, h, wd), device=dy.device, dtype=torch.float32)
    L.check(L.load().ddk_conv_small_s2_dgrad(L.ptr(dy), L.ptr(_f32(w)), L.ptr(dx), b, cin, cout, h, wd, L.stream()), "conv_small_s2_dgrad")
    return dx


def conv_small_s2_wgrad(x, dy, want_bias=True):
    """(dW [C_out, C_in, 3, 3], db [C_out] or None) of conv_small_s2."""
    b, cin, h, wd = _nchw(x, "conv_small_s2_wgrad").shape
    cout = _nchw(dy, "conv_small_s2_wgrad").shape[1]
    if tuple(dy.shape) != (b, cout, (h + 1) // 2, (wd + 1) // 2):
        raise L.DDKError(f"conv_small_s2_wgrad: dy {tuple(dy.shape)} is not the output of x {tuple(x.shape)}")
    xp, dyp = L.ptr(x), L.ptr(dy)
    lib = L.load()
    nbytes = lib.ddk_conv_small_s2_wgrad_workspace_bytes(b, cin, cout, h, wd)
    if nbytes == 0:
        raise L.DDKError(f"conv_small_s2_wgrad: 1 <= channels <= 32 (got {cin} -> {cout})")
    ws = _ws(x.device, nbytes, "small_wgrad")
    dw = torch.empty((cout, cin, 3, 3), device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if want_bias else None
    L.check(lib.ddk_conv_small_s2_wgrad(xp, dyp, L.ptr(dw), L.ptr(db), b, cin, cout, h, wd, L.ptr(ws), ws.numel() * 4, L.stream()),
            "conv_small_s2_wgrad")
    return dw, db


def convt_small_s2(x, w, bias=None):
    """nn.ConvTranspose2d(C_in, C_out, 4, stride=2, padding=1) on NCHW, 1 <= C <= 32: [B, C_in, H, W] -> [B, C_out, 2H, 2W]."""
    b, c, h, wd, cin, cout = _small_conv_shapes(x, w, "convt_small_s2", True)
    if c != cin:
        raise L.DDKError(f"convt_small_s2: the input has {c} channels, the weight takes {cin}")
    out = torch.empty((b, cout, 2 * h, 2 * wd), device=x.device, dtype=torch.float32)
    L.check(L.load().ddk_convt_small_s2(L.ptr(x), L.ptr(_f32(w)), L.ptr(bias), L.ptr(out), b, cin, cout, h, wd, L.stream()), "convt_small_s2")
    return out


def convt_small_s2_dgrad(dy, w):
    """Input gradient of convt_small_s2: dy [B, C_out, 2H, 2W] -> [B, C_in, H, W]."""
    b, c, ho, wo, cin, cout = _small_conv_shapes(dy, w, "convt_small_s2_dgrad", True)
    if c != cout or ho % 2 or wo % 2:
        raise L.DDKError(f"convt_small_s2_dgrad: dy {tuple(dy.shape)} is not an output of a [{cin} -> {cout}] layer")
    dx = torch.empty((b, cin, ho // 2, wo // 2), device=dy.device, dtype=torch.float32)
    L.check(L.load().ddk_convt_small_s2_dgrad(L.ptr(dy), L.ptr(_f32(w)), L.ptr(dx), b, cin, cout, ho // 2, wo // 2, L.stream()),
            "convt_small_s2_dgrad")
    return dx


def convt_small_s2_wgrad(x, dy, want_bias=True):
    """(dW [C_in, C_out, 4, 4], db [C_out] or None) of convt_small_s2."""
    b, cin, h, wd = _nchw(x, "convt_small_s2_wgrad").shape
    cout = _nchw(dy, "convt_small_s2_wgrad").shape[1]
    if tuple(dy.shape) != (b, cout, 2 * h, 2 * wd):
        raise L.DDKError(f"convt_small_s2_wgrad: dy {tuple(dy.shape)} is not the output of x {tuple(x.shape)}")
    xp, dyp = L.ptr(x), L.ptr(dy)
    lib = L.load()
    nbytes = lib.ddk_convt_small_s2_wgrad_workspace_bytes(b, cin, cout, h, wd)
    if nbytes == 0:
        raise L.DDKError(f"convt_small_s2_wgrad: 1 <= channels <= 32 (got {cin} -> {cout})")
    ws = _ws(x.device, nbytes, "small_wgrad")
    dw = torch.empty((cin, cout, 4, 4), device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if want_bias else None
    L.check(lib.ddk_convt_small_s2_wgrad(xp, dyp, L.ptr(dw), L.ptr(db), b, cin, cout, h, wd, L.ptr(ws), ws.numel() * 4, L.stream()),
            "convt_small_s2_wgrad")
    return dw, db


# ------------------------------------------------------------------ training batches from a resident uint8 array
def image_batch_rows_per_group(hs, ws, c, size, row_taps, col_taps):
    """output rows one workgroup of image_batch takes for this shape (host arithmetic); 0: the shape is not taken"""
    return int(L.load().ddk_image_batch_rows_per_group(hs, ws, c, size, row_taps, col_taps))


def image_batch(images, index, tables, S, flip=False, seed=0, epoch=0):
    """[B, C, S, S] fp32 in [-1, 1]: the transform chain of utils/image_batch.py of images[index[b]], one launch.  images: uint8
    [N, Hs, Ws, C] on the device; index: int64 [B] on the device; tables: (row_start int32 [S], row_w fp32 [S, row_taps], col_start
    int32 [S], col_w fp32 [S, col_taps]) on the device, utils.image_batch.Transform's.  flip: mirror along W the images that
    utils.image_batch.flip_bits(index, seed, epoch) names.  An index outside [0, N) gives an all-NaN image."""
    row_start, row_w, col_start, col_w = tables
    if images.dtype != torch.uint8 or images.dim() != 4:
        raise L.DDKError(f"image_batch: images must be uint8 [N, H, W, C], got {images.dtype} {tuple(images.shape)}")
    if index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
        raise L.DDKError(f"image_batch: index must be int64 [B], got {index.dtype} {tuple(index.shape)}")
    n, hs, ws, c = images.shape
    S = int(S)
    if (row_start.dtype != torch.int32 or col_start.dtype != torch.int32 or tuple(row_start.shape) != (S,) or tuple(col_start.shape) != (S,)
            or row_w.dim() != 2 or col_w.dim() != 2 or row_w.shape[0] != S or col_w.shape[0] != S):
        raise L.DDKError(f"image_batch: the tables of size {S} are (int32 [S], fp32 [S, taps]) per axis, got {tuple(row_start.shape)} "
                         f"{row_start.dtype}, {tuple(row_w.shape)}, {tuple(col_start.shape)} {col_start.dtype}, {tuple(col_w.shape)}")
    b = index.numel()
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = torch.empty((b, c, S, S), device=images.device, dtype=torch.float32)
    L.check(L.load().ddk_image_batch(L.ptr(images), n, hs, ws, c, L.ptr(index), b, L.ptr(row_start), L.ptr(_f32(row_w)), row_w.shape[1],
                                     L.ptr(col_start), L.ptr(_f32(col_w)), col_w.shape[1], S, int(bool(flip)), seed,
                                     int(epoch) & 0xFFFFFFFF, L.ptr(out), L.stream()), "image_batch")
    return out
