"""conv3x3_gn_wlocal_kernel's two chunk loops -- the compile-time one of cin = 256 and the run-time one of every other width --
at the smallest shapes that reach each of their paths.  Every case is held to a torch-CPU fp64 Block (conv3x3 -> GroupNorm -> Mish
+ time shift + addend) at test_kernels_gpu.py's bar for this op, max|diff| / max|ref| < 2e-5, and must be bit-stable over A / B / A
launches through the same device buffers with B on other inputs: a fragment read ahead of its barrier, or a weight register
reloaded under its MFMAs, would show as a changed bit."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err, to_nchw, to_nhwc

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3

CASES = [  # id, H, W, c0, c1, N, groups, source slabs, addend slabs
    ("c256-two-n-tiles", 8, 8, 256, 0, 64, 8, 1, 1),        # compile-time loop, two n tiles, 8 channels per group
    ("c128+128", 8, 8, 128, 128, 64, 2, 1, 1),               # compile-time loop, two sources, 32 channels per group
    ("c32-one-chunk", 8, 8, 32, 0, 64, 8, 1, 1),             # run-time loop: one chunk, no steady state
    ("c64-both-parities", 8, 8, 64, 0, 64, 2, 1, 1),         # one chunk of each V buffer
    ("c96-odd-tail", 8, 8, 96, 0, 64, 8, 1, 1),              # odd chunk count: the tail of the loop unrolled by two
    ("c256+64-lds-limit", 8, 8, 256, 64, 64, 8, 1, 1),       # 320 channels: the LDS limit
    ("c64-4x16", 4, 16, 64, 0, 64, 8, 1, 1),                 # patch geometry that is not square
    ("c256-slabs", 8, 8, 256, 0, 64, 8, 2, 2),               # split-K source and a slab addend on the compile-time loop
]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def ops():
    from ddk import ops as o
    from ddk import lib
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


def mish64(v):
    return v * torch.tanh(F.softplus(v))


def make_inputs(H, W, cin, N, S, SA, seed):
    """one launch's varying inputs (NCHW on the CPU): source slabs, time shift, addend slabs"""
    return dict(src=[rnd(B, cin, H, W, seed=seed + k) for k in range(S)], temb=rnd(B, N, seed=seed + 10),
                add=[rnd(B, N, H, W, seed=seed + 20 + k) for k in range(SA)])


def reference(inp, par, groups):
    """the Block in fp64 on the CPU"""
    x = sum(s.double() for s in inp["src"]) + (par["sbias"].double()[None, :, None, None] if par["sbias"] is not None else 0)
    a = sum(s.double() for s in inp["add"]) + (par["abias"].double()[None, :, None, None] if par["abias"] is not None else 0)
    h = F.group_norm(F.conv2d(x, par["w"].double(), par["bias"].double(), padding=1), groups, par["gamma"].double(), par["beta"].double(),
                     eps=1e-5)
    return mish64(h) + inp["temb"].double()[:, :, None, None] + a


@pytest.mark.parametrize("name,H,W,c0,c1,N,groups,S,SA", CASES, ids=[c[0] for c in CASES])
def test_wlocal_loop(ops, name, H, W, c0, c1, N, groups, S, SA):
    L = ops.L
    lib = L.load()
    cin = c0 + c1
    assert lib.ddk_conv3x3_gn_mish_wino_ok(H, W, cin, c0, N, groups)
    slabbed = S > 1 or SA > 1
    par = dict(w=rnd(N, cin, 3, 3, seed=1, scale=(cin * 9) ** -0.5), bias=rnd(N, seed=2, scale=0.1), gamma=1 + rnd(N, seed=3, scale=0.2),
               beta=rnd(N, seed=4, scale=0.2), sbias=rnd(cin, seed=5, scale=0.3) if slabbed else None,
               abias=rnd(N, seed=6, scale=0.3) if slabbed else None)
    wl = ops.pack_conv_weight_wino_local(par["w"].to(DEV))
    bias, gamma, beta = par["bias"].to(DEV), par["gamma"].to(DEV), par["beta"].to(DEV)
    sbias = par["sbias"].to(DEV) if slabbed else None
    abias = par["abias"].to(DEV) if slabbed else None
    # the device buffers every launch of this case goes through
    src = torch.empty(S, B, H, W, cin, device=DEV)
    x0 = torch.empty(B, H, W, c0, device=DEV)
    x1 = torch.empty(B, H, W, c1, device=DEV) if c1 else None
    temb = torch.empty(B, N, device=DEV)
    add = torch.empty(SA, B, H, W, N, device=DEV)
    out = torch.empty(B, H, W, N, device=DEV)

    def launch(inp):
        src.copy_(torch.stack([to_nhwc(s) for s in inp["src"]]))
        x0.copy_(src[0][..., :c0])
        if c1:
            x1.copy_(src[0][..., c0:])
        temb.copy_(inp["temb"])
        add.copy_(torch.stack([to_nhwc(a) for a in inp["add"]]))
        out.fill_(float("nan"))
        if slabbed:
            L.check(lib.ddk_conv3x3_gn_mish_slabs(L.ptr(src), S, src.stride(0), L.ptr(sbias), cin, L.ptr(wl), L.ptr(bias), L.ptr(gamma),
                                                  L.ptr(beta), temb.data_ptr(), temb.stride(0), L.ptr(add), SA, add.stride(0), L.ptr(abias),
                                                  L.ptr(out), B, H, W, N, groups, 1e-5, L.stream()), "conv3x3_gn_mish_slabs")
        else:
            L.check(lib.ddk_conv3x3_gn_mish_wino(L.ptr(x0), c0, L.ptr(x1), c1, L.ptr(wl), L.ptr(bias), L.ptr(gamma), L.ptr(beta),
                                                 temb.data_ptr(), temb.stride(0), L.ptr(add), L.ptr(out), B, H, W, N, groups, 1e-5,
                                                 L.stream()), "conv3x3_gn_mish_wino")
        return out.cpu()

    in_a, in_b = make_inputs(H, W, cin, N, S, SA, 100), make_inputs(H, W, cin, N, S, SA, 200)
    out_a, out_b, out_a2 = launch(in_a), launch(in_b), launch(in_a)
    for tag, got, inp in (("A", out_a, in_a), ("B", out_b, in_b)):
        ref = reference(inp, par, groups)
        err = rel_err(to_nchw(got).double(), ref)
        print(f"{name} {tag}: max|diff| / max|ref| = {err:.3e}")
        assert err < 2e-5
    assert not torch.equal(out_a, out_b)
    assert torch.equal(out_a, out_a2)
