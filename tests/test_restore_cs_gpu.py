"""DDNM compressed sensing on the GPU (DDPM.restore_cs, ddk_sampler_run_restore_cs, ddk_p_sample_update_restore_cs,
ddk_hadamard_measure, ddk_hadamard_adjoint; csrc/hadamard.hip) against tests/hadamard_ref.py, the method restated in float64 around
oracle/unet_ref with oracle/philox_ref draws.

The butterflies' order is the kernel's own, so the lone op is held bit for bit only where every intermediate is exact (test 1) and
to a derived bar elsewhere.  With u = 2^-24, L = log2 N + 2 and alpha = sum |x0| / sqrt(N) over the plane:

    |got - ref| <= |c1| L u ((N - m) / sqrt(N) alpha + sum |w| / sqrt(N)) + 4 u (|c1 x0'| + |c2 x| + |sigma z|)

elementwise.  A sum of N terms by any pairwise tree of depth log2 N is within log2 N u sum |terms|; the one multiply by fp32(s) adds
two roundings (s itself and the product), hence L.  A coefficient of the first transform is off by at most L u alpha, and only the
N - m unmeasured ones reach the result, each with weight 1 / sqrt(N); the second transform's own error is L u sum |w| / sqrt(N).  The
update's five roundings are each half an ulp of one of its terms.  measure and adjoint are held to the one-transform form,
L u sum |input| / sqrt(N).

Shapes: both kernel forms (a plane of at most 32768 pixels takes one launch, a 256 x 256 plane three), one, three and eight channels,
W != H, N = 512 where s is no power of two.  Chains: 1e-4 abs against the restatement with the same argmax and 1e-5 between the
Python loop and the native sampler, as for the other restore kinds; graph replay equals eager launches bit for bit."""
import json
import math

import numpy as np
import pytest
import torch

import chain_cases as CC
import hadamard_ref as HR
from helpers import ddpm_cfg, to_nchw as nchw, to_nhwc as nhwc
from oracle import diffusion_ref as D
from utils import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = (2, 3, 16, 16)
TOL = 1e-4
BETAS = D.beta_schedule("linear", 1000)
CFG = ddpm_cfg(32, 3, 16)
SEED = 1409
KINDS = [dict(), dict(ddim=True, eta=0.0)]
IDS = ["ancestral", "ddim"]
U24 = 2.0 ** -24
# (C, H, W, B): the plane form up to N = 32768, the scratch form at 256 x 256
SHAPES = [(3, 16, 16, 3), (1, 16, 32, 3), (8, 32, 32, 2), (3, 64, 64, 3), (3, 128, 128, 2), (1, 128, 256, 2), (3, 256, 256, 1), (1, 256, 256, 3)]
EXACT = [(3, 16, 16, 3), (3, 64, 64, 2), (3, 256, 256, 1), (1, 256, 256, 2)]      # N a power of 4: s is a power of two


def _rows(N):
    return [4] + ([100] if N == 256 else []) + [N // 4, N - 4, N]


CASES = [(c, h, w, b, m) for c, h, w, b in SHAPES for m in _rows(h * w)]
EXACT_CASES = [(c, h, w, b, m) for c, h, w, b in EXACT for m in _rows(h * w)]


def _perm(N, seed=0):
    return np.random.default_rng(seed).permutation(N).astype(np.int32)


def _dev(perm):
    return torch.from_numpy(np.ascontiguousarray(perm)).to(DEV)


def _inputs(c, h, w, B, m, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, c, h, w)
    x = 2 * torch.randn(shape, generator=g)
    e = torch.randn(shape, generator=g)
    y = (torch.rand((B, c, m), generator=g) * 2 - 1).contiguous()
    t = torch.tensor([0, 7, 3])[:B]
    return x, e, y, t, CC.hand_tables(g)


def _plane_sum(v):
    """sum |v| over the last axis of a [B, C, N] array, as a [B, C, 1, 1] float64 tensor"""
    return torch.from_numpy(np.abs(v).sum(axis=-1)).reshape(v.shape[0], v.shape[1], 1, 1)


def _first_term(x0, w, N, m):
    """L u ((N - m) / sqrt(N) alpha + sum |w| / sqrt(N)) per plane, [B, C, 1, 1] float64"""
    L = math.log2(N) + 2
    alpha = _plane_sum(HR.planes(x0)) / math.sqrt(N)
    return L * U24 * ((N - m) / math.sqrt(N) * alpha + _plane_sum(w) / math.sqrt(N))


# ---------------------------------------------------------------- 1. exact cases: they carry the indexing
def _exact_inputs(c, h, w, B, m, seed):
    """x in {-1, 0, 1}, sparse; y = integer s; the int64 restatement of x0' N = H(select(y / s, H(Pi x)))"""
    N = h * w
    rng = np.random.default_rng(seed)
    x = np.zeros((B, c, N), dtype=np.int64)
    for b in range(B):
        for ch in range(c):
            idx = rng.choice(N, size=min(N // 16, 64), replace=False)
            x[b, ch, idx] = rng.choice([-1, 1], size=idx.size)
    ky = rng.integers(-20, 21, size=(B, c, m))
    perm = _perm(N, seed + 1)
    a = x[..., perm.astype(np.int64)]
    kv = HR.fwht_int(a)                   # v = s kv
    kw = kv.copy()
    kw[..., :m] = ky                      # w = s kw
    ko = HR.fwht_int(kw)                  # x0'[perm[j]] = s s ko[j] = ko[j] / N
    # the precondition: every intermediate of both transforms is an integer below 2^24 in units of s (any partial sum is bounded by
    # the sum of the inputs' magnitudes)
    assert int(np.abs(a).sum(axis=-1).max()) < 2 ** 24 and int(np.abs(kw).sum(axis=-1).max()) < 2 ** 24
    out = np.zeros((B, c, N), dtype=np.float64)
    out[..., perm.astype(np.int64)] = ko.astype(np.float64) / N      # exact: an integer below 2^24 over a power of two
    s = 1.0 / math.sqrt(N)
    assert s == float(np.float32(s))      # N is a power of 4
    return (torch.from_numpy(x.astype(np.float32).reshape(B, c, h, w)), torch.from_numpy((ky * s).astype(np.float32)), perm,
            torch.from_numpy(out.reshape(B, c, h, w)))


@pytest.mark.parametrize("c,h,w,B,m", EXACT_CASES)
def test_exact_step_equals_the_integer_restatement_bit_for_bit(c, h, w, B, m):
    from ddk import ops
    x, y, perm, want = _exact_inputs(c, h, w, B, m, 11 * c + h + m)
    g = torch.Generator().manual_seed(m)
    e = torch.randn(x.shape, generator=g)
    one, zero = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    t = torch.zeros(B, dtype=torch.long, device=DEV)      # row 0: c1 = 1, c2 = 0, no draw
    got = ops.p_sample_update_restore_cs_(nhwc(x).to(DEV), nhwc(e).to(DEV), y.to(DEV), _dev(perm), t, c_recip=one, c_recipm1=zero, c1=one,
                                          c2=zero, sigma=one, seed=5, stream_id=1)
    got = nchw(got.cpu()).double()
    assert torch.equal(got, want), float((got - want).abs().max())
    # the invariant, exactly: the measured coefficients of the result are y
    assert np.array_equal(HR.measure(got, perm, m), y.double().numpy())


@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_measure_of_a_delta_and_of_a_constant(c, h, w, B):
    from ddk import ops
    N = h * w
    s32 = np.float32(1.0 / math.sqrt(N))
    perm = _perm(N, 3)
    x = torch.zeros(B, c, N)
    pix = [(17 * b + 5 * ch + 3) % N for b in range(B) for ch in range(c)]
    for i, p in enumerate(pix):
        x[i // c, i % c, p] = 1.0
    y = ops.hadamard_measure(nhwc(x.reshape(B, c, h, w)).to(DEV), _dev(perm), N).cpu().numpy()
    inv = np.argsort(perm)
    k = np.arange(N)
    for i, p in enumerate(pix):
        j0 = int(inv[p])
        sign = np.where(np.array([bin(int(v)).count("1") for v in (k & j0)]) % 2 == 0, 1.0, -1.0).astype(np.float32)
        assert np.array_equal(y[i // c, i % c], sign * s32)
    # perm = identity, a constant plane: (sqrt(N) c, 0, ...), the zeros exact
    const = torch.full((B, c, h, w), 0.375)
    y = ops.hadamard_measure(nhwc(const).to(DEV), _dev(np.arange(N, dtype=np.int32)), N).cpu().numpy()
    assert not y[..., 1:].any()
    assert np.array_equal(y[..., 0], np.full((B, c), np.float32(s32 * np.float32(N * 0.375))))
    assert abs(float(y[0, 0, 0]) - math.sqrt(N) * 0.375) <= 2 * U24 * math.sqrt(N)


@pytest.mark.parametrize("c,h,w,B", [(3, 16, 16, 3), (1, 16, 32, 3), (3, 128, 128, 2), (1, 256, 256, 2)])
def test_with_every_coefficient_measured_x0_does_not_matter(c, h, w, B):
    from ddk import ops
    N = h * w
    x, e, y, t, tab = _inputs(c, h, w, B, N, 5 + h)
    x2, e2 = _inputs(c, h, w, B, N, 6 + h)[:2]
    tabd = {k: v.to(DEV) for k, v in tab.items()}
    tabd["c2"] = torch.zeros_like(tabd["c2"])          # x itself enters only through x0
    pd, td, yd = _dev(_perm(N)), t.to(DEV), y.to(DEV)
    a = ops.p_sample_update_restore_cs_(nhwc(x).to(DEV), nhwc(e).to(DEV), yd, pd, td, **tabd, seed=9, stream_id=2)
    b = ops.p_sample_update_restore_cs_(nhwc(x2).to(DEV), nhwc(e2).to(DEV), yd, pd, td, **tabd, seed=9, stream_id=2)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- 2. the lone op on generic inputs, within the derived bar
@pytest.mark.parametrize("c,h,w,B,m", CASES)
def test_lone_op_within_the_derived_bar(c, h, w, B, m):
    from ddk import ops
    N = h * w
    x, e, y, t, tab = _inputs(c, h, w, B, m, 31 * c + h + w + m)
    seed, stream = 97531, 4
    z = CC.philox_draws(B, c, h, w, t, seed, stream)
    perm = _perm(N, m)
    sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
    want, x0, x0p, wsel = HR.step(x, e, y.double().numpy(), perm, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], sg, z)
    col = lambda v: v.reshape(-1, 1, 1, 1).double()
    c1, c2 = col(tab["c1"][t]), col(tab["c2"][t])
    first = _first_term(x0, wsel, N, m)
    bar = c1.abs() * first + 4 * U24 * ((c1 * x0p).abs() + (c2 * x.double()).abs() + (col(sg) * z.double()).abs())
    xs = nhwc(x).to(DEV)
    ops.p_sample_update_restore_cs_(xs, nhwc(e).to(DEV), y.to(DEV), _dev(perm), t.to(DEV), **{k: v.to(DEV) for k, v in tab.items()}, seed=seed,
                                    stream_id=stream)
    got = nchw(xs.cpu())
    assert got.shape == want.shape and torch.isfinite(got).all()
    err = (got.double() - want).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max())
    form = "plane form" if N <= 32768 else "scratch form"
    print(f"lone cs op c={c} {h}x{w} B={B} m={m} ({form}): max abs error {float(err.max()):.3g}, worst ratio to the bar {ratio:.3g}")
    assert bool((err <= bar).all()), ratio
    # 3. the invariant at row 0, which returns x0' itself: A(x_out) = y, A applied in float64, within the bar's first term (which is
    # below the bar at every element)
    inv = np.abs(HR.measure(got[0:1], perm, m) - y[0:1].double().numpy())
    lim = float(first[0].max())
    print(f"  row 0: |A(x_out) - y| max {float(inv.max()):.3g}, ratio to the first term {float(inv.max()) / lim:.3g}")
    assert float(inv.max()) <= float(first[0].min())


@pytest.mark.parametrize("c,h,w,B", SHAPES)
def test_measure_adjoint_and_round_trip(c, h, w, B):
    from ddk import ops
    N = h * w
    L = math.log2(N) + 2
    g = torch.Generator().manual_seed(N + c)
    x = torch.randn(B, c, h, w, generator=g)
    perm = _perm(N, 7)
    pd, xd = _dev(perm), nhwc(x).to(DEV)
    worst = {}
    for m in _rows(N):
        y = ops.hadamard_measure(xd, pd, m).cpu()
        assert y.shape == (B, c, m)
        bar = L * U24 * _plane_sum(HR.planes(x)).reshape(B, c, 1) / math.sqrt(N)
        err = (y.double() - torch.from_numpy(HR.measure(x, perm, m))).abs()
        assert bool((err <= bar).all())
        worst["measure"] = max(worst.get("measure", 0.0), float((err / bar).max()))
        yin = (torch.rand((B, c, m), generator=g) * 2 - 1).contiguous()
        back = nchw(ops.hadamard_adjoint(yin.to(DEV), pd, h, w).cpu())
        bar = L * U24 * _plane_sum(yin.double().numpy()) / math.sqrt(N)
        err = (back.double() - HR.adjoint(yin.numpy(), perm, (B, c, h, w))).abs()
        assert bool((err <= bar).all())
        worst["adjoint"] = max(worst.get("adjoint", 0.0), float((err / bar).max()))
    # adjoint(measure(x, m = N)) is x, within the two-transform bar with nothing measured
    rt = nchw(ops.hadamard_adjoint(ops.hadamard_measure(xd, pd, N), pd, h, w).cpu())
    bar = _first_term(x, HR.measure(x, perm, N), N, 0)
    err = (rt.double() - x.double()).abs()
    worst["round trip"] = float((err / bar).max())
    print(f"hadamard ops c={c} {h}x{w} B={B}: worst ratios to the bar {worst}")
    assert bool((err <= bar).all())


# ---------------------------------------------------------------- 5. bit identity
@pytest.mark.parametrize("c,h,w,B", [(3, 16, 16, 3), (3, 128, 128, 2), (3, 256, 256, 1)])
def test_two_calls_of_every_op_agree_bit_for_bit(c, h, w, B):
    from ddk import ops
    N = h * w
    m = N // 4
    x, e, y, t, tab = _inputs(c, h, w, B, m, 77 + h)
    tabd = {k: v.to(DEV) for k, v in tab.items()}
    pd, xd, ed, yd, td = _dev(_perm(N)), nhwc(x).to(DEV), nhwc(e).to(DEV), y.to(DEV), t.to(DEV)
    for op in (lambda: ops.p_sample_update_restore_cs_(xd.clone(), ed, yd, pd, td, **tabd, seed=3, stream_id=1),
               lambda: ops.hadamard_measure(xd, pd, m), lambda: ops.hadamard_adjoint(yd, pd, h, w)):
        a, b = op(), op()
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---------------------------------------------------------------- argument faults
def test_argument_faults_run_no_kernel():
    from ddk import lib as L
    from ddk import ops
    tab = {k: torch.ones(4, device=DEV) for k in ("c_recip", "c_recipm1", "c1", "c2", "sigma")}
    t = torch.zeros(1, dtype=torch.long, device=DEV)

    def call(h, w, c, m):
        x = torch.full((1, h, w, c), 0.25, device=DEV)
        before = x.clone()
        perm = torch.arange(h * w, dtype=torch.int32, device=DEV)
        with pytest.raises(L.DDKError):
            ops.p_sample_update_restore_cs_(x, torch.ones_like(x), torch.zeros(1, c, max(m, 1), device=DEV), perm, t, **tab)
        torch.cuda.synchronize()
        assert torch.equal(x, before)
        with pytest.raises(L.DDKError):
            ops.hadamard_measure(x, perm, m)

    call(24, 16, 3, 8)
    call(16, 48, 3, 8)
    call(512, 16, 3, 8)
    call(8, 16, 3, 8)
    call(16, 16, 9, 8)
    call(16, 16, 3, 6)
    call(16, 16, 3, 260)
    x = torch.zeros(1, 16, 16, 3, device=DEV)
    with pytest.raises(L.DDKError):      # a perm of the wrong length or type never reaches the library
        ops.hadamard_measure(x, torch.arange(128, dtype=torch.int32, device=DEV), 8)
    with pytest.raises(L.DDKError):
        ops.hadamard_measure(x, torch.arange(256, dtype=torch.int64, device=DEV), 8)


# ---------------------------------------------------------------- 4. the tiny DDPM, "8" steps
@pytest.fixture(scope="module")
def tiny():
    return CC.tiny_ddpm(CFG)


M_TINY = 100
PERM_TINY = _perm(256, 0)


@pytest.fixture(scope="module")
def data():
    clean = 0.25 * syn.synthetic_normal(SHAPE, "cs.x")
    assert float(clean.abs().max()) < 1
    y = torch.from_numpy(HR.measure(clean, PERM_TINY, M_TINY)).float().contiguous()
    return y, syn.synthetic_normal(SHAPE, "cs.xT")


@pytest.fixture(scope="module")
def reference(tiny, data):
    """the restatement's chains, computed once and shared"""
    _, eps = tiny
    y, x_T = data
    return {i: HR.CS(BETAS, "8").run(eps, x_T, y, PERM_TINY, SEED, **kw) for i, kw in zip(IDS, KINDS)}


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_tiny_vs_restatement(tiny, data, reference, kw):
    m, _ = tiny
    y, x_T = data
    got = m.restore_cs(y.to(DEV), respacing="8", x_T=x_T, seed=SEED, **kw).cpu()      # perm: the default, cs_perm(256, 0)
    want = reference[IDS[KINDS.index(kw)]]
    err = float((got - want).abs().max())
    print(f"DDNM cs tiny DDPM, 8 steps {kw}: max abs error {err:.3g}")
    assert torch.isfinite(got).all() and got.shape == SHAPE
    assert err < TOL, err
    assert torch.equal(CC.argmax(got), CC.argmax(want))
    # the invariant.  The last row has c1 = 1 and |x0| <= 1 (clamped): alpha <= sqrt(N); w is the result's own transform
    N = 256
    wsel = HR.fwht(HR.planes(got)[..., PERM_TINY.astype(np.int64)])
    lim = _first_term(torch.ones(SHAPE), wsel, N, M_TINY)
    inv = np.abs(wsel[..., :M_TINY] - y.double().numpy())
    print(f"  |A(x_out) - y| max {float(inv.max()):.3g}, ratio to the first term {float(inv.max()) / float(lim.min()):.3g}")
    assert float(inv.max()) <= float(lim.min())
    # the unmeasured part is the model's: the result is not A+ y
    assert float((got - HR.adjoint(y.numpy(), PERM_TINY, SHAPE).float()).abs().max()) > 1e-2


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_graph_equals_eager_bit_for_bit(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    graphed = m.restore_cs(y.to(DEV), PERM_TINY, respacing="8", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "use_graph", False):
        eager = m.restore_cs(y.to(DEV), PERM_TINY, respacing="8", x_T=x_T, seed=SEED, **kw)
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_python_loop_equals_native(tiny, data, kw):
    m, _ = tiny
    y, x_T = data
    native = m.restore_cs(y.to(DEV), respacing="8", x_T=x_T, seed=SEED, **kw)
    with CC.toggled(m, "native_sampler", False):
        loop = m.restore_cs(y.to(DEV), respacing="8", x_T=x_T, seed=SEED, **kw)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, cs 8 steps {kw}: {err:.3g}")
    assert err < 1e-5


def test_tail_parts_is_zero_for_every_shape(tiny):
    from models import Unet
    m, _ = tiny
    plan = m._eps_model_nhwc().plan()
    assert plan.restore_cs_tail_parts(2, 16, 16) == 0
    u = Unet(ddpm_cfg(128, 3, 32))
    u.flops(1, 32, 32)
    for b, h, w in ((32, 32, 32), (8, 64, 64), (4, 128, 128), (1, 256, 256)):
        assert u._plan.restore_cs_tail_parts(b, h, w) == 0
    assert u._plan.restore_tail_parts(32, 32, 32, 2) == 8       # the shape has a fused tail; the plane-wide kind declines it


def test_cs_and_ancestral_chains_share_a_workspace(tiny, data, reference):
    """a compressed-sensing chain and a plain ancestral chain on the same plan, workspace, state buffer, tables and t_start, run
    alternately, then a chain with another batch of measurements through the same cached graph: each reproduces its own first result
    bit for bit (the kind and m are in the graph key; y and perm are staged by every call), and both batches come out right"""
    from ddk import lib as L
    from ddk import ops
    m, eps = tiny
    y, x_T = data
    tables, use = m._spaced_tables("8", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    nbytes = lib.ddk_sampler_restore_cs_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes == lib.ddk_sampler_workspace_bytes(plan.handle, 2, 16, 16, K - 1) + 4 * (16 * 16 + 2 * 2 * 16 * 16 * 3)
    pd = _dev(PERM_TINY)
    x0 = ops.nchw_to_nhwc(x_T.to(DEV).contiguous())
    ys = {"a": y.to(DEV), "b": (0.5 * y).to(DEV).contiguous()}

    def launch(what, a, tmap, stream):
        if what is None:
            return lib.ddk_sampler_run_spaced(a, tmap, stream)
        return lib.ddk_sampler_run_restore_cs(a, tmap, L.ptr(ys[what]), L.ptr(pd), M_TINY, stream)

    sh = CC.SharedWorkspace(plan, tables, use, x0, nbytes, SEED, launch)
    with CC.workspace(plan, nbytes) as ws:
        first = {}
        for what in ("a", None, "a", None, "b", "a", None, "b"):
            got = sh.run(ws, what)
            if what not in first:
                first[what] = got
            assert torch.equal(got, first[what]), (what, float((got - first[what]).abs().max()))
        assert not torch.equal(first["a"], first[None]) and not torch.equal(first["a"], first["b"])
        # the library's own entry and the model's method are the same chain
        via_model = m.restore_cs(y.to(DEV), PERM_TINY, respacing="8", x_T=x_T, seed=SEED)
        assert torch.equal(ops.nhwc_to_nchw(first["a"]), via_model)
        # both batches through the one graph are right
        assert float((ops.nhwc_to_nchw(first["a"]).cpu() - reference["ancestral"]).abs().max()) < TOL
        want_b = HR.CS(BETAS, "8").run(eps, x_T, 0.5 * y, PERM_TINY, SEED)
        assert float((ops.nhwc_to_nchw(first["b"]).cpu() - want_b).abs().max()) < TOL


def test_chain_faults(tiny):
    """the chain entry: injected noise, a null operand, a bad m and a shape the kind does not take are DDK_ERR_ARG"""
    from ddk import lib as L
    m, _ = tiny
    tables, use = m._spaced_tables("8", False, 0.0)
    plan = m._eps_model_nhwc().plan()
    lib = plan._lib
    K = len(use)
    tmap = CC.timestep_map(use)
    nbytes = lib.ddk_sampler_restore_cs_workspace_bytes(plan.handle, 2, 16, 16, K - 1)
    assert nbytes > 0 and lib.ddk_sampler_restore_cs_workspace_bytes(plan.handle, 2, 16, 48, K - 1) == 0
    x = torch.zeros(2, 16, 16, 3, device=DEV)
    y = torch.zeros(2, 3, 100, device=DEV)
    pd = _dev(PERM_TINY)
    ws = CC.fresh_workspace(nbytes)
    noise = torch.zeros((K, *x.shape), device=DEV)
    args = lambda noise=None, H=16: CC.sampler_args(plan, x, tables, K - 1, ws, nbytes, seed=SEED, noise=noise, shape=(2, H, 16))
    run = lib.ddk_sampler_run_restore_cs
    assert run(args(noise), tmap, L.ptr(y), L.ptr(pd), 100, L.stream()) == -1 and "noise" in L.last_error()
    assert run(args(), tmap, None, L.ptr(pd), 100, L.stream()) == -1 and "null" in L.last_error()
    assert run(args(), tmap, L.ptr(y), None, 100, L.stream()) == -1 and "null" in L.last_error()
    for bad in (0, 2, 102, 260):
        assert run(args(), tmap, L.ptr(y), L.ptr(pd), bad, L.stream()) == -1 and "multiple of 4" in L.last_error()
    assert run(args(H=48), tmap, L.ptr(y), L.ptr(pd), 100, L.stream()) == -1 and "powers of two" in L.last_error()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    with pytest.raises(L.DDKError):
        plan.sample_restore_cs_nhwc(x, y, pd[:128].contiguous(), tables, K - 1, timesteps=use)


def test_scratch_form_chain_256():
    """two steps at 3 x 256 x 256, B = 1, on a 32-wide model: the three-launch form inside a chain.  The native chain against the
    Python loop over the lone op, graph replay against eager launches, and the invariant"""
    m, _ = CC.tiny_ddpm(ddpm_cfg(32, 3, 256))
    N, mm = 65536, 16384
    shape = (1, 3, 256, 256)
    perm = _perm(N, 1)
    clean = 0.25 * syn.synthetic_normal(shape, "cs256.x")
    y = torch.from_numpy(HR.measure(clean, perm, mm)).float().contiguous()
    x_T = syn.synthetic_normal(shape, "cs256.xT")
    native = m.restore_cs(y.to(DEV), perm, respacing="2", x_T=x_T, seed=SEED)
    with CC.toggled(m, "use_graph", False):
        eager = m.restore_cs(y.to(DEV), perm, respacing="2", x_T=x_T, seed=SEED)
    assert torch.equal(native, eager)
    with CC.toggled(m, "native_sampler", False):
        loop = m.restore_cs(y.to(DEV), perm, respacing="2", x_T=x_T, seed=SEED)
    err = float((loop - native).abs().max())
    print(f"Python loop vs native, cs 256 x 256, 2 steps: {err:.3g}")
    assert torch.isfinite(native).all() and err < 1e-5
    got = native.cpu()
    wsel = HR.fwht(HR.planes(got)[..., perm.astype(np.int64)])
    lim = _first_term(torch.ones(shape), wsel, N, mm)
    inv = np.abs(wsel[..., :mm] - y.double().numpy())
    print(f"  |A(x_out) - y| max {float(inv.max()):.3g}, ratio to the first term {float(inv.max()) / float(lim.min()):.3g}")
    assert float(inv.max()) <= float(lim.min())


# ---------------------------------------------------------------- the command line
def test_cs_cli_and_evaluator(tmp_path):
    """cs_model_samples.py --measure_input and evaluate_restoration.py --task cs with synthetic weights on four 16 x 16 images, each in
    a fresh process: the files, their shapes and the JSON keys"""
    cfg_path, images_path, imgs, env = CC.cli_files(tmp_path, CC.cli_cfg(), 4, 16)
    CC.run_script("cs_model_samples.py", "--synthetic", cfg_path, "--saved_model", "clitest", "--images", images_path, "--measure_input",
                  "--ratio", "0.25", "--perm_seed", "2", "--timestep_respacing", "10", "--batch_size", "3", "--seed", "3", "--out_dir", tmp_path,
                  env=env)
    out = np.load(tmp_path / "clitest_cs_r0.25_p2_10.npy")
    meas = np.load(tmp_path / "clitest_cs_r0.25_p2_10_measurements.npy")
    assert out.shape == (4, 16, 16, 3) and out.dtype == np.float32
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 255
    assert meas.shape == (4, 3, 64) and meas.dtype == np.float32
    want = HR.measure(torch.from_numpy(imgs.astype(np.float64)).permute(0, 3, 1, 2) / 255 * 2 - 1, _perm(256, 2), 64)
    assert np.abs(meas - want).max() < 1e-5
    CC.run_script("evaluate_restoration.py", "--synthetic", cfg_path, "--images", images_path, "--task", "cs", "--ratio", "0.25",
                  "--timestep_respacing", "10", "--batch_size", "3", "--json", tmp_path / "score.json", env=env)
    res = json.loads((tmp_path / "score.json").read_text())
    s, mt = res["settings"], res["metrics"]
    assert (s["task"], s["method"], s["ratio"], s["perm_seed"], s["m"], s["unet_forwards"], s["n_images"]) == ("cs", "ddnm_cs", 0.25, 0, 64, 10, 4)
    assert {"restored", "adjoint", "consistency"} <= set(mt)
    for name in ("restored", "adjoint"):
        assert set(mt[name]) == {"psnr", "ssim"} and mt[name]["psnr"]["n"] == 4 and np.isfinite(mt[name]["psnr"]["mean"])
    assert {"mean", "stderr", "n", "max"} <= set(mt["consistency"])
    print(f"cs evaluator (synthetic weights): {json.dumps(mt)}")
