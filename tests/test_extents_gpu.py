"""No kernel may write, or depend on, bytes outside its tensors.

The buffer-contents table (tests/test_buffer_contents_gpu.py) is run once more, each case BUILT and run inside tests/guard.py's
guard_bands: every input moved to the device, every output, scratch, packed weight and plan workspace is an interior view between two
256 KiB bands of a repeating word.  Per case: two plain runs give the reference bits; then under each of poison.WORDS, and for the
op-level cases once more with every pointer only 16-byte aligned (skew = 16: what include/ddk.h promises, where torch alone hands out
512-byte aligned blocks), asserted are

  (a) tensors were banded, transfers among them,
  (b) no band was written (the message is the list of violations: call site, shape, side, byte offsets),
  (c) the results are bit-identical to the plain run: relocating a tensor and changing what lies beside it changes nothing,
  (d) float results are finite.

A store outside an allocation fails (b) under at least two of the three words (a stray 0.0 is invisible among zeros); a result that
depends on bytes beside an input -- a halo or tail load masked by a multiply, an fmaxf over a padded lane -- fails (c).

The cases added here are the entries the table lacks because they allocate nothing through torch.empty: the in-place sampler updates,
circular_spectrum, the two newer metrics and ema_update_.  They store into the caller's tensor, which is where an extent error goes
unseen; each is also held to what its own GPU test compares against, reference and bar unchanged, since the same bits from a wrong
kernel prove nothing.

Which cases hand the library a tensor from outside any band is found by guard.py's audit of ddk.lib.ptr, not listed: an op-level
table case for which it reports anything must have a variant here in which it reports nothing.  The variants house by hand what a
builder computes on the device, house torch.tensor(device=...) / full / ones / clone results as they are made, and let operands a
wrapper derives with torch ops (and the library only reads) be housed where they are handed over.  For plans and training steps,
where the models' own torch ops and autograd feed the library, the audit's findings are printed."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import guard
from guard import format_violation, guard_bands, rehouse
from poison import NAN, WORDS
from test_buffer_contents_gpu import CASES, NOT_BIT_REPRODUCIBLE, Case, _first_difference, _same, _snap

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24

nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous()
nchw = lambda v: v.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def ops():
    from ddk import lib
    from ddk import ops as o
    assert lib.load().ddk_device_ok() == 1, lib.last_error()
    return o


class Checked(Case):
    """a Case with verify(results): the snapshot of a run against the reference and bar of the op's own GPU test"""

    def __init__(self, run, verify):
        super().__init__(run)
        self.verify = verify


EXTRA = {}        # name -> builder(ops) -> Checked; as CASES, but the builder runs inside the bands too


def extra(name):
    def reg(fn):
        assert name not in EXTRA and name not in CASES, name
        EXTRA[name] = fn
        return fn
    return reg


def _to_dev(tab):
    return {k: v.to(DEV) for k, v in tab.items()}


def _device_draws(ops, shape, t, seed, stream):
    """the device's own draws [B, H, W, C] (ddk_randn: the ops' Philox call and keying), row b drawn at step t[b], checked against
    oracle/philox_ref as the lone-op tests do"""
    from oracle import philox_ref as PR
    z_dev = torch.stack([ops.randn(shape, DEV, seed, int(tb), stream)[b] for b, tb in enumerate(t)]).cpu()
    z_ref = torch.from_numpy(np.stack([PR.philox_normal(math.prod(shape), seed, int(tb), stream).reshape(shape)[b] for b, tb in enumerate(t)]))
    assert float((z_dev - z_ref).abs().max()) < 1e-5
    return z_dev


# ================================================================== in-place updates, both target forms
# Target forms: a tensor that reached the device through Tensor.to (housed by the transfer hook) and one made on the device and
# housed by hand (guard.rehouse).  (3, 6, 10, 3) has 180 elements per image: a ragged grid and no whole 256-thread row.
UPDATE_SHAPES = [(3, 16, 16, 3), (3, 6, 10, 3)]


def _targets(x):
    """(x moved to the device, a device-made copy housed by hand)"""
    return x.to(DEV), rehouse(x.to(DEV) * 1.0)


def _update_case(shape):
    """tests/test_kernels_gpu.py test_p_sample_update_bit_exact: injected noise bit for bit against oracle/diffusion_ref, the
    in-kernel draw within 2e-6 of the same update with oracle/philox_ref's draws"""
    def build(ops):
        from oracle import diffusion_ref as D
        from oracle import philox_ref
        from test_buffer_contents_gpu import rnd
        buf = D.schedule_buffers("linear", 1000)
        sigma = (0.5 * buf["posterior_log_variance_clipped"]).exp()
        x, eh, z = rnd(*shape, seed=110, scale=1.5), rnd(*shape, seed=111), rnd(*shape, seed=112)
        t, t321 = torch.tensor([0, 500, 999]), torch.full((3,), 321, dtype=torch.long)
        tb = {k: buf[v].to(DEV) for k, v in (("c_recip", "sqrt_recip_alphas_cumprod"), ("c_recipm1", "sqrt_recipm1_alphas_cumprod"),
                                             ("c1", "posterior_mean_coef1"), ("c2", "posterior_mean_coef2"))}
        tb["sigma"] = sigma.to(DEV)
        ehd, zd, td, t321d = eh.to(DEV), z.to(DEV), t.to(DEV), t321.to(DEV)
        seed, stream = 0x1234567887654321, 5

        def run():
            res = []
            for target in _targets(x):
                res.append(ops.p_sample_update_(target, ehd, td, noise=zd, **tb))
            for target in _targets(x):
                res.append(ops.p_sample_update_(target, ehd, t321d, seed=seed, stream_id=stream, **tb))
            return tuple(res)

        def verify(res):
            ref = D.p_sample_update(buf, x, t, eh, z)
            assert torch.equal(res[0], ref) and torch.equal(res[1], ref)
            zp = torch.from_numpy(philox_ref.philox_normal(x.numel(), seed, 321, stream)).reshape(x.shape)
            ref_p = D.p_sample_update(buf, x, t321, eh, zp)
            assert torch.equal(res[2], res[3]) and (res[2] - ref_p).abs().max() < 2e-6
        return Checked(run, verify)
    return build


def _hand(g, keys):
    scale = {"c_recip": 3.0, "c_recipm1": 2.0, "c1": 1.0, "c2": 1.0, "c3": -0.5, "sigma": 0.5, "ka": 1.0, "kb": 1.0, "ja": 1.0}
    return {k: torch.rand(8, generator=g) * scale[k] for k in keys}


def _multistep_case(shape):
    """tests/test_dpm_solver_gpu.py test_update_kernel_bit_exact: the fp32 torch expression in the kernel's order, bit for bit"""
    def build(ops):
        g = torch.Generator().manual_seed(5)
        x, e, h = 2 * torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.rand(shape, generator=g) * 2 - 1
        t = torch.tensor([0, 7, 3])
        tab = _hand(g, ("c_recip", "c_recipm1", "c1", "c2", "c3"))
        ed, td, dtab = e.to(DEV), t.to(DEV), _to_dev(tab)

        def run():
            res = []
            for xs, hs in zip(_targets(x), _targets(h)):
                ops.p_sample_update_multistep_(xs, ed, hs, td, **dtab)
                res += [xs, hs]
            return tuple(res)

        def verify(res):
            col = lambda k: tab[k][t].reshape(-1, 1, 1, 1).to(DEV)
            xd, hd = x.to(DEV), h.to(DEV)
            x0 = (col("c_recip") * xd - col("c_recipm1") * e.to(DEV)).clamp(-1, 1)
            want = ((col("c1") * x0 + col("c2") * xd) + col("c3") * hd).cpu()
            for xs, hs in (res[:2], res[2:]):
                assert torch.equal(xs, want) and torch.equal(hs, x0.cpu())
        return Checked(run, verify)
    return build


def _inpaint_case(shape):
    """tests/test_inpaint_gpu.py test_update_kernel_matches_torch_expression: the fp32 torch expression with philox_ref draws, 1e-5;
    row 0 (tau = 0) returns the known value exactly"""
    def build(ops):
        g = torch.Generator().manual_seed(5)
        B, per = shape[0], math.prod(shape[1:])
        x, e = 2 * torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        kn, mk = torch.rand(shape, generator=g) * 2 - 1, (torch.rand(shape, generator=g) > 0.5).float()
        t = torch.tensor([0, 7, 3])
        tab = _hand(g, ("c_recip", "c_recipm1", "c1", "c2", "sigma", "ka", "kb", "ja"))
        tab["jb"] = torch.tensor([0.0, 0.0, 0.0, 0.3, 0.0, 0.0, 0.0, 0.7])
        tab["ka"][0], tab["kb"][0] = 1.0, 0.0
        seed, stream = 12345, 3
        ed, kd, md, td, dtab = e.to(DEV), kn.to(DEV), mk.to(DEV), t.to(DEV), _to_dev(tab)

        def run():
            return tuple(ops.p_sample_update_inpaint_(xs, ed, kd, md, td, **dtab, seed=seed, stream_id=stream) for xs in _targets(x))

        def verify(res):
            from oracle import philox_ref as PR
            z = {s: torch.from_numpy(np.stack([PR.philox_normal(B * per, seed, int(tb), s).reshape(shape)[b] for b, tb in enumerate(t)]))
                 for s in (stream, stream | (1 << 30), stream | (1 << 29))}
            col = lambda k: tab[k][t].reshape(-1, 1, 1, 1)
            x0 = (col("c_recip") * x - col("c_recipm1") * e).clamp(-1, 1)
            x_unk = (col("c1") * x0 + col("c2") * x) + (t > 0).float().reshape(-1, 1, 1, 1) * col("sigma") * z[stream]
            x_kn = col("ka") * kn + col("kb") * z[stream | (1 << 30)]
            want = torch.where(mk != 0, x_kn, x_unk)
            want = torch.where(col("jb") != 0, col("ja") * want + col("jb") * z[stream | (1 << 29)], want)
            assert torch.equal(res[0], res[1])
            assert float((res[0] - want).abs().max()) < 1e-5
            assert torch.equal(res[0][0][mk[0] != 0], kn[0][mk[0] != 0])
        return Checked(run, verify)
    return build


for _s in UPDATE_SHAPES:
    _tag = "-".join(map(str, _s))
    EXTRA[f"p_sample_update-{_tag}"] = _update_case(_s)
    EXTRA[f"p_sample_update_multistep-{_tag}"] = _multistep_case(_s)
    EXTRA[f"p_sample_update_inpaint-{_tag}"] = _inpaint_case(_s)


# ================================================================== restore updates: (3, 16, 16, 3), n = 2, a checkerboard mask
def _restore_case(kind):
    """the lone-op tests of tests/test_restore_gpu.py, test_restore_masked_gpu.py, test_restore_solver_gpu.py, test_restore_noisy_gpu.py
    and test_colorize_gpu.py: the restatement's step on the same inputs and the device's own draws, bit for bit; y is NaN wherever the
    mask is 0"""
    def build(ops):
        import chain_cases as CC
        import restore_gray_ref as RG
        import restore_masked_ref as RM
        import restore_noisy_ref as RN
        import restore_ref as RR
        import restore_solver_ref as RS
        B, c, h, w, n = 3, 3, 16, 16, 2
        g = torch.Generator().manual_seed(17 * n + c + h)
        shape = (B, c, h, w)
        x, e = 2 * torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        hist = torch.rand(shape, generator=g) * 2 - 1
        y0 = torch.rand(B, 1 if kind == "gray" else c, h // n, w // n, generator=g) * 2 - 1
        t = torch.tensor([0, 7, 3])
        if kind == "multistep":
            tab = _hand(g, ("c_recip", "c_recipm1", "c1", "c2", "c3"))
            tab["c1"][0], tab["c2"][0], tab["c3"][0], tab["c3"][3] = 1.0, 0.0, 0.0, 0.0
        elif kind in ("noisy", "gray"):
            tab = CC.hand_tables(g, noisy=True)
            if kind == "gray":              # as tests/test_colorize_gpu.py: this kind's row 0 has lam = 1
                tab["lam"][0] = 1.0
        else:
            tab = _hand(g, ("c_recip", "c_recipm1", "c1", "c2", "sigma"))
            tab["c1"][0], tab["c2"][0] = 1.0, 0.0
        seed, stream = 24680, 5
        mk = None if kind == "plain" else CC.mask("checker", B, h // n, w // n)
        y = y0 if mk is None else torch.where(CC.sel(mk, y0), y0, torch.full_like(y0, float("nan")))
        ed, td, dtab = nhwc(e).to(DEV), t.to(DEV), _to_dev(tab)
        yd = (y[:, 0].contiguous() if kind == "gray" else nhwc(y)).to(DEV)
        md = None if mk is None else mk.to(DEV)
        kw = dict(seed=seed, stream_id=stream)

        def run():
            xs = rehouse(nhwc(x).to(DEV))
            if kind == "plain":
                return (ops.p_sample_update_restore_(xs, ed, yd, n, td, **dtab, **kw),)
            if kind == "masked":
                return (ops.p_sample_update_restore_masked_(xs, ed, yd, md, n, td, **dtab, **kw),)
            if kind == "noisy":
                return (ops.p_sample_update_restore_noisy_(xs, ed, yd, md, n, td, **dtab, **kw),)
            if kind == "gray":
                return (ops.p_sample_update_restore_gray_(xs, ed, yd, md, n, "luma", td, **dtab, **kw),)
            hs = rehouse(nhwc(hist).to(DEV))
            return ops.p_sample_update_restore_multistep_(xs, ed, hs, yd, md, n, td, **dtab), hs

        def verify(res):
            row = lambda k: tab[k][t]
            rows = [row(k) for k in ("c_recip", "c_recipm1", "c1", "c2")]
            got = nchw(res[0])
            if kind == "multistep":
                want_x, want_h = RS.step(x, e, hist, y, mk, n, *rows, row("c3"))
                assert torch.equal(got, want_x) and torch.equal(nchw(res[1]), want_h)
                return
            z = _device_draws(ops, (B, h, w, c), t, seed, stream).permute(0, 3, 1, 2)
            sg = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
            if kind == "plain":
                want = RR.step(x, e, y, n, *rows, sg, z)
            elif kind == "masked":
                want = RM.step(x, e, y, mk, n, *rows, sg, z)
            elif kind == "noisy":
                want = RN.step(x, e, y, mk, n, *rows, sg, row("lam"), row("sgm"), z)
            else:
                want = RG.step(x, e, y, mk, n, "luma", *rows, sg, row("lam"), row("sgm"), z)
            assert torch.equal(got, want), float((got - want).abs().max())
        return Checked(run, verify)
    return build


for _k in ("plain", "masked", "multistep", "noisy", "gray"):
    EXTRA["p_sample_update_restore" + ("" if _k == "plain" else "_" + _k) + "-3-16-16-3-n2"] = _restore_case(_k)


# ================================================================== the noisy deconvolution step and circular_spectrum
@functools.lru_cache(maxsize=None)
def _fft_host(c, h, w, B):
    """host operands and data of a lone DDNM+ deconvolution step, as tests/test_restore_fft_noisy_gpu.py makes them: made once"""
    import fft_conv_ref as FR
    from test_restore_fft_noisy_gpu import _operands, _tables
    g = torch.Generator().manual_seed(31 * c + h + 3 * w)
    shape, name, sigma_y = (B, c, h, w), "disk", 0.5
    tab = _tables()
    Mf, Pf, gain, nsc = _operands(name, h, w, sigma_y, tab["c1"])
    clean = (0.5 * torch.randn(shape, generator=g)).clamp(-1, 1)
    y = torch.from_numpy(FR.apply(clean, FR.spectrum(FR.preset(name), h, w))).float() + sigma_y * torch.randn(shape, generator=g)
    x, e = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    return tab, Mf, Pf, gain, nsc, y, x, e


def _spectrum_bar(y, Pf, h, w):
    """per plane, 2-norm: the forward transform's 8 L u ||F2 y|| (Higham Thm 24.2 with 8 u per bit, as DESIGN.md section 3.18 counts
    it; ||F2 y|| = sqrt(N) ||y||) and the complex multiply's 4 u, times max |S|"""
    L = math.log2(h * w)
    smax = float(np.abs(Pf[..., 0] + 1j * Pf[..., 1]).max())
    norm = np.sqrt((y.double().numpy() ** 2).sum(axis=(-2, -1)) * h * w)
    return (8 * L + 4) * U24 * smax * norm


def _natural(v, h, w):
    import fft_noisy_ref as FN
    v = v.double().numpy()
    return FN.to_natural(v[..., 0] + 1j * v[..., 1], h, w)


def _fft_noisy_case(c, h, w, B):
    """tests/test_restore_fft_noisy_gpu.py test_lone_step_within_the_derived_bar: fft_noisy_ref.step in float64 and the bar derived in
    that module's docstring"""
    def build(ops):
        import fft_noisy_ref as FN
        from test_restore_fft_noisy_gpu import _draws, _norm
        tab, Mf, Pf, gain, nsc, y, x, e = _fft_host(c, h, w, B)
        Md, gd, nd, Pd = (torch.from_numpy(v).to(DEV) for v in (Mf, gain, nsc, Pf))
        t = torch.tensor([0, 7, 3][:B])
        yd, ed, td, dtab = nhwc(y).to(DEV), nhwc(e).to(DEV), t.to(DEV), _to_dev(tab)
        seed, stream = 97531, 4

        def run():
            Yd = ops.circular_spectrum(yd, Pd)
            xs = rehouse(nhwc(x).to(DEV))
            return ops.p_sample_update_restore_fft_noisy_(xs, ed, Md, gd, nd, Yd, td, **dtab, seed=seed, stream_id=stream), Yd

        def verify(res):
            N, L, M = h * w, math.log2(h * w), Mf != 0
            Yhat = _natural(res[1], h, w)
            Yp = np.fft.ifft2(np.where(M, Yhat, 0.0), axes=(-2, -1)).real
            z = _draws(B, c, h, w, t, seed, stream)
            s = torch.where(t > 0, tab["sigma"][t], torch.zeros(B))
            want, x0, x0p, n, lam, phi = FN.step(x, e, M, gain, Yhat, tab["c_recip"][t], tab["c_recipm1"][t], tab["c1"][t], tab["c2"][t], s,
                                                 torch.from_numpy(nsc)[t], z)
            col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)
            c1, c2 = col(tab["c1"][t]), col(tab["c2"][t])
            bar = np.abs(c1) * (16 * L * U24 * (_norm(x0) + _norm(Yp)) + 4 * U24 * _norm(x0p)) + 16 * L * U24 * col(phi.max(axis=(1, 2))) * _norm(z) + \
                4 * U24 * (np.abs(c1) * _norm(x0p) + np.abs(c2) * _norm(x) + _norm(n))
            got = nchw(res[0])
            err = _norm(got.double() - want)
            assert (err <= bar).all(), float((err / bar).max())
        return Checked(run, verify)
    return build


EXTRA["p_sample_update_restore_fft_noisy-3-16-16-3"] = _fft_noisy_case(3, 16, 16, 3)
EXTRA["p_sample_update_restore_fft_noisy-2-128-256-1-scratch"] = _fft_noisy_case(1, 128, 256, 2)


@extra("circular_spectrum-3-16-16-3")
def _(ops):
    """against numpy.fft in float64: S . F2(y) per plane, within _spectrum_bar"""
    _, _, Pf, _, _, y, _, _ = _fft_host(3, 16, 16, 3)
    yd, Pd = nhwc(y).to(DEV), torch.from_numpy(Pf).to(DEV)

    def verify(res):
        want = (Pf[..., 0].astype(np.float64) + 1j * Pf[..., 1]) * np.fft.fft2(y.double().numpy(), axes=(-2, -1))
        err = np.sqrt((np.abs(_natural(res[0], 16, 16) - want) ** 2).sum(axis=(-2, -1)))
        bar = _spectrum_bar(y, Pf, 16, 16)
        assert (err <= bar).all() and (bar < 1e-3 * np.sqrt((np.abs(want) ** 2).sum(axis=(-2, -1)))).all(), float((err / bar).max())
    return Checked(lambda: (ops.circular_spectrum(yd, Pd),), verify)


# ================================================================== metrics: 150 x 24 rows against 90 x 24
@functools.lru_cache(maxsize=None)
def _int_rows():
    import sample_metrics_ref as R
    return R.int_features(121, 150, 24, 0), R.int_features(122, 90, 24, 1)


@extra("manifold_ball_counts-150-90-24")
def _(ops):
    """tests/test_sample_metrics_ext_gpu.py test_ball_counts_on_integer_rows: equal to kid_ref.ball_counts"""
    import kid_ref as K
    import sample_metrics_ref as R
    a, b = _int_rows()
    radii = [R.radii(a, k).astype(np.float32) for k in (1, 5)]
    ad, bd, rd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), [torch.from_numpy(r).to(DEV) for r in radii]

    def verify(res):
        for got, r in zip(res, radii):
            assert np.array_equal(got.numpy(), K.ball_counts(a, r, b))
    return Checked(lambda: tuple(ops.manifold_ball_counts(ad, r, bd) for r in rd), verify)


def _mmd_case(segments):
    """tests/test_sample_metrics_ext_gpu.py test_exact_arithmetic: integer rows, gamma = 1/64, kid_ref.sums_exact within EXACT_RTOL"""
    def build(ops):
        import kid_ref as K
        a, b = _int_rows()
        ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)

        def verify(res):
            got, want = res[0].numpy(), K.sums_exact(a, b, segments, 1.0 / 64, 1.0)
            assert got.shape == (segments, 3) and np.all(np.abs(got - want) <= K.EXACT_RTOL * np.abs(want))
        return Checked(lambda: (ops.poly_mmd_sums(ad, bd, segments, 1.0 / 64, 1.0),), verify)
    return build


EXTRA["poly_mmd_sums-150-90-24-segments1"] = _mmd_case(1)
EXTRA["poly_mmd_sums-150-90-24-segments3"] = _mmd_case(3)


@extra("ema_update-100003")
def _(ops):
    """tests/test_backward_gpu.py: e * decay + (1 - decay) * p within 1e-6; both parameter vectors housed by hand"""
    from test_buffer_contents_gpu import rnd
    n = 100003
    e, p = rnd(n, seed=82), rnd(n, seed=80)

    def run():
        ed, pd = rehouse(e.to(DEV) * 1.0), rehouse(p.to(DEV) * 1.0)
        ops.ema_update_(ed, pd, 0.995)
        return ed, pd

    def verify(res):
        assert torch.equal(res[1], p) and (res[0] - (e * 0.995 + (1 - 0.995) * p)).abs().max() < 1e-6
    return Checked(run, verify)


# ================================================================== table builders with inputs made on the device: variants that house them
# No list says which cases these are: the audit at the library's door (guard_bands.unbanded) finds a table case that hands the library
# a tensor from outside any band, and the check below then demands a variant of it here, in which the audit finds nothing.
VARIANT_OF = {}       # table case -> its variant in EXTRA


def variant(base, tag):
    def reg(fn):
        VARIANT_OF[base] = f"{base}-{tag}"
        return extra(f"{base}-{tag}")(fn)
    return reg


def _gn_train_slabs_variant(B, H, W, C, S):
    """_gn_train_slabs_case computes x on the device from the slabs (a sum, which no patched path sees); here it is housed by hand"""
    def build(ops):
        gen = torch.Generator().manual_seed(5)
        slabs = torch.randn(S, B, H, W, C, generator=gen).to(DEV)
        bias, gamma, beta = (torch.randn(C, generator=gen).to(DEV) for _ in range(3))
        temb = torch.randn(B, C, generator=gen).to(DEV)
        x = rehouse((slabs.sum(0) + bias).contiguous())

        def run():
            res = []
            for drop in (0.0, 0.1):
                raw = torch.empty_like(x)
                y = ops.groupnorm_mish_train(raw, gamma, beta, temb=temb, drop_p=drop, seed=7, layer=3, slabs=slabs, conv_bias=bias)
                dx, dt, sums = ops.groupnorm_mish_bwd(x, gamma, beta, slabs[0], drop, 7, 3, dy_slabs=slabs)
                res += [raw, y, dx, dt, *sums]
            return tuple(res)

        def verify(res):
            """the table's own case on the same inputs: housing x changes no bit"""
            want = _snap(CASES[f"groupnorm_train_slabs-{B}-{H}-{W}-{C}-{S}"](ops)())
            assert _same(res, want), _first_difference(res, want)
        return Checked(run, verify)
    return build


for _c in ((64, 2, 2, 256, 8), (3, 8, 8, 256, 4)):
    variant("groupnorm_train_slabs-" + "-".join(map(str, _c)), "rehoused_x")(_gn_train_slabs_variant(*_c))


@variant("elementwise_and_layout", "rehoused_nhwc")
def _(ops):
    """the table's case hands pad_channels a permuted copy made on the device (5 channels: the odd tail of a padded row); here that copy
    is housed by hand"""
    from helpers import to_nhwc
    from test_buffer_contents_gpu import rnd
    small = rnd(3, 5, 6, 7, seed=90).to(DEV)
    small_nhwc = rehouse(to_nhwc(small).contiguous())

    def run():
        return ops.pad_channels(small_nhwc, 32), ops.nhwc_to_nchw(ops.nchw_to_nhwc(small, 32), 5)

    def verify(res):
        want = _snap(CASES["elementwise_and_layout"](ops)())
        assert _same(res, (want[11], want[10])), _first_difference(res, (want[11], want[10]))
        assert torch.equal(res[0][..., :5], to_nhwc(small.cpu())) and int(res[0][..., 5:].count_nonzero()) == 0 and torch.equal(res[1], small.cpu())
    return Checked(run, verify)


# Elsewhere in the table a builder or a run hands the library tensors that torch made on the device: torch.tensor(..., device=...),
# torch.full / torch.ones (accumulators, `.grad` slots), x.clone() (the leaves of the backward cases).  Each such case runs once more
# with those makers' results passed through guard.rehouse.
_MAKERS = ((torch, "tensor"), (torch, "full"), (torch, "ones"), (torch, "full_like"), (torch, "ones_like"), (torch.Tensor, "clone"))


@contextlib.contextmanager
def _device_made_rehoused():
    saved = [(owner, name, getattr(owner, name), name in owner.__dict__) for owner, name in _MAKERS]

    def housed(fn):
        def made(*a, **k):
            out = fn(*a, **k)
            return rehouse(out) if torch.is_tensor(out) and out.grad_fn is None and "out" not in k else out
        return made
    for owner, name, fn, _ in saved:
        setattr(owner, name, housed(fn))
    try:
        yield
    finally:
        for owner, name, fn, own in saved:
            if own:
                setattr(owner, name, fn)
            else:
                delattr(owner, name)          # Tensor.clone is inherited: leave no attribute behind


def _device_made_variant(name, door=False):
    """door: the wrapper itself derives operands with torch ops (folded weights, a converted mask); those, which the library only
    reads, are housed where they are handed over (guard.house_at_the_door)"""
    def build(ops):
        with _device_made_rehoused():
            built = CASES[name](ops)
        c = built if isinstance(built, Case) else Case(built)

        def run():
            if door:
                guard.house_at_the_door()
            with _device_made_rehoused():
                return c.run()
        return Case(run, c.ref, c.bar)
    return build


DEVICE_MADE = [n for n in CASES if n.startswith(("conv_bwd-", "groupnorm_train-3-4-4-256", "chan_layernorm_bwd-", "small_gemm-", "small_n_conv_bwd-",
                                                 "train_step-")) or n in ("time_embed_fwd_bwd", "bias_grad", "grad_norm_clip_adam-100003",
                                                                          "pack_weights-ragged_channels")]
WRAPPER_MADE = ["linattn_small_from_x-2-6-6-96", "linattn_small_from_x-2-2-2-64", "attention_folded-2-32-32", "attention_kv_context-5-16-16",
                "attention_split_from_x-2-8-8-32", "image_metrics", "time_embed_fwd_bwd"]
for _n in DEVICE_MADE:
    variant(_n, "device_made_rehoused")(_device_made_variant(_n, door=_n in WRAPPER_MADE))
for _n in WRAPPER_MADE:
    if _n not in DEVICE_MADE:
        variant(_n, "operands_housed")(_device_made_variant(_n, door=True))


# ================================================================== the one check, over the table and the added cases
ALL = {**CASES, **EXTRA}
OP_LEVEL = [n for n in ALL if not n.startswith(("plan-", "train_step-"))]


def _built(ops, name):
    built = ALL[name](ops)
    return built if isinstance(built, Case) else Case(built)


def _finite(res, what):
    for t in res:
        assert t is None or not t.is_floating_point() or bool(torch.isfinite(t).all()), what


def _under_bands(ops, name, word, skew, plain, reproducible):
    where = f"{name} under word {word:#010x}, skew {skew}"
    with guard_bands(word, skew=skew) as g:
        c = _built(ops, name)             # built inside the block: its inputs are housed in bands
        got = _snap(c.run())              # (synchronizes)
        found = g.check()
        housed = {r.base.untyped_storage().data_ptr() for r in g._records}
        for buf in ops._scratch.values():            # cached scratch was dropped on entry: what is cached now was allocated inside bands
            assert not torch.is_tensor(buf) or buf.untyped_storage().data_ptr() in housed, f"{where}: cached scratch outside bands"
    assert g.count > 0 and g.transfers > 0, f"{where}: banded {dict(g.kinds)}"
    assert not found, f"{where}: bytes outside a tensor were written\n" + "\n".join(map(format_violation, found))
    _finite(got, f"{where}: not finite")
    if reproducible:
        assert _same(plain, got), f"{where}: the result depends on where its tensors lie or on what lies beside them: {_first_difference(plain, got)}"
    else:
        from helpers import rel_err
        for r, want in zip(got, c.ref()):
            assert r is None or rel_err(r, want) < c.bar, f"{where}: off its reference"
    return g


def _handed_over_unbanded(runs):
    """what the wrappers handed to the library from outside any band, over the banded runs of a case: lines for a message"""
    seen = {}
    for g in runs:
        for (site, shape, dtype), n in g.unbanded.items():
            seen[site, shape, dtype] = max(n, seen.get((site, shape, dtype), 0))
    return [f"  {site}: {shape} {dtype}, {n} times" for (site, shape, dtype), n in sorted(seen.items(), key=str)]


@pytest.mark.parametrize("name", list(ALL))
def test_no_byte_outside_a_tensor_is_written_or_read(ops, name):
    c = _built(ops, name)
    plain, again = _snap(c.run()), _snap(c.run())
    reproducible = _same(plain, again)
    if not reproducible:
        assert name in NOT_BIT_REPRODUCIBLE, f"{name}: two plain runs differ ({_first_difference(plain, again)}) and it is not listed"
        assert c.ref is not None and c.bar is not None, f"{name}: listed as not bit-reproducible but has no reference / bar"
    _finite(plain, f"{name}: plain run is not finite")
    if isinstance(c, Checked):
        c.verify(plain)
    runs = [_under_bands(ops, name, word, 0, plain, reproducible) for word in WORDS]
    if name in OP_LEVEL:      # the 16-byte contract of include/ddk.h: every empty-family tensor and every transfer 16 bytes past a 512-byte line
        runs.append(_under_bands(ops, name, NAN, 16, plain, reproducible))
    outside = _handed_over_unbanded(runs)
    print(f"{name}: banded per run {[dict(g.kinds) for g in runs]}; handed to the library from outside any band: {len(outside)}")
    if name in OP_LEVEL and name in CASES:
        assert not outside or VARIANT_OF.get(name) in EXTRA, \
            f"{name} hands the library tensors that lie in no band and has no variant that houses them:\n" + "\n".join(outside)
    elif name in OP_LEVEL:
        assert not outside, f"{name}: still handed to the library from outside any band:\n" + "\n".join(outside)
    elif outside:         # plans and training steps: torch's own intermediates (autograd, the models' torch ops) are expected here
        print("\n".join(outside[:12]))


# ================================================================== the harness itself, on the device (torch ops only)
@pytest.mark.parametrize("word", WORDS)
def test_the_check_sees_a_write_outside_a_device_tensor(word):
    mark = 0x12345678          # every byte differs from each word's
    with pytest.raises(guard.GuardError) as caught:
        with guard_bands(word, skew=16) as g:
            past, front = torch.empty((3, 6, 10, 3), device=DEV, dtype=torch.int32), torch.ones(7, dtype=torch.int32).to(DEV)
            clean = torch.zeros(100, device=DEV)
            assert past.data_ptr() % 512 == 16 and front.data_ptr() % 512 == 16 and clean.data_ptr() % 512 == 0
            assert g.check() == [] and (g.count, g.transfers) == (3, 1)
            past.as_strided((1,), (1,), past.storage_offset() + past.numel()).fill_(mark)        # one element past the end
            front.as_strided((1,), (1,), front.storage_offset() - 1).fill_(mark)                 # one before the start: both inside the allocation
            clean.fill_(1.0)
    found = {v.shape: v for v in caught.value.violations}
    assert set(found) == {(3, 6, 10, 3), (7,)}
    assert (found[(3, 6, 10, 3)].side, found[(3, 6, 10, 3)].first, found[(3, 6, 10, 3)].last) == ("after", 0, 3)
    assert (found[(7,)].side, found[(7,)].first, found[(7,)].last, found[(7,)].nbytes) == ("before", -4, -1, 4)
    assert bool((front == 1).all()) and all("test_extents_gpu.py" in v.site for v in found.values())


def test_nothing_is_banded_while_a_stream_is_capturing():
    with guard_bands(NAN) as g, torch.cuda.graph(torch.cuda.CUDAGraph()):
        t = torch.empty(64, device=DEV)
        t.fill_(2.0)
    assert g.count == 0 and t.untyped_storage().nbytes() < guard.BAND
