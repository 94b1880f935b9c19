"""tests/nonfinite_ref.py on the CPU: what the footprint rules of test_nonfinite_gpu.py catch.  Each test writes an op twice in plain
torch -- as the reference defines it, and with the defect a kernel could have -- and asserts that the rule passes the first and
rejects the second; where the defect is invisible on finite data, that is asserted too."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_ref as NF
from oracle import diffusion_ref as D


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------ the helpers themselves
def test_plant_kinds_and_sets():
    x = rnd(3, 4, 5, seed=1)
    for v, k in zip(NF.VALUES, (NF.K_NAN, NF.K_PINF, NF.K_NINF)):
        p = NF.plant(x, (1, 2, 3), v)
        assert torch.isfinite(x).all(), "plant works on a copy"
        assert int(NF.nonfinite(p).sum()) == 1 and bool(NF.nonfinite(p)[1, 2, 3]) and int(NF.kinds(p)[1, 2, 3]) == k
        assert int(NF.kinds(p).sum()) == k
        assert NF.exact(p, NF.plant(x, (1, 2, 3), NF.NAN)) and NF.exact_kinds(p, p)
        assert NF.exact_kinds(p, NF.plant(x, (1, 2, 3), NF.NAN)) == (k == NF.K_NAN)
        assert not NF.exact(p, x) and not NF.exact(p, NF.plant(x, (1, 2, 4), v))
    with pytest.raises(ValueError):
        NF.plant(x, (1, 2, 3), 1.0)
    with pytest.raises(ValueError):
        NF.plant(x, (1, 2), NF.NAN)
    with pytest.raises(ValueError):
        NF.exact(x, x[:2])


def test_within_asks_for_both_inclusions():
    x = torch.zeros(2, 4)
    ref = NF.plant(x, (0, 1), NF.NAN)
    allowed = torch.zeros(2, 4, dtype=torch.bool)
    allowed[0, :3] = True
    wider = NF.plant(ref, (0, 2), NF.PINF)
    assert NF.within(ref, ref, allowed) and NF.within(wider, ref, allowed)
    assert not NF.within(x, ref, allowed), "the reference's element is missing"
    assert not NF.within(NF.plant(ref, (0, 3), NF.NAN), ref, allowed), "one element outside the allowed set"
    assert not NF.within(NF.plant(ref, (1, 1), NF.NAN), ref, allowed), "the other image"


def test_isolated_compares_bits_of_the_other_images():
    clean = rnd(3, 2, 2, seed=2)
    planted = clean.clone()
    planted[1] = NF.NAN
    assert NF.isolated(planted, clean, 1) and not NF.isolated(planted, clean, 0)
    moved = planted.clone()
    moved[2, 0, 0] = torch.nextafter(moved[2, 0, 0], torch.tensor(9.0))
    assert not NF.isolated(moved, clean, 1), "one ulp in another image"
    zero = torch.zeros(3, 2)
    assert not NF.isolated(-zero, zero, 1), "-0.0 and 0.0 are different bits"


# ------------------------------------------------------------------ the clamp of the reverse step
def _step(x, t, eps, z, buf, clamp):
    """oracle.diffusion_ref.p_sample_update with the clamp handed in"""
    ex = lambda k: D.extract(buf[k], t)
    x0 = clamp(ex("sqrt_recip_alphas_cumprod") * x - ex("sqrt_recipm1_alphas_cumprod") * eps)
    mean = ex("posterior_mean_coef1") * x0 + ex("posterior_mean_coef2") * x
    mask = (1 - (t == 0).float()).reshape(-1, 1, 1, 1)
    return mean + mask * (0.5 * ex("posterior_log_variance_clipped")).exp() * z


def clamp_fmax_fmin(x0):
    """fminf(fmaxf(x0, -1), 1): returns the bound where x0 is NaN"""
    return torch.fmin(torch.fmax(x0, torch.tensor(-1.0)), torch.tensor(1.0))


def clamp_select(x0):
    """x0 < -1 ? -1 : (x0 > 1 ? 1 : x0): a comparison with NaN is false, so NaN falls through"""
    return torch.where(x0 < -1.0, torch.tensor(-1.0), torch.where(x0 > 1.0, torch.tensor(1.0), x0))


@pytest.mark.parametrize("value", NF.VALUES)
@pytest.mark.parametrize("into", ["eps", "x"])
def test_clamp_that_swallows_nan_is_rejected(value, into):
    buf = D.schedule_buffers("linear", 1000)
    x, eps, z = rnd(3, 3, 4, 4, seed=3, scale=1.5), rnd(3, 3, 4, 4, seed=4), rnd(3, 3, 4, 4, seed=5)
    t = torch.tensor([0, 500, 999])
    where = (1, 2, 3, 3)
    xp, ep = (NF.plant(x, where, value), eps) if into == "x" else (x, NF.plant(eps, where, value))
    ref = D.p_sample_update(buf, xp, t, eps_hat=ep, noise=z)
    good, bad = _step(xp, t, ep, z, buf, clamp_select), _step(xp, t, ep, z, buf, clamp_fmax_fmin)
    assert NF.exact_kinds(good, ref), NF.describe(good, ref)
    assert NF.isolated(good, _step(x, t, eps, z, buf, clamp_select), 1)
    if value != value and into == "eps":
        assert not NF.exact(bad, ref), "fmax / fmin turn the NaN into -1: the rule must see it"
        assert torch.isfinite(bad).all(), "the defect in full: a NaN in eps_hat leaves a finite sample"
        assert int(NF.nonfinite(ref).sum()) == 1 and bool(NF.nonfinite(ref)[where])
    else:       # an Inf is clamped to the bound by either form, and a NaN in x also reaches the output through c2 * x
        assert NF.exact_kinds(bad, ref)
    # finite data: the three forms agree bit for bit
    fin = D.p_sample_update(buf, x, t, eps_hat=eps, noise=z)
    assert torch.equal(_step(x, t, eps, z, buf, clamp_select), fin) and torch.equal(_step(x, t, eps, z, buf, clamp_fmax_fmin), fin)


def test_select_clamp_keeps_the_bits_of_finite_values():
    v = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, 1e-45, -1e-45, 0.99999994, -1.0000001])
    assert torch.equal(clamp_select(v).view(torch.int32), v.clamp(-1, 1).view(torch.int32))
    assert torch.equal(clamp_select(v).view(torch.int32), clamp_fmax_fmin(v).view(torch.int32))
    assert torch.isnan(clamp_select(torch.tensor([NF.NAN]))).all() and torch.isnan(torch.tensor([NF.NAN]).clamp(-1, 1)).all()


def test_vlb_floor_that_hides_nan_is_rejected():
    """log(fmaxf(cdf, 1e-12)) reports log(1e-12) for a NaN CDF; the reference's clamp(min=1e-12) keeps the NaN"""
    cdf = NF.plant(torch.rand(2, 8, generator=torch.Generator().manual_seed(6)), (1, 5), NF.NAN)
    ref = torch.log(cdf.clamp(min=1e-12))
    bad = torch.log(torch.fmax(cdf, torch.tensor(1e-12)))
    good = torch.log(torch.where(cdf < 1e-12, torch.tensor(1e-12), cdf))
    assert NF.exact_kinds(good, ref) and torch.equal(good[0], ref[0])
    assert not NF.exact(bad, ref) and torch.isfinite(bad).all()


# ------------------------------------------------------------------ the output stage's per-image minimum and maximum
def fix_samples_skipping_nan(x):
    """fminf / fmaxf reductions: the NaN is skipped, the image is scaled by the range of the rest"""
    b = x.shape[0]
    flat = x.reshape(b, -1)
    nan = torch.isnan(flat)           # (nan_to_num's semantics for NaN alone: an Inf stays what it is)
    lo = torch.where(nan, torch.tensor(float("inf")), flat).min(dim=1).values[:, None, None, None]
    hi = torch.where(nan, torch.tensor(float("-inf")), flat).max(dim=1).values[:, None, None, None]
    return (((x - lo) / (hi - lo)) * 255.0).permute(0, 2, 3, 1)


@pytest.mark.parametrize("value", NF.VALUES)
def test_min_max_that_skips_nan_is_rejected(value):
    x = rnd(3, 3, 5, 4, seed=7)
    xp = NF.plant(x, (1, 2, 4, 3), value)
    ref = torch.from_numpy(D.fix_samples(xp))
    bad = fix_samples_skipping_nan(xp)
    assert NF.isolated(ref, torch.from_numpy(D.fix_samples(x)), 1)
    if value == NF.PINF:      # the range is +Inf: every finite element becomes 0 and the planted one Inf / Inf
        assert int(NF.nonfinite(ref).sum()) == 1 and bool(torch.isnan(ref[1, 4, 3, 2]))
    else:                     # NaN - lo, or (x + Inf) / Inf: the whole planted image is NaN
        assert bool(torch.isnan(ref[1]).all()) and int(NF.nonfinite(ref).sum()) == ref[1].numel()
    assert NF.exact_kinds(torch.from_numpy(D.fix_samples(xp.clone())), ref)
    if value != value:
        assert not NF.exact(bad, ref) and int(NF.nonfinite(bad).sum()) == 1, "only the one element: the rule must see it"
    else:
        assert NF.exact_kinds(bad, ref), "an Inf is a minimum or a maximum in either form"
    assert torch.equal(fix_samples_skipping_nan(x), torch.from_numpy(D.fix_samples(x))), "the same on finite data"


# ------------------------------------------------------------------ a conv that reads its batch neighbour under an exact zero
def conv3x3_neighbour_times_zero(x, w, b):
    """3x3, padding 1, on the images stacked along H: the row above an image's first row is the batch neighbour's last row, read and
    multiplied by 0 -- as a tile that holds several images does when it masks its halo after the load instead of before"""
    B, C, H, W = x.shape
    tall = x.permute(1, 0, 2, 3).reshape(1, C, B * H, W)
    rows = torch.arange(B * H)
    out = torch.zeros(1, w.shape[0], B * H, W, dtype=x.dtype)
    for ky in range(3):
        src = rows + ky - 1
        same = ((src >= 0) & (src < B * H) & (src.clamp(0, B * H - 1) // H == rows // H)).to(x.dtype)        # 1 inside the image, else 0
        taken = tall[:, :, src.clamp(0, B * H - 1), :] * same.view(1, 1, -1, 1)
        out = out + F.conv2d(taken, w[:, :, ky:ky + 1, :], padding=(0, 1))
    return out.reshape(w.shape[0], B, H, W).permute(1, 0, 2, 3) + b.view(1, -1, 1, 1)


def test_neighbour_row_times_zero_fails_isolated_and_passes_on_finite_data():
    x, w, b = rnd(3, 4, 4, 4, seed=8).double(), rnd(5, 4, 3, 3, seed=9).double(), rnd(5, seed=10).double()
    ref_clean = F.conv2d(x, w, b, padding=1)
    leaky_clean = conv3x3_neighbour_times_zero(x, w, b)
    assert (leaky_clean - ref_clean).abs().max() < 1e-12, "on finite data the defect cannot be seen"
    for where in ((1, 3, 3, 3), (1, 0, 0, 0)):        # the image's last pixel leaks down into image 2, its first up into image 0
        xp = NF.plant(x, where, NF.NAN)
        ref, leaky = F.conv2d(xp, w, b, padding=1), conv3x3_neighbour_times_zero(xp, w, b)
        assert NF.isolated(ref, ref_clean, 1) and NF.exact(ref, ref)
        assert not NF.isolated(leaky, leaky_clean, 1), "0 * NaN is NaN: the neighbour's rows must change"
        assert not NF.exact(leaky, ref)
    ref_corner = F.conv2d(NF.plant(x, (1, 0, 0, 0), NF.NAN), w, b, padding=1)
    assert int(NF.nonfinite(ref_corner).sum()) == 4 * 5, "the reference footprint on a corner: a 2 x 2 neighbourhood, every output channel"


# ------------------------------------------------------------------ Winograd F(2x2, 3x3)
BT = torch.tensor([[1., 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G = torch.tensor([[1., 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def conv3x3_winograd(x, w, b, leak=0):
    """3x3, padding 1, NCHW, as F(2x2, 3x3): A^T [sum_c (G g G^T) o (B^T d B)] A per 2x2 output tile.  leak > 0: the defect -- every
    tile also adds 0 * (the first product of the tile `leak` to its right), as a kernel does that sums one tile too many under a mask."""
    B, C, H, W = x.shape
    Hp, Wp = H + (H & 1), W + (W & 1)
    xp = F.pad(x, (1, 1 + Wp - W, 1, 1 + Hp - H))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                   # [B, C, ty, tx, 4, 4]
    V = torch.einsum("ik,bcyxkl,jl->bcyxij", BT, d, BT)
    U = torch.einsum("ik,nckl,jl->ncij", G, w, G)
    M = torch.einsum("bcyxij,ncij->bnyxij", V, U)
    if leak:
        M = M + 0.0 * torch.roll(M, -leak, dims=3)[..., :1, :1]
    Y = torch.einsum("ik,bnyxkl,jl->bnyxij", AT, M, AT)                      # [B, N, ty, tx, 2, 2]
    out = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], Hp, Wp)[:, :, :H, :W]
    return out + b.view(1, -1, 1, 1)


@pytest.mark.parametrize("H,W", [(4, 4), (5, 7), (8, 6)])
def test_winograd_restatement_passes_within_and_a_leak_of_one_tile_fails(H, W):
    x, w, b = rnd(3, 4, H, W, seed=11).double(), rnd(6, 4, 3, 3, seed=12).double(), rnd(6, seed=13).double()
    clean = conv3x3_winograd(x, w, b)
    assert (clean - F.conv2d(x, w, b, padding=1)).abs().max() < 1e-12
    assert (conv3x3_winograd(x, w, b, leak=1) - clean).abs().max() == 0, "on finite data the leak cannot be seen"
    for y, xx in ((0, 0), (H - 1, W - 1), (1, 2), (H // 2, 0)):
        for value in NF.VALUES:
            where = (1, y, xx, 3)                                            # NHWC index of the planted element
            xp = NF.plant(x, (1, 3, y, xx), value)
            ref = F.conv2d(xp, w, b, padding=1).permute(0, 2, 3, 1)
            allowed = NF.wino_allowed(tuple(ref.shape), where)
            got = conv3x3_winograd(xp, w, b).permute(0, 2, 3, 1)
            assert NF.within(got, ref, allowed), NF.describe(got, ref, allowed)
            assert NF.within(ref, ref, allowed), "the direct footprint lies inside the allowed set"
            assert NF.isolated(got, clean.permute(0, 2, 3, 1), 1)
            leaky = conv3x3_winograd(xp, w, b, leak=1).permute(0, 2, 3, 1)
            if xx >= 3:          # there is a tile to the left whose patch does not hold column xx: it must stay finite, and does not
                assert not NF.within(leaky, ref, allowed), NF.describe(leaky, ref, allowed)


def test_wino_allowed_geometry():
    a = NF.wino_allowed((3, 4, 4, 2), (1, 0, 0, 1))          # corner: only tile (0, 0), whose patch is rows -1 .. 2
    assert int(a.sum()) == 2 * 2 * 2 and bool(a[1, :2, :2].all()) and not bool(a[0].any()) and not bool(a[2].any())
    a = NF.wino_allowed((3, 4, 4, 2), (1, 1, 2, 0))          # row 1: tiles 0 and 1 (patches -1 .. 2 and 1 .. 4); column 2: both as well
    assert bool(a[1].all())
    a = NF.wino_allowed((1, 5, 7, 1), (0, 4, 6, 0))          # odd sizes: the last, ragged tile and the one before (row 4 is in 1 .. 4)
    assert bool(a[0, 2:5, 4:7].all()) and int(a.sum()) == 3 * 3
    # the transposed conv: the direct footprint of input (y, x) is output rows 2y - 1 .. 2y + 2, inside the allowed set
    x, w = rnd(1, 2, 4, 4, seed=14).double(), rnd(2, 3, 4, 4, seed=15).double()
    for y, xx in ((0, 0), (3, 3), (1, 2)):
        ref = F.conv_transpose2d(NF.plant(x, (0, 1, y, xx), NF.NAN), w, stride=2, padding=1).permute(0, 2, 3, 1)
        a = NF.wino_allowed(tuple(ref.shape), (0, y, xx, 1), tile=2, patch=3, transpose=True)
        assert NF.within(ref, ref, a) and int(a.sum()) < a.numel()
        rows = a[0, :, :, 0].any(dim=1).nonzero().flatten().tolist()
        cols = a[0, :, :, 0].any(dim=0).nonzero().flatten().tolist()
        # by hand: phase 0 of tile t reads rows 2t - 1 .. 2t + 1 and writes 4t, 4t + 2; phase 1 reads 2t .. 2t + 2 and writes 4t + 1, 4t + 3
        want = {0: [0, 1, 2, 3], 3: [4, 5, 6, 7], 1: [0, 1, 2, 3, 4, 6], 2: [1, 3, 4, 5, 6, 7]}
        assert rows == want[y] and cols == want[xx], (y, xx, rows, cols)
