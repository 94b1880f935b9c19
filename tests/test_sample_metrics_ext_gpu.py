"""ddk_poly_mmd_sums and ddk_manifold_ball_counts (csrc/manifold.hip) against tests/kid_ref.py, and
compute_kid / compute_density_coverage / evaluate_ddpm.py on top of them.

Bars.  Integer rows with gamma = 1/64: every dot product and every t is exact in fp32, k is the kernel's own fp32 (t t) t, so the
three sums equal the restatement up to the order of the double summation, a relative 1e-13: one missing, doubled or misplaced pair, a
diagonal element or a neighbour segment's row shows.  Real-valued rows: each sum within the rounding bound kid_ref derives per pair
(sum e; the observed |err| / sum e is printed).  Ball counts: equal on integer rows; on real rows between the counts with every pair
inside sample_metrics_ref.MARGIN of the radius decided against and for membership, such pairs being at most 1 % of a case."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kid_ref as K
import sample_metrics_ref as R
from helpers import ddpm_cfg
from poison import WORDS, poisoned_allocations, repoison

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 1.0 / 64

# (S, ma, mb, D): the smallest shapes at which each thing can go wrong
SHAPES = {
    "smallest": (1, 2, 2, 4),
    "ragged_ma_ne_mb_d_tail": (1, 130, 90, 40),         # ragged second tile, ma != mb, a D tail below one LDS stage
    "segments_inside_a_tile": (3, 130, 130, 32),        # segments 1 and 2 start at rows 130 and 260
    "three_tiles_k_tail_8": (1, 300, 257, 72),
    "many_tiny_segments": (100, 8, 8, 32),
    "real_width": (1, 1000, 1000, 2048),
}
REAL_SHAPES = ("ragged_ma_ne_mb_d_tail", "three_tiles_k_tail_8", "real_width")
BALL_SHAPES = ((150, 90, 32), (130, 300, 40), (8, 1, 4), (300, 257, 72))             # (Na, Nb, D)


def _ops():
    from ddk import ops
    return ops


def _dev(x):
    return torch.tensor(np.asarray(x), device=DEV)


def _sums(a, b, segments=1, gamma=None, coef0=1.0):
    out = _ops().poly_mmd_sums(_dev(a), _dev(b), segments, gamma, coef0)
    assert out.dtype == torch.float64 and tuple(out.shape) == (segments, 3) and out.is_cuda
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_pair(name):
    s, ma, mb, d = SHAPES[name]
    a, b = R.int_features(101, s * ma, d, 0), R.int_features(102, s * mb, d, 1)
    return a, b, K.sums_exact(a, b, s, GAMMA, 1.0)


@functools.lru_cache(maxsize=None)
def _real_pair(name):
    s, ma, mb, d = SHAPES[name]
    a, b = R.real_features(R.REF_SEED, s * ma, d, 0.0), R.real_features(R.SAMPLE_SEED, s * mb, d, 0.05)
    return (a, b) + K.sums_f64(a, b, s)


def _assert_exact(got, want):
    rel = np.abs(got - want) / np.abs(want)
    print(f"relative difference to the restatement, worst {rel.max():.2e}")
    assert np.all(np.abs(got - want) <= K.EXACT_RTOL * np.abs(want)), (np.argwhere(rel > K.EXACT_RTOL)[:5], got.ravel()[:6], want.ravel()[:6])


# ---------------------------------------------------------------- the sums
@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_arithmetic(name):
    a, b, want = _int_pair(name)
    _assert_exact(_sums(a, b, SHAPES[name][0], GAMMA, 1.0), want)


def test_scaled_unit_rows_against_asymmetric_b():
    """a = 8 e_i: k(a_i, a_j) = 1 off the diagonal and k(a_i, b_j) reads the single element b_j[i], so a transposed epilogue or a
    swapped s0 / s1 (which a symmetric pair of sets would hide) lands in the wrong slot"""
    a = 8.0 * np.eye(64, dtype=np.float32)[:40]
    b = R.int_features(31, 37, 64, 0)
    want = K.sums_exact(a, b, 1, GAMMA, 1.0)
    got = _sums(a, b, 1, GAMMA, 1.0)
    assert got[0, 0] == 40 * 39 == want[0, 0] and want[0, 1] != want[0, 0]
    _assert_exact(got, want)
    swapped = _sums(b, a, 1, GAMMA, 1.0)
    _assert_exact(swapped, want[:, [1, 0, 2]])


def test_one_dominant_row():
    """one row of each set scaled by 50: its diagonal term is some 10^5 times the whole off-diagonal sum, which must still match"""
    a, b = R.int_features(111, 130, 40, 0), R.int_features(112, 90, 40, 1)
    a[7] *= 50
    b[88] *= 50
    want = K.sums_exact(a, b, 1, GAMMA, 1.0)
    diagonal = float(K.kernel_exact(a[7:8], a[7:8], GAMMA, 1.0)[0, 0])
    assert diagonal > 1e3 * abs(want[0, 0])
    _assert_exact(_sums(a, b, 1, GAMMA, 1.0), want)


def test_gamma_and_coef0_are_used():
    a, b, _ = _int_pair("ragged_ma_ne_mb_d_tail")
    for gamma, coef0 in ((1.0 / 32, 1.0), (GAMMA, 0.5), (GAMMA, -2.0)):          # (t keeps one sign: no cancellation in the sums)
        _assert_exact(_sums(a, b, 1, gamma, coef0), K.sums_exact(a, b, 1, gamma, coef0))


def _check_real(a, b, segments, want, bound, label):
    got = _sums(a, b, segments)
    ratio = np.abs(got - want) / bound
    print(f"{label}: |err| / sum e = {ratio.ravel()}")
    assert np.all(np.abs(got - want) <= bound)
    again = _sums(a, b, segments)
    assert np.array_equal(again.view(np.int64), got.view(np.int64))                      # the same bits from run to run


@pytest.mark.parametrize("name", REAL_SHAPES)
def test_real_features_within_derived_bound(name):
    a, b, want, bound = _real_pair(name)
    _check_real(a, b, SHAPES[name][0], want, bound, SHAPES[name])
    if name != "real_width":                                                             # the bound has teeth: the diagonal would show
        wrong = K.sums_with_diagonal(a, b, SHAPES[name][0])
        assert np.all(np.abs(wrong - want)[:, :2] > 1000 * bound[:, :2])


@pytest.mark.parametrize("case", range(len(R.REAL_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.REAL_CASES])
def test_real_fixture_within_derived_bound(case):
    ref, smp = R.real_case(case)
    want, bound = K.sums_f64(ref, smp)
    _check_real(ref, smp, 1, want, bound, R.REAL_CASES[case])


def test_width_padded_to_a_multiple_of_four():
    """D = 70 goes through the wrapper's zero padding; gamma stays 1 / 70"""
    a, b = R.real_features(1, 50, 70, 0.0), R.real_features(2, 33, 70, 0.05)
    want, bound = K.sums_f64(a, b)
    _check_real(a, b, 1, want, bound, (1, 50, 33, 70))


# ---------------------------------------------------------------- KID
def test_compute_kid_kernels_numpy_and_reference():
    from utils.sample_metrics import compute_kid
    ref, smp = R.real_features(R.REF_SEED, 400, 64, 0.0), R.real_features(R.SAMPLE_SEED, 350, 64, 0.1)
    want, bar = K.kid(ref, smp, 5, 128, 0)
    got, host = compute_kid(ref, smp, subsets=5, subset_size=128, use_gpu=True), compute_kid(ref, smp, subsets=5, subset_size=128, use_gpu=False)
    for key in ("kid_mean", "kid_std", "kid_full"):
        print(f"{key}: kernels {got[key]:.9e}, numpy {host[key]:.9e}, float64 {want[key]:.9e}, bound {bar[key]:.2e}, "
              f"|kernels - f64| / bound {abs(got[key] - want[key]) / bar[key]:.4f}")
        assert abs(got[key] - want[key]) <= bar[key] and abs(host[key] - want[key]) <= bar[key], key
        assert abs(want[key]) > 10 * bar[key], key                                       # the value is not lost in its bound
    assert compute_kid(ref, smp, subsets=5, subset_size=128) == got                      # a device is present: the default is the kernels
    clamped = compute_kid(ref[:40], smp[:25], subsets=3, subset_size=1000, use_gpu=True)   # m = 25
    want_c, bar_c = K.kid(ref[:40], smp[:25], 3, 25, 0)
    assert all(abs(clamped[k] - want_c[k]) <= bar_c[k] for k in clamped)


# ---------------------------------------------------------------- ball counts
def _counts(a, ra, b):
    out = _ops().manifold_ball_counts(_dev(a), _dev(ra), _dev(b))
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(a),)
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", BALL_SHAPES, ids=["x".join(map(str, s)) for s in BALL_SHAPES])
def test_ball_counts_on_integer_rows(shape):
    from utils.sample_metrics import compute_density_coverage
    na, nb, d = shape
    a, b = R.int_features(121, na, d, 0), R.int_features(122, nb, d, 1)
    for k in (1, 5, 7):
        radii = _ops().manifold_radii(_dev(a), k).cpu().numpy()
        assert np.array_equal(radii, R.radii(a, k).astype(np.float32))
        got, want = _counts(a, radii, b), K.ball_counts(a, radii, b)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        dc = compute_density_coverage(a, b, k=k, use_gpu=True)
        assert dc == compute_density_coverage(a, b, k=k, use_gpu=False) == K.density_coverage(a, b, k)
    assert compute_density_coverage(a, b) == compute_density_coverage(a, b, k=5, use_gpu=True)
    self_density, self_coverage = compute_density_coverage(a, a, k=5, use_gpu=True)
    assert self_coverage == 1.0 and self_density >= 6 / 5


@pytest.mark.parametrize("shape", BALL_SHAPES, ids=["x".join(map(str, s)) for s in BALL_SHAPES])
def test_ball_counts_on_real_rows(shape):
    na, nb, d = shape
    a, b = R.real_features(R.REF_SEED, na, d, 0.0), R.real_features(R.SAMPLE_SEED, nb, d, 0.1)
    for k in (1, 5, 7):
        radii = _ops().manifold_radii(_dev(a), k).cpu().numpy()
        low, high, share = K.ball_count_range(a, radii, b)
        got = _counts(a, radii, b)
        print(f"{shape} k = {k}: pairs within the margin {share:.5f}, counts sum {got.sum()} in [{low.sum()}, {high.sum()}]")
        assert share <= K.AMBIGUOUS_PAIR_CAP
        assert np.all(low <= got) and np.all(got <= high), np.flatnonzero((got < low) | (got > high))[:8]
        assert np.array_equal(_counts(a, radii, b), got)


def test_counts_beyond_one_column_range():
    """more than 8 column tiles: several workgroups add to one row's count, each after walking several tiles"""
    a, b = R.int_features(131, 137, 16, 0), R.int_features(132, 9 * 128 + 5, 16, 1)
    radii = R.radii(a, 3).astype(np.float32)
    got, want = _counts(a, radii, b), K.ball_counts(a, radii, b)
    assert np.array_equal(got, want)
    first, last = K.ball_counts(a, radii, b[:5 * 128]), K.ball_counts(a, radii, b[5 * 128:])
    assert np.any((first > 0) & (last > 0))                                              # some row's count comes from both ends of the walk


# ---------------------------------------------------------------- buffers, refusals, the tool
def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def test_results_do_not_depend_on_buffer_contents():
    """sums, counts and both workspaces filled with each poison word before the call: bit-identical results, and from run to run"""
    ops = _ops()
    a, b, _ = _int_pair("segments_inside_a_tile")
    ra, rb, _, _ = _real_pair("ragged_ma_ne_mb_d_tail")
    xa, xb = _dev(R.int_features(121, 150, 32, 0)), _dev(R.int_features(122, 90, 32, 1))
    da, db, dra, drb = _dev(a), _dev(b), _dev(ra), _dev(rb)
    radii = ops.manifold_radii(xa, 5)

    def run():
        res = (ops.poly_mmd_sums(da, db, 3, GAMMA, 1.0), ops.poly_mmd_sums(dra, drb), ops.manifold_ball_counts(xa, radii, xb))
        torch.cuda.synchronize()
        return tuple(_bits(t).cpu().clone() for t in res)

    plain = run()
    assert all(torch.equal(p, q) for p, q in zip(plain, run()))
    for word in WORDS:
        assert repoison(word) >= 2                                                       # the cached workspaces of both entries
        with poisoned_allocations(word) as p:
            got = run()
        assert p.count >= 3, "the results must come from the patched allocation paths"
        assert all(torch.equal(x, y) for x, y in zip(plain, got)), f"word {word:#010x}"


def test_c_entries_refuse_bad_arguments():
    """DDK_REQUIRE in front of any device work: the entry returns -1 and names the argument"""
    from ddk import lib as L
    lib = L.load()
    x = torch.zeros((16, 8), device=DEV)
    sums = torch.zeros(3, device=DEV, dtype=torch.float64)
    counts = torch.zeros(16, device=DEV, dtype=torch.int32)
    r = torch.zeros(16, device=DEV)
    ws = torch.zeros(1024, device=DEV)
    px, pw, ps = L.ptr(x), L.ptr(ws), L.ptr(sums)

    def mmd(a=px, b=px, s=1, ma=8, mb=8, d=8, out=ps, w=pw, nbytes=4096):
        return lib.ddk_poly_mmd_sums(a, b, s, ma, mb, d, 0.125, 1.0, out, w, nbytes, L.stream())

    assert mmd() == 0
    for kw, word in ((dict(a=None), "null"), (dict(out=None), "null"), (dict(d=6), "multiple of 4"), (dict(ma=1), "ma >= 2"), (dict(mb=1), "mb >= 2"),
                     (dict(a=px + 4), "16-byte aligned"), (dict(out=ps + 4), "8-byte aligned"), (dict(w=pw + 8), "workspace"),
                     (dict(nbytes=16), "workspace"), (dict(w=None), "workspace"), (dict(s=0), "S >= 1")):
        assert mmd(**kw) == -1, kw
        assert "poly_mmd_sums" in L.last_error() and word in L.last_error(), (kw, L.last_error())

    def balls(a=px, ra=L.ptr(r), na=16, b=px, nb=16, d=8, out=L.ptr(counts), w=pw, nbytes=4096):
        return lib.ddk_manifold_ball_counts(a, ra, na, b, nb, d, out, w, nbytes, L.stream())

    assert balls() == 0
    for kw, word in ((dict(ra=None), "null"), (dict(out=None), "null"), (dict(d=6), "multiple of 4"), (dict(na=0), "Na, Nb"),
                     (dict(b=px + 4), "16-byte aligned"), (dict(nbytes=64), "workspace"), (dict(w=pw + 4), "workspace")):
        assert balls(**kw) == -1, kw
        assert "manifold_ball_counts" in L.last_error() and word in L.last_error(), (kw, L.last_error())
    torch.cuda.synchronize()


def test_ops_wrappers_raise_before_device_work():
    from ddk import lib as L
    ops = _ops()
    x = torch.from_numpy(R.int_features(61, 20, 8, 0))
    xd, rd = x.to(DEV), torch.zeros(20, device=DEV)
    with pytest.raises(L.DDKError):
        ops.poly_mmd_sums(xd, x)                                                        # a host tensor
    with pytest.raises(L.DDKError):
        ops.manifold_ball_counts(xd, rd.cpu(), xd)
    nan = xd.clone()
    nan[3, 2] = float("nan")
    for bad in (dict(a=nan, b=xd), dict(a=xd, b=xd, segments=3), dict(a=xd, b=xd[:10], segments=10), dict(a=xd, b=xd[:, :4]),
                dict(a=xd.double(), b=xd), dict(a=xd, b=xd, gamma=float("inf"))):
        with pytest.raises(ValueError):
            ops.poly_mmd_sums(**bad)
    for a, r, b in ((nan, rd, xd), (xd, rd[:19], xd), (xd, rd.double(), xd), (xd, rd, xd[:, :4]), (xd, None, xd)):
        with pytest.raises(ValueError):
            ops.manifold_ball_counts(a, r, b)


def test_evaluate_ddpm_cli_with_the_new_flags(tmp_path):
    """evaluate_ddpm.py --kid --density_coverage on a tiny synthetic DDPM: the old seven keys first, then the five new ones, all
    equal to extended_sample_metrics"""
    from utils.sample_metrics import extended_sample_metrics
    rng = np.random.default_rng(7)
    files = {}
    for name, shift in (("ref", 0.0), ("sample", 0.05)):
        pool = np.maximum(0.5 * rng.standard_normal((24, 2048)) + 0.3 + shift, 0).astype(np.float32)
        spatial = np.maximum(0.5 * rng.standard_normal((24, 2023)) + 0.3 + shift, 0).astype(np.float32)
        soft = rng.random((24, 10))
        files[name] = tmp_path / f"{name}.npz"
        np.savez(files[name], pool_3=pool, spatial=spatial, softmax=soft / soft.sum(axis=1, keepdims=True))
    cfg = ddpm_cfg(32, 3, 16, T=25)      # (at T = 20 the linear schedule ends on beta = 1: alphas_cumprod = 0, the VLB is NaN)
    cfg.update(model="ddpm", dataset="cifar10", batch_size=2)
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    out = tmp_path / "metrics.json"
    script = os.path.join(ROOT, "downsampled-diffusion_amd", "evaluate_ddpm.py")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "downsampled-diffusion_amd"))
    r = subprocess.run([sys.executable, script, "--synthetic", str(tmp_path / "cfg.json"), "--max_batches", "1", "--seed", "3", "--json",
                        str(out), "--sample_acts", str(files["sample"]), "--ref_acts", str(files["ref"]), "--kid", "--kid_subsets", "4",
                        "--kid_subset_size", "16", "--density_coverage"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    metrics = json.loads(out.read_text())
    want = extended_sample_metrics(str(files["ref"]), str(files["sample"]), kid=True, density_coverage=True, kid_subsets=4, kid_subset_size=16)
    assert list(metrics) == ["vlb", "L_simple", "is", "fid", "sfid", "precision", "recall", "kid_mean", "kid_std", "kid_full", "density",
                             "coverage"]
    for key in list(metrics)[2:]:
        assert metrics[key] is not None and metrics[key] == want[key], key
