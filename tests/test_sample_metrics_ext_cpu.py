"""KID and density / coverage on the host (utils/sample_metrics.py): the numpy paths against tests/kid_ref.py,
the documented subset draw, the clamp of the subset size, argument errors, extended_sample_metrics, the tools' flags and the C ABI's
four new names.  The kernels themselves are in test_sample_metrics_ext_gpu.py, their host half in test_sample_metrics_ext_host.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kid_ref as K
import sample_metrics_ref as R
import utils.sample_metrics as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "downsampled-diffusion_amd")
ENV = dict(os.environ, PYTHONPATH=PKG)
NEW = ("ddk_poly_mmd_workspace_bytes", "ddk_poly_mmd_sums", "ddk_manifold_ball_counts_workspace_bytes", "ddk_manifold_ball_counts")


# ---------------------------------------------------------------- the sums
@pytest.mark.parametrize("case", range(len(R.INT_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.INT_CASES])
def test_numpy_sums_on_integer_fixtures(case):
    """every dot and every t is exact in float32 (gamma = 1/64): only the order of the float64 sums is open"""
    ref, smp = R.int_case(case)
    got, want = SM.poly_mmd_sums_numpy(ref, smp, 1, 1.0 / 64, 1.0, row_block=64), K.sums_exact(ref, smp, 1, 1.0 / 64, 1.0)
    assert got.dtype == np.float64 and got.shape == (1, 3)
    assert np.all(np.abs(got - want) <= K.EXACT_RTOL * np.abs(want)), (got, want)


def test_numpy_sums_segments_start_anywhere():
    a, b = R.int_features(71, 3 * 50, 32, 0), R.int_features(72, 3 * 37, 32, 1)
    got, want = SM.poly_mmd_sums_numpy(a, b, 3, 1.0 / 64, 1.0, row_block=16), K.sums_exact(a, b, 3, 1.0 / 64, 1.0)
    assert got.shape == (3, 3) and np.all(np.abs(got - want) <= K.EXACT_RTOL * np.abs(want))
    assert len({tuple(r) for r in want}) == 3                                            # the segments differ: none is read for another


@pytest.mark.parametrize("case", range(len(R.REAL_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.REAL_CASES])
def test_numpy_sums_on_real_fixtures_within_derived_bound(case):
    ref, smp = R.real_case(case)
    got = SM.poly_mmd_sums_numpy(ref, smp)
    want, bound = K.sums_f64(ref, smp)
    print(f"{R.REAL_CASES[case]}: |err| / bound {np.abs(got - want) / bound}")
    assert np.all(np.abs(got - want) <= bound)
    wrong = K.sums_with_diagonal(ref, smp)                                               # the bound is tight enough to see the diagonal
    assert np.all(np.abs(wrong - want)[0, :2] > 10 * bound[0, :2])


# ---------------------------------------------------------------- KID
def test_subset_draw_is_reproducible_and_as_documented():
    ri, si = SM.kid_subset_indices(50, 40, 4, 16, seed=5)
    again = SM.kid_subset_indices(50, 40, 4, 16, seed=5)
    assert ri.shape == si.shape == (4, 16) and np.array_equal(ri, again[0]) and np.array_equal(si, again[1])
    rng = np.random.Generator(np.random.PCG64(5))                                        # restated from the docstring, in its order
    for s in range(4):
        assert np.array_equal(ri[s], rng.choice(50, size=16, replace=False))
        assert np.array_equal(si[s], rng.choice(40, size=16, replace=False))
    assert all(len(set(row)) == 16 for row in ri) and all(len(set(row)) == 16 for row in si)    # without replacement
    assert ri.max() < 50 and si.max() < 40 and min(ri.min(), si.min()) >= 0
    assert not np.array_equal(ri, SM.kid_subset_indices(50, 40, 4, 16, seed=6)[0])
    assert "PCG64" in SM.kid_subset_indices.__doc__ and "replace=False" in SM.kid_subset_indices.__doc__


def test_compute_kid_numpy_against_reference():
    ref, smp = R.real_features(R.REF_SEED, 120, 64, 0.0), R.real_features(R.SAMPLE_SEED, 90, 64, 0.1)
    got = SM.compute_kid(ref, smp, subsets=5, subset_size=32, seed=3, use_gpu=False)
    want, bar = K.kid(ref, smp, 5, 32, 3)
    assert list(got) == ["kid_mean", "kid_std", "kid_full"]
    for key in got:
        print(f"{key}: {got[key]:.9e} vs {want[key]:.9e}, |err| / bound {abs(got[key] - want[key]) / bar[key]:.4f}")
        assert isinstance(got[key], float) and abs(got[key] - want[key]) <= bar[key], key
    assert want["kid_full"] > 10 * bar["kid_full"] and want["kid_std"] > 10 * bar["kid_std"]       # the values are not lost in the bound
    assert SM.compute_kid(ref, smp, subsets=5, subset_size=32, seed=3, use_gpu=False) == got
    assert SM.compute_kid(ref, smp, subsets=5, subset_size=32, seed=4, use_gpu=False)["kid_full"] == got["kid_full"]
    assert SM.compute_kid(ref, smp, subsets=5, subset_size=32, seed=4, use_gpu=False)["kid_mean"] != got["kid_mean"]


def test_kid_of_one_distribution_is_near_zero_and_grows_with_the_shift():
    a, b = R.real_features(1, 300, 64, 0.0), R.real_features(2, 300, 64, 0.0)
    same = SM.compute_kid(a, b, subsets=10, subset_size=100, use_gpu=False)
    far = SM.compute_kid(a, R.real_features(2, 300, 64, 0.3), subsets=10, subset_size=100, use_gpu=False)
    assert abs(same["kid_full"]) < 0.05 * far["kid_full"] and abs(same["kid_mean"]) < 3 * same["kid_std"] + 1e-12
    assert far["kid_mean"] > 10 * far["kid_std"] > 0


def test_subset_size_is_clamped_to_the_smaller_set():
    ref, smp = R.real_features(1, 40, 32, 0.0), R.real_features(2, 25, 32, 0.1)
    got = SM.compute_kid(ref, smp, subsets=3, subset_size=1000, seed=0, use_gpu=False)
    want, bar = K.kid(ref, smp, 3, 25, 0)                                                # m = 25: every subset holds all 25 samples
    for key in got:
        assert abs(got[key] - want[key]) <= bar[key], key
    ri, si = SM.kid_subset_indices(40, 25, 3, 25, 0)
    assert all(sorted(row) == list(range(25)) for row in si)


# ---------------------------------------------------------------- density / coverage
@pytest.mark.parametrize("case", range(len(R.INT_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.INT_CASES])
@pytest.mark.parametrize("k", [1, 5])
def test_numpy_ball_counts_and_density_coverage_on_integer_fixtures(case, k):
    ref, smp = R.int_case(case)
    radii = R.radii(ref, k).astype(np.float32)
    got = SM.ball_counts_numpy(ref, radii, smp, row_block=64)
    assert got.dtype == np.int32 and np.array_equal(got, K.ball_counts(ref, radii, smp))
    dc = SM.compute_density_coverage(ref, smp, k=k, use_gpu=False)
    assert dc == K.density_coverage(ref, smp, k)
    assert 0 < dc[1] < 1 and dc[0] > 0                                                   # neither is trivial on these fixtures


def test_numpy_ball_counts_on_real_fixture():
    ref, smp = R.real_features(R.REF_SEED, 150, 40, 0.0), R.real_features(R.SAMPLE_SEED, 90, 40, 0.1)
    radii = R.radii(ref, 5).astype(np.float32)
    low, high, share = K.ball_count_range(ref, radii, smp)
    got = SM.ball_counts_numpy(ref, radii, smp)
    assert share <= K.AMBIGUOUS_PAIR_CAP and np.all(low <= got) and np.all(got <= high) and high.sum() > 0


@pytest.mark.parametrize("k", [1, 5, 7])
def test_a_set_against_itself(k):
    for x in (R.int_features(81, 130, 24, 0), R.real_features(82, 130, 24, 0.0)):
        density, coverage = SM.compute_density_coverage(x, x, k=k, use_gpu=False)
        assert coverage == 1.0 and density >= (k + 1) / k


# ---------------------------------------------------------------- argument errors
def test_argument_errors():
    x, y = R.real_features(1, 20, 8, 0.0), R.real_features(2, 12, 8, 0.0)
    for fn in (SM.compute_kid, SM.compute_density_coverage):
        for bad in ((x.astype(np.float64), y), (x, y[:, :4]), (x[0], y), (x, np.full_like(y, np.nan))):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(*bad, use_gpu=False)
    for kw in (dict(subsets=0), dict(subsets=2.5), dict(subset_size=1), dict(subset_size=True)):
        with pytest.raises(ValueError, match="compute_kid"):
            SM.compute_kid(x, y, use_gpu=False, **kw)
    with pytest.raises(ValueError, match="at least 2 rows"):
        SM.compute_kid(x, y[:1], use_gpu=False)
    for k in (0, 8, 2.0):
        with pytest.raises(ValueError, match="k must be"):
            SM.compute_density_coverage(x, y, k=k, use_gpu=False)
    with pytest.raises(ValueError, match="k \\+ 1"):
        SM.compute_density_coverage(x[:5], y, k=5, use_gpu=False)
    with pytest.raises(ValueError):
        SM.poly_mmd_sums_numpy(x, y, 3)                                                  # 20 rows do not split into 3 segments
    with pytest.raises(ValueError):
        SM.poly_mmd_sums_numpy(x[:4], y[:4], 4)                                          # segments of one row


def test_ops_wrappers_raise_before_device_work():
    """bad arguments are ValueErrors before anything touches a device; good host tensors reach the device check"""
    import torch
    from ddk import lib as L
    from ddk import ops
    x, r = torch.from_numpy(R.int_features(61, 20, 8, 0)), torch.zeros(20)
    for bad in (dict(segments=0), dict(segments=3), dict(segments=20), dict(segments=1.0), dict(gamma=float("nan")), dict(coef0="1")):
        with pytest.raises(ValueError, match="poly_mmd_sums"):
            ops.poly_mmd_sums(x, x, **bad)
    for a, b in ((x.double(), x), (x, x[:, :4]), (x[0], x), ([[1.0]], x)):
        with pytest.raises(ValueError, match="poly_mmd_sums"):
            ops.poly_mmd_sums(a, b)
        with pytest.raises(ValueError, match="manifold_ball_counts"):
            ops.manifold_ball_counts(a, r, b)
    for bad_r in (r[:19], r.double(), None):
        with pytest.raises(ValueError, match="ra must be"):
            ops.manifold_ball_counts(x, bad_r, x)
    with pytest.raises(L.DDKError, match="ROCm"):
        ops.poly_mmd_sums(x, x)
    with pytest.raises(L.DDKError, match="ROCm"):
        ops.manifold_ball_counts(x, r, x)


# ---------------------------------------------------------------- extended_sample_metrics and the tools
@pytest.fixture(scope="module")
def act_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ext_acts")
    rng = np.random.default_rng(11)
    pools = {}
    for name, shift in (("ref", 0.0), ("sample", 0.05)):
        pools[name] = np.maximum(0.5 * rng.standard_normal((24, SM.POOL_DIM)) + 0.3 + shift, 0).astype(np.float32)
        soft = rng.random((24, 10))
        np.savez(d / f"{name}.npz", pool_3=pools[name], softmax=soft / soft.sum(axis=1, keepdims=True))
    st = SM.compute_statistics(pools["ref"])
    np.savez(d / "ref_stats.npz", mu=st.mu, sigma=st.sigma)
    return d, pools


def test_extended_sample_metrics_keeps_the_five_keys_first_and_equal(act_files):
    d, pools = act_files
    base = SM.sample_metrics(d / "ref.npz", d / "sample.npz")
    assert SM.SAMPLE_METRICS == ('is', 'fid', 'sfid', 'precision', 'recall') and list(base) == list(SM.SAMPLE_METRICS)
    ext = SM.extended_sample_metrics(d / "ref.npz", d / "sample.npz", kid=True, density_coverage=True, kid_subsets=4, kid_subset_size=16)
    assert list(ext) == list(SM.SAMPLE_METRICS) + ["kid_mean", "kid_std", "kid_full", "density", "coverage"] == list(SM.SAMPLE_METRICS) + list(SM.EXTENDED_METRICS)
    assert {k: ext[k] for k in base} == base
    kid = SM.compute_kid(pools["ref"], pools["sample"], subsets=4, subset_size=16)
    assert {k: ext[k] for k in kid} == kid
    assert (ext["density"], ext["coverage"]) == SM.compute_density_coverage(pools["ref"], pools["sample"])
    only_dc = SM.extended_sample_metrics(d / "ref.npz", d / "sample.npz", density_coverage=True)
    assert list(only_dc) == list(SM.SAMPLE_METRICS) + ["density", "coverage"] and only_dc["density"] == ext["density"]
    # a statistics-only reference has no rows: the requested keys are there and None
    stats = SM.extended_sample_metrics(d / "ref_stats.npz", d / "sample.npz", kid=True, density_coverage=True)
    assert list(stats) == list(ext) and all(stats[k] is None for k in SM.EXTENDED_METRICS) and stats["fid"] == base["fid"]


def test_compare_datasets_cli_flags(act_files, tmp_path):
    d, pools = act_files
    script, out = os.path.join(PKG, "compare_datasets.py"), tmp_path / "cmp.json"
    common = [sys.executable, script, "--ds_1", str(d / "ref.npz"), "--ds_2", str(d / "sample.npz"), "--json", str(out)]
    # (without the flags: test_sample_metrics_cpu.py::test_compare_datasets_cli pins the four keys and their values, as before)
    r = subprocess.run(common + ["--kid", "--kid_subsets", "4", "--kid_subset_size", "16", "--density_coverage"], capture_output=True,
                       text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(out.read_text())
    assert list(got) == ["fid", "sfid", "precision", "recall", "kid_mean", "kid_std", "kid_full", "density", "coverage"]
    want = SM.extended_sample_metrics(d / "ref.npz", d / "sample.npz", kid=True, density_coverage=True, kid_subsets=4, kid_subset_size=16)
    assert got == {k: want[k] for k in got}
    r = subprocess.run(common + ["--kid", "--kid_subset_size", "1"], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 2 and "--kid_subset_size" in r.stderr


def test_evaluate_ddpm_new_flags_parse():
    """the likelihood half needs the device (its run with the flags is in test_sample_metrics_ext_gpu.py); here the parser"""
    script = os.path.join(PKG, "evaluate_ddpm.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0
    for flag in ("--kid", "--kid_subsets", "--kid_subset_size", "--density_coverage"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, script, "--kid"], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 2 and "--sample_acts" in r.stderr
    r = subprocess.run([sys.executable, script, "--sample_acts", "s.npz", "--ref_acts", "r.npz", "--kid", "--kid_subsets", "0"],
                       capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 2 and "--kid_subsets" in r.stderr
    src = open(script).read()
    assert "SAMPLE_METRICS = ('is', 'fid', 'sfid', 'precision', 'recall')" in src        # the default key list is the old one


# ---------------------------------------------------------------- the C ABI
def test_header_signatures_and_library_agree_on_the_new_entries():
    from ddk import lib as L
    from ddk import ops
    hdr = open(os.path.join(ROOT, "include", "ddk.h")).read()
    declared = set(re.findall(r"\b(ddk_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in declared and name in L.SIGNATURES
        assert getattr(lib, name) is not None
        params = re.search(r"\b" + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[name][1]), name
    assert len(L.SIGNATURES["ddk_poly_mmd_sums"][1]) == 12 and len(L.SIGNATURES["ddk_poly_mmd_workspace_bytes"][1]) == 3
    assert len(L.SIGNATURES["ddk_manifold_ball_counts"][1]) == 10 and len(L.SIGNATURES["ddk_manifold_ball_counts_workspace_bytes"][1]) == 2
    assert L.load().ddk_version() == L.ABI_VERSION == 400
    assert callable(ops.poly_mmd_sums) and callable(ops.manifold_ball_counts)


def test_workspace_size_queries_are_host_arithmetic():
    """one double per 128 x 128 tile: the upper triangles of a x a and b x b, the rectangle a x b; 0 for shapes the entry refuses"""
    from ddk import lib as L
    lib = L.load()
    tiles = lambda ma, mb: (lambda ta, tb: ta * (ta + 1) // 2 + tb * (tb + 1) // 2 + ta * tb)(-(-ma // 128), -(-mb // 128))
    for s, ma, mb in ((1, 2, 2), (1, 130, 90), (3, 130, 130), (1, 300, 257), (100, 8, 8), (100, 1000, 1000), (1, 10000, 10000)):
        assert lib.ddk_poly_mmd_workspace_bytes(s, ma, mb) == 8 * s * tiles(ma, mb), (s, ma, mb)
    assert lib.ddk_poly_mmd_workspace_bytes(1, 10000, 10000) == 8 * (2 * 79 * 80 // 2 + 79 * 79)
    for s, ma, mb in ((0, 8, 8), (1, 1, 8), (1, 8, 1), (2, (1 << 23) + 1, 8), (1 << 23, 2, 3)):
        assert lib.ddk_poly_mmd_workspace_bytes(s, ma, mb) == 0, (s, ma, mb)
    assert lib.ddk_manifold_ball_counts_workspace_bytes(150, 90) == 4 * 240 and lib.ddk_manifold_ball_counts_workspace_bytes(0, 5) == 0
