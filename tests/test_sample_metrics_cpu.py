"""utils/sample_metrics.py on the host: Frechet distance against scipy's sqrtm and a closed form, Inception score, the activation
file reader, the numpy path of precision / recall against tests/sample_metrics_ref.py, the fixtures' own figures (the bars of
test_sample_metrics_gpu.py rest on them), and the CLIs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sample_metrics_ref as R
import utils.sample_metrics as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "downsampled-diffusion_amd")
ENV = dict(os.environ, PYTHONPATH=PKG)


# ---------------------------------------------------------------- Frechet distance
@pytest.mark.parametrize("n,d,rtol", [(500, 64, 1e-10), (2000, 256, 1e-10)])
def test_frechet_matches_sqrtm(n, d, rtol):
    pytest.importorskip("scipy")
    s1 = SM.compute_statistics(R.correlated_relu(1, n, d))
    s2 = SM.compute_statistics(R.correlated_relu(2, n, d) * 1.1 + 0.05)
    want, imag = R.frechet(s1.mu, s1.sigma, s2.mu, s2.sigma)
    got = s1.frechet_distance(s2)
    print(f"{n} x {d}: frechet {got:.12g}, sqrtm form {want:.12g}, relative difference {abs(got - want) / want:.2e}, sqrtm imaginary part {imag:.1e}")
    assert want > 0 and abs(got - want) <= rtol * want
    assert abs(s2.frechet_distance(s1) - got) <= rtol * want                             # symmetric in its arguments


def test_frechet_rank_deficient_stays_finite():
    pytest.importorskip("scipy")
    s1 = SM.compute_statistics(R.correlated_relu(3, 40, 64))                             # 40 rows of 64 features: rank <= 39
    s2 = SM.compute_statistics(R.correlated_relu(4, 40, 64) + 0.1)
    assert np.linalg.matrix_rank(s1.sigma) < 64
    want, imag = R.frechet(s1.mu, s1.sigma, s2.mu, s2.sigma)
    got = s1.frechet_distance(s2)
    print(f"rank-deficient 40 x 64: frechet {got:.12g}, sqrtm form {want:.12g}, relative difference {abs(got - want) / want:.2e}, "
          f"sqrtm imaginary part {imag:.1e}")
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * want


def test_frechet_closed_form_for_diagonal_gaussians():
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0.1, 2.0, 48), rng.uniform(0.1, 2.0, 48)
    m1, m2 = rng.standard_normal(48), rng.standard_normal(48)
    got = SM.FIDStatistics(m1, np.diag(a)).frechet_distance(SM.FIDStatistics(m2, np.diag(b)))
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(got - want) <= 1e-12 * want


def test_frechet_of_a_set_with_itself_is_zero():
    s = SM.compute_statistics(R.correlated_relu(6, 300, 96))
    assert abs(s.frechet_distance(s)) <= 1e-9 * np.trace(s.sigma)


def test_compute_statistics_is_numpy_mean_and_cov():
    x = R.correlated_relu(7, 50, 12).astype(np.float32)
    s = SM.compute_statistics(x)
    assert np.array_equal(s.mu, np.mean(x, axis=0).astype(np.float64)) and np.array_equal(s.sigma, np.cov(x, rowvar=False))
    with pytest.raises(ValueError):
        SM.compute_statistics(x[:1])
    with pytest.raises(ValueError):
        SM.FIDStatistics(np.zeros(3), np.zeros((4, 4)))
    with pytest.raises(ValueError):
        SM.FIDStatistics(np.zeros(3), np.eye(3)).frechet_distance(SM.FIDStatistics(np.zeros(4), np.eye(4)))


# ---------------------------------------------------------------- Inception score
def test_inception_score_closed_forms():
    split, c = 10, 5
    n = 2 * split + 3                                                                    # two whole splits and a ragged third
    uniform = np.full((n, c), 1.0 / c)
    assert abs(SM.compute_inception_score(uniform, split_size=split) - 1.0) <= 1e-12
    onehot = np.eye(c)[np.arange(3 * split) % c]                                         # every split holds each class equally often
    assert abs(SM.compute_inception_score(onehot, split_size=split) - c) <= 1e-12
    ragged = np.eye(c)[np.arange(n) % c]                                                 # the last split has 3 of the 5 classes: score 3
    assert abs(SM.compute_inception_score(ragged, split_size=split) - (c + c + 3) / 3.0) <= 1e-12
    rng = np.random.default_rng(8)
    p = rng.random((n, c)) + 0.01
    p /= p.sum(axis=1, keepdims=True)
    assert abs(SM.compute_inception_score(p, split_size=split) - R.inception_score(p, split)) <= 1e-12
    assert SM.compute_inception_score(p) == SM.compute_inception_score(p, split_size=5000)


# ---------------------------------------------------------------- the fixtures, and the numpy path on them
@pytest.mark.parametrize("case", range(len(R.INT_CASES)))
def test_integer_fixtures_and_numpy_path(case):
    ref, smp = R.int_case(case)
    p, r = R.prec_recall(ref, smp)
    on_ref, on_smp = R.boundary_pairs(ref, smp)
    print(f"{R.INT_CASES[case]}: precision {p:.3f} recall {r:.3f}, pairs exactly on a boundary {on_ref} + {on_smp}")
    assert (round(p, 3), round(r, 3), on_ref, on_smp) == R.INT_EXPECT[case]
    # every fp32 distance is exact: the float32 form equals float64
    assert np.array_equal(R.dist_fp32(ref, smp).astype(np.float64), R.dist(ref, smp))
    assert float(np.abs(R.dist(ref, ref)).max()) < 2 ** 24
    assert np.array_equal(SM.radii_numpy(ref), R.radii(ref).astype(np.float32))
    rr, rs = SM.radii_numpy(ref), SM.radii_numpy(smp)
    got, want = SM.members_numpy(ref, rr, smp, rs), R.members(ref, rr, smp, rs)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert SM.compute_prec_recall(ref, smp, use_gpu=False) == (p, r)
    assert SM.compute_prec_recall(smp, ref, use_gpu=False) == R.prec_recall(smp, ref) != (p, r)      # the orientation matters
    # a `<` written for `<=` would lose the boundary pairs
    d = R.dist(ref, smp)
    strict = ((d < rr[:, None].astype(np.float64)).any(axis=0).mean(), (d < rs[None, :].astype(np.float64)).any(axis=1).mean())
    assert strict != (p, r)
    # row blocks smaller than the set: the same result
    assert np.array_equal(SM.radii_numpy(ref, row_block=37), rr)
    got = SM.members_numpy(ref, rr, smp, rs, row_block=37)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_real_fixture_margin_and_ambiguity_cap():
    """the figures test_sample_metrics_gpu.py rests on: what fp32 costs the GEMM form of the distance, and how many rows lie too
    close to a boundary to be compared"""
    for case, recorded in enumerate(R.DIST_FP32_DEV):
        ref, smp = R.real_case(case)
        dev = R.fp32_deviation(ref, smp)
        rr, rs = R.radii(ref).astype(np.float32), R.radii(smp).astype(np.float32)
        amb_r, amb_s = R.ambiguous(ref, rr, smp, rs)
        p, r = R.prec_recall(ref, smp)
        print(f"{R.REAL_CASES[case]}: fp32 form off by {dev:.3e} of |u|^2 + |v|^2 (recorded {recorded:.1e}), ambiguous rows "
              f"{amb_r.mean():.4f} / {amb_s.mean():.4f}, precision {p:.3f} recall {r:.3f}")
        assert 0.5 * recorded < dev <= recorded
        assert amb_r.mean() <= R.AMBIGUOUS_CAP and amb_s.mean() <= R.AMBIGUOUS_CAP
        assert 0.05 < p < 0.95 and 0.05 < r < 0.95                                       # neither trivial
        assert (ref >= 0).all() and (smp >= 0).all() and ref.dtype == np.float32
    assert R.MARGIN == 8 * max(R.DIST_FP32_DEV)


def test_compute_prec_recall_rejects_bad_input():
    ref, smp = R.int_case(2)
    for bad in (ref.astype(np.float64), ref[0], ref[:3]):
        with pytest.raises(ValueError):
            SM.compute_prec_recall(bad, smp, use_gpu=False)
    with pytest.raises(ValueError):
        SM.compute_prec_recall(ref, smp[:, :8], use_gpu=False)
    nan = smp.copy()
    nan[1, 1] = np.inf
    with pytest.raises(ValueError):
        SM.compute_prec_recall(ref, nan, use_gpu=False)


# ---------------------------------------------------------------- activation files
def _acts(seed, n, shift=0.0):
    rng = np.random.default_rng(seed)
    pool = np.maximum(0.5 * rng.standard_normal((n, SM.POOL_DIM)) + 0.3 + shift, 0).astype(np.float32)
    spatial = np.maximum(0.5 * rng.standard_normal((n, SM.SPATIAL_DIM)) + 0.3 + shift, 0).astype(np.float32)
    soft = rng.random((n, 10))
    return pool, spatial, soft / soft.sum(axis=1, keepdims=True)


@pytest.fixture(scope="module")
def act_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("acts")
    pool_r, spatial_r, _ = _acts(1, 20)
    pool_s, spatial_s, soft_s = _acts(2, 16, 0.05)
    np.savez(d / "ref_full.npz", pool_3=pool_r, spatial=spatial_r)
    np.savez(d / "sample_full.npz", pool_3=pool_s, spatial=spatial_s, softmax=soft_s)
    np.savez(d / "sample_pool.npz", pool_3=pool_s)
    sr, ss = SM.compute_statistics(pool_r), SM.compute_statistics(spatial_r)
    np.savez(d / "ref_stats.npz", mu=sr.mu, sigma=sr.sigma, mu_s=ss.mu, sigma_s=ss.sigma)
    np.savez(d / "ref_stats_pool.npz", mu=sr.mu, sigma=sr.sigma)
    np.savez(d / "no_pool.npz", spatial=spatial_r, mu=sr.mu)
    np.savez(d / "bad_width.npz", pool_3=pool_r[:, :100])
    full = SM.sample_metrics(d / "ref_full.npz", d / "sample_full.npz")                   # once: two 2048-wide Frechet distances
    return d, dict(pool_r=pool_r, spatial_r=spatial_r, pool_s=pool_s, spatial_s=spatial_s, soft_s=soft_s, full=full)


def test_load_activations_key_combinations(act_files):
    d, arr = act_files
    full = SM.load_activations(d / "sample_full.npz")
    assert np.array_equal(full.pool, arr["pool_s"]) and np.array_equal(full.spatial, arr["spatial_s"]) and np.array_equal(full.softmax, arr["soft_s"])
    assert np.array_equal(full.stats.sigma, np.cov(arr["pool_s"], rowvar=False)) and full.stats_spatial.mu.shape == (SM.SPATIAL_DIM,)
    pool = SM.load_activations(d / "sample_pool.npz")
    assert pool.spatial is None and pool.stats_spatial is None and pool.softmax is None and pool.pool is not None
    stats = SM.load_activations(d / "ref_stats.npz")
    assert stats.pool is None and stats.spatial is None and stats.stats.mu.shape == (SM.POOL_DIM,) and stats.stats_spatial is not None
    assert SM.load_activations(d / "ref_stats_pool.npz").stats_spatial is None
    for bad in ("no_pool.npz", "bad_width.npz"):
        with pytest.raises(ValueError):
            SM.load_activations(d / bad)


def test_sample_metrics_never_guesses(act_files):
    d, arr = act_files
    full = arr["full"]
    assert list(full) == ["is", "fid", "sfid", "precision", "recall"] and all(v is not None for v in full.values())
    sr, ss = SM.compute_statistics(arr["pool_r"]), SM.compute_statistics(arr["pool_s"])
    assert full["fid"] == ss.frechet_distance(sr)
    assert full["is"] == SM.compute_inception_score(arr["soft_s"])
    assert (full["precision"], full["recall"]) == SM.compute_prec_recall(arr["pool_r"], arr["pool_s"])
    # statistics-only reference: FID and sFID as before, no precision / recall
    stats = SM.sample_metrics(d / "ref_stats.npz", d / "sample_full.npz")
    assert stats["fid"] == full["fid"] and stats["sfid"] == full["sfid"] and stats["precision"] is None and stats["recall"] is None
    # no spatial features, no softmax on the sample side
    pool = SM.sample_metrics(d / "ref_full.npz", d / "sample_pool.npz")
    assert pool["is"] is None and pool["sfid"] is None and pool["fid"] == full["fid"] and pool["precision"] == full["precision"]


# ---------------------------------------------------------------- the tools
def test_compare_datasets_cli(act_files, tmp_path):
    d, arr = act_files
    out = tmp_path / "cmp.json"
    r = subprocess.run([sys.executable, os.path.join(PKG, "compare_datasets.py"), "--ds_1", str(d / "ref_full.npz"), "--ds_2",
                        str(d / "sample_full.npz"), "--json", str(out)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    want = arr["full"]
    got = json.loads(out.read_text())
    assert list(got) == ["fid", "sfid", "precision", "recall"] and got == {k: want[k] for k in got}
    assert "Results:" in r.stdout and "Dataset 1:" in r.stdout and f"({d / 'ref_full.npz'} vs. {d / 'sample_full.npz'})" in r.stdout
    assert json.loads(r.stdout[r.stdout.index("{"):]) == got                             # the reference's printed block
    # a statistics-only reference batch: precision / recall are null, nothing is guessed
    r = subprocess.run([sys.executable, os.path.join(PKG, "compare_datasets.py"), "--ds_1", str(d / "ref_stats.npz"), "--ds_2",
                        str(d / "sample_full.npz")], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout[r.stdout.index("{"):])
    assert got["fid"] == want["fid"] and got["sfid"] == want["sfid"] and got["precision"] is None and got["recall"] is None


def test_evaluate_ddpm_activation_flags_parse():
    """the likelihood half of evaluate_ddpm.py needs the device, so its run with the flags is in test_sample_metrics_gpu.py; here: the
    flags exist, go together, and without them the explanatory line is the one the tool has always printed"""
    script = os.path.join(PKG, "evaluate_ddpm.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0 and "--sample_acts" in r.stdout and "--ref_acts" in r.stdout
    r = subprocess.run([sys.executable, script, "--sample_acts", "x.npz"], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 2 and "go together" in r.stderr
    src = open(script).read()
    assert "print('Sample metrics (IS, FID, sFID, precision, recall): the TF-Inception evaluator is out of scope; reported as null.')" in src
