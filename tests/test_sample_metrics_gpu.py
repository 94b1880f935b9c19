"""ddk_knn_radii and ddk_manifold_members (csrc/manifold.hip) against tests/sample_metrics_ref.py, and
compute_prec_recall / evaluate_ddpm.py on top of them.

Bars.  Integer features (sample_metrics_ref.int_features): every fp32 distance is exact, so radii and flags equal the float64
restatement bit for bit, boundary ties included.  Real-valued features: radii within MARGIN 2 max|x|^2 of float64, flags equal for
every row and column that has no pair within MARGIN (|u|^2 + |v|^2) of its boundary (MARGIN = 8 x the fp32 numpy form's own
deviation = 4.2e-6, sample_metrics_ref.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_metrics_ref as R
from helpers import ddpm_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from ddk import ops
    return ops


def _dev(x):
    return None if x is None else torch.tensor(np.asarray(x), device=DEV)


def _radii(x, k=3):
    return _ops().manifold_radii(_dev(x), k).cpu().numpy()


def _members(a, ra, b, rb):
    a_in, b_in = _ops().manifold_members(_dev(a), _dev(ra), _dev(b), _dev(rb))
    return (None if a_in is None else a_in.cpu().numpy()), (None if b_in is None else b_in.cpu().numpy())


def _check_exact(a, b, k=3):
    """radii of both sets and both flag vectors, with either set as `a`: equal to the restatement"""
    ra, rb = R.radii(a, k).astype(np.float32), R.radii(b, k).astype(np.float32)
    got_ra, got_rb = _radii(a, k), _radii(b, k)
    assert got_ra.dtype == np.float32 and np.array_equal(got_ra, ra), np.abs(got_ra - ra).max()
    assert np.array_equal(got_rb, rb), np.abs(got_rb - rb).max()
    for u, ru, v, rv in ((a, ra, b, rb), (b, rb, a, ra)):
        want_u, want_v = R.members(u, ru, v, rv)
        got_u, got_v = _members(u, ru, v, rv)
        assert got_u.dtype == np.bool_ and got_u.shape == (len(u),) and got_v.shape == (len(v),)
        assert np.array_equal(got_u, want_u), np.flatnonzero(got_u != want_u)
        assert np.array_equal(got_v, want_v), np.flatnonzero(got_v != want_v)
    return ra, rb


@pytest.mark.parametrize("case", range(len(R.INT_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.INT_CASES])
def test_integer_fixtures_bit_equal(case):
    ref, smp = R.int_case(case)
    _check_exact(ref, smp)


@pytest.mark.parametrize("case", range(len(R.INT_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.INT_CASES])
def test_compute_prec_recall_equals_numpy_path(case):
    from utils.sample_metrics import compute_prec_recall
    ref, smp = R.int_case(case)
    got, host = compute_prec_recall(ref, smp, use_gpu=True), compute_prec_recall(ref, smp, use_gpu=False)
    print(f"{R.INT_CASES[case]}: kernels {got}, numpy {host}")
    assert got == host == R.prec_recall(ref, smp)
    assert compute_prec_recall(ref, smp) == got                     # a device is present: the default is the kernels


@pytest.mark.parametrize("case", range(len(R.REAL_CASES)), ids=[f"{a}x{b}x{d}" for a, b, d, _ in R.REAL_CASES])
def test_real_fixture_within_margin(case):
    ref, smp = R.real_case(case)
    for x in (ref, smp):
        want, got = R.radii(x), _radii(x).astype(np.float64)
        bar = R.MARGIN * 2.0 * R.norms(x).max()
        err = float(np.abs(got - want).max())
        print(f"{R.REAL_CASES[case]}: |radii - f64| {err:.3e} (bar {bar:.3e}), relative to 2 max|x|^2 {err / (2.0 * R.norms(x).max()):.3e}")
        assert err <= bar
    rr, rs = R.radii(ref).astype(np.float32), R.radii(smp).astype(np.float32)
    want_r, want_s = R.members(ref, rr, smp, rs)
    amb_r, amb_s = R.ambiguous(ref, rr, smp, rs)
    got_r, got_s = _members(ref, rr, smp, rs)
    print(f"{R.REAL_CASES[case]}: ambiguous {amb_r.mean():.4f} / {amb_s.mean():.4f}, differing flags {(got_r != want_r).sum()} / "
          f"{(got_s != want_s).sum()}, outside the ambiguous rows {((got_r != want_r) & ~amb_r).sum()} / {((got_s != want_s) & ~amb_s).sum()}")
    assert amb_r.mean() <= R.AMBIGUOUS_CAP and amb_s.mean() <= R.AMBIGUOUS_CAP
    assert np.array_equal(got_r[~amb_r], want_r[~amb_r]) and np.array_equal(got_s[~amb_s], want_s[~amb_s])
    # the same bits from run to run
    again_r, again_s = _members(ref, rr, smp, rs)
    assert np.array_equal(again_r, got_r) and np.array_equal(again_s, got_s)
    assert np.array_equal(_radii(ref).view(np.uint32), _radii(ref).view(np.uint32))


TILE = 128
# (Na, Nb, D): where a tile kernel breaks
SHAPES = {
    "n_k_plus_1": (4, 5, 8),                        # N = k + 1 and N = 5: far less than one tile
    "ragged_137_257": (137, 257, 64),               # a ragged last tile on both sides, 2 and 3 tiles
    "one_k_step": (50, 33, 4),                      # D = 4: one 8-feature group, half of it padding
    "pad_d20": (70, 41, 20),                        # D % 4 == 0 but not a whole LDS stage
    "pad_d2023": (40, 24, 2023),                    # through the wrapper's zero padding, the `spatial` width
    "full_tile": (TILE, 2 * TILE, 64),              # no ragged edge at all
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    na, nb, d = SHAPES[name]
    _check_exact(R.int_features(11, na, d, 0), R.int_features(12, nb, d, 1))


def test_column_split_and_walk():
    """The radii launch splits a row block's columns over workgroups as soon as there is more than one column tile (N > 128) and a
    launch would otherwise be small; above 8 column tiles a workgroup also walks several tiles with its running lists."""
    ops = _ops()
    n_one, n_split, n_walk = ops.MANIFOLD_TILE, 2 * ops.MANIFOLD_TILE + 1, 8 * ops.MANIFOLD_TILE + 76
    assert ops.manifold_radii_splits(n_one) == 1
    assert ops.manifold_radii_splits(n_split) == 3                                      # one tile per workgroup
    tiles = -(-n_walk // ops.MANIFOLD_TILE)
    assert 1 < ops.manifold_radii_splits(n_walk) < tiles                                # 9 tiles over 5 workgroups: 2, 2, 2, 2, 1
    x = R.int_features(21, n_walk, 64, 0)
    y = R.int_features(22, n_split, 64, 1)
    _check_exact(x, y)


def test_identity_rows_against_asymmetric_b():
    """a = unit vectors: d(a_i, b_j) = 1 - 2 b_j[i] + |b_j|^2 reads single elements of b, so a swapped row / column in the epilogue
    (which a symmetric b would hide) puts the flags in the wrong place"""
    a = np.eye(64, dtype=np.float32)
    b = R.int_features(31, 37, 64, 0)
    _check_exact(a, b, k=1)


@pytest.mark.parametrize("k", [1, 7])
def test_k_limits(k):
    _check_exact(R.int_features(41, 150, 32, 0), R.int_features(42, 90, 32, 1), k=k)


def test_null_radii_skip_an_output():
    ref, smp = R.int_case(2)
    rr, rs = R.radii(ref).astype(np.float32), R.radii(smp).astype(np.float32)
    want_r, want_s = R.members(ref, rr, smp, rs)
    a_in, b_in = _members(ref, None, smp, rs)
    assert b_in is None and np.array_equal(a_in, want_r)
    a_in, b_in = _members(ref, rr, smp, None)
    assert a_in is None and np.array_equal(b_in, want_s)


def test_identical_rows_and_zero_features():
    same = np.tile(R.int_features(51, 1, 24, 0), (6, 1))
    assert np.array_equal(_radii(same), np.zeros(6, dtype=np.float32))                  # radius exactly 0 ...
    a_in, b_in = _members(same, np.zeros(6, np.float32), same, np.zeros(6, np.float32))
    assert a_in.all() and b_in.all()                                                    # ... and membership by 0 <= 0
    zero = np.zeros((10, 8), dtype=np.float32)
    assert np.array_equal(_radii(zero), np.zeros(10, dtype=np.float32))
    a_in, b_in = _members(zero, np.zeros(10, np.float32), same[:, :8] * 0, np.zeros(6, np.float32))
    assert a_in.all() and b_in.all()
    far = same + 1.0                                                                    # every pair at distance 24 > 0: nobody is a member
    a_in, b_in = _members(same, np.zeros(6, np.float32), far, np.zeros(6, np.float32))
    assert not a_in.any() and not b_in.any()


def test_argument_errors_raise_before_device_work():
    from ddk import lib as L
    ops = _ops()
    x = torch.from_numpy(R.int_features(61, 20, 8, 0))
    r = torch.zeros(20)
    with pytest.raises(L.DDKError):
        ops.manifold_radii(x)                                                           # CPU tensor
    with pytest.raises(L.DDKError):
        ops.manifold_members(x, r, x, r)
    xd, rd = x.to(DEV), r.to(DEV)
    with pytest.raises(L.DDKError):
        ops.manifold_members(xd, r, xd, rd)                                             # CPU radii
    for bad in (xd.double(), xd.half(), xd[0], xd[:0], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            ops.manifold_radii(bad)
    for k in (0, 8, 2.0):
        with pytest.raises(ValueError):
            ops.manifold_radii(xd, k)
    with pytest.raises(ValueError):
        ops.manifold_radii(xd[:3], 3)                                                   # N < k + 1
    nan = xd.clone()
    nan[3, 2] = float("nan")
    with pytest.raises(ValueError):
        ops.manifold_radii(nan)
    with pytest.raises(ValueError):
        ops.manifold_members(xd, rd, nan, rd)
    with pytest.raises(ValueError):
        ops.manifold_members(xd, rd, xd[:, :4], rd)                                     # widths differ
    with pytest.raises(ValueError):
        ops.manifold_members(xd, rd[:19], xd, rd)                                       # one radius per row
    with pytest.raises(ValueError):
        ops.manifold_members(xd, rd.double(), xd, rd)
    with pytest.raises(ValueError):
        ops.manifold_members(xd, None, xd, None)


def test_c_entry_rejects_bad_arguments():
    """DDK_REQUIRE in front of any device work: the entry returns an error code and names the argument"""
    from ddk import lib as L
    lib = L.load()
    x = torch.zeros((8, 8), device=DEV)
    out = torch.zeros(8, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    args = lambda n, d, k, nbytes: (L.ptr(x), n, d, k, L.ptr(out), L.ptr(ws), nbytes, L.stream())
    assert lib.ddk_knn_radii(*args(8, 8, 3, 4096 * 4)) == 0
    for n, d, k, nbytes in ((8, 6, 3, 16384), (8, 8, 0, 16384), (8, 8, 8, 16384), (3, 8, 3, 16384), (8, 8, 3, 16)):
        assert lib.ddk_knn_radii(*args(n, d, k, nbytes)) != 0
        assert "knn_radii" in L.last_error()


def test_evaluate_ddpm_cli_with_activations(tmp_path):
    """evaluate_ddpm.py --sample_acts / --ref_acts on a tiny synthetic DDPM: the five keys come from sample_metrics"""
    from utils.sample_metrics import sample_metrics
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
                        str(out), "--sample_acts", str(files["sample"]), "--ref_acts", str(files["ref"])],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    metrics = json.loads(out.read_text())
    want = sample_metrics(str(files["ref"]), str(files["sample"]))
    assert list(metrics) == ["vlb", "L_simple", "is", "fid", "sfid", "precision", "recall"]
    for key in ("is", "fid", "sfid", "precision", "recall"):
        assert metrics[key] is not None and metrics[key] == want[key], key
    assert "out of scope" not in r.stdout
