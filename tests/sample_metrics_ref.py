"""The sample metrics restated in float64 numpy for the tests of csrc/manifold.hip and utils/sample_metrics.py.

Written from the formulas, not from the code under test: squared distance d(u, v) = max(|u|^2 - 2 u.v + |v|^2, 0); the radius of a
row is element k of its sorted distances to every row of its own set, itself included; a row of `a` is a member when some row j of
`b` has d <= rb[j], and the other way round; precision is the fraction of samples inside some reference sphere, recall the fraction
of reference rows inside some sample sphere.  ``frechet`` goes through scipy's sqrtm of the unsymmetric product, as the reference
does; the code under test never does.

Fixtures.  ``int_features``: integers in -3..3 (+ s for about half the rows), so every norm and dot product is an integer far below
2^24 and every fp32 distance is exact in any summation order: the kernels must equal numpy bit for bit there, boundary ties (d == r)
included.  ``real_features``: ReLU-like non-negative float32 rows, where fp32 rounding shows and the comparison needs a margin.
"""
import functools

import numpy as np

# (ref rows, sample rows, D, shift of the sample set): ref seed 1 / shift 0, sample seed 2.  What the float64 restatement gives:
#   200 x 137 x 64, shift 1: precision 0.635, recall 0.855, 13 pairs exactly on a reference row's radius and 18 on a sample's
#   300 x 257 x 96, shift 2: precision 0.424, recall 0.890, 16 and 27
#   130 x  70 x 20, shift 1: precision 0.814, recall 0.923, 12 and 27
# so neither result is trivial, and a `<` written for `<=` fails.
INT_CASES = ((200, 137, 64, 1), (300, 257, 96, 2), (130, 70, 20, 1))
INT_EXPECT = ((0.635, 0.855, 13, 18), (0.424, 0.890, 16, 27), (0.814, 0.923, 12, 27))
REF_SEED, SAMPLE_SEED = 1, 2

# (ref rows, sample rows, D, shift of the sample set)
REAL_CASES = ((384, 300, 2048, 0.05), (257, 190, 520, 0.1))

# max |d_fp32 - d_float64| / (|u|^2 + |v|^2) over all pairs of REAL_CASES (ref x sample, ref x ref, sample x sample), d_fp32 being the
# same GEMM form in numpy float32 on the CPU (dist_fp32; test_sample_metrics_cpu.py re-measures it).  The kernel is held to 8 x the
# larger: its MFMA sums the same products in an equally long fmaf chain of another order, which the hardware guide bounds at
# 3.5e-7 sum|a b| <= 1.75e-7 (|u|^2 + |v|^2) for K <= 4096.
# (Measured 3.79e-7 and 5.14e-7; the ref x sample pairs alone give 2.98e-7 and 3.02e-7, the rest comes from the near-zero
# distances of a set to itself.)
DIST_FP32_DEV = (3.9e-7, 5.3e-7)
MARGIN = 8 * max(DIST_FP32_DEV)
AMBIGUOUS_CAP = 0.02          # at most this fraction of a set's rows may have a pair too close to a boundary to be compared


def int_features(seed, n, d, s=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, (n, d)) + s * (rng.random((n, 1)) < 0.5)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def int_case(i):
    """(ref, sample) float32 of INT_CASES[i]; cached, treat as read-only"""
    nr, ns, d, s = INT_CASES[i]
    ref, smp = int_features(REF_SEED, nr, d, 0), int_features(SAMPLE_SEED, ns, d, s)
    ref.setflags(write=False)
    smp.setflags(write=False)
    return ref, smp


def real_features(seed, n, d, shift=0.0):
    """max(0.5 N(0, 1) + 0.3 + shift g, 0) as float32, g a fixed N(0, 1) direction per feature width"""
    g = np.random.default_rng(1000 + d).standard_normal(d)
    x = 0.5 * np.random.default_rng(seed).standard_normal((n, d)) + 0.3 + shift * g[None, :]
    return np.maximum(x, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def real_case(i):
    nr, ns, d, shift = REAL_CASES[i]
    ref, smp = real_features(REF_SEED, nr, d, 0.0), real_features(SAMPLE_SEED, ns, d, shift)
    ref.setflags(write=False)
    smp.setflags(write=False)
    return ref, smp


def norms(x):
    x = np.asarray(x, dtype=np.float64)
    return (x * x).sum(axis=1)


def dist(u, v):
    """float64 [len(u), len(v)]"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return np.maximum(norms(u)[:, None] - 2.0 * (u @ v.T) + norms(v)[None, :], 0.0)


def dist_fp32(u, v):
    """the same form with every operation in numpy float32"""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    nu, nv = (u * u).sum(axis=1, dtype=np.float32), (v * v).sum(axis=1, dtype=np.float32)
    return np.maximum(nu[:, None] - np.float32(2.0) * (u @ v.T) + nv[None, :], np.float32(0.0))


def scale(u, v):
    """|u|^2 + |v|^2 per pair: what the margin is relative to"""
    return norms(u)[:, None] + norms(v)[None, :]


def radii(x, k=3):
    return np.sort(dist(x, x), axis=1)[:, k]


def members(a, ra, b, rb):
    """(a_in, b_in) bool; a None radius vector gives a None output"""
    d = dist(a, b)
    a_in = None if rb is None else (d <= np.asarray(rb, dtype=np.float64)[None, :]).any(axis=1)
    b_in = None if ra is None else (d <= np.asarray(ra, dtype=np.float64)[:, None]).any(axis=0)
    return a_in, b_in


def ambiguous(a, ra, b, rb, margin=MARGIN):
    """(rows of a, rows of b) bool: those with a pair whose float64 distance lies within margin (|u|^2 + |v|^2) of the radius it is
    compared with, so that a correct fp32 evaluation may decide either way"""
    d, tol = dist(a, b), margin * scale(a, b)
    amb_a = (np.abs(d - np.asarray(rb, dtype=np.float64)[None, :]) <= tol).any(axis=1)
    amb_b = (np.abs(d - np.asarray(ra, dtype=np.float64)[:, None]) <= tol).any(axis=0)
    return amb_a, amb_b


def boundary_pairs(ref, smp, k=3):
    """number of (ref, sample) pairs whose distance equals the reference row's radius, and the sample's"""
    d = dist(ref, smp)
    return int((d == radii(ref, k)[:, None]).sum()), int((d == radii(smp, k)[None, :]).sum())


def fp32_deviation(ref, smp):
    """what DIST_FP32_DEV records, for one case"""
    return max(float((np.abs(dist_fp32(u, v).astype(np.float64) - dist(u, v)) / scale(u, v)).max())
               for u, v in ((ref, smp), (ref, ref), (smp, smp)))


def prec_recall(ref, smp, k=3):
    ref_in, smp_in = members(ref, radii(ref, k), smp, radii(smp, k))
    return float(smp_in.mean()), float(ref_in.mean())


def frechet(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2), the real part; also returns the largest imaginary part sqrtm left"""
    from scipy import linalg
    covmean = linalg.sqrtm(np.asarray(sigma1, dtype=np.float64) @ np.asarray(sigma2, dtype=np.float64))
    imag = float(np.abs(np.imag(covmean)).max()) if np.iscomplexobj(covmean) else 0.0
    diff = np.asarray(mu1, dtype=np.float64) - np.asarray(mu2, dtype=np.float64)
    return float(diff @ diff + np.trace(sigma1) + np.trace(sigma2) - 2.0 * np.trace(np.real(covmean))), imag


def inception_score(preds, split_size=5000):
    preds = np.asarray(preds, dtype=np.float64)
    scores = []
    for i in range(0, len(preds), split_size):
        p = preds[i:i + split_size]
        marginal = p.mean(axis=0, keepdims=True)
        terms = np.zeros_like(p)
        np.divide(p, marginal, out=terms, where=p > 0)
        np.log(terms, out=terms, where=p > 0)
        scores.append(np.exp((p * terms).sum(axis=1).mean()))
    return float(np.mean(scores))


def correlated_relu(seed, n, d, rank=None):
    """ReLU features with correlated columns; rank < d makes the covariance rank-deficient beyond n < d"""
    rng = np.random.default_rng(seed)
    r = d if rank is None else rank
    mix = rng.standard_normal((r, d)) / np.sqrt(r)
    return np.maximum(rng.standard_normal((n, r)) @ mix + 0.2, 0.0)
