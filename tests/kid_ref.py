"""KID and density / coverage restated in float64 numpy for the tests of ddk_poly_mmd_sums / ddk_manifold_ball_counts
(csrc/manifold.hip) and of utils/sample_metrics.py.  Features, ``dist`` and ``radii`` come from
tests/sample_metrics_ref.py.

Written from the formulas, not from the code under test.  Kernel k(x, y) = (gamma x.y + coef0)^3; per segment g of ma rows of `a` and
mb rows of `b`: s0 = sum_{i != j} k(a_i, a_j), s1 = sum_{i != j} k(b_i, b_j), s2 = sum_{i, j} k(a_i, b_j); the unbiased
MMD^2 = s0 / (ma (ma - 1)) + s1 / (mb (mb - 1)) - 2 s2 / (ma mb).  KID: mean and population standard deviation of MMD^2 over subsets,
and the same estimator once over all rows.  Ball counts: counts[i] = #{ j : d(a_i, b_j) <= ra[i] }; density = sum counts / (k N_b),
coverage = mean(counts > 0).

Two forms of the sums:
  * ``sums_exact``: for fixtures on which every dot product and every t = gamma dot + coef0 is exact in float32 (integer rows, gamma a
    power of two).  k is then DEFINED by the kernel's arithmetic, float32 (t t) t with two roundings, and only the order of the double
    summation is left open: the kernels must agree to a relative 1e-13.
  * ``sums_f64`` with ``sums_bound``: float64 throughout, and per sum the rounding bound of an fp32 evaluation, derived below.

The bound, per pair.  With T = |gamma x.y + coef0| and s = gamma sum_i |x_i y_i|: an fp32 fmaf chain of D products is off by at most
D 2^-24 s / gamma in the dot product (one rounding per step, each of a partial sum bounded by sum |x_i y_i|, to first order), rounding
gamma to fp32 and the fmaf that forms t add 2 2^-24 s and 2 2^-24 T at the most, so |t - T| <= delta = (D + 2) 2^-24 s + 2 2^-24 T.
Then |t^3 - T^3| <= 3 (T + delta)^2 delta, and the two roundings of (t t) t add at most 3 2^-24 (T + delta)^3 (2 roundings, with
room for the second-order term).  e = 3 (T + delta)^2 delta + 3 2^-24 (T + delta)^3; a sum of k's is off by at most the sum of e
over its pairs (the double summation adds 1e-13 relative, far below).  The symmetric sums leave the diagonal out of sum e as well.
"""
import numpy as np

import sample_metrics_ref as R

EPS = 2.0 ** -24
EXACT_RTOL = 1e-13
AMBIGUOUS_PAIR_CAP = 0.01     # ball counts on real features: at most this share of a case's pairs may lie within the margin


def _segments(a, b, segments):
    a, b = np.asarray(a), np.asarray(b)
    assert len(a) % segments == 0 and len(b) % segments == 0
    ma, mb = len(a) // segments, len(b) // segments
    for g in range(segments):
        yield g, a[g * ma:(g + 1) * ma], b[g * mb:(g + 1) * mb]


def _sum_without_diagonal(m):
    m = np.array(m, dtype=np.float64)
    np.fill_diagonal(m, 0.0)
    return float(m.sum())


def kernel_exact(u, v, gamma, coef0):
    """float32 [len(u), len(v)]: (t t) t in float32 from the exact t; asserts that dot and t ARE exact in float32"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    dot = u @ v.T
    assert np.abs(dot).max() < 2.0 ** 24 and np.array_equal(dot, np.rint(dot)), "fixture: dot products must be integers below 2^24"
    t64 = gamma * dot + coef0
    t = t64.astype(np.float32)
    assert np.array_equal(t.astype(np.float64), t64), "fixture: t must be exact in float32"
    return (t * t) * t


def sums_exact(a, b, segments=1, gamma=1.0 / 64, coef0=1.0):
    out = np.empty((segments, 3), dtype=np.float64)
    for g, u, v in _segments(a, b, segments):
        out[g] = (_sum_without_diagonal(kernel_exact(u, u, gamma, coef0)), _sum_without_diagonal(kernel_exact(v, v, gamma, coef0)),
                  float(kernel_exact(u, v, gamma, coef0).astype(np.float64).sum()))
    return out


def _pair_terms(u, v, gamma, coef0, d):
    """(K, e) float64 [len(u), len(v)]: the kernel values and the per-pair rounding bound of the module docstring"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    t = gamma * (u @ v.T) + coef0
    s = gamma * (np.abs(u) @ np.abs(v).T)
    big = np.abs(t)
    delta = (d + 2) * EPS * s + 2 * EPS * big
    e = 3.0 * (big + delta) ** 2 * delta + 3.0 * EPS * (big + delta) ** 3
    return t ** 3, e


def sums_f64(a, b, segments=1, gamma=None, coef0=1.0):
    """(sums, bound), both float64 [S, 3]; gamma None = 1 / D"""
    d = np.asarray(a).shape[1]
    gamma = 1.0 / d if gamma is None else gamma
    sums, bound = np.empty((segments, 3)), np.empty((segments, 3))
    for g, u, v in _segments(a, b, segments):
        for m, (p, q, skip) in enumerate(((u, u, True), (v, v, True), (u, v, False))):
            k, e = _pair_terms(p, q, gamma, coef0, d)
            sums[g, m] = _sum_without_diagonal(k) if skip else float(k.sum())
            bound[g, m] = _sum_without_diagonal(e) if skip else float(e.sum())
    return sums, bound


def sums_with_diagonal(a, b, segments=1, gamma=None, coef0=1.0):
    """the mistake the bound must catch: the symmetric sums with i == j included"""
    d = np.asarray(a).shape[1]
    gamma = 1.0 / d if gamma is None else gamma
    out = np.empty((segments, 3))
    for g, u, v in _segments(a, b, segments):
        out[g] = [float(_pair_terms(p, q, gamma, coef0, d)[0].sum()) for p, q in ((u, u), (v, v), (u, v))]
    return out


def mmd2(sums, ma, mb):
    sums = np.asarray(sums, dtype=np.float64)
    return sums[:, 0] / (ma * (ma - 1.0)) + sums[:, 1] / (mb * (mb - 1.0)) - 2.0 * sums[:, 2] / (float(ma) * mb)


def mmd2_bound(bound, ma, mb):
    """the sums' bounds through the estimator: every term at its worst"""
    bound = np.asarray(bound, dtype=np.float64)
    return bound[:, 0] / (ma * (ma - 1.0)) + bound[:, 1] / (mb * (mb - 1.0)) + 2.0 * bound[:, 2] / (float(ma) * mb)


def subset_indices(n_ref, n_sample, subsets, m, seed):
    """the draw compute_kid documents: one PCG64 generator; per subset first the reference's rows, then the sample's"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref_idx, smp_idx = [], []
    for _ in range(subsets):
        ref_idx.append(rng.choice(n_ref, size=m, replace=False))
        smp_idx.append(rng.choice(n_sample, size=m, replace=False))
    return np.array(ref_idx), np.array(smp_idx)


def kid(ref, smp, subsets=100, subset_size=1000, seed=0):
    """(dict(kid_mean, kid_std, kid_full), dict of the same keys: the rounding bound of each).  mean: the mean of the subsets' bounds;
    std: the largest of them (the standard deviation moves by at most the root mean square of the changes of its arguments)."""
    ref, smp = np.asarray(ref), np.asarray(smp)
    m = min(subset_size, len(ref), len(smp))
    ri, si = subset_indices(len(ref), len(smp), subsets, m, seed)
    sums, bound = sums_f64(ref[ri.reshape(-1)], smp[si.reshape(-1)], subsets)
    per, per_bound = mmd2(sums, m, m), mmd2_bound(bound, m, m)
    full, full_bound = sums_f64(ref, smp, 1)
    value = dict(kid_mean=float(per.mean()), kid_std=float(per.std()), kid_full=float(mmd2(full, len(ref), len(smp))[0]))
    bar = dict(kid_mean=float(per_bound.mean()), kid_std=float(per_bound.max()), kid_full=float(mmd2_bound(full_bound, len(ref), len(smp))[0]))
    return value, bar


def ball_counts(a, ra, b):
    """int64 [len(a)] from float64 distances"""
    return (R.dist(a, b) <= np.asarray(ra, dtype=np.float64)[:, None]).sum(axis=1)


def ball_count_range(a, ra, b, margin=R.MARGIN):
    """(low, high, share): per row the counts with every pair within margin (|u|^2 + |v|^2) of the radius decided against / for
    membership, and those pairs' share of all pairs.  A correct fp32 evaluation lies in [low, high]."""
    d, tol, r = R.dist(a, b), margin * R.scale(a, b), np.asarray(ra, dtype=np.float64)[:, None]
    low, high = (d <= r - tol).sum(axis=1), (d <= r + tol).sum(axis=1)
    return low, high, float((high - low).sum()) / d.size


def density_coverage(ref, smp, k=5):
    counts = ball_counts(ref, R.radii(ref, k), smp)
    return float(counts.sum()) / (k * len(smp)), float((counts > 0).mean())
