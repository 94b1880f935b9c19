"""Sample metrics from Inception activations: FID, sFID, Inception score and improved precision / recall.

The second half of the reference's evaluator (utils/evaluator.py): everything after the Inception network.  The network itself is
NOT here: the activations come from any Inception port as an ``.npz`` file, or, for the reference side of
FID / sFID, from one of the published guided-diffusion reference batches, which carry ``mu`` / ``sigma`` / ``mu_s`` / ``sigma_s``.

Moments, Frechet distance and Inception score are float64 numpy, once per evaluation.  Precision / recall is three passes over
N x N x D distances: on a ROCm device they run on the HIP kernels of csrc/manifold.hip (ddk.ops.manifold_radii /
manifold_members); without one, a row-blocked numpy float32 path evaluates the same formula.  Both are
fp32; the reference's distances are fp16 whenever that stays finite, so its values can differ from these in the third decimal.

Beyond the reference's table, and only where asked for (extended_sample_metrics): KID (compute_kid) and
density / coverage (compute_density_coverage), on the same kernels' tiles (ddk.ops.poly_mmd_sums / manifold_ball_counts) or their
numpy float32 counterparts.  sample_metrics and SAMPLE_METRICS are the reference's five keys and stay that.
"""
import numpy as np

PREC_RECALL_K = 3             # reference ManifoldEstimator nhood_sizes=(3,)
POOL_DIM, SPATIAL_DIM = 2048, 2023
SAMPLE_METRICS = ('is', 'fid', 'sfid', 'precision', 'recall')


class FIDStatistics:
    def __init__(self, mu, sigma):
        self.mu = np.atleast_1d(np.asarray(mu, dtype=np.float64))
        self.sigma = np.atleast_2d(np.asarray(sigma, dtype=np.float64))
        if self.mu.ndim != 1 or self.sigma.shape != (self.mu.shape[0], self.mu.shape[0]):
            raise ValueError(f"FIDStatistics: mu {self.mu.shape} and sigma {self.sigma.shape} do not belong together")

    def frechet_distance(self, other):
        """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2)  (reference utils/evaluator.py:39-82).

        The reference takes scipy's sqrtm of the unsymmetric product S1 S2, discards the imaginary part rounding leaves, and,
        when the product is singular enough for sqrtm to return non-finite values, adds 1e-6 to both diagonals and tries again.
        Here the trace is taken from a symmetric problem instead: with R = S1^(1/2) from eigh (negative rounding eigenvalues
        set to 0), S1 S2 and R S2 R have the same eigenvalues, R S2 R is symmetric positive semi-definite, and
        tr (S1 S2)^(1/2) = sum sqrt(max(eigvalsh(R S2 R), 0)).  No scipy, no imaginary part to discard, and the value stays finite
        for rank-deficient covariances (fewer samples than features), so there is no 1e-6 fallback and nothing is added."""
        if self.mu.shape != other.mu.shape:
            raise ValueError(f"frechet_distance: mean vectors have different lengths: {self.mu.shape}, {other.mu.shape}")
        diff = self.mu - other.mu
        w, v = np.linalg.eigh(self.sigma)
        root = (v * np.sqrt(np.maximum(w, 0.0))) @ v.T
        m = root @ other.sigma @ root
        ev = np.linalg.eigvalsh(0.5 * (m + m.T))
        tr_covmean = np.sqrt(np.maximum(ev, 0.0)).sum()
        return float(diff.dot(diff) + np.trace(self.sigma) + np.trace(other.sigma) - 2.0 * tr_covmean)


def compute_statistics(acts):
    """Mean and covariance of activation rows [N, D] (reference utils/evaluator.py:128-131)."""
    acts = np.asarray(acts)
    if acts.ndim != 2 or acts.shape[0] < 2:
        raise ValueError(f"compute_statistics: need at least two rows of [N, D] activations, got {acts.shape}")
    return FIDStatistics(np.mean(acts, axis=0), np.cov(acts, rowvar=False))


def compute_inception_score(preds, split_size=5000):
    """The reference's Inception score on given softmax outputs [N, C]: the mean over splits of exp(mean_i KL(p_i || mean p))
    (utils/evaluator.py:139-146).  A zero probability contributes 0 (the limit of p log p)."""
    preds = np.asarray(preds, dtype=np.float64)
    if preds.ndim != 2 or preds.shape[0] < 1:
        raise ValueError(f"compute_inception_score: need [N, C] softmax outputs, got {preds.shape}")
    scores = []
    for i in range(0, len(preds), split_size):
        part = preds[i:i + split_size]
        with np.errstate(divide='ignore', invalid='ignore'):
            kl = part * (np.log(part) - np.log(np.mean(part, 0, keepdims=True)))
        kl = np.where(part > 0, kl, 0.0)
        scores.append(np.exp(np.mean(np.sum(kl, 1))))
    return float(np.mean(scores))


# ---------------------------------------------------------------- precision / recall
def _features(name, x, what="compute_prec_recall"):
    x = np.ascontiguousarray(x)
    if x.ndim != 2 or x.dtype != np.float32:
        raise ValueError(f"{what}: {name} must be a float32 [N, D] array, got {x.dtype} {x.shape}")
    if not np.isfinite(x).all():
        raise ValueError(f"{what}: {name} holds non-finite features")
    return x


def _dist_block(u, nu, v, nv):
    """float32 [len(u), len(v)]: max((|u|^2 - 2 u.v) + |v|^2, 0), the reference's _batch_pairwise_distances in fp32"""
    return np.maximum((nu[:, None] - np.float32(2.0) * (u @ v.T)) + nv[None, :], np.float32(0.0))


def _norms(x):
    return np.einsum('ij,ij->i', x, x)


def radii_numpy(x, k=PREC_RECALL_K, row_block=1024):
    x = _features("x", x)
    nx = _norms(x)
    out = np.empty(len(x), dtype=np.float32)
    for r0 in range(0, len(x), row_block):
        d = _dist_block(x[r0:r0 + row_block], nx[r0:r0 + row_block], x, nx)
        out[r0:r0 + row_block] = np.partition(d, k, axis=1)[:, k]
    return out


def members_numpy(a, ra, b, rb, row_block=1024):
    a, b = _features("a", a), _features("b", b)
    na, nb = _norms(a), _norms(b)
    a_in, b_in = np.zeros(len(a), dtype=bool), np.zeros(len(b), dtype=bool)
    for r0 in range(0, len(a), row_block):
        d = _dist_block(a[r0:r0 + row_block], na[r0:r0 + row_block], b, nb)
        a_in[r0:r0 + row_block] = (d <= rb[None, :]).any(axis=1)
        b_in |= (d <= ra[r0:r0 + row_block, None]).any(axis=0)
    return a_in, b_in


def gpu_available():
    import torch
    return torch.cuda.is_available()


def compute_prec_recall(acts_ref, acts_sample, k=PREC_RECALL_K, use_gpu=None):
    """(precision, recall) of Kynkaanniemi et al. 2019 with the reference's orientation (utils/evaluator.py:148-156, 278-312):
    precision = the fraction of samples inside the k-NN sphere of some reference row, recall = the fraction of reference rows inside
    the sphere of some sample.  use_gpu: None = the HIP kernels when a ROCm device is present, else the numpy float32 path."""
    ref, smp = _features("acts_ref", acts_ref), _features("acts_sample", acts_sample)
    if ref.shape[1] != smp.shape[1]:
        raise ValueError(f"compute_prec_recall: feature widths differ: {ref.shape[1]} and {smp.shape[1]}")
    if min(len(ref), len(smp)) < k + 1:
        raise ValueError(f"compute_prec_recall: both sets need at least k + 1 = {k + 1} rows, got {len(ref)} and {len(smp)}")
    if use_gpu is None:
        use_gpu = gpu_available()
    if use_gpu:
        import torch
        from ddk import ops
        a, b = (torch.from_numpy(x if x.flags.writeable else x.copy()).cuda() for x in (ref, smp))
        ref_in, smp_in = ops.manifold_members(a, ops.manifold_radii(a, k), b, ops.manifold_radii(b, k))
        return int(smp_in.sum().item()) / len(smp), int(ref_in.sum().item()) / len(ref)
    ref_in, smp_in = members_numpy(ref, radii_numpy(ref, k), smp, radii_numpy(smp, k))
    return int(smp_in.sum()) / len(smp), int(ref_in.sum()) / len(ref)


# ---------------------------------------------------------------- KID
KID_DEGREE, KID_COEF0 = 3, 1.0                   # k(x, y) = (x.y / D + 1)^3: torch-fidelity's and clean-fid's `kid`
KID_GATHER_ELEMS = 1 << 28                       # features of one side gathered on the device per call, at most (1 GiB of fp32)
EXTENDED_METRICS = ('kid_mean', 'kid_std', 'kid_full', 'density', 'coverage')


def poly_mmd_sums_numpy(a, b, segments=1, gamma=None, coef0=KID_COEF0, row_block=1024):
    """float64 [S, 3]: per segment sum_{i != j} k(a_i, a_j), sum_{i != j} k(b_i, b_j), sum_{i, j} k(a_i, b_j) with
    k = (gamma x.y + coef0)^3.  What ddk.ops.poly_mmd_sums computes, in numpy: float32 dots, t = gamma dot + coef0 and k = (t t) t in
    float32, the sums in float64; the diagonal is excluded by index.  a [S ma, D], b [S mb, D]; gamma None = 1 / D."""
    a, b = _features("a", a, "poly_mmd_sums"), _features("b", b, "poly_mmd_sums")
    if a.shape[1] != b.shape[1] or len(a) % segments or len(b) % segments or len(a) // segments < 2 or len(b) // segments < 2:
        raise ValueError(f"poly_mmd_sums: need {segments} segments of at least 2 rows and one width, got {a.shape} and {b.shape}")
    g, c = np.float32(1.0 / a.shape[1] if gamma is None else gamma), np.float32(coef0)
    ma, mb = len(a) // segments, len(b) // segments
    out = np.zeros((segments, 3), dtype=np.float64)

    def total(u, v, skip_diagonal):
        s = 0.0
        for r0 in range(0, len(u), row_block):
            t = g * (u[r0:r0 + row_block] @ v.T) + c
            k = (t * t) * t
            if skip_diagonal:
                i = np.arange(len(k))
                k[i, r0 + i] = 0.0
            s += float(k.sum(dtype=np.float64))
        return s

    for s in range(segments):
        u, v = a[s * ma:(s + 1) * ma], b[s * mb:(s + 1) * mb]
        out[s] = total(u, u, True), total(v, v, True), total(u, v, False)
    return out


def mmd2_from_sums(sums, ma, mb):
    """The unbiased MMD^2 estimate of each row of sums [S, 3]: s0 / (ma (ma - 1)) + s1 / (mb (mb - 1)) - 2 s2 / (ma mb)."""
    sums = np.asarray(sums, dtype=np.float64)
    return sums[:, 0] / (ma * (ma - 1.0)) + sums[:, 1] / (mb * (mb - 1.0)) - 2.0 * sums[:, 2] / (float(ma) * mb)


def kid_subset_indices(n_ref, n_sample, subsets, m, seed=0):
    """(ref_idx, sample_idx), int64 [subsets, m]: the rows of each KID subset.  One generator, numpy.random.Generator(PCG64(seed));
    for subset 0, 1, .. in turn it is asked first for ``choice(n_ref, size=m, replace=False)``, then for
    ``choice(n_sample, size=m, replace=False)`` (numpy's defaults otherwise: shuffle=True).  Nothing else draws from it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref_idx, smp_idx = np.empty((subsets, m), dtype=np.int64), np.empty((subsets, m), dtype=np.int64)
    for s in range(subsets):
        ref_idx[s] = rng.choice(n_ref, size=m, replace=False)
        smp_idx[s] = rng.choice(n_sample, size=m, replace=False)
    return ref_idx, smp_idx


def _two_sets(what, acts_ref, acts_sample):
    ref, smp = _features("acts_ref", acts_ref, what), _features("acts_sample", acts_sample, what)
    if ref.shape[1] != smp.shape[1]:
        raise ValueError(f"{what}: feature widths differ: {ref.shape[1]} and {smp.shape[1]}")
    return ref, smp


def compute_kid(acts_ref, acts_sample, subsets=100, subset_size=1000, seed=0, use_gpu=None):
    """Kernel Inception Distance (Binkowski et al. 2018): the unbiased MMD^2 between the two sets of float32 [N, D] rows with the
    kernel k(x, y) = (x.y / D + 1)^3.  Returns dict(kid_mean, kid_std, kid_full):

    * kid_mean / kid_std: mean and population standard deviation (ddof = 0) over `subsets` subsets of
      m = min(subset_size, N_ref, N_sample) rows from each set, drawn without replacement as kid_subset_indices documents, of
      MMD^2 = s0 / (m (m - 1)) + s1 / (m (m - 1)) - 2 s2 / m^2, with s0 = sum_{i != j} k(ref_i, ref_j), s1 the same over the sample
      rows and s2 = sum_{i, j} k(ref_i, sample_j);
    * kid_full: the same estimator once over all rows of both sets (N_ref and N_sample may differ), which no subset draw enters.

    The sums are ddk.ops.poly_mmd_sums on a ROCm device (rows gathered on the device into one [subsets m, D] matrix per set) and
    poly_mmd_sums_numpy without one: fp32 dot products and kernel values, float64 sums; other implementations run in float64 or
    float16 throughout and differ from this in the low digits.  use_gpu None: the kernels when a device is present."""
    what = "compute_kid"
    ref, smp = _two_sets(what, acts_ref, acts_sample)
    for name, v in (("subsets", subsets), ("subset_size", subset_size)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < (1 if name == "subsets" else 2):
            raise ValueError(f"{what}: {name} must be an integer of at least {1 if name == 'subsets' else 2}, got {v!r}")
    if min(len(ref), len(smp)) < 2:
        raise ValueError(f"{what}: both sets need at least 2 rows, got {len(ref)} and {len(smp)}")
    m = int(min(subset_size, len(ref), len(smp)))
    ref_idx, smp_idx = kid_subset_indices(len(ref), len(smp), int(subsets), m, seed)
    if use_gpu is None:
        use_gpu = gpu_available()
    if use_gpu:
        import torch
        from ddk import ops
        a, b = (torch.from_numpy(x if x.flags.writeable else x.copy()).cuda() for x in (ref, smp))
        full = ops.poly_mmd_sums(a, b, 1, None, KID_COEF0).cpu().numpy()
        chunk = max(1, min(int(subsets), KID_GATHER_ELEMS // (m * ref.shape[1]), ops.POLY_MMD_MAX_ROWS // m))
        parts = []
        for s0 in range(0, int(subsets), chunk):
            ia = torch.from_numpy(ref_idx[s0:s0 + chunk].reshape(-1)).cuda()
            ib = torch.from_numpy(smp_idx[s0:s0 + chunk].reshape(-1)).cuda()
            parts.append(ops.poly_mmd_sums(a.index_select(0, ia), b.index_select(0, ib), len(ia) // m, None, KID_COEF0).cpu().numpy())
        sums = np.concatenate(parts)
    else:
        full = poly_mmd_sums_numpy(ref, smp, 1, None, KID_COEF0)
        sums = poly_mmd_sums_numpy(ref[ref_idx.reshape(-1)], smp[smp_idx.reshape(-1)], int(subsets), None, KID_COEF0)
    per = mmd2_from_sums(sums, m, m)
    return dict(kid_mean=float(per.mean()), kid_std=float(per.std()), kid_full=float(mmd2_from_sums(full, len(ref), len(smp))[0]))


# ---------------------------------------------------------------- density / coverage
DENSITY_COVERAGE_K = 5                           # Naeem et al. 2020, the value their reference code and its users report


def ball_counts_numpy(a, ra, b, row_block=1024):
    """int32 [len(a)]: the number of rows j of b with d(a_i, b_j) <= ra[i], float32 distances as in members_numpy"""
    a, b = _features("a", a, "ball_counts"), _features("b", b, "ball_counts")
    na, nb = _norms(a), _norms(b)
    out = np.empty(len(a), dtype=np.int32)
    for r0 in range(0, len(a), row_block):
        d = _dist_block(a[r0:r0 + row_block], na[r0:r0 + row_block], b, nb)
        out[r0:r0 + row_block] = (d <= ra[r0:r0 + row_block, None]).sum(axis=1)
    return out


def compute_density_coverage(acts_ref, acts_sample, k=DENSITY_COVERAGE_K, use_gpu=None):
    """(density, coverage) of Naeem et al. 2020 ("Reliable fidelity and diversity metrics for generative models").  With r_i the
    distance of reference row i to its k-th nearest other reference row (manifold_radii(ref, k), so k <= 7) and
    counts[i] = #{ j : d(ref_i, sample_j) <= r_i }: density = sum_i counts[i] / (k N_sample), which may exceed 1, and
    coverage = mean_i (counts[i] > 0).  Squared fp32 distances as in compute_prec_recall; use_gpu as there."""
    what = "compute_density_coverage"
    ref, smp = _two_sets(what, acts_ref, acts_sample)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 7:
        raise ValueError(f"{what}: k must be an integer in 1..7, got {k!r}")
    k = int(k)
    if len(ref) < k + 1:
        raise ValueError(f"{what}: the reference set needs at least k + 1 = {k + 1} rows, got {len(ref)}")
    if use_gpu is None:
        use_gpu = gpu_available()
    if use_gpu:
        import torch
        from ddk import ops
        a, b = (torch.from_numpy(x if x.flags.writeable else x.copy()).cuda() for x in (ref, smp))
        counts = ops.manifold_ball_counts(a, ops.manifold_radii(a, k), b).cpu().numpy()
    else:
        counts = ball_counts_numpy(ref, radii_numpy(ref, k), smp)
    return int(counts.sum(dtype=np.int64)) / (k * len(smp)), int((counts > 0).sum()) / len(ref)


# ---------------------------------------------------------------- files
class Activations:
    """What one .npz holds: pool / spatial activation rows (or None), their statistics (stats never None, stats_spatial may be),
    softmax outputs (or None)."""

    def __init__(self, pool, stats, spatial, stats_spatial, softmax):
        self.pool, self.stats, self.spatial, self.stats_spatial, self.softmax = pool, stats, spatial, stats_spatial, softmax


def _rows(path, name, arr, width=None):
    arr = np.asarray(arr)
    if arr.ndim != 2 or arr.shape[0] < 2 or (width is not None and arr.shape[1] != width):
        raise ValueError(f"{path}: {name} must be [N, {width if width is not None else 'C'}] with N >= 2, got {arr.shape}")
    return arr


def load_activations(path):
    """Read an activation file: required ``pool_3`` [N, 2048], or ``mu`` / ``sigma`` instead; optional ``spatial`` [N, 2023], or
    ``mu_s`` / ``sigma_s``; optional ``softmax`` [N, C].  The statistics names are those of the published guided-diffusion reference
    batches.  Rows are kept as float32 (what the distance kernels take); statistics are float64."""
    with np.load(path) as f:
        keys = set(f.files)
        pool = spatial = softmax = stats_spatial = None
        if 'pool_3' in keys:
            pool = np.ascontiguousarray(_rows(path, 'pool_3', f['pool_3'], POOL_DIM), dtype=np.float32)
            stats = compute_statistics(f['pool_3'])
        elif 'mu' in keys and 'sigma' in keys:
            stats = FIDStatistics(f['mu'], f['sigma'])
        else:
            raise ValueError(f"{path}: needs 'pool_3' activations or 'mu' and 'sigma' statistics, has {sorted(keys)}")
        if 'spatial' in keys:
            spatial = np.ascontiguousarray(_rows(path, 'spatial', f['spatial'], SPATIAL_DIM), dtype=np.float32)
            stats_spatial = compute_statistics(f['spatial'])
        elif 'mu_s' in keys and 'sigma_s' in keys:
            stats_spatial = FIDStatistics(f['mu_s'], f['sigma_s'])
        if 'softmax' in keys:
            softmax = _rows(path, 'softmax', f['softmax'])
    return Activations(pool, stats, spatial, stats_spatial, softmax)


def sample_metrics(ref, sample, k=PREC_RECALL_K):
    """The five sample metrics of the reference's table from two Activations (or two paths); None wherever an input is missing."""
    ref = load_activations(ref) if isinstance(ref, (str, bytes)) or hasattr(ref, '__fspath__') else ref
    sample = load_activations(sample) if isinstance(sample, (str, bytes)) or hasattr(sample, '__fspath__') else sample
    out = dict.fromkeys(SAMPLE_METRICS)
    if sample.softmax is not None:
        out['is'] = compute_inception_score(sample.softmax)
    out['fid'] = sample.stats.frechet_distance(ref.stats)
    if ref.stats_spatial is not None and sample.stats_spatial is not None:
        out['sfid'] = sample.stats_spatial.frechet_distance(ref.stats_spatial)
    if ref.pool is not None and sample.pool is not None:
        out['precision'], out['recall'] = compute_prec_recall(ref.pool, sample.pool, k)
    return out


def extended_sample_metrics(ref, sample, kid=False, density_coverage=False, k=PREC_RECALL_K, kid_subsets=100, kid_subset_size=1000,
                            kid_seed=0, density_coverage_k=DENSITY_COVERAGE_K, use_gpu=None):
    """sample_metrics' five keys, unchanged and first, then ``kid_mean`` / ``kid_std`` / ``kid_full`` with kid=True and ``density`` /
    ``coverage`` with density_coverage=True (the order of EXTENDED_METRICS).  The new metrics need the pool_3 rows of both files:
    where a file holds statistics only, their keys are None."""
    ref = load_activations(ref) if isinstance(ref, (str, bytes)) or hasattr(ref, '__fspath__') else ref
    sample = load_activations(sample) if isinstance(sample, (str, bytes)) or hasattr(sample, '__fspath__') else sample
    out = sample_metrics(ref, sample, k)
    rows = ref.pool is not None and sample.pool is not None
    if kid:
        out.update(dict.fromkeys(EXTENDED_METRICS[:3]))
        if rows:
            out.update(compute_kid(ref.pool, sample.pool, kid_subsets, kid_subset_size, kid_seed, use_gpu))
    if density_coverage:
        out.update(dict.fromkeys(EXTENDED_METRICS[3:]))
        if rows:
            out['density'], out['coverage'] = compute_density_coverage(ref.pool, sample.pool, density_coverage_k, use_gpu)
    return out
