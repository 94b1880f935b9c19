"""Sample metrics from Inception activations: FID, sFID, Inception score and improved precision / recall.

The second half of the reference's evaluator (utils/evaluator.py): everything after the Inception network.  The network itself is
NOT here: the activations come from any Inception port as an ``.npz`` file, or, for the reference side of
FID / sFID, from one of the published guided-diffusion reference batches, which carry ``mu`` / ``sigma`` / ``mu_s`` / ``sigma_s``.

Moments, Frechet distance and Inception score are float64 numpy, once per evaluation.  Precision / recall is three passes over
N x N x D distances: on a ROCm device they run on the HIP kernels of csrc/manifold.hip (ddk.ops.manifold_radii /
manifold_members); without one, a row-blocked numpy float32 path evaluates the same formula.  Both are
fp32; the reference's distances are fp16 whenever that stays finite, so its values can differ from these in the third decimal.
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
def _features(name, x):
    x = np.ascontiguousarray(x)
    if x.ndim != 2 or x.dtype != np.float32:
        raise ValueError(f"compute_prec_recall: {name} must be a float32 [N, D] array, got {x.dtype} {x.shape}")
    if not np.isfinite(x).all():
        raise ValueError(f"compute_prec_recall: {name} holds non-finite features")
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
