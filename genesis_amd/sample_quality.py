"""Sample quality beside FID, on the device: improved precision and recall (Kynkaanniemi et al. 2019), density and
coverage (Naeem et al. 2020) and KID (Binkowski et al. 2018), all from the FID Inception pool features that
genesis_amd/fid.py produces.  The all-pairs work runs on gx_manifold.hip in fp64 with no N x M matrix in memory
(include/genesis_hip.h states the arithmetic); the final means, sums and ratios are fp64 device ops, and every function
reads the device once, in one small copy at the end.  There is no CPU path.

With real features R [N, D] and generated features F [M, D] (fp32), d2 the squared Euclidean distance and
rho_k(x_i; X) the k-th smallest d2 from x_i to the OTHER rows of X (squared; no square root anywhere):
    precision = mean_j [exists i: d2(f_j, r_i) <= rho_k(r_i; R)]        recall = mean_i [exists j: d2(r_i, f_j) <= rho_k(f_j; F)]
    density   = sum_j sum_i [d2(f_j, r_i) <= rho_k(r_i; R)] / (k M)     coverage = mean_i [min_j d2(r_i, f_j) <= rho_k(r_i; R)]
    KID       = mean over subsets of the unbiased MMD^2 with kappa(x, y) = (x . y / D + 1)^3
Exact ties (duplicate images, a sample that equals a data image) compare as <=, which is true.

The features are the FID Inception ones.  The precision / recall paper used VGG-16 features: numbers from here are
comparable only with tools that use the same (FID Inception pool) features."""
import ctypes

import numpy as np
import torch

from . import _lib
from . import fid as _fid
from ._lib import GenesisHipError

def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _features(x, what):
    """A contiguous fp32 device matrix [rows, D], or GenesisHipError."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise GenesisHipError('%s: expected a device tensor (there is no CPU path), got %s'
                              % (what, getattr(x, 'device', type(x).__name__)))
    if x.dtype != torch.float32 or x.dim() != 2:
        raise GenesisHipError('%s: expected fp32 features [rows, D], got %s %s' % (what, x.dtype, tuple(x.shape)))
    return x.contiguous()


def _same_space(real, fake, what):
    real, fake = _features(real, what), _features(fake, what)
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise GenesisHipError('%s: real %s on %s and generated %s on %s do not share a feature space'
                              % (what, tuple(real.shape), real.device, tuple(fake.shape), fake.device))
    return real, fake


class FeatureBank(object):
    """A preallocated fp32 [capacity, dims] device buffer that feature batches are appended to."""

    def __init__(self, dims, capacity, device):
        self.dims, self.capacity, self.device = int(dims), int(capacity), torch.device(device)
        if self.device.type != 'cuda':
            raise GenesisHipError('FeatureBank: the bank lives on the HIP device, not on %s' % self.device)
        if self.dims < 1 or self.capacity < 1:
            raise GenesisHipError('FeatureBank: dims and capacity must be positive, got %d, %d' % (self.dims, self.capacity))
        self.buffer = torch.empty(self.capacity, self.dims, dtype=torch.float32, device=self.device)
        self.device = self.buffer.device
        self.count = 0

    def append(self, feats):
        if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or feats.dim() != 2 \
                or feats.shape[1] != self.dims or feats.device != self.device:
            raise GenesisHipError('FeatureBank.append: expected fp32 features [B, %d] on %s, got %s %s on %s'
                                  % (self.dims, self.device, getattr(feats, 'dtype', None),
                                     tuple(getattr(feats, 'shape', ())), getattr(feats, 'device', None)))
        n = feats.shape[0]
        if self.count + n > self.capacity:
            raise GenesisHipError('FeatureBank.append: %d + %d rows overflow the capacity %d' % (self.count, n, self.capacity))
        self.buffer[self.count:self.count + n].copy_(feats)
        self.count += n

    @property
    def features(self):
        return self.buffer[:self.count]


# ---- the three device calls ----
def knn_radii(X, k):
    """fp64 device [N]: the squared distance of every row of X [N, D] to its k-th nearest other row."""
    X = _features(X, 'knn_radii')
    N, D = X.shape
    need = _lib.query('gx_knn_radii_ws_bytes', N, int(k))
    ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=X.device)
    out = torch.empty(N, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        _lib.call('gx_knn_radii', _ptr(X), N, D, int(k), _ptr(out), _ptr(ws), ws.numel() * 8, _stream())
    return out


def manifold_counts(Q, R, radii2):
    """(hits int32 [M], covered int32 [N]) for queries Q [M, D] against references R [N, D] with R's radii [N] (fp64):
    hits[j] = #{i: d2(q_j, r_i) <= radii2[i]}, covered[i] = 1 if any query lies in r_i's ball."""
    Q, R = _same_space(Q, R, 'manifold_counts')
    if not isinstance(radii2, torch.Tensor) or radii2.device != R.device or radii2.dtype != torch.float64 \
            or tuple(radii2.shape) != (R.shape[0],):
        raise GenesisHipError('manifold_counts: expected fp64 device radii [%d] beside the references' % R.shape[0])
    radii2 = radii2.contiguous()
    hits = torch.empty(Q.shape[0], dtype=torch.int32, device=Q.device)
    covered = torch.empty(R.shape[0], dtype=torch.int32, device=Q.device)
    with torch.cuda.device(Q.device):
        _lib.call('gx_manifold_counts', _ptr(Q), Q.shape[0], _ptr(R), R.shape[0], Q.shape[1], _ptr(radii2), _ptr(hits),
                  _ptr(covered), _stream())
    return hits, covered


def kid_indices(num_real, num_fake, subset_size, num_subsets, seed=0):
    """(ix int32 [S, m] into the generated rows, iy int32 [S, m] into the real rows): each row drawn without replacement
    from numpy.random.default_rng(seed), in the order subset 0 ix, subset 0 iy, subset 1 ix, ..."""
    rng = np.random.default_rng(seed)
    ix = np.empty((num_subsets, subset_size), np.int32)
    iy = np.empty((num_subsets, subset_size), np.int32)
    for s in range(num_subsets):
        ix[s] = rng.choice(num_fake, subset_size, replace=False)
        iy[s] = rng.choice(num_real, subset_size, replace=False)
    return ix, iy


def kid_sums(real, fake, ix, iy):
    """fp64 device [S, 3]: per subset the sums of kappa over the generated pairs a != b, the real pairs a != b, and all
    generated x real pairs.  ix / iy: integer [S, m] (host or device) into the rows of fake / real."""
    real, fake = _same_space(real, fake, 'kid_sums')
    idx = []
    for name, v, n in (('ix', ix, fake.shape[0]), ('iy', iy, real.shape[0])):
        v = torch.as_tensor(v)
        if v.dim() != 2 or v.dtype not in (torch.int32, torch.int64) or v.numel() == 0:
            raise GenesisHipError('kid_sums: %s must be an integer matrix [S, m], got %s %s' % (name, v.dtype, tuple(v.shape)))
        if not v.is_cuda and (int(v.min()) < 0 or int(v.max()) >= n):
            raise GenesisHipError('kid_sums: %s holds an index outside [0, %d)' % (name, n))
        idx.append(v.to(device=real.device, dtype=torch.int32).contiguous())
    ix, iy = idx
    if ix.shape != iy.shape:
        raise GenesisHipError('kid_sums: ix %s and iy %s differ in shape' % (tuple(ix.shape), tuple(iy.shape)))
    S, m = ix.shape
    need = _lib.query('gx_kid_sums_ws_bytes', m, S)
    ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=real.device)
    sums = torch.empty(S, 3, dtype=torch.float64, device=real.device)
    with torch.cuda.device(real.device):
        _lib.call('gx_kid_sums', _ptr(fake), fake.shape[0], _ptr(ix), _ptr(real), real.shape[0], _ptr(iy), m,
                  real.shape[1], S, _ptr(sums), _ptr(ws), ws.numel() * 8, _stream())
    return sums


def kid_from_sums(sums, m):
    """fp64 device [2] = (mean, standard deviation) over subsets of
    mmd2_s = (sums[s, 0] + sums[s, 1]) / (m (m - 1)) - 2 sums[s, 2] / m^2  (the deviation as numpy.std: ddof = 0)."""
    mmd2 = (sums[:, 0] + sums[:, 1]) / float(m * (m - 1)) - 2.0 * sums[:, 2] / float(m * m)
    return torch.stack([mmd2.mean(), mmd2.std(unbiased=False)])


# ---- the metrics, as fp64 device scalars (no device read) ----
def _precision_recall_dev(real, fake, k):
    hits_f, _ = manifold_counts(fake, real, knn_radii(real, k))
    hits_r, _ = manifold_counts(real, fake, knn_radii(fake, k))
    return torch.stack([(hits_f > 0).sum().double() / fake.shape[0], (hits_r > 0).sum().double() / real.shape[0]])


def _density_coverage_dev(real, fake, k):
    hits, covered = manifold_counts(fake, real, knn_radii(real, k))
    return torch.stack([hits.sum(dtype=torch.int64).double() / float(k * fake.shape[0]),
                        covered.sum(dtype=torch.int64).double() / real.shape[0]])


def _kid_dev(real, fake, num_subsets, max_subset_size, seed):
    m = min(real.shape[0], fake.shape[0], int(max_subset_size))
    if m < 2:
        raise GenesisHipError('kid: needs at least 2 real and 2 generated rows per subset, have m = %d' % m)
    ix, iy = kid_indices(real.shape[0], fake.shape[0], m, int(num_subsets), seed)
    return kid_from_sums(kid_sums(real, fake, ix, iy), m)


def precision_recall(real, fake, k=3):
    """(precision, recall) of generated features `fake` [M, D] against real features `real` [N, D] (FID Inception features,
    not the paper's VGG-16 ones)."""
    real, fake = _same_space(real, fake, 'precision_recall')
    p, r = _precision_recall_dev(real, fake, k).cpu().tolist()
    return p, r


def density_coverage(real, fake, k=5):
    """(density, coverage) of `fake` [M, D] against `real` [N, D]."""
    real, fake = _same_space(real, fake, 'density_coverage')
    d, c = _density_coverage_dev(real, fake, k).cpu().tolist()
    return d, c


def kid(real, fake, num_subsets=100, max_subset_size=1000, seed=0):
    """(mean, standard deviation over subsets) of the MMD^2 estimates between `real` and `fake`, subsets of
    m = min(N, M, max_subset_size) rows each drawn as kid_indices does."""
    real, fake = _same_space(real, fake, 'kid')
    mean, std = _kid_dev(real, fake, num_subsets, max_subset_size, seed).cpu().tolist()
    return mean, std


def sample_quality(real, fake, k_pr=3, k_dc=5, kid_subsets=100, kid_subset_size=1000, seed=0):
    """dict(precision, recall, density, coverage, kid, kid_std) of `fake` against `real`; one device read."""
    real, fake = _same_space(real, fake, 'sample_quality')
    vals = torch.cat([_precision_recall_dev(real, fake, k_pr), _density_coverage_dev(real, fake, k_dc),
                      _kid_dev(real, fake, kid_subsets, kid_subset_size, seed)]).cpu().tolist()
    return dict(zip(('precision', 'recall', 'density', 'coverage', 'kid', 'kid_std'), vals))


def sample_quality_from_model(model, test_loader, batch_size=10, num_images=10000, feat_dim=2048, k_pr=3, k_dc=5,
                              kid_subsets=100, kid_subset_size=1000, seed=0, weights=None):
    """fid.fid_from_model's image selection, eval() / train() handling, `weights` forms and sample() loop, with every
    image's features computed once into two banks.  Returns dict(fid, precision, recall, density, coverage, kid, kid_std,
    num_real, num_fake); `fid` is fid_from_model's value bit for bit on the same inputs and seed (FIDStatistics over the
    banked features, which do not depend on the batch an image was computed in)."""
    model.eval()
    try:
        dev = next(model.parameters()).device
        if isinstance(weights, _fid.FIDInception):
            net = weights
        elif weights is None:
            net = _fid.load_fid_inception(device=dev)
        else:
            net = _fid.FIDInception.from_state_dict(weights, dev)
        used = (num_images // batch_size) * batch_size
        if used < 2:
            raise GenesisHipError('sample_quality_from_model: need at least 2 images, have %d' % used)
        real, gen = FeatureBank(feat_dim, used, net.device), FeatureBank(feat_dim, used, net.device)
        count = 0
        for batch in test_loader:
            x = _fid._images_of(batch)
            take = min(x.shape[0], num_images - count)
            if count < used:
                real.append(net.features(x[:min(take, used - count)].to(net.device, torch.float32).contiguous(), feat_dim))
            count += take
            if count >= num_images:
                break
        count = 0
        for _ in range(num_images // batch_size + 1):
            if count >= num_images:
                break
            with torch.no_grad():
                img, _ = model.sample(batch_size)
            take = min(img.shape[0], num_images - count)
            if count < used:
                gen.append(net.features(img[:min(take, used - count)].to(net.device, torch.float32).contiguous(), feat_dim))
            count += take
        stats = []
        for bank in (real, gen):
            st = _fid.FIDStatistics(net, feat_dim)
            st.update_features(bank.features)
            stats.append(st.compute())
        out = dict(fid=_fid.frechet_distance(*stats[0], *stats[1]))
        out.update(sample_quality(real.features, gen.features, k_pr, k_dc, kid_subsets, kid_subset_size, seed))
        out.update(num_real=real.count, num_fake=gen.count)
        return out
    finally:
        model.train()
