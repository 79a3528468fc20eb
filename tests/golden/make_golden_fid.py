"""Generates tests/golden/fid_frechet.npz from the REAL reference function third_party/pytorch_fid/fid_score.py:
calculate_frechet_distance (scipy.linalg.sqrtm), imported from /root/reference in the build container.  fid_score.py
imports torchvision (through inception.py) and imageio at module level; neither is installed, and the distance needs
neither, so both are replaced by empty stand-ins in sys.modules here.

Cases (mu and the unbiased covariance of seeded random features, as np.mean / np.cov(rowvar=False) of
get_activations' output):
  full64, full192   two full-rank pairs (N = 400 / 600 samples of 64 / 192 correlated, shifted features)
  rank64            a rank-deficient pair: N = 40 and 50 samples of 64 features (covariance ranks 39 and 49)
  same64            identical statistics (the first full64 set against itself): FID 0
Each case stores mu1, sigma1, mu2, sigma2 and `fid` = the reference's value; rank64 also stores the relative residual of
the reference's matrix square root, |covmean^2 - sigma1 sigma2|_F / |sigma1 sigma2|_F, from which the test derives its bar."""
import os.path as osp
import sys
import types

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
REFERENCE_ROOT = '/root/reference'


def import_reference_fid():
    tv = types.ModuleType('torchvision')
    tv.models = types.ModuleType('torchvision.models')
    tv.models.inception = types.ModuleType('torchvision.models.inception')
    for cls in ('InceptionA', 'InceptionC', 'InceptionE'):
        setattr(tv.models.inception, cls, type(cls, (object,), {}))
    io = types.ModuleType('imageio')
    io.imread = None
    sys.modules.update({'torchvision': tv, 'torchvision.models': tv.models,
                        'torchvision.models.inception': tv.models.inception, 'imageio': io})
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    from third_party.pytorch_fid import fid_score
    return fid_score


def features(rng, n, d, shift, scale):
    a = rng.randn(d, d) * scale / np.sqrt(d)
    return np.maximum(rng.randn(n, d) @ a + shift, 0) + 0.1 * rng.rand(n, d)


def stats(x):
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def main():
    F = import_reference_fid()
    from scipy import linalg
    rng = np.random.RandomState(2024)
    out = {}
    cases = {'full64': (400, 400, 64), 'full192': (600, 600, 192), 'rank64': (40, 50, 64)}
    for name, (n1, n2, d) in cases.items():
        m1, s1 = stats(features(rng, n1, d, 0.3, 1.0))
        m2, s2 = stats(features(rng, n2, d, 0.5, 1.3))
        out.update({name + '_mu1': m1, name + '_sigma1': s1, name + '_mu2': m2, name + '_sigma2': s2,
                    name + '_fid': np.float64(F.calculate_frechet_distance(m1, s1, m2, s2))})
        if name == 'rank64':
            prod = s1.dot(s2)
            cm, _ = linalg.sqrtm(prod, disp=False)
            out[name + '_sqrtm_residual'] = np.float64(np.linalg.norm(cm.dot(cm) - prod) / np.linalg.norm(prod))
    m, s = out['full64_mu1'], out['full64_sigma1']
    out.update({'same64_mu1': m, 'same64_sigma1': s, 'same64_mu2': m, 'same64_sigma2': s,
                'same64_fid': np.float64(F.calculate_frechet_distance(m, s, m, s))})
    np.savez_compressed(osp.join(HERE, 'fid_frechet.npz'), **out)
    print({k: float(v) for k, v in out.items() if np.ndim(v) == 0})


if __name__ == '__main__':
    main()
