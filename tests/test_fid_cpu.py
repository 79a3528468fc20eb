"""FID without a GPU: the FID Inception weight loader (key layout, BN folding) and frechet_distance against the reference's
own calculate_frechet_distance (tests/golden/fid_frechet.npz, tests/golden/make_golden_fid.py)."""
import os.path as osp

import numpy as np
import pytest
import torch

from tests import fid_restatement as R

HERE = osp.dirname(osp.abspath(__file__))


def _sd(seed=0):
    from genesis_amd import fid
    return R.random_state_dict(fid.expected_shapes(), seed)


def test_layer_table_is_the_fid_inception():
    from genesis_amd import fid
    L = fid.layer_table()
    assert len(L) == 94
    assert len({l[0] for l in L}) == 94
    kernels = {(l[3], l[4]) for l in L}
    assert kernels == {(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1)}
    shapes = fid.expected_shapes()
    assert len(shapes) == 5 * 94
    assert shapes['Mixed_7c.branch3x3dbl_3b.conv.weight'] == (384, 384, 3, 1)
    assert shapes['Mixed_6e.branch7x7dbl_5.conv.weight'] == (192, 192, 1, 7)
    assert shapes['Conv2d_1a_3x3.conv.weight'] == (32, 3, 3, 3)


def test_loader_folds_bn_within_one_ulp():
    from genesis_amd import fid
    sd = _sd()
    sd['AuxLogits.fc.weight'] = torch.zeros(1000, 768)          # ignored, like fc.* and num_batches_tracked
    net = fid.FIDInception.from_state_dict(sd, device='cpu')
    assert len(net.folded) == 94
    for name, (w, b) in net.folded.items():
        g, beta, mean, var = [sd['%s.bn.%s' % (name, p)].double() for p in ('weight', 'bias', 'running_mean', 'running_var')]
        s = g / torch.sqrt(var + 1e-3)
        w64 = sd[name + '.conv.weight'].double() * s[:, None, None, None]
        b64 = beta - mean * s
        for got, exact in ((w, w64), (b, b64)):
            assert got.dtype == torch.float32 and got.shape == exact.shape
            ulp = torch.from_numpy(np.spacing(np.abs(got.numpy()))).double()
            assert bool(((got.double() - exact).abs() <= ulp).all()), name


def test_loader_reads_a_weights_file(tmp_path):
    from genesis_amd import fid
    sd = _sd(1)
    p = str(tmp_path / fid.WEIGHTS_FILE)
    torch.save(sd, p)
    a = fid.FIDInception.from_state_dict(p, device='cpu')
    b = fid.load_fid_inception(p, device='cpu')
    for name in a.folded:
        assert torch.equal(a.folded[name][0], b.folded[name][0]) and torch.equal(a.folded[name][1], b.folded[name][1])


@pytest.mark.parametrize('change', ['missing', 'extra', 'shape'])
def test_loader_names_the_offending_key(change):
    from genesis_amd import fid
    from genesis_amd._lib import GenesisHipError
    sd = _sd()
    if change == 'missing':
        key = 'Mixed_6c.branch7x7dbl_3.bn.running_var'
        del sd[key]
    elif change == 'extra':
        key = 'Mixed_5b.branch9x9.conv.weight'
        sd[key] = torch.zeros(3)
    else:
        key = 'Mixed_7b.branch3x3_2a.conv.weight'
        sd[key] = torch.zeros(384, 384, 3, 1)
    with pytest.raises(GenesisHipError, match=key.replace('.', r'\.')):
        fid.FIDInception.from_state_dict(sd, device='cpu')


def test_missing_weights_file_is_named_and_not_downloaded(tmp_path, monkeypatch):
    from genesis_amd import fid
    from genesis_amd._lib import GenesisHipError
    monkeypatch.setattr(torch.hub, 'get_dir', lambda: str(tmp_path))
    assert fid.default_weights_path() == osp.join(str(tmp_path), 'checkpoints', fid.WEIGHTS_FILE)
    with pytest.raises(GenesisHipError, match=fid.WEIGHTS_FILE):
        fid.load_fid_inception()
    assert not osp.exists(osp.join(str(tmp_path), 'checkpoints'))


def _golden():
    return np.load(osp.join(HERE, 'golden', 'fid_frechet.npz'))


def _case(g, c):
    return g[c + '_mu1'], g[c + '_sigma1'], g[c + '_mu2'], g[c + '_sigma2']


@pytest.mark.parametrize('case', ['full64', 'full192'])
def test_frechet_distance_full_rank_matches_reference(case):
    from genesis_amd.fid import frechet_distance
    g = _golden()
    got, ref = frechet_distance(*_case(g, case)), float(g[case + '_fid'])
    assert abs(got - ref) <= 1e-8 * abs(ref), (got, ref)


def test_frechet_distance_rank_deficient_matches_reference():
    """N = 40 / 50 samples of 64 features: sigma1 sigma2 has D - r = 25 zero eigenvalues.  Both implementations see each
    of them perturbed by round-off of order eps |sigma1 sigma2|_2 (the reference's sqrtm residual is stored in the golden
    and is of that order), and tr sqrt takes its square root: bar = 2 (D - r) sqrt(eps |sigma1 sigma2|_2)."""
    from genesis_amd.fid import frechet_distance
    g = _golden()
    mu1, s1, mu2, s2 = _case(g, 'rank64')
    D, r = s1.shape[0], min(np.linalg.matrix_rank(s1), np.linalg.matrix_rank(s2))
    assert r < D
    norm = np.linalg.norm(s1.dot(s2), 2)
    assert float(g['rank64_sqrtm_residual']) < 1e3 * np.finfo(np.float64).eps
    bar = 2 * (D - r) * np.sqrt(np.finfo(np.float64).eps * norm)
    got, ref = frechet_distance(mu1, s1, mu2, s2), float(g['rank64_fid'])
    print('rank-deficient: |ours - reference| = %.3g, bar %.3g' % (abs(got - ref), bar))
    assert abs(got - ref) <= bar, (got, ref, bar)


def test_frechet_distance_of_identical_statistics_is_zero():
    from genesis_amd.fid import frechet_distance
    g = _golden()
    assert abs(frechet_distance(*_case(g, 'same64'))) <= 1e-10
    assert abs(float(g['same64_fid'])) <= 1e-10


def test_frechet_distance_of_shifted_means():
    from genesis_amd.fid import frechet_distance
    s = np.diag([1.0, 4.0])
    assert frechet_distance(np.zeros(2), s, np.ones(2), s) == pytest.approx(2.0, abs=1e-12)
