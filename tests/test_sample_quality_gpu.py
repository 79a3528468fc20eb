"""Sample quality on the device (genesis_amd/sample_quality.py, gx_manifold.hip) against the fp64 numpy restatement
(tests/sample_quality_restatement.py): k-NN radii, manifold counts (compared exactly, exact ties included), the four
manifold metrics, the KID sums, repeatability, the feature bank, the output buffers' surroundings, and
sample_quality_from_model end to end beside fid_from_model."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import fid_restatement as FR
from tests import sample_quality_restatement as SR

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U53 = 2.0 ** -53
MIN_GAP = 1e-9

# (seed, N, M, D, k, kind); seed 4 gets duplicates (R[9] = R[5], F[3] = R[5], F[11] = F[2]); seed 7: a D that is a multiple
# of 4 but not of the kernel's chunk of 32
CASES = [(1, 37, 29, 64, 3, 'plain'), (2, 130, 67, 2048, 3, 'abs'), (3, 65, 64, 192, 5, 'abs'), (4, 33, 31, 768, 1, 'plain'),
         (5, 9, 7, 2048, 6, 'abs'), (6, 257, 129, 2048, 3, 'abs'), (7, 37, 29, 68, 3, 'plain')]
IDS = ['seed%d_N%d_M%d_D%d_k%d_%s' % c for c in CASES]


@functools.lru_cache(maxsize=None)
def reference(case):
    """The inputs and everything the restatement says about them, computed once per case and shared (read only)."""
    seed, N, M, D, k, kind = case
    R, F = SR.make_features(seed, N, M, D, kind)
    if seed == 4:
        R[9] = R[5]
        F[3] = R[5]
        F[11] = F[2]
    rad_r, rad_f = SR.knn_radii(R, k), SR.knn_radii(F, k)
    d_fr = SR.sqdist(F, R)
    ref = dict(R=R, F=F, rad_r=rad_r, rad_f=rad_f, d_fr=d_fr,
               fr=SR.manifold_counts(F, R, rad_r, d_fr), rf=SR.manifold_counts(R, F, rad_f, d_fr.T.copy()),
               gap=min(SR.min_relative_gap(d_fr, rad_r), SR.min_relative_gap(d_fr.T, rad_f)),
               ties=SR.count_ties(d_fr, rad_r) + SR.count_ties(d_fr.T, rad_f))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # (a copy: the shared references are read only)


def _check_radii(got, want, D):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    zero = want == 0
    assert np.array_equal(got[zero], want[zero])                       # exactly 0 where the restatement's are 0
    rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
    worst = float(rel.max()) if rel.size else 0.0
    print('radii: worst relative error %.3g (bound %.3g)' % (worst, 100 * (D + 2) * U53))
    assert worst <= 100 * (D + 2) * U53


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_radii_counts_and_metrics_against_the_restatement(case):
    from genesis_amd import sample_quality as SQ
    seed, N, M, D, k, kind = case
    ref = reference(case)
    # integer results are compared exactly: legitimate only if no comparison sits on a rounding edge
    assert ref['gap'] >= MIN_GAP, ref['gap']
    if seed == 4:
        assert ref['ties'] == 7 and int((ref['rad_r'] == 0).sum()) == 2 and int((ref['rad_f'] == 0).sum()) == 2
    R, F = _dev(ref['R']), _dev(ref['F'])
    rad_r, rad_f = SQ.knn_radii(R, k), SQ.knn_radii(F, k)
    _check_radii(rad_r, ref['rad_r'], D)
    _check_radii(rad_f, ref['rad_f'], D)
    for (Q, X, rad), (hits_ref, cov_ref) in (((F, R, rad_r), ref['fr']), ((R, F, rad_f), ref['rf'])):
        hits, covered = SQ.manifold_counts(Q, X, rad)
        assert hits.dtype == torch.int32 and covered.dtype == torch.int32
        assert np.array_equal(hits.cpu().numpy(), hits_ref), 'hits differ at %s' % np.nonzero(hits.cpu().numpy() != hits_ref)[0]
        assert np.array_equal(covered.cpu().numpy(), cov_ref)
        again = SQ.manifold_counts(Q, X, rad)                             # a repeat is bit-identical
        assert torch.equal(again[0], hits) and torch.equal(again[1], covered)
    assert torch.equal(SQ.knn_radii(R, k), rad_r)
    got = SQ.precision_recall(R, F, k) + SQ.density_coverage(R, F, k)
    want = SR.precision_recall(ref['R'], ref['F'], k) + SR.density_coverage(ref['R'], ref['F'], k)
    print('P / R / D / C: %s (restatement %s)' % (got, want))
    for g, w in zip(got, want):
        assert isinstance(g, float) and abs(g - w) <= 1e-15 * abs(w)
    assert got == SQ.precision_recall(R, F, k) + SQ.density_coverage(R, F, k)


def test_distance_is_symmetric_and_position_independent():
    """d2(a, b) has the same bits wherever the pair is evaluated: a row's radius does not move when the set is permuted
    (other tile positions, other argument order), and the ties of the duplicate case come out true on the device."""
    from genesis_amd import sample_quality as SQ
    ref = reference(CASES[5])
    R = _dev(ref['R'])
    perm = torch.from_numpy(np.random.default_rng(0).permutation(R.shape[0])).to(DEV)
    assert torch.equal(SQ.knn_radii(R[perm], 3), SQ.knn_radii(R, 3)[perm])
    # R queried against R with R's own k = 1 radii: the nearest neighbour of r_i sits exactly ON r_i's ball, a tie per ball that
    # was computed with the arguments the other way round and in another launch
    rad = SQ.knn_radii(R, 1)
    hits, covered = SQ.manifold_counts(R, R, rad)
    assert int(covered.min()) == 1 and int(hits.min()) >= 1
    d = SR.sqdist(ref['R'], ref['R'])
    rad_ref = SR.knn_radii(ref['R'], 1)
    assert SR.min_relative_gap(d, rad_ref) >= MIN_GAP and SR.count_ties(d, rad_ref) >= R.shape[0]
    want = SR.manifold_counts(ref['R'], ref['R'], rad_ref, d)
    assert np.array_equal(hits.cpu().numpy(), want[0]) and int(want[0].sum()) >= 2 * R.shape[0]


def test_smallest_problem():
    """(N, M, D, k) = (2, 1, 4, 1), radii for R only."""
    from genesis_amd import sample_quality as SQ
    R = np.float32([[0, 0, 0, 0], [1, 2, 0, 0]])
    F = np.float32([[0.5, 0, 0, 0]])
    rad = SQ.knn_radii(_dev(R), 1)
    assert rad.cpu().tolist() == [5.0, 5.0] == SR.knn_radii(R, 1).tolist()
    hits, covered = SQ.manifold_counts(_dev(F), _dev(R), rad)               # d2 = 0.25, 4.25
    assert hits.cpu().tolist() == [2] and covered.cpu().tolist() == [1, 1]
    hits, covered = SQ.manifold_counts(_dev(F), _dev(R), _dev(np.float64([0.25, 4.0])))     # a tie, and a miss
    assert hits.cpu().tolist() == [1] and covered.cpu().tolist() == [1, 0]
    assert SQ.density_coverage(_dev(R), _dev(F), 1) == SR.density_coverage(R, F, 1) == (2.0, 1.0)


# (case, m, S): m = M = 29; the smallest m; an m above the 64-row tile, whose subsets share rows
KID_CASES = [(CASES[0], 29, 3), (CASES[0], 2, 1), (CASES[5], 100, 2), (CASES[6], 29, 2)]


@pytest.mark.parametrize('case,m,S', KID_CASES, ids=['%s_m%d_S%d' % (IDS[CASES.index(c)], m, s) for c, m, s in KID_CASES])
def test_kid_sums_against_the_restatement(case, m, S):
    from genesis_amd import sample_quality as SQ
    seed, N, M, D, _, _ = case
    ref = reference(case)
    ix, iy = SQ.kid_indices(N, M, m, S, seed)
    if S > 1 and m > 64:
        assert len(set(ix[0]) & set(ix[1])) > 0 and len(set(iy[0]) & set(iy[1])) > 0       # repeated rows across subsets
    R, F = _dev(ref['R']), _dev(ref['F'])
    sums = SQ.kid_sums(R, F, ix, iy)
    want = SR.kid_sums(ref['R'], ref['F'], ix, iy)
    got = sums.cpu().numpy()
    assert got.shape == (S, 3) and got.dtype == np.float64
    rel = np.abs(got - want) / np.abs(want)
    print('KID sums: worst relative error %.3g (bound %.3g)' % (float(rel.max()), 100 * 3 * D * U53))
    assert float(rel.max()) <= 100 * 3 * D * U53
    assert torch.equal(SQ.kid_sums(R, F, _dev(ix), _dev(iy)), sums)           # a repeat (device indices) is bit-identical


def test_kid_is_the_combination_of_its_sums():
    from genesis_amd import sample_quality as SQ
    seed, N, M, D, _, _ = CASES[1]
    ref = reference(CASES[1])
    R, F = _dev(ref['R']), _dev(ref['F'])
    mean, std = SQ.kid(R, F, num_subsets=5, max_subset_size=40, seed=12)
    ix, iy = SQ.kid_indices(N, M, 40, 5, 12)
    sums = SQ.kid_sums(R, F, ix, iy).cpu().numpy()
    mmd2 = (sums[:, 0] + sums[:, 1]) / (40 * 39) - 2.0 * sums[:, 2] / (40 * 40)
    assert isinstance(mean, float) and isinstance(std, float)
    scale = float(np.abs(sums).max()) / (40 * 39)
    assert abs(mean - mmd2.mean()) <= 8 * U53 * scale and abs(std - mmd2.std()) <= 8 * U53 * scale
    assert (mean, std) == SQ.kid(R, F, num_subsets=5, max_subset_size=40, seed=12)
    # max_subset_size above both sets: m = min(N, M)
    m1 = SQ.kid(R, F, num_subsets=2, max_subset_size=1000, seed=1)
    ix, iy = SQ.kid_indices(N, M, min(N, M), 2, 1)
    assert m1 == tuple(SQ.kid_from_sums(SQ.kid_sums(R, F, ix, iy), min(N, M)).cpu().tolist())
    all_of_it = SQ.sample_quality(R, F, k_pr=3, k_dc=5, kid_subsets=5, kid_subset_size=40, seed=12)
    assert (all_of_it['precision'], all_of_it['recall']) == SQ.precision_recall(R, F, 3)
    assert (all_of_it['density'], all_of_it['coverage']) == SQ.density_coverage(R, F, 5)
    assert (all_of_it['kid'], all_of_it['kid_std']) == (mean, std)
    assert sorted(all_of_it) == ['coverage', 'density', 'kid', 'kid_std', 'precision', 'recall']


def test_feature_bank_chunking_does_not_matter():
    from genesis_amd import sample_quality as SQ
    from genesis_amd._lib import GenesisHipError
    R, F = SR.make_features(21, 60, 60, 192, 'abs')
    R, F = _dev(R), _dev(F)
    res = []
    for split in ((7, 23, 30), (60,)):
        banks = []
        for X in (R, F):
            bank = SQ.FeatureBank(192, 64, DEV)
            i = 0
            for n in split:
                bank.append(X[i:i + n])
                i += n
            assert bank.count == 60 and tuple(bank.features.shape) == (60, 192)
            banks.append(bank)
        assert torch.equal(banks[0].features, R) and torch.equal(banks[1].features, F)
        res.append(SQ.sample_quality(banks[0].features, banks[1].features, kid_subsets=3, kid_subset_size=50, seed=2))
    assert res[0] == res[1]
    bank = SQ.FeatureBank(192, 64, DEV)
    bank.append(R)
    for bad, msg in ((R[:5], 'overflow'), (R[:2].double(), 'expected fp32'), (R[:2].cpu(), 'expected fp32'),
                     (R[:2, :64], 'expected fp32'), (R[0], 'expected fp32')):
        with pytest.raises(GenesisHipError, match=msg):
            bank.append(bad)
    assert bank.count == 60


def test_canaries_behind_every_output_buffer():
    """Straight through the C ABI with padded buffers: nothing outside radii2 [N], hits [M], covered [N], sums [S, 3] and the
    workspaces' stated sizes is written."""
    from genesis_amd import _lib
    seed, N, M, D, k, _ = CASES[2]
    ref = reference(CASES[2])
    R, F = _dev(ref['R']), _dev(ref['F'])
    PAD, CAN_D, CAN_I = 64, -7.25, -77

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wsn = _lib.query('gx_knn_radii_ws_bytes', N, k) // 8
    ws = torch.full((wsn + PAD,), CAN_D, dtype=torch.float64, device=DEV)
    rad = torch.full((N + PAD,), CAN_D, dtype=torch.float64, device=DEV)
    _lib.call('gx_knn_radii', p(R), N, D, k, p(rad), p(ws), wsn * 8, st)
    hits = torch.full((M + PAD,), CAN_I, dtype=torch.int32, device=DEV)
    covered = torch.full((N + PAD,), CAN_I, dtype=torch.int32, device=DEV)
    _lib.call('gx_manifold_counts', p(F), M, p(R), N, D, p(rad), p(hits), p(covered), st)
    m, S = 30, 2
    ix, iy = (_dev(a) for a in SR.kid_indices(N, M, m, S, 0))
    ix, iy = ix.int(), iy.int()
    kwn = _lib.query('gx_kid_sums_ws_bytes', m, S) // 8
    kws = torch.full((kwn + PAD,), CAN_D, dtype=torch.float64, device=DEV)
    sums = torch.full((S * 3 + PAD,), CAN_D, dtype=torch.float64, device=DEV)
    _lib.call('gx_kid_sums', p(F), M, p(ix), p(R), N, p(iy), m, D, S, p(sums), p(kws), kwn * 8, st)
    torch.cuda.synchronize()
    for buf, n, can in ((ws, wsn, CAN_D), (rad, N, CAN_D), (hits, M, CAN_I), (covered, N, CAN_I), (kws, kwn, CAN_D),
                        (sums, S * 3, CAN_D)):
        assert bool((buf[n:] == can).all())
        assert not bool((buf[:n] == can).any())                            # ... and every element inside was written
    assert np.array_equal(hits[:M].cpu().numpy(), ref['fr'][0]) and np.array_equal(covered[:N].cpu().numpy(), ref['fr'][1])


# ---- end to end ----
class _Loader(object):
    def __init__(self, imgs, bs):
        self.imgs, self.bs = imgs, bs

    def __iter__(self):
        for i in range(0, self.imgs.shape[0], self.bs):
            yield {'input': self.imgs[i:i + self.bs]}


class _PoolModel(torch.nn.Module):
    """sample(n) serves the next n images of a fixed pool."""

    def __init__(self, pool):
        super(_PoolModel, self).__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.pool, self.i = pool, 0

    def sample(self, n):
        idx = torch.arange(self.i, self.i + n) % self.pool.shape[0]
        self.i += n
        return self.pool[idx.to(DEV)], None


@pytest.fixture(scope='module')
def net():
    from genesis_amd import fid
    return fid.FIDInception.from_state_dict(FR.random_state_dict(fid.expected_shapes(), 7), DEV)


@pytest.fixture(scope='module')
def images():
    real = torch.rand(40, 3, 32, 32, generator=torch.Generator().manual_seed(8)).to(DEV)
    pool = torch.rand(40, 3, 32, 32, generator=torch.Generator().manual_seed(10)).to(DEV)
    return real, pool


def test_from_model_matches_fid_from_model_and_the_public_functions(net, images):
    from genesis_amd import fid
    from genesis_amd import sample_quality as SQ
    real, pool = images
    kw = dict(batch_size=10, num_images=35, weights=net)                    # the first 30 of each set are used
    model = _PoolModel(pool).train()
    out = SQ.sample_quality_from_model(model, _Loader(real, 10), kid_subsets=4, kid_subset_size=20, seed=3, **kw)
    assert model.training
    assert sorted(out) == ['coverage', 'density', 'fid', 'kid', 'kid_std', 'num_fake', 'num_real', 'precision', 'recall']
    assert out['num_real'] == 30 and out['num_fake'] == 30
    assert out['fid'] == fid.fid_from_model(_PoolModel(pool), _Loader(real, 10), **kw)           # bit for bit
    fr, ff = net.features(real[:30]), net.features(pool[:30])
    want = SQ.sample_quality(fr, ff, kid_subsets=4, kid_subset_size=20, seed=3)
    assert want == {k: out[k] for k in want}
    assert (out['precision'], out['recall']) == SQ.precision_recall(fr, ff, 3)
    assert (out['density'], out['coverage']) == SQ.density_coverage(fr, ff, 5)
    assert (out['kid'], out['kid_std']) == SQ.kid(fr, ff, 4, 20, 3)


def test_from_model_does_not_depend_on_the_batch_size(net, images):
    from genesis_amd import sample_quality as SQ
    real, pool = images
    outs = [SQ.sample_quality_from_model(_PoolModel(pool), _Loader(real, 10), batch_size=bs, num_images=35, feat_dim=192,
                                         kid_subsets=3, kid_subset_size=1000, weights=net) for bs in (5, 7)]
    assert outs[0] == outs[1], outs
    assert outs[0]['num_real'] == 35 and all(np.isfinite(v) for v in outs[0].values())
