"""No-GPU checks of the sample-quality metrics (genesis_amd/sample_quality.py, gx_manifold.hip): the fp64 restatement on
closed-form cases, and the boundary: the header declares the entry points, every argument check fires with its message
through the C ABI before any device call, the KID index draws follow the documented order, host tensors are refused."""
import ctypes

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from tests import sample_quality_restatement as SR

P = ctypes.c_void_p(64)          # a non-null, 16-byte aligned stand-in: every call below stops in host validation


# ---- the restatement on closed-form cases ----
def test_identical_sets():
    """F identical to R: every f_j sits on r_j (d2 = 0 <= rho), so precision = recall = coverage = 1.  The unbiased MMD^2
    of a set against itself (m = N, both subsets the whole set) is (2 / m) (mean off-diagonal kappa - mean diagonal kappa),
    which is not 0 in general; it is 0 to round-off when all rows are one vector, where every comparison is also an exact tie."""
    R, _ = SR.make_features(11, 23, 5, 16)
    assert SR.precision_recall(R, R.copy(), 3) == (1.0, 1.0)
    assert SR.density_coverage(R, R.copy(), 5)[1] == 1.0
    m = len(R)
    idx = np.arange(m)[None, :]
    sums = SR.kid_sums(R, R, idx, idx)
    kappa = (R.astype(np.float64) @ R.astype(np.float64).T / 16 + 1.0) ** 3
    off = (kappa.sum() - np.trace(kappa)) / (m * (m - 1))
    want = 2.0 / m * (off - np.trace(kappa) / m)
    got = SR.kid_from_sums(sums, m)[0]
    assert abs(got - want) <= 1e-12 * np.abs(kappa).max()
    C = np.tile(np.float32([0.5, -1.25, 2.0, 0.75]), (9, 1))
    assert SR.precision_recall(C, C, 3) == (1.0, 1.0) and SR.density_coverage(C, C, 5) == (9 / 5.0 * 1.0, 1.0)
    mean, std = SR.kid(C, C, num_subsets=4, max_subset_size=6, seed=3)
    scale = (float(C[0].astype(np.float64) @ C[0].astype(np.float64)) / 4 + 1.0) ** 3
    assert abs(mean) <= 1e-14 * scale and std <= 1e-14 * scale


def test_two_far_apart_clusters():
    rng = np.random.default_rng(0)
    R = rng.standard_normal((12, 8)).astype(np.float32)
    F = (rng.standard_normal((10, 8)) + 1000.0).astype(np.float32)
    assert SR.precision_recall(R, F, 3) == (0.0, 0.0)
    assert SR.density_coverage(R, F, 5) == (0.0, 0.0)


R3 = np.float32([[0, 0, 0, 0], [1, 0, 0, 0], [0, 2, 0, 0]])
F3 = np.float32([[0, 0, 0, 0], [3, 0, 0, 0], [0, 2, 0, 0]])


def test_hand_computed_example():
    """D = 4, N = 3.  d2 among R: (0,1) = 1, (0,2) = 4, (1,2) = 5.  f0 = r0, f1 = (3,0,0,0), f2 = r2."""
    assert SR.sqdist(R3, R3).tolist() == [[0, 1, 4], [1, 0, 5], [4, 5, 0]]
    assert SR.knn_radii(R3, 1).tolist() == [1, 1, 4]
    assert SR.knn_radii(R3, 2).tolist() == [4, 5, 5]
    # d2(f, r): f0 -> (0, 1, 4), f1 -> (9, 4, 13), f2 -> (4, 5, 0) against the k = 1 radii (1, 1, 4): f0's 1 <= 1 and 4 <= 4 are ties
    hits, covered = SR.manifold_counts(F3, R3, SR.knn_radii(R3, 1))
    assert hits.tolist() == [3, 0, 1] and covered.tolist() == [1, 1, 1]
    assert SR.precision_recall(R3, F3, 1)[0] == 2 / 3.0
    assert SR.density_coverage(R3, F3, 1) == (4 / 3.0, 1.0)
    # kappa = (x . y / 4 + 1)^3: all off-diagonal dot products inside F and inside R are 0 -> 6 each; across:
    # f0 . r = 0 (3 x 1), f1 . r = (0, 3, 0) -> 1 + 1.75^3 + 1, f2 . r = (0, 0, 4) -> 1 + 1 + 2^3
    idx = np.arange(3)[None, :]
    assert SR.kid_sums(R3, F3, idx, idx).tolist() == [[6.0, 6.0, 3 + (2 + 1.75 ** 3) + 10]]
    assert SR.kid_from_sums(np.float64([[6.0, 6.0, 20.359375]]), 3)[0] == 12 / 6.0 - 2 * 20.359375 / 9


# ---- the boundary ----
def test_header_declares_the_entry_points():
    decls = _lib.declarations()
    want = {'gx_knn_radii': 8, 'gx_knn_radii_ws_bytes': 2, 'gx_manifold_counts': 9, 'gx_kid_sums': 13,
            'gx_kid_sums_ws_bytes': 2}
    for name, nargs in want.items():
        assert name in decls, name
        assert len(decls[name][1]) == nargs, (name, decls[name])
        assert decls[name][0] == ('size_t' if name.endswith('_ws_bytes') else 'int')
    assert _lib.query('gx_knn_radii_ws_bytes', 130, 3) == 3 * 3 * 130 * 8          # [tiles = 3][k][N] doubles
    assert _lib.query('gx_kid_sums_ws_bytes', 100, 3) == 3 * 3 * 2 * 2 * 8          # [S][3][tiles^2] doubles
    assert _lib.query('gx_knn_radii_ws_bytes', 130, 9) == 0 and _lib.query('gx_kid_sums_ws_bytes', 1, 3) == 0


BIG = 1 << 30
KNN_BAD = [
    ((P, 5, 64, 5, P, P, BIG, None), r'k = 5 needs at least k \+ 1 rows, have N = 5'),         # k > N - 1
    ((P, 20, 64, 9, P, P, BIG, None), r'k must be in \[1, 8\], not 9'),
    ((P, 20, 64, 0, P, P, BIG, None), r'k must be in \[1, 8\], not 0'),
    ((P, 20, 6, 3, P, P, BIG, None), r'D must be a multiple of 4 in \[4, 8192\], not 6'),
    ((P, 20, 8196, 3, P, P, BIG, None), r'D must be a multiple of 4 in \[4, 8192\], not 8196'),
    ((None, 20, 64, 3, P, P, BIG, None), 'gx_knn_radii: null pointer'),
    ((P, 20, 64, 3, None, P, BIG, None), 'gx_knn_radii: null pointer'),
    ((P, 20, 64, 3, P, None, BIG, None), 'gx_knn_radii: null pointer'),
    ((P, 20, 64, 3, P, P, 20 * 3 * 8 - 1, None), r'workspace too small \(479 bytes, need 480\)'),
    ((ctypes.c_void_p(68), 20, 64, 3, P, P, BIG, None), '16-byte aligned'),
]
COUNTS_BAD = [
    ((P, 7, P, 9, 6, P, P, P, None), r'D must be a multiple of 4 in \[4, 8192\], not 6'),
    ((P, 7, None, 9, 64, P, P, P, None), 'gx_manifold_counts: null pointer'),
    ((P, 7, P, 9, 64, None, P, P, None), 'gx_manifold_counts: null pointer'),
    ((P, 7, P, 9, 64, P, None, P, None), 'gx_manifold_counts: null pointer'),
    ((P, 7, P, 9, 64, P, P, None, None), 'gx_manifold_counts: null pointer'),
    ((P, 0, P, 9, 64, P, P, P, None), r'M and N must be in \[1, 2097152\], not 0, 9'),
    ((P, 7, P, 0, 64, P, P, P, None), r'M and N must be in \[1, 2097152\], not 7, 0'),
]
KID_BAD = [
    ((P, 9, P, P, 9, P, 5, 6, 2, P, P, BIG, None), r'D must be a multiple of 4 in \[4, 8192\], not 6'),
    ((P, 9, None, P, 9, P, 5, 64, 2, P, P, BIG, None), 'gx_kid_sums: null pointer'),
    ((P, 9, P, P, 9, P, 5, 64, 2, None, P, BIG, None), 'gx_kid_sums: null pointer'),
    ((P, 9, P, P, 9, P, 1, 64, 2, P, P, BIG, None), r'm must be in \[2, 65536\], not 1'),
    ((P, 9, P, P, 9, P, 5, 64, 0, P, P, BIG, None), r'S must be in \[1, 21845\], not 0'),
    ((P, 0, P, P, 9, P, 5, 64, 2, P, P, BIG, None), 'NX and NY must be at least 1'),
    ((P, 9, P, P, 9, P, 5, 64, 2, P, P, 2 * 3 * 8 - 1, None), r'workspace too small \(47 bytes, need 48\)'),
]


@pytest.mark.parametrize('name,args,msg', [('gx_knn_radii', a, m) for a, m in KNN_BAD] +
                         [('gx_manifold_counts', a, m) for a, m in COUNTS_BAD] + [('gx_kid_sums', a, m) for a, m in KID_BAD])
def test_argument_checks_fire_without_a_gpu(name, args, msg):
    with pytest.raises(_lib.GenesisHipError, match=msg):
        _lib.call(name, *args)


def test_kid_index_draws_follow_the_documented_order():
    from genesis_amd import sample_quality as SQ
    N, M, m, S, seed = 37, 29, 11, 4, 5
    ix, iy = SQ.kid_indices(N, M, m, S, seed)
    assert ix.shape == (S, m) and iy.shape == (S, m) and ix.dtype == np.int32 and iy.dtype == np.int32
    rng = np.random.default_rng(seed)
    for s in range(S):                       # subset 0 ix, subset 0 iy, subset 1 ix, ...
        assert ix[s].tolist() == rng.choice(M, m, replace=False).tolist()
        assert iy[s].tolist() == rng.choice(N, m, replace=False).tolist()
        assert len(set(ix[s].tolist())) == m and len(set(iy[s].tolist())) == m
    rx, ry = SR.kid_indices(N, M, m, S, seed)
    assert np.array_equal(ix, rx) and np.array_equal(iy, ry)
    assert ix.max() < M and iy.max() < N and iy.max() >= M          # ix indexes the generated rows, iy the real ones


def test_python_functions_refuse_host_tensors():
    from genesis_amd import sample_quality as SQ
    a, b = torch.rand(12, 8), torch.rand(10, 8)
    rad = torch.rand(12, dtype=torch.float64)
    idx = torch.zeros(2, 4, dtype=torch.int32)
    for fn, args in ((SQ.knn_radii, (a, 3)), (SQ.manifold_counts, (b, a, rad)), (SQ.precision_recall, (a, b)),
                     (SQ.density_coverage, (a, b)), (SQ.kid, (a, b)), (SQ.kid_sums, (a, b, idx, idx)),
                     (SQ.sample_quality, (a, b))):
        with pytest.raises(_lib.GenesisHipError, match='no CPU path'):
            fn(*args)
    with pytest.raises(_lib.GenesisHipError, match='lives on the HIP device'):
        SQ.FeatureBank(8, 16, 'cpu')
