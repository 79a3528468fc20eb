"""The case tables of tests/test_igemm_plans_gpu.py against the host planners of gx_igemm.hip restated in Python, a written
enumeration of the classes and tails those planners can produce, the FastDiv magic numbers, and the refusals the host decides --
all without a GPU.

Every declared record is recomputed here from the row's shape alone (fwd_splits, wgrad_splits, fwd_small_ok, the `few` rule, the
stride-2 weight gradient's slab count): a row whose declaration the restated planner does not reproduce fails here, before a GPU
is asked; the GPU file then asserts that the launch recorded the same.  The tables must cover the enumeration and hold the rows
they were asked to hold, so a deleted or re-pointed row fails on the CPU."""
import re

import numpy as np
import pytest

from genesis_amd import hip_ops
from genesis_amd._lib import GenesisHipError
from tests import test_igemm_plans_gpu as I
from tests.test_igemm_plans_gpu import cd

BM, BN, BK = 64, 128, 16


# ===================================================================================================== the planners, restated
def fwd_splits(M, Ncols, K):
    """gx_igemm.hip fwd_splits: only where the tiles leave most of the chip idle and the contraction is long enough."""
    tiles, nchunks = cd(Ncols, BN) * cd(M, BM), cd(K, BK)
    if tiles >= 128 or nchunks < 8:
        return 1
    return max(1, min(cd(256, tiles), nchunks // 4, 16))


def wgrad_splits(M, Ncols, K):
    return max(1, min(cd(768, cd(M, BM) * cd(Ncols, BN)), cd(K, BK), 256))


def fwd_small_ok(N, Cin, Cout, H, W, k, s, p):
    if k != 3 or s != 2 or p != 1 or H % 2 or W % 2 or Cin > 64:
        return False
    q = cd(N * (H // 2) * (W // 2), 256)
    return cd(Cout, 8) * q >= 512 and q <= 65535


def plan_fwd(dims, workspace=True):
    """gx_conv2d_direct_fwd_ws: the split where fwd_splits says so and a workspace is there, else gx_conv2d_direct_fwd: the
    stride-2 kernel where fwd_small_ok says so, else one launch of the implicit GEMM."""
    N, Cin, Cout, H, W, k, s, p = dims
    M, Ncols, K = I.generic_shape(dims)[2]['f']
    ns, nchunks = fwd_splits(M, Ncols, K), cd(K, BK)
    if ns > 1 and workspace:
        return I.FW(cd(Ncols, BN), cd(M, BM), ns, cd(nchunks, ns))
    if fwd_small_ok(*dims):
        return I.S2F(cd(Cout, 8), cd(N * (H // 2) * (W // 2), 256))
    return I.FW(cd(Ncols, BN), cd(M, BM), 1, nchunks)


def plan_dg(dims):
    M, Ncols, K = I.generic_shape(dims)[2]['d']
    return I.DG(cd(Ncols, BN), cd(M, BM), cd(K, BK))


def plan_s2_dg(dims, cin_n):
    """gx_conv3x3s2_dgrad_small_ex: CIB = 2 for cin_n <= 2 else 4; UB = 8 (`few`) below 512 workgroups."""
    N, Cin, Cout, H, W = dims
    cib = 2 if cin_n <= 2 else 4
    gx, gy = cd(cin_n, cib), cd(N * (H // 2) * (W // 2), 256)
    return I.S2D(cib, 8 if gx * gy < 512 else 1, gx, gy)


def s2_wgrad_slabs(dims):
    N, Cin, Cout, H, W = dims
    P = N * (H // 2) * (W // 2)
    return max(1, min(cd(2048, Cin * cd(Cout, 8)), 64, cd(P, 1024)))


# ===================================================================================================== the enumeration
# What the planners above can produce, written out; the tables must cover it.
#   igemm_fwd   one launch or a split (2 .. 16 slabs), each with one or several 64-channel tiles (grid_y); the split even, uneven
#               (the last written slab shorter) or with EMPTY slabs (ceil(nchunks / ns) ns - nchunks >= a whole slab: the kernel
#               must write zeros there); the contraction index divided by k k and k for k = 1 .. 5 (FastDiv: d = 1 the shortcut,
#               2 / 4 / 16 the powers of two whose magic is 0, 3 / 5 / 9 / 25 the general case)
#   igemm_dg    one launch; MODE 1 divides by the stride on three branches (1, 2, other); grid_x a multiple of 8 or not (the XCD
#               map's remainder); input rows the stride leaves without a window
#   wgrad       1 or several slabs (up to ceil(768 / tiles), capped by the chunks), several tiles along either axis
#   s2_fwd      one instantiation (8 output channels per thread); reached only with >= 512 workgroups, after the split's rule
#   s2_dg       CIB in {2, 4} x UB in {1, 8}: four instantiations
#   s2 wgrad    S = 1 .. 64 slabs of the pixel range
REQUIRED_FWD = {('single', 1), ('single', 2), ('split', 1), ('split', 2)}             # (path, grid_y: 1 or several)
REQUIRED_DG_STRIDES = {1, 2, 3}
REQUIRED_K = {1, 2, 3, 4, 5}
REQUIRED_GENERIC_TAILS = {'pad0', 'pad_window', 'rect', 's3', 'f.m_tail', 'f.m_tiles', 'f.n_tail', 'f.n_tiles', 'f.k_tail', 'f.k_lt_wave',
                          'f.straddle', 'f.splitk', 'f.splitk_uneven', 'f.slab_empty', 'd.m_tail', 'd.m_tiles', 'd.n_tail', 'd.n_tiles',
                          'd.k_tail', 'd.straddle', 'd.xcd_rem', 'd.zero_rows', 'w.m_tail', 'w.m_tiles', 'w.n_tail', 'w.n_tiles',
                          'w.k_tail', 'w.splitk'}
REQUIRED_S2_FWD_TAILS = {'co_tail', 'pix_tail', 'straddle', 'rect', 'cin_max', 'exact_512', 'splitk', 'split_over_small'}
REQUIRED_S2_DG = {(4, 1), (2, 1), (4, 8), (2, 8)}                                      # (CIB, UB)
REQUIRED_S2_DG_TAILS = {'ci_tail', 'co_tail_ub', 'partial', 'pix_tail', 'rect', 'straddle', 'one_block'}
REQUIRED_S2_WG_SLABS = {1, 2, 5}
ROWS = {'generic': 12, 's2_fwd': 6, 's2_dg': 9, 's2_wg': 4, 'sylvester': 6, 'refusals': 13}
# the shapes the tables were asked to hold
ASKED_GENERIC = {(2, 3, 5, 7, 11, 1, 1, 0), (2, 5, 3, 6, 10, 2, 2, 0), (1, 4, 6, 9, 13, 3, 3, 1), (2, 3, 4, 8, 5, 4, 2, 1),
                 (1, 2, 3, 4, 6, 3, 1, 3), (9, 2, 5, 14, 12, 3, 2, 0), (3, 4, 8, 12, 44, 3, 2, 1), (2, 3, 70, 9, 7, 3, 2, 1),
                 (1, 70, 3, 6, 6, 3, 1, 1), (1, 16, 130, 6, 10, 3, 1, 1), (1, 21, 8, 6, 6, 5, 1, 2), (1, 40, 8, 4, 4, 5, 2, 2)}
ASKED_S2_FWD = {(1, 3, 60, 256, 256), (5, 3, 60, 116, 116), (1, 2, 58, 128, 512), (1, 64, 60, 256, 256), (1, 16, 128, 126, 128)}
ASKED_S2_DG = {((1, 5, 3, 512, 512), 5, 5, 'small'), ((1, 7, 3, 724, 364), 7, 7, 'small'), ((1, 2, 3, 1024, 512), 2, 2, 'small'),
               ((2, 6, 10, 12, 20), 3, 6, 'small'), ((3, 4, 5, 6, 10), 1, 1, 'lead'), ((3, 4, 5, 6, 10), 1, 1, 'ex'),
               ((3, 4, 5, 6, 10), 1, 2, 'ex'), ((3, 4, 5, 6, 10), 1, 4, 'ex'), ((2, 3, 4, 2, 2), 3, 3, 'small')}
ASKED_S2_WG = {((2, 6, 10, 12, 20), 1), ((3, 3, 9, 34, 62), 2), ((5, 2, 17, 66, 62), 5), ((1, 3, 5, 2, 2), 1)}


def test_no_row_was_removed_and_ids_are_unique():
    tables = {'generic': I.GENERIC_CASES, 's2_fwd': I.S2_FWD_CASES, 's2_dg': I.S2_DG_CASES, 's2_wg': I.S2_WG_CASES,
              'sylvester': I.SYLVESTER_CASES, 'refusals': I.WRAPPER_REFUSALS}
    assert {k: len(v) for k, v in tables.items()} == ROWS
    ids = [r['id'] for r in I.GENERIC_CASES + I.S2_FWD_CASES + I.S2_DG_CASES] + [c[0] for c in I.S2_WG_CASES + I.SYLVESTER_CASES]
    assert len(ids) == len(set(ids))
    assert {r['dims'] for r in I.GENERIC_CASES} == ASKED_GENERIC
    assert ASKED_S2_FWD <= {r['dims'] for r in I.S2_FWD_CASES}
    assert {(r['dims'], r['cin_n'], r['dxc'], r['via']) for r in I.S2_DG_CASES} == ASKED_S2_DG
    assert {(c[1], c[2]) for c in I.S2_WG_CASES} == ASKED_S2_WG
    syl = {(c[1], c[3], c[4], c[2][3:]) for c in I.SYLVESTER_CASES}
    assert {('conv', 2, 0, (6, 10)), ('conv', 2, 0, (5, 7)), ('deconv', 2, 1, (3, 5)), ('conv', 1, 0, (3, 6)), ('deconv', 1, 0, (3, 6))} <= syl
    assert [c for c in I.SYLVESTER_CASES if c[5] is None and c[2][3] & (c[2][3] - 1) == 0 and c[2][4] & (c[2][4] - 1) == 0]


@pytest.mark.parametrize('row', I.GENERIC_CASES, ids=I._ids(I.GENERIC_CASES))
def test_generic_rows_declare_what_the_planners_give(row):
    dims = row['dims']
    assert set(row['fwd']) == set(row['dg']) == set(hip_ops.PLAN_FIELDS)
    assert row['fwd'] == plan_fwd(dims), plan_fwd(dims)
    assert row['dg'] == plan_dg(dims), plan_dg(dims)
    assert row['wsplit'] == wgrad_splits(*I.generic_shape(dims)[2]['w'])
    assert not fwd_small_ok(*dims)
    assert set(row['tails']) == I.generic_tails(dims, row['fwd'], row['dg'], row['wsplit']), sorted(I.generic_tails(dims, row['fwd'], row['dg'], row['wsplit']))
    # (the weight gradient writes every slab its reduce reads: zs == nsplit on every row)
    nchunks = cd(I.generic_shape(dims)[2]['w'][2], BK)
    assert cd(nchunks, cd(nchunks, row['wsplit'])) == row['wsplit']


def test_generic_rows_are_what_their_point_says():
    """The figures the rows were chosen for, from the restated geometry."""
    by = {r['dims']: r for r in I.GENERIC_CASES}
    assert I.generic_shape((2, 3, 5, 7, 11, 1, 1, 0))[2]['f'][2] == 3 and by[(2, 3, 5, 7, 11, 1, 1, 0)]['wsplit'] == 10
    assert (9 + 2 * 1 - 3) % 3 == 2                                                     # the stride-3 row's remainder
    assert I.generic_shape((1, 2, 3, 4, 6, 3, 1, 3))[:2] == (8, 10)                     # pad 3: the output is larger than the input
    assert by[(9, 2, 5, 14, 12, 3, 2, 0)]['dg']['grid_x'] == 12 and by[(9, 2, 5, 14, 12, 3, 2, 0)]['wsplit'] == 17
    assert by[(3, 4, 8, 12, 44, 3, 2, 1)]['dg']['grid_x'] == 13 and by[(3, 4, 8, 12, 44, 3, 2, 1)]['wsplit'] == 25
    r = by[(2, 3, 70, 9, 7, 3, 2, 1)]
    assert r['fwd']['grid_y'] == 2 and 70 % 64 == 6 and I.generic_shape(r['dims'])[2]['d'][2] == 630
    assert by[(1, 70, 3, 6, 6, 3, 1, 1)]['dg']['grid_y'] == 2 and by[(1, 70, 3, 6, 6, 3, 1, 1)]['fwd']['nsplit'] == 10
    r = by[(1, 16, 130, 6, 10, 3, 1, 1)]['fwd']
    assert (r['grid_y'], r['nsplit'], r['chunks_per_split']) == (3, 2, 5) and cd(16 * 9, 16) == 9          # 5 + 4 chunks
    r = by[(1, 21, 8, 6, 6, 5, 1, 2)]['fwd']
    assert (r['nsplit'], r['chunks_per_split']) == (8, 5) and cd(21 * 25, 16) == 33 and 7 * 5 >= 33 > 6 * 5    # slab 7 is empty
    r = by[(1, 40, 8, 4, 4, 5, 2, 2)]['fwd']
    assert (r['nsplit'], r['chunks_per_split']) == (15, 5) and cd(40 * 25, 16) == 63 and 13 * 5 >= 63 > 12 * 5  # slabs 13, 14
    assert I.generic_shape((1, 40, 8, 4, 4, 5, 2, 2))[2]['f'][1] == 4


def test_generic_table_covers_the_enumeration():
    fwd = {('split' if r['fwd']['nsplit'] > 1 else 'single', min(r['fwd']['grid_y'], 2)) for r in I.GENERIC_CASES}
    assert REQUIRED_FWD <= fwd, REQUIRED_FWD - fwd
    assert REQUIRED_DG_STRIDES <= {r['dims'][6] for r in I.GENERIC_CASES}
    assert REQUIRED_K == {r['dims'][5] for r in I.GENERIC_CASES}
    tails = set().union(*[r['tails'] for r in I.GENERIC_CASES])
    assert REQUIRED_GENERIC_TAILS <= tails, REQUIRED_GENERIC_TAILS - tails
    assert {r['act'] for r in I.GENERIC_CASES} == {None, 'relu', 'elu'}
    # bias + activation both in the split's reduce launch and in the single launch's epilogue
    assert {r['act'] for r in I.GENERIC_CASES if r['fwd']['nsplit'] > 1} >= {'relu', 'elu'}
    assert {r['act'] for r in I.GENERIC_CASES if r['fwd']['nsplit'] == 1} >= {'relu', 'elu'}
    assert {r['wsplit'] for r in I.GENERIC_CASES} >= {1, 10, 17, 25}


@pytest.mark.parametrize('row', I.S2_FWD_CASES, ids=I._ids(I.S2_FWD_CASES))
def test_s2_forward_rows_declare_what_the_planners_give(row):
    dims = row['dims'] + (3, 2, 1)
    assert row['plan'] == plan_fwd(dims), plan_fwd(dims)
    if row['plan']['nsplit'] > 1:
        assert row['fallback'] == plan_fwd(dims, workspace=False), plan_fwd(dims, workspace=False)
    else:
        assert row['fallback'] is None and row['plan']['family'] == 's2_fwd' and fwd_small_ok(*dims)
    assert I.small_predicate(row['dims']) == fwd_small_ok(*dims)
    assert set(row['tails']) == I.s2_fwd_tails(row['dims'], row['plan']), sorted(I.s2_fwd_tails(row['dims'], row['plan']))


def test_s2_forward_table_covers_the_enumeration():
    tails = set().union(*[r['tails'] for r in I.S2_FWD_CASES])
    assert REQUIRED_S2_FWD_TAILS <= tails, REQUIRED_S2_FWD_TAILS - tails
    fam = {(r['plan']['family'], r['fallback']['family'] if r['fallback'] else None) for r in I.S2_FWD_CASES}
    assert fam == {('s2_fwd', None), ('igemm_fwd', 'igemm_fwd'), ('igemm_fwd', 's2_fwd')}
    # 126 x 128 -> 128 channels: 16 x 16 = 256 workgroups, so only the split's rule holds; both rules hold at 2048 channels on 32 x 40
    assert not fwd_small_ok(1, 16, 128, 126, 128, 3, 2, 1) and fwd_splits(128, 63 * 64, 144) == 2
    assert fwd_small_ok(1, 16, 2048, 32, 40, 3, 2, 1) and fwd_splits(2048, 320, 144) == 2
    assert {r['plan']['grid_x'] * r['plan']['grid_y'] for r in I.S2_FWD_CASES if r['plan']['family'] == 's2_fwd'} == {512, 528}
    assert max(r['dims'][1] for r in I.S2_FWD_CASES if r['plan']['family'] == 's2_fwd') == 64


@pytest.mark.parametrize('row', I.S2_DG_CASES, ids=I._ids(I.S2_DG_CASES))
def test_s2_data_gradient_rows_declare_what_the_planners_give(row):
    assert row['plan'] == plan_s2_dg(row['dims'], row['cin_n']), plan_s2_dg(row['dims'], row['cin_n'])
    assert set(row['tails']) == I.s2_dg_tails(row, row['plan']), sorted(I.s2_dg_tails(row, row['plan']))
    assert row['cin_n'] <= row['dxc'] and (row['via'] != 'small' or row['dxc'] == row['dims'][1]) and (row['via'] != 'lead' or row['dxc'] == row['cin_n'])


def test_s2_data_gradient_table_covers_the_enumeration():
    assert REQUIRED_S2_DG == {(1 << r['plan']['lG'], r['plan']['nq']) for r in I.S2_DG_CASES}
    tails = set().union(*[r['tails'] for r in I.S2_DG_CASES])
    assert REQUIRED_S2_DG_TAILS <= tails, REQUIRED_S2_DG_TAILS - tails
    assert {r['via'] for r in I.S2_DG_CASES} == {'small', 'ex', 'lead'}
    assert max(r['dims'][0] * r['dims'][1] * r['dims'][3] * r['dims'][4] for r in I.S2_DG_CASES) == 7 * 724 * 364      # the largest tensor


def test_s2_weight_gradient_rows_declare_their_slab_count():
    for rid, dims, S in I.S2_WG_CASES:
        assert S == s2_wgrad_slabs(dims), (rid, s2_wgrad_slabs(dims))
    assert REQUIRED_S2_WG_SLABS <= {c[2] for c in I.S2_WG_CASES}
    assert {c[1][2] % 8 for c in I.S2_WG_CASES} >= {1, 2, 5}            # Cout tails of the 8-channel blocks


# ===================================================================================================== the family list
def test_plan_families_are_the_headers():
    """hip_ops.PLAN_FAMILIES, in order, against the GX_PLAN_* family defines of include/genesis_hip.h: the four gx_igemm.hip
    families are appended after GX_PLAN_SMALLCIN."""
    from genesis_amd import _lib
    assert hip_ops.PLAN_FAMILIES == ('none', 'tap_c3', 'tap_dt', 'tap_dg', 'tap_c5', 'kq_c3', 'kq_dt', 'kq_dg', 'kq_c3h', 'kq_dth', 'kq_dgh',
                                     'kq_c5h', 'wino', 'smallcin', 'igemm_fwd', 'igemm_dg', 's2_fwd', 's2_dg')
    assert hip_ops.PLAN_FAMILIES[-4:] == I.IGEMM_FAMILIES
    text = open(_lib.HEADER_PATH).read()
    fields = ('FIELDS', 'FAMILY', 'FORM', 'LTH', 'LTW', 'LG', 'NQ', 'PIXELS', 'RT_TH', 'RT_TW', 'TILES_H', 'TILES_W', 'GRID_X', 'GRID_Y', 'GRID_Z',
              'NSPLIT', 'CHUNKS', 'NFULL', 'STATS')
    defs = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r'#define GX_PLAN_(\w+) (\d+)', text) if m.group(1) not in fields}
    assert defs == {name: i for i, name in enumerate(hip_ops.PLAN_FAMILIES)}, defs
    assert int(re.search(r'#define GX_PLAN_FIELDS (\d+)', text).group(1)) == len(hip_ops.PLAN_FIELDS) == 18


# ===================================================================================================== FastDiv
def make_fastdiv(d):
    """gx_igemm.hip make_fastdiv: (mul, shift) of the round-up method, the 33-bit magic stored minus 2^32."""
    if d == 1:
        return 0, 0
    s = 0
    while (1 << s) < d:
        s += 1
    m = ((1 << (32 + s)) + d - 1) // d - (1 << 32)
    assert 0 <= m < 1 << 32, (d, m)             # it must fit the unsigned it is stored in
    return m, s


def fdiv(n, d):
    """gx_igemm.hip fdiv on an array of n, in the kernel's 32-bit unsigned arithmetic."""
    if d == 1:
        return n
    mul, shift = make_fastdiv(d)
    n = n.astype(np.uint64)
    t = (n * np.uint64(mul)) >> np.uint64(32)                       # __umulhi
    return ((t + (((n - t) & np.uint64(0xFFFFFFFF)) >> np.uint64(1))) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift - 1)


@pytest.mark.parametrize('d', range(1, 26))
def test_fastdiv_equals_floor_division(d):
    """Every divisor k k and k of k <= 5 (and the small Wo / Ho Wo of the rows) against // : all n below 2^16, every multiple
    boundary m d - 1, m d, m d + 1 near the powers of two up to 2^31, the last values below 2^31, and a seeded sample."""
    top = (1 << 31) - 1
    ns = [np.arange(0, 1 << 16, dtype=np.int64), np.arange(top - (1 << 12), top + 1, dtype=np.int64)]
    for e in range(16, 32):
        base = ((1 << e) // d) * d
        ns.append(np.arange(base - 2 * d - 2, base + 2 * d + 3, dtype=np.int64))
    ns.append(np.random.RandomState(d).randint(0, top, size=200000).astype(np.int64))
    n = np.concatenate(ns)
    n = n[(n >= 0) & (n <= top)]
    assert n.max() == top
    got = fdiv(n, d)
    assert np.array_equal(got.astype(np.int64), n // d), (d, n[got.astype(np.int64) != n // d][:5])
    if d in (2, 4, 8, 16):
        assert make_fastdiv(d)[0] == 0          # a power of two: the magic is exactly 2^32, stored as 0


def test_fastdiv_restatement_is_the_sources():
    """The three lines this file restates, as they stand in gx_igemm.hip."""
    import os.path as osp
    src = open(osp.join(osp.dirname(hip_ops.__file__), 'csrc', 'gx_igemm.hip')).read()
    assert 'const unsigned long long m = ((1ull << (32 + s)) + d - 1) / d - (1ull << 32);' in src
    assert 'return (t + ((n - t) >> 1)) >> (f.shift - 1);' in src
    assert 'if (f.d == 1) return n;' in src
    assert 'if (tiles >= 128 || nchunks < 8) return 1;' in src and 'int nsplit = gx_ceil_div(768, tiles);' in src
    assert 'return wgs >= 512 &&' in src and '< 512;' in src


# ===================================================================================================== refusals on the host
G8 = (2, 3, 5, 8, 6)           # N, Cin, Cout, H, W


def _fwd(dims):
    from genesis_amd import _lib
    _lib.call('gx_conv2d_direct_fwd', None, None, None, 0, None, *dims, None)


def _fwd_ws(dims):
    from genesis_amd import _lib
    _lib.call('gx_conv2d_direct_fwd_ws', None, None, None, 0, None, *dims, None, 0, None)


def _dgrad(dims):
    from genesis_amd import _lib
    _lib.call('gx_conv2d_direct_dgrad', None, None, None, *dims, None)


def _wgrad(dims, nb=0):
    from genesis_amd import _lib
    _lib.call('gx_conv2d_direct_wgrad', None, None, None, *dims, None, nb, None)


def _s2_dgrad(dims, cin_n=1):
    from genesis_amd import _lib
    _lib.call('gx_conv3x3s2_dgrad_small', None, None, None, *dims, cin_n, None)


def _s2_dgrad_ex(dims, cin_n=1, dxc=1):
    from genesis_amd import _lib
    _lib.call('gx_conv3x3s2_dgrad_small_ex', None, None, None, *dims, cin_n, dxc, None)


def _s2_wgrad(dims, nb=0):
    from genesis_amd import _lib
    _lib.call('gx_conv3x3s2_wgrad_small', None, None, None, *dims, None, nb, None)


HOST_REFUSALS = [
    ('fwd-k6', lambda: _fwd(G8 + (6, 1, 3)), 'kernel <= 5x5'),
    ('fwd-ws-k6', lambda: _fwd_ws(G8 + (6, 1, 3)), 'kernel <= 5x5'),
    ('dgrad-k6', lambda: _dgrad(G8 + (6, 1, 3)), 'kernel <= 5x5'),
    ('wgrad-k6', lambda: _wgrad(G8 + (6, 1, 3)), 'kernel <= 5x5'),
    ('fwd-empty-output', lambda: _fwd((2, 3, 5, 3, 6, 5, 1, 0)), 'empty output'),
    ('fwd-ws-empty-output', lambda: _fwd_ws((2, 3, 5, 8, 2, 3, 2, 0)), 'empty output'),
    ('dgrad-empty-output', lambda: _dgrad((2, 3, 5, 3, 6, 5, 1, 0)), 'empty output'),
    ('wgrad-empty-output', lambda: _wgrad((2, 3, 5, 3, 6, 5, 1, 0)), 'empty output'),
    ('fwd-stride-0', lambda: _fwd(G8 + (3, 0, 1)), 'stride >= 1'),
    ('s2-dgrad-odd-h', lambda: _s2_dgrad((2, 3, 5, 7, 6)), 'even H, W'),
    ('s2-dgrad-ex-odd-w', lambda: _s2_dgrad_ex((2, 3, 5, 8, 5)), 'even H, W'),
    ('s2-wgrad-odd-h', lambda: _s2_wgrad((2, 3, 5, 7, 6)), 'even H, W'),
    ('s2-dgrad-cout-342', lambda: _s2_dgrad((2, 3, 342, 8, 6)), 'Cout <= 341'),
    ('s2-dgrad-cin-n-0', lambda: _s2_dgrad((2, 3, 5, 8, 6), 0), '1 <= cin_n <= Cin'),
    ('s2-dgrad-ex-dxc-below-cin-n', lambda: _s2_dgrad_ex((2, 3, 5, 8, 6), 2, 1), 'dx_channels (1) < cin_n (2)'),
    # the weight gradients' workspace, one byte short of what their queries ask for (2 x 5 x 27 and 64 x 5 x 3 x 9 floats)
    ('wgrad-short-workspace', lambda: _wgrad(G8 + (3, 2, 1), 2 * 5 * 27 * 4 - 1), 'workspace too small'),
    ('s2-wgrad-short-workspace', lambda: _s2_wgrad(G8, 64 * 5 * 3 * 9 * 4 - 1), 'workspace too small'),
    # ... and with room enough the same calls reach the check behind it
    ('wgrad-null-pointers', lambda: _wgrad(G8 + (3, 2, 1), 2 * 5 * 27 * 4), 'null pointer'),
    ('s2-wgrad-null-pointers', lambda: _s2_wgrad(G8, 64 * 5 * 3 * 9 * 4), 'null pointer'),
    ('s2-dgrad-cout-341-null-pointers', lambda: _s2_dgrad((2, 3, 341, 8, 6)), 'null pointer'),
    ('fwd-k5-null-pointers', lambda: _fwd(G8 + (5, 1, 2)), 'null pointer'),
]


@pytest.mark.parametrize('rid,call,message', HOST_REFUSALS, ids=[r[0] for r in HOST_REFUSALS])
def test_refusals_raise_without_a_gpu(rid, call, message):
    """The shape and workspace checks of these entry points come before their pointer checks: every pointer is NULL, so a refusal
    that stopped refusing meets the null-pointer check behind it (another message: this test fails), never a launch."""
    before = hip_ops.conv_last_plan()
    with pytest.raises(GenesisHipError, match=re.escape(message)):
        call()
    assert hip_ops.conv_last_plan() == before


def test_workspace_queries():
    from genesis_amd import _lib
    assert _lib.query('gx_conv2d_direct_wgrad_ws_bytes', *G8, 3, 2, 1) == 2 * 5 * 27 * 4
    assert _lib.query('gx_conv3x3s2_wgrad_small_ws_bytes', *G8) == 64 * 5 * 3 * 9 * 4
    assert _lib.query('gx_conv2d_direct_fwd_ws_bytes', *G8, 3, 2, 1) == 0                       # no split: no workspace
    assert _lib.query('gx_conv2d_direct_fwd_ws_bytes', 1, 70, 3, 6, 6, 3, 1, 1) == 10 * 3 * 36 * 4
    for q in ('gx_conv2d_direct_fwd_ws_bytes', 'gx_conv2d_direct_wgrad_ws_bytes'):                # a shape the entry point refuses
        assert _lib.query(q, *G8, 6, 1, 3) == 0 and _lib.query(q, 2, 3, 5, 3, 6, 5, 1, 0) == 0
    for row in I.GENERIC_CASES:
        M, Ncols, _ = I.generic_shape(row['dims'])[2]['w']
        assert _lib.query('gx_conv2d_direct_wgrad_ws_bytes', *row['dims']) == row['wsplit'] * M * Ncols * 4, row['id']
        M, Ncols, _ = I.generic_shape(row['dims'])[2]['f']
        ns = row['fwd']['nsplit']
        assert _lib.query('gx_conv2d_direct_fwd_ws_bytes', *row['dims']) == (ns * M * Ncols * 4 if ns > 1 else 0), row['id']
