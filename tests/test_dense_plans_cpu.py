"""The case tables of tests/test_dense_plans_gpu.py against the host decisions of genesis_amd/csrc/gx_dense.hip restated in
Python, and against a written enumeration of the classes those decisions can produce -- all without a GPU.

Every row DECLARES the class it is meant to reach (workgroup size, vectorisation flags and what turns each off, launch kind, mask,
bias-gradient copies, accumulate bits, ragged axes, chunk plan, grids); mirror_* below derive the class again from the row's sizes,
row strides and element offsets, so a typo in a table is found here and not on the GPU.  The tables must hold the rows the plan
names and cover the enumeration, so a deleted or re-pointed row fails here.  The exact-operand generator is checked on the
reference alone: fp32 and fp64 CPU results agree bit for bit for every row, and every mask source holds zeros, negatives and
positives."""
import pytest
import torch

import genesis_amd.hip_ops  # noqa: F401  (a broken import is an error here, not a skip of the module below)
from genesis_amd import _lib
from tests import test_dense_plans_gpu as T

ROW_COUNTS = {'fwd': 12, 'fwd_cases': 72, 'bwd': 28, 'nn': 8, 'seq': 5, 'lstm': 5, 'cell': 3, 'refusals': 14}


def ceil_div(a, b):
    return -(-a // b)


# ---- the dispatch restated (gx_dense.hip, the extern "C" block)
def mirror_threads(Kc):                              # dense_threads
    return 1024 if Kc >= 1024 else 256


def mirror_fwd_vec(K, ldx, x_start, w_start):
    """gx_linear_fwd_ld: (vec_w, vec_x, why vec_w is off, why vec_x is off); *_start: element offset inside a 16-byte aligned
    allocation."""
    w_why = 'K%4' if K % 4 else 'w_ptr' if w_start % 4 else None
    x_why = 'vec_w' if w_why else 'ldx%4' if ldx % 4 else 'x_ptr' if x_start % 4 else None
    return int(w_why is None), int(x_why is None), w_why, x_why


def mirror_bwd_vec(N, ldg, g_start, y_start, mask):
    """gx_linear_bwd_ex: (vec, the first condition that turns it off)."""
    why = 'N%4' if N % 4 else 'ldg%4' if ldg % 4 else 'g_ptr' if g_start % 4 else 'y_ptr' if (mask and y_start % 4) else None
    return int(why is None), why


def mirror_bwd_launch(need_dx, need_dw, M, N, K):
    """-> [(kind, grid, threads)] in launch order."""
    if need_dx and need_dw:
        return [('pair', (ceil_div(K, 16), ceil_div(M, 16) + ceil_div(N, 16)), mirror_threads(max(M, N)))]
    out = []
    if need_dx:
        out.append(('dx', (ceil_div(K, 16), ceil_div(M, 16)), mirror_threads(N)))
    if need_dw:
        out.append(('dw', (ceil_div(K, 16), ceil_div(N, 16)), mirror_threads(M)))
    return out


def mirror_nn(M, K, N):
    tiles = ceil_div(N, 64)
    nchunk = min(tiles, 128)                          # matmul_nn_chunks
    cols = ceil_div(ceil_div(N, nchunk), 64) * 64
    used = ceil_div(N, cols)
    return dict(plan=(nchunk, cols, used), fwd_grid=(ceil_div(M, 8), ceil_div(N, 1024)), dw_grid=(ceil_div(K, 16), ceil_div(N, 256)),
                dx_grid=(used, ceil_div(M, 32), ceil_div(K, 64)))


def mirror_lstm(B, H):
    """-> (grid, steps one whole-sequence launch takes)."""
    if B <= 0 or H <= 0 or H % 16:
        return None, 0
    grid = (H // 16, ceil_div(B, 16))
    return grid, 16 if grid[0] * grid[1] <= 128 else 0


def ragged(**axes):
    return ''.join(k for k, v in axes.items() if v % 16)


def contraction(row):
    """[(the contraction length, may it be vectorised)] of the launches a backward row takes."""
    return {'pair': [(row['N'], True), (row['M'], False)], 'dx': [(row['N'], True)], 'dw': [(row['M'], False)]}[row['kind']]


# ---- every row's declared class is what the restated rules give
@pytest.mark.parametrize('row', T.FWD_ROWS, ids=lambda r: r['id'])
def test_forward_rows_declare_what_the_dispatch_derives(row):
    M, N, K = row['M'], row['N'], row['K']
    ldx = K + row['x_pad']
    got = mirror_fwd_vec(K, ldx, T.embed_start(ldx, row['x_off']), T.embed_start(K, row['w_off']))
    assert got == (row['vec_w'], row['vec_x'], row['w_why'], row['x_why'])
    assert mirror_threads(K) == row['threads']
    assert ragged(M=M, N=N, K=K) == row['ragged']
    assert (K % (row['threads'] // 4) != 0) == row['tail']            # 16 contraction indices per wave and step
    assert T.embed_start(N + row['y_pad'], 0) % 4 == 0
    assert set(row['combos']) <= set(T.ALL6)


@pytest.mark.parametrize('row', T.BWD_ROWS, ids=lambda r: r['id'])
def test_backward_rows_declare_what_the_dispatch_derives(row):
    M, N, K = row['M'], row['N'], row['K']
    ldg = N + row['g_pad']
    assert mirror_bwd_vec(N, ldg, T.embed_start(ldg, row['g_off']), T.embed_start(ldg, row['y_off']), row['mask']) == (row['vec'], row['why'])
    launches = mirror_bwd_launch(row['kind'] != 'dw', row['kind'] != 'dx', M, N, K)
    assert len(launches) == 1 and launches[0][0] == row['kind'] and launches[0][2] == row['threads']
    assert ragged(M=M, N=N, K=K) == row['ragged']
    assert row['mask'] in T.ACTS and row['db'] in ('none', 'db', 'db2') and row['acc'] in (0, 1, 2, 3)
    assert row['kind'] != 'dx' or row['db'] == 'none'                  # db is produced together with dw
    assert not row['acc'] & 1 or (row['kind'] != 'dw' and row['dx_pad'] is not None)
    assert not row['y_off'] or row['mask']
    if row['acc']:
        assert K >= 32                                                 # more than one column tile: only the first may write db


@pytest.mark.parametrize('row', T.NN_ROWS, ids=lambda r: r['id'])
def test_matmul_rows_declare_what_the_dispatch_derives(row):
    M, K, N = row['M'], row['K'], row['N']
    m = mirror_nn(M, K, N)
    assert {k: row[k] for k in m} == m
    nchunk, cols, used = m['plan']
    assert used <= nchunk and cols % 64 == 0 and N % 4 == 0
    assert _lib.query('gx_matmul_nn_bwd_ws_bytes', M, N, K) == nchunk * M * K * 4
    assert T.embed_start(K, row['x_off']) % 4 == row['x_off']


def test_matmul_workspace_of_a_non_positive_size_is_zero():
    for args in ((0, 8, 4), (3, 0, 4), (3, 8, 0), (-1, 8, 4)):
        assert _lib.query('gx_matmul_nn_bwd_ws_bytes', *args) == 0


@pytest.mark.parametrize('row', T.SEQ_ROWS, ids=lambda r: '%(T)dx%(B)dx%(H)d' % r)
def test_sequence_rows_declare_what_the_dispatch_derives(row):
    grid, cap = mirror_lstm(row['B'], row['H'])
    assert grid == row['grid']
    assert _lib.query('gx_lstm_seq_max_steps', row['B'], row['H']) == cap
    assert row['path'] == ('seq' if 1 < row['T'] <= cap else 'step')          # LSTMFn / ARPriorKLFn: 1 < T <= lstm_seq_steps(B, H)
    if row['path'] == 'seq':
        assert grid[0] * grid[1] <= 64                 # no sequence launch above the grids the suite already runs


def test_lstm_capacity_boundaries():
    q = lambda B, H: _lib.query('gx_lstm_seq_max_steps', B, H)  # noqa: E731
    assert q(128, 256) == 16 and q(129, 256) == 0              # 16 x 8 = 128 workgroups; 16 x 9 = 144
    assert q(2048, 16) == 16 and q(2049, 16) == 0
    assert q(2, 24) == 0 and q(2, 8) == 0 and q(0, 16) == 0 and q(2, 0) == 0
    assert _lib.query('gx_lstm_seq_ws_bytes') == 64
    for B, H in ((128, 256), (129, 256), (2048, 16), (2049, 16), (2, 24), (33, 48), (16, 80)):
        assert q(B, H) == mirror_lstm(B, H)[1]


# ---- the tables hold the rows the plan names and cover the enumeration
def has(rows, **want):
    return any(all(r[k] == v for k, v in want.items()) for r in rows)


def test_table_sizes():
    assert len(T.FWD_ROWS) == ROW_COUNTS['fwd'] and len(T.FWD_CASES) == ROW_COUNTS['fwd_cases']
    assert len(T.BWD_ROWS) == ROW_COUNTS['bwd'] and len(T.NN_ROWS) == ROW_COUNTS['nn'] and len(T.SEQ_ROWS) == ROW_COUNTS['seq']
    assert len(T.LSTM_SHAPES) == ROW_COUNTS['lstm'] and len(T.CELL_SHAPES) == ROW_COUNTS['cell']
    assert len(T.REFUSALS) == ROW_COUNTS['refusals']
    for rows in (T.FWD_ROWS, T.BWD_ROWS, T.NN_ROWS):
        assert len({r['id'] for r in rows}) == len(rows)


def test_forward_table_covers_the_enumeration():
    R = T.FWD_ROWS
    for M, N, K, extra in ((3, 5, 1028, dict(threads=1024, vec_w=1, vec_x=1, tail=True)), (3, 5, 1030, dict(threads=1024, vec_w=0)),
                           (17, 33, 20, dict(vec_w=1, vec_x=1)), (7, 5, 3, {}), (1, 1, 1, {}), (16, 16, 16, {}), (33, 17, 70, {})):
        assert has(R, M=M, N=N, K=K, **extra), (M, N, K)
    assert has(R, vec_w=1, vec_x=0, x_why='x_ptr') and has(R, vec_w=1, vec_x=0, x_why='ldx%4')
    assert any(r['w_why'] == 'w_ptr' and r['K'] % 4 == 0 for r in R)
    assert has(R, w_why='K%4') and has(R, vec_w=1, vec_x=1)
    assert any(r['threads'] == 1024 and r['tail'] for r in R)                          # 1024 threads x ragged contraction
    assert any(r['threads'] == 1024 and r['tail'] and not r['vec_w'] for r in R)       # ... on the scalar path too
    assert any(r['vec_w'] and r['vec_x'] and r['K'] % 16 for r in R)                   # vec on x contraction % 16 != 0
    assert any(r['K'] < 16 for r in R)                                                 # shorter than one wave's first step
    assert any(r['x_pad'] for r in R) and any(r['y_pad'] for r in R)
    for threads in (256, 1024):
        seen = {c for r in R if r['threads'] == threads for c in r['combos']}
        assert {a for a, _ in seen} == set(T.ACTS) and {b for _, b in seen} == {True, False}, threads
    flt = [r for r in R if r['flt']]
    assert {r['threads'] for r in flt} == {256, 1024}
    for r in R:
        assert r['M'] * r['K'] <= 33 * 1280 and r['N'] <= 33


def test_backward_table_covers_the_enumeration():
    R = T.BWD_ROWS
    assert has(R, kind='pair', M=3, N=1028, K=5) and has(R, kind='pair', M=1030, N=5, K=3, vec=0)
    assert has(R, kind='pair', M=17, N=36, K=20, vec=1) and has(R, kind='pair', M=7, N=5, K=3)
    assert has(R, kind='dx', N=1028) and has(R, kind='dx', N=20) and has(R, kind='dw', M=1030) and has(R, kind='dw', M=7)
    for why in (None, 'N%4', 'ldg%4', 'g_ptr', 'y_ptr'):
        assert has(R, why=why), why
    assert any(r['why'] == 'y_ptr' and r['g_off'] == 0 and r['mask'] for r in R)        # y unaligned, g aligned
    for kind in ('pair', 'dx', 'dw'):
        for mask in T.ACTS:
            assert has(R, kind=kind, mask=mask), (kind, mask)
        assert {r['threads'] for r in R if r['kind'] == kind} == {256, 1024}, kind
        assert {r['threads'] for r in R if r['kind'] == kind and r['flt']} == {256, 1024}, kind
    for db in ('none', 'db', 'db2'):
        assert has(R, kind='pair', db=db) and has(R, kind='dw', db=db), db
    # accumulate x more than one column tile.  The separate launches take their own bit each: a dw-only launch has no dx, so bit 1
    # cannot reach it; a dx-only launch with both bits set must leave out_dw alone
    assert {r['acc'] for r in R if r['kind'] == 'pair' and r['K'] >= 32} == {0, 1, 2, 3}
    assert {r['acc'] for r in R if r['kind'] == 'dx' and r['K'] >= 32} == {0, 1, 3}
    assert {r['acc'] for r in R if r['kind'] == 'dw' and r['K'] >= 32} == {0, 2}
    assert any(r['acc'] & 2 and r['db'] == 'db2' and r['K'] >= 32 for r in R)
    assert any(r['mask'] == 'elu' and r['acc'] & 1 for r in R) and any(r['mask'] == 'elu' and r['acc'] & 2 for r in R)
    assert any(r['kind'] == 'dx' and not r['acc'] & 1 and r['dx_pad'] for r in R)      # out_dx into a row-strided destination
    assert any(r['kind'] == 'pair' and not r['acc'] & 1 and r['dx_pad'] for r in R)
    assert any(r['threads'] == 1024 and any(kc >= 1024 and kc % 256 for kc, _ in contraction(r)) for r in R)
    assert any(r['vec'] and r['N'] % 16 for r in R if r['kind'] != 'dw')               # vec on x contraction % 16 != 0
    assert any(r['threads'] == 1024 and min(kc for kc, _ in contraction(r)) < 16 for r in R if r['kind'] == 'pair')
    assert any(r['x_pad'] for r in R) and any(r['g_pad'] and r['mask'] for r in R)
    for r in R:
        assert max(r['M'], r['N'], r['K']) <= 1030


def test_matmul_table_covers_the_enumeration():
    R = T.NN_ROWS
    for M, K, N, plan in ((3, 5, 8196, (128, 128, 65)), (33, 70, 260, (5, 64, 5)), (3, 8, 4, (1, 64, 1)), (9, 17, 1028, (17, 64, 17)),
                          (2, 3, 16388, (128, 192, 86))):
        assert has(R, M=M, K=K, N=N, plan=plan), (M, K, N)
    assert any(r['plan'][2] < r['plan'][0] for r in R)                                  # used < nchunk
    assert has(R, need_dx=False) and has(R, need_dw=False) and has(R, out_dw=True) and has(R, x_off=1)
    assert any(r['N'] % 64 == 4 for r in R) and any(r['dx_grid'][1] > 1 and r['dx_grid'][2] > 1 for r in R)
    assert any(r['fwd_grid'][1] == 2 and r['N'] - 1024 == 4 for r in R)                 # second column block, one live thread
    assert any(4 * T.math.isqrt(r['N'] // 4) ** 2 == r['N'] and r['N'] > 4 for r in R) and has(R, N=4)


def test_lstm_tables_hold_the_named_shapes():
    assert T.LSTM_SHAPES == [(3, 1, 5, 48), (2, 16, 8, 80), (3, 33, 7, 16), (1, 17, 4, 48), (17, 2, 3, 16)]
    assert T.CELL_SHAPES == [(5, 7, 48), (16, 20, 80), (33, 3, 16)]
    assert [(r['T'], r['B'], r['H'], r['path']) for r in T.SEQ_ROWS] == [(3, 33, 48, 'seq'), (16, 2, 16, 'seq'), (1, 3, 16, 'step'),
                                                                        (17, 2, 16, 'step'), (2, 129, 256, 'step')]
    assert {h % 64 for _, _, _, h in T.LSTM_SHAPES} >= {48, 16}                         # waves with unequal work
    want = {'matmul_nn_fwd w+1', 'matmul_nn_fwd N=6', 'matmul_nn_bwd w+1', 'matmul_nn_bwd g+1', 'matmul_nn_bwd dw+1',
            'matmul_nn_bwd N=6', 'lstm_seq_fwd T=17', 'lstm_seq_bwd T=17', 'lstm_seq_fwd B=129 H=256', 'lstm_seq_bwd B=129 H=256',
            'lstm_seq_fwd w_hh+1', 'lstm_step_fwd w_hh+1', 'lstm_step_fwd h_prev without c_prev', 'lstm_step_bwd no incoming gradient'}
    assert set(T.REFUSALS) == want
    for name, (_, entry) in T.REFUSALS.items():
        assert entry == 'gx_' + name.split()[0]


# ---- the premise of the exact rows, on the reference alone
def same(a32, b64):
    return torch.equal(a32.double(), b64)


@pytest.mark.parametrize('rid,act,bias', T.FWD_CASES)
def test_exact_forward_operands_make_fp32_equal_fp64(rid, act, bias):
    row = T.row_by_id(T.FWD_ROWS, rid)
    ops = T.fwd_operands(row, bias)
    for t in (ops['x'], ops['w']) + ((ops['b'],) if bias else ()):
        assert bool(((t == t.round()) & (t.abs() <= 3)).all())
    pre32, out32 = T.fwd_reference(ops, act, torch.float32)
    pre64, out64 = T.fwd_reference(ops, act)
    assert same(pre32, pre64) and float(pre64.abs().max()) < 2 ** 24
    keep = pre64 > 0 if act == 'elu' else torch.ones_like(pre64, dtype=torch.bool)        # (ELU's negative side: expm1)
    assert same(out32[keep], out64[keep])
    T.lossless(out64[keep])


@pytest.mark.parametrize('row', T.BWD_ROWS, ids=lambda r: r['id'])
def test_exact_backward_operands_make_fp32_equal_fp64(row):
    ops = T.bwd_operands(row)
    for k, t in ops.items():
        if t is not None and k != 'y':
            assert bool(((t == t.round()) & (t.abs() <= 3)).all()), k
    if row['mask']:
        y = ops['y']
        assert bool(((y * 8 == (y * 8).round()) & (y >= -1) & (y <= 2)).all())
        assert bool((y == 0).any()) and bool((y < 0).any()) and bool((y > 0).any()) and bool((y == -1).any())
    r32, r64 = T.bwd_reference(row, ops, torch.float32), T.bwd_reference(row, ops)
    for k in ('dx', 'dw', 'db', 'db2'):
        assert same(r32[k], r64[k]), k
        T.lossless(r64[k])
        assert float(r64[k].abs().max()) * 8 < 2 ** 24                 # multiples of 1/8: every partial sum is representable


@pytest.mark.parametrize('row', T.NN_ROWS, ids=lambda r: r['id'])
def test_exact_matmul_operands_make_fp32_equal_fp64(row):
    ops = T.nn_operands(row)
    r32, r64 = T.nn_reference(ops, torch.float32), T.nn_reference(ops)
    for k in ('y', 'dx', 'dw'):
        assert same(r32[k], r64[k]), k
        T.lossless(r64[k])
    # the largest sum any order of partial sums could reach stays representable
    assert 9 * max(row['M'], row['K'], row['N']) < 2 ** 24
