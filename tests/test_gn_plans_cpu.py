"""The case tables of tests/test_gn_plans_gpu.py against a written enumeration of the kernels and plans the GroupNorm host
dispatch (genesis_amd/csrc/gx_norm.hip) can pick, the gx_gn_last_plan record before any launch, the input builder's margin
conditions for every row, the refusals the host decides and the dispatch's own answers (gx_gn_fwd_plan / gx_gn_bwd_plan) for
every row and case -- all without a GPU.

The enumeration is derived from the dispatch (cited per block) and written out here; the tables must cover it, so a deleted or
re-pointed row fails on the CPU.  mirror_* restate plan_reg / small_threads / proj_split_ok / the thread choices in Python: every
row's DECLARED plan must be what the mirror derives from its shape, so a typo in a table is found here and not on the GPU."""
import ctypes
import threading

import pytest

from tests import test_gn_plans_gpu as T

# ---- the classes some row must declare
# plan_reg: W % 4 == 0, H W >= 256, cpg a power of two; P doubles until H W / (256 P) <= 8, F = H W / (256 P); U = cpg P units,
# UPW doubles until U / UPW <= 16; refused when UPW F > 8 or UPW > 2.  GX_GN_REG_DISPATCH instantiates exactly these <F, UPW>:
REG_PAIRS = [(1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (2, 2), (4, 2)]
REG_P_OF_F8 = [1, 2, 4, 8, 16]                  # <8, 1> is the only pair that runs with P > 1 (P > 1 needs H W > 2048, so F = 8)
# small_threads: H W < 256, W % 4 == 0, cpg <= 64, m = cpg H W <= 4096 -> round_up(m / 4, 64) threads
SMALL_THREADS = [64, 256, 1024]
# gn_plan_fwd: threads = 1024 (m >= 16384), 512 (m >= 2048), 256; gn_plan_bwd: 1024 (H W >= 4096), 256 (>= 1024), 64
TWOPASS_FWD_THREADS = [256, 512, 1024]
TWOPASS_BWD_THREADS = [64, 256, 1024]
# gn_plan_bwd, a staged register plan: UPW == 1, 1024 threads, Cout == 4 -> gn_relu_bwd_stage_kernel<F, 4, WP, KEEP = F < 8>
STAGE_CLASSES = [(F, int(F < 8), wp) for F in (1, 2, 4, 8) for wp in (0, 1)]
# gn_plan_bwd's first branch: CT = 4 (Cout <= 4) or 8
SPLIT_CT = [4, 8]
# every kernel of gx_gn_last_plan that a backward with a mode-3 source can reach
PROJ_KERNELS = ['bwd_stage', 'bwd_reg_staged', 'bwd_reg', 'bwd_small', 'bwd_twopass', 'bwd_split']
# gx_defer_flush_gn: rounds of 48 records, clash rounds (one destination twice), the immediate accumulating reduce (queue of 128)
DEFER_BRANCHES = ['table_rounds', 'clash_rounds', 'immediate_accumulate']
ROW_COUNTS = {'rows': 25, 'offset': 2, 'views': 7, 'parts': 4, 'proj': 14}
CASE_COUNTS = {'views': 14, 'parts_fwd': 24, 'parts_bwd': 24, 'proj': 21, 'defer': 2, 'refusals': 7}


# ---- the dispatch restated
def pow2(v):
    return v > 0 and v & (v - 1) == 0


def mirror_plan_reg(cpg, H, W):
    HW = H * W
    if W % 4 or HW < 256 or not pow2(cpg):
        return None
    P = 1
    while HW // (256 * P) > 8:
        P *= 2
    F = HW // (256 * P)
    U, UPW = cpg * P, 1
    while U // UPW > 16:
        UPW *= 2
    if UPW * F > 8 or UPW > 2:
        return None
    return dict(F=F, UPW=UPW, P=P, threads=64 * (U // UPW))


def mirror_small_threads(cpg, H, W):
    HW, m = H * W, cpg * H * W
    if HW >= 256 or W % 4 or cpg > 64 or m > 4096:
        return 0
    return (m // 4 + 63) // 64 * 64


def mirror_class(cpg, H, W):
    m, HW = cpg * H * W, H * W
    pl, st = mirror_plan_reg(cpg, H, W), mirror_small_threads(cpg, H, W)
    if pl:
        return T.REG(pl['F'], pl['UPW'], pl['P'], pl['threads'])
    if st:
        return T.SMALL(st)
    return T.TWOPASS(int(W % 4 == 0), 1024 if m >= 16384 else (512 if m >= 2048 else 256), 1024 if HW >= 4096 else (256 if HW >= 1024 else 64))


def mirror_split_ok(cpg, H, W, Cout):
    HW = H * W
    return cpg <= 8 and 1 <= Cout <= 8 and W % 4 == 0 and HW % 4096 == 0 and HW // 4096 >= 2 and not mirror_plan_reg(cpg, H, W)


def mirror_proj(r):
    cpg, H, W, Cout = r['cpg'], r['H'], r['W'], r['Cout']
    HW = H * W
    if mirror_split_ok(cpg, H, W, Cout):
        return 'bwd_split', dict(threads=256, CT=4 if Cout <= 4 else 8, chunks=HW // 4096)
    c = mirror_class(cpg, H, W)
    if c['family'] == 'reg':
        geo = dict(F=c['F'], UPW=c['UPW'], P=c['P'], threads=c['bthreads'])
        if Cout * HW * 4 > 128 * 1024:
            return 'bwd_reg', geo
        if c['UPW'] == 1 and c['bthreads'] == 1024 and Cout == 4:
            return 'bwd_stage', dict(geo, lds=Cout * HW * 4, CT=4, KEEP=int(c['F'] < 8))
        return 'bwd_reg_staged', dict(geo, lds=Cout * HW * 4)
    return 'bwd_' + c['family'], dict(threads=c['bthreads'])


# ---- the tables
ALL_ROWS = T.ROWS + T.OFFSET_ROWS + T.VIEW_ROWS + T.PROJ_ROWS


def test_ids_are_unique_and_no_row_was_removed():
    ids = [r['id'] for r in ALL_ROWS]
    assert len(ids) == len(set(ids))
    assert {k: len(v) for k, v in T.TABLES.items()} == ROW_COUNTS
    assert dict(views=len(T.VIEW_CASES), parts_fwd=len(T.PART_FWD_CASES), parts_bwd=len(T.PART_BWD_CASES), proj=len(T.PROJ_CASES),
                defer=len(T.DEFER_ROUNDS), refusals=len(T.REFUSALS)) == CASE_COUNTS


@pytest.mark.parametrize('r', T.ROWS + T.OFFSET_ROWS + T.VIEW_ROWS, ids=lambda r: r['id'])
def test_declared_class_is_what_the_dispatch_derives(r):
    assert r['cls'] == mirror_class(r['cpg'], r['H'], r['W']), r['id']
    assert r['N'] * r['cpg'] * r['groups'] * r['H'] * r['W'] * 4 <= 1 << 20, 'operands stay within 1 MB'
    assert set(T.fwd_plan(r)) == set(T.bwd_plan(r)) == set(T.FIELDS)


@pytest.mark.parametrize('r', T.PROJ_ROWS, ids=lambda r: r['id'])
def test_declared_projected_plan_is_what_the_dispatch_derives(r):
    kernel, fields = mirror_proj(r)
    assert (r['kernel'], r['fields']) == (kernel, fields), r['id']
    assert r['N'] * r['cpg'] * r['groups'] * r['H'] * r['W'] * 4 <= 1 << 20
    for wp in r['wps']:
        assert set(T.proj_plan(r, wp)) == set(T.FIELDS)
        # wpart / bpart only where gx_gn_relu_bwd_proj_fuses_wgrad says so
        assert not wp or kernel in ('bwd_stage', 'bwd_reg_staged', 'bwd_split')


def test_the_tables_cover_the_enumerated_classes():
    reg = [r['cls'] for r in T.ROWS if r['cls']['family'] == 'reg']
    assert sorted({(c['F'], c['UPW']) for c in reg}) == sorted(REG_PAIRS)
    assert sorted(c['P'] for c in reg if (c['F'], c['UPW']) == (8, 1)) == REG_P_OF_F8
    assert all(c['P'] == 1 for c in reg if c['F'] < 8)
    small = [r for r in T.ROWS if r['cls']['family'] == 'small']
    assert sorted({r['cls']['fthreads'] for r in small}) == SMALL_THREADS
    assert any(r['cpg'] * r['H'] * r['W'] == 4096 for r in small) and any(r['cpg'] * r['H'] * r['W'] // 4 == 12 for r in small)
    for vec in (1, 0):
        two = [r for r in T.ROWS if r['cls']['family'] == 'twopass' and r['cls']['vec'] == vec]
        assert {r['cls']['fthreads'] for r in two} >= ({256, 1024} if not vec else set(TWOPASS_FWD_THREADS)), vec
    two = [r for r in T.ROWS if r['cls']['family'] == 'twopass']
    assert sorted({r['cls']['fthreads'] for r in two}) == TWOPASS_FWD_THREADS
    assert sorted({r['cls']['bthreads'] for r in two}) == TWOPASS_BWD_THREADS
    # the backward's blocks of GCH = 8 channels: one ragged block, a whole and a ragged one, two whole and a ragged one; a power of two
    # that plan_reg refuses; H W < 256 that small_threads refuses
    cpgs = {r['cpg'] for r in two if r['cls']['vec']}
    assert {3, 12, 20, 64, 128} <= cpgs
    assert any(r['cpg'] % 8 and r['cpg'] > 8 and r['H'] * r['W'] >= 4096 for r in two)
    assert any(r['cpg'] % 8 and r['H'] * r['W'] >= 256 for r in two)                    # no power of two on >= 256 pixels
    assert any(r['N'] >= 128 for r in T.ROWS)                                          # gn_param_reduce_kernel's 256 threads
    # gx_xcd_tile in the backward register kernels: grids that are no multiple of 8, and some that are
    grids = {r['N'] * r['groups'] for r in T.ROWS if r['cls']['family'] == 'reg'} | {
        r['N'] * r['groups'] for r in T.PROJ_ROWS if r['kernel'] in ('bwd_stage', 'bwd_reg_staged', 'bwd_reg')}
    assert {1, 3, 5, 7, 9, 17, 8} <= grids
    # statistics under cancellation: a register row and a two-pass row
    assert {r['cls']['family'] for r in T.OFFSET_ROWS} == {'reg', 'twopass'}


def test_views_and_partial_slabs_run_on_every_family():
    fam = lambda r: (r['cls']['family'], r['cls']['vec'])      # noqa: E731
    want = {('reg', 1), ('small', 1), ('twopass', 1), ('twopass', 0)}
    assert {fam(r) for r in T.VIEW_ROWS} == want and {fam(r) for r in T.PART_ROWS} == want
    assert all(r['H'] != r['W'] for r in T.VIEW_ROWS)
    for f in (('reg', 1), ('small', 1), ('twopass', 1)):       # both orders (the scalar kernels need W = 2)
        assert {r['H'] > r['W'] for r in T.VIEW_ROWS if fam(r) == f} == {True, False}, f
    assert {m for _, m in T.VIEW_CASES} == {1, 2}
    assert {(ns, b) for _, ns, b in T.PART_FWD_CASES} == {(ns, b) for ns in (1, 2, 3) for b in (False, True)}
    assert {(ns, m) for _, ns, m in T.PART_BWD_CASES} == {(ns, m) for ns in (2, 3) for m in (0, 1, 2)}


def test_the_projected_rows_cover_the_enumerated_classes():
    assert sorted({r['kernel'] for r in T.PROJ_ROWS}) == sorted(PROJ_KERNELS)
    stage = [(r['fields']['F'], r['fields']['KEEP'], wp) for r, wp in T.PROJ_CASES if r['kernel'] == 'bwd_stage']
    assert sorted(set(stage)) == sorted(STAGE_CLASSES)
    assert any(r['kernel'] == 'bwd_stage' and r['fields']['lds'] == 128 * 1024 for r in T.PROJ_ROWS)      # the staging boundary
    assert sum(1 for r in T.PROJ_ROWS if r['kernel'] == 'bwd_stage' and r['gate']) == 2
    staged = [r for r in T.PROJ_ROWS if r['kernel'] == 'bwd_reg_staged']
    assert any(r['fields']['UPW'] == 2 for r in staged) and any(r['fields']['threads'] < 1024 for r in staged)
    assert any(r['Cout'] == 8 and 1 in r['wps'] for r in staged)
    unstaged = [r for r in T.PROJ_ROWS if r['kernel'] == 'bwd_reg']
    assert unstaged and all(r['Cout'] * r['H'] * r['W'] * 4 > 128 * 1024 and r['wps'] == (0,) for r in unstaged)
    split = [r for r in T.PROJ_ROWS if r['kernel'] == 'bwd_split']
    assert sorted({r['fields']['CT'] for r in split}) == SPLIT_CT and {r['fields']['chunks'] for r in split} == {2, 4}
    assert any(r['H'] != r['W'] for r in split) and any(r['cpg'] < 4 for r in split) and any(r['Cout'] == 5 and r['gate'] for r in split)
    assert any(not pow2(r['cpg']) for r in split)


def test_the_deferred_rounds_reach_the_three_branches():
    reached = set()
    for count, shared in T.DEFER_ROUNDS.values():
        assert len(shared) == 3 and all(0 <= i < count for i in shared)
        if count > 48:
            reached.add('table_rounds')
        if len(shared) > 1:
            reached.add('clash_rounds')
        if count > 128:
            reached.add('immediate_accumulate')
            # two sharing calls come after the queue is full: the second immediate reduce lands on what the first left (an
            # overwrite shows); the third is queued, so the flush adds to both; one more immediate record has its own destination
            assert sum(1 for i in shared if i >= 128) >= 2 and min(shared) < 128 and count - 1 not in shared
    assert sorted(reached) == sorted(DEFER_BRANCHES)
    assert {C for C, _ in T.DEFER_SHAPES} == {8, 16, 24}


# ---- the input builder
@pytest.mark.parametrize('r', T.INPUT_ROWS, ids=lambda r: r['id'])
def test_input_margin_conditions(r):
    """No fp64 pre-activation within MARGIN of zero after at most three passes; at most 1e-3 of the elements moved."""
    inp = T.inputs_of(r)
    pre = T.pre_activation(inp['y'], inp['gamma'], inp['beta'], r['groups'])
    assert float(pre.abs().min()) >= T.MARGIN
    assert inp['passes'] <= T.MAX_PASSES and inp['moved'] <= T.MAX_MOVED
    assert inp['y'].dtype == inp['gamma'].dtype == inp['beta'].dtype and str(inp['y'].dtype) == 'torch.float32'
    print('%s: %d passes, %.2e of the elements moved' % (r['id'], inp['passes'], inp['moved']))


# ---- the record, the refusals, the queries
def test_last_plan_is_none_before_any_launch():
    """The record is per thread: a thread that never launched a GroupNorm kernel reads kernel 'none' and zeros."""
    from genesis_amd import _lib, hip_ops
    assert 'gx_gn_last_plan' in _lib.declarations()
    assert hip_ops.GN_PLAN_FIELDS == T.FIELDS
    assert hip_ops.GN_PLAN_KERNELS == ('none', 'fwd_reg', 'fwd_small', 'fwd_twopass', 'bwd_reg', 'bwd_reg_staged', 'bwd_stage',
                                       'bwd_small', 'bwd_twopass', 'bwd_split')
    got = {}

    def read():
        got['plan'] = hip_ops.gn_last_plan()
        buf = (ctypes.c_int * 4)(7, 7, 7, 7)
        got['n'] = int(_lib.load().gx_gn_last_plan(buf, 2))            # a short buffer: only n fields are written
        got['buf'] = list(buf)
    t = threading.Thread(target=read)
    t.start()
    t.join()
    assert got['plan'] == T.plan('none'), got
    assert got['n'] == len(T.FIELDS) and got['buf'] == [0, 0, 7, 7]
    assert int(_lib.load().gx_gn_last_plan(None, 0)) == len(T.FIELDS)


def test_the_header_names_every_field_and_kernel():
    import os.path as osp
    import re
    from genesis_amd import hip_ops
    header = open(osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), 'include', 'genesis_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define (GX_GN_\w+) (\d+)', header)}
    assert defs['GX_GN_PLAN_FIELDS'] == len(T.FIELDS)
    assert [defs['GX_GN_' + k.upper()] for k in hip_ops.GN_PLAN_KERNELS] == list(range(len(hip_ops.GN_PLAN_KERNELS)))
    assert [defs['GX_GN_PLAN_' + k.upper()] for k in T.FIELDS] == list(range(len(T.FIELDS)))


@pytest.mark.parametrize('name,what', [(n, w) for n, w, _ in T.REFUSALS], ids=['%s-%s' % (n, w.replace(' ', '-')) for n, w, _ in T.REFUSALS])
def test_refusals_raise_without_a_gpu(name, what):
    """Decided on the host before any launch (and a refused call leaves the record alone)."""
    from genesis_amd import hip_ops
    before = hip_ops.gn_last_plan()
    T.check_refusal(name, what)
    assert hip_ops.gn_last_plan() == before


def test_fuses_wgrad_query_without_a_gpu():
    T.test_fuses_wgrad_query()
    from genesis_amd import _lib
    for r in T.PROJ_ROWS:
        fuses = _lib.query('gx_gn_relu_bwd_proj_fuses_wgrad', r['cpg'] * r['groups'], r['H'], r['W'], r['groups'], r['Cout'])
        assert bool(fuses) == (r['kernel'] in ('bwd_stage', 'bwd_reg_staged', 'bwd_split')), r['id']
        ws = _lib.query('gx_gn_relu_bwd_proj_ws_bytes', r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups'], r['Cout'])
        plain = _lib.query('gx_gn_relu_bwd_ws_bytes', r['N'], r['cpg'] * r['groups'])
        assert (ws > plain) == (r['kernel'] == 'bwd_split'), r['id']


# ---- the library's own plan (gx_gn_fwd_plan / gx_gn_bwd_plan: the functions the launchers call, asked without a launch)
def _shape(r):
    return r['N'], r['cpg'] * r['groups'], r['H'], r['W'], r['groups']


def _proj_ws(r):
    from genesis_amd import _lib
    return _lib.query('gx_gn_relu_bwd_proj_ws_bytes', *_shape(r), r['Cout'])


@pytest.mark.parametrize('r', T.ROWS + T.OFFSET_ROWS + T.VIEW_ROWS, ids=lambda r: r['id'])
def test_declared_plans_are_the_librarys_plans(r):
    """What the GPU tests assert of the launch's record holds of the dispatch itself, for every slab count the cases use."""
    from genesis_amd import hip_ops
    assert hip_ops.gn_fwd_plan(*_shape(r)) == T.fwd_plan(r)
    assert hip_ops.gn_bwd_plan(*_shape(r)) == T.bwd_plan(r)
    if any(q is r for q, _ in T.VIEW_CASES):         # (the second source's mode is not an argument of the plan)
        assert hip_ops.gn_bwd_plan(*_shape(r), g1_nsplit=1) == T.bwd_plan(r, 1, 1)
    for ns in sorted({ns for q, ns, _ in T.PART_FWD_CASES if q is r}):
        assert hip_ops.gn_fwd_plan(*_shape(r), ns) == T.fwd_plan(r, ns)
    for ns, mode0 in sorted({(ns, m) for q, ns, m in T.PART_BWD_CASES if q is r}):
        assert hip_ops.gn_bwd_plan(*_shape(r), g0_mode=mode0, g0_nsplit=ns, g1_nsplit=5 - ns) == T.bwd_plan(r, ns, 5 - ns)


@pytest.mark.parametrize('r,wp', T.PROJ_CASES, ids=['%s-wp%d' % (r['id'], wp) for r, wp in T.PROJ_CASES])
def test_declared_projected_plans_are_the_librarys_plans(r, wp):
    from genesis_amd import hip_ops
    got = hip_ops.gn_bwd_plan(*_shape(r), g0_mode=3, g0_ctot=r['Cout'], g0_nsplit=0, want_wpart=wp, ws_bytes=_proj_ws(r))
    assert got == T.proj_plan(r, wp)


@pytest.mark.parametrize('r', [r for r in T.PROJ_ROWS if r['kernel'] == 'bwd_split'], ids=lambda r: r['id'])
def test_a_plain_workspace_falls_through_the_chunked_branch(r):
    """Pins the last condition of the ladder's first line, `ws_bytes >= gx_gn_relu_bwd_proj_ws_bytes(...)`: with the workspace of
    gx_gn_relu_bwd_ws_bytes a chunked shape is not refused for its workspace but falls through to the rest of the ladder -- no
    register plan, so the two-pass kernel, which cannot write wpart / bpart (the third REFUSALS entry)."""
    from genesis_amd import _lib, hip_ops
    plain = _lib.query('gx_gn_relu_bwd_ws_bytes', r['N'], r['cpg'] * r['groups'])
    assert plain < _proj_ws(r)
    kw = dict(g0_mode=3, g0_ctot=r['Cout'], g0_nsplit=0, ws_bytes=plain)
    assert hip_ops.gn_bwd_plan(*_shape(r), **kw) == T.plan('bwd_twopass', vec=1, threads=1024, grid=r['N'] * r['groups'])
    assert hip_ops.gn_bwd_plan(*_shape(r), want_wpart=True, **kw) == T.plan('none')
    assert hip_ops.gn_bwd_plan(*_shape(r), **dict(kw, ws_bytes=_proj_ws(r) - 4))['kernel'] == 'bwd_twopass'         # 4 bytes short
    assert hip_ops.gn_bwd_plan(*_shape(r), **dict(kw, ws_bytes=plain - 4)) == T.plan('none')      # below the plain workspace: refused


def test_the_queries_agree_with_the_plan_over_a_sweep():
    """gx_gn_relu_bwd_proj_fuses_wgrad != 0 iff the plan with wpart and the query's workspace is a kernel; the query's workspace
    exceeds the plain one iff that plan is the chunked path."""
    from genesis_amd import _lib, hip_ops
    sizes = [2 ** k for k in range(1, 9)]
    count, kernels = 0, set()
    for cpg in (1, 2, 3, 4, 8, 16, 32, 64):
        for groups in (1, 8):
            for H in sizes:
                for W in [w for w in sizes if H * w <= 65536]:
                    for Cout in range(1, 9):
                        C = cpg * groups
                        ws = _lib.query('gx_gn_relu_bwd_proj_ws_bytes', 1, C, H, W, groups, Cout)
                        plain = _lib.query('gx_gn_relu_bwd_ws_bytes', 1, C)
                        fuses = _lib.query('gx_gn_relu_bwd_proj_fuses_wgrad', C, H, W, groups, Cout)
                        kernel = hip_ops.gn_bwd_plan(1, C, H, W, groups, g0_mode=3, g0_ctot=Cout, g0_nsplit=0, want_wpart=True,
                                                     ws_bytes=ws)['kernel']
                        assert (fuses != 0) == (kernel != 'none'), (cpg, groups, H, W, Cout, fuses, kernel)
                        assert (ws > plain) == (kernel == 'bwd_split'), (cpg, groups, H, W, Cout, ws, plain, kernel)
                        count, kernels = count + 1, kernels | {kernel}
    assert count == 8 * 2 * 8 * sum(1 for H in sizes for W in sizes if H * W <= 65536)
    assert kernels == {'none', 'bwd_stage', 'bwd_reg_staged', 'bwd_split'}


def test_the_queries_leave_the_record_alone():
    from genesis_amd import _lib, hip_ops
    before = hip_ops.gn_last_plan()
    assert hip_ops.gn_fwd_plan(2, 16, 32, 32, 2)['kernel'] == 'fwd_reg' and hip_ops.gn_bwd_plan(2, 16, 4, 4, 2)['kernel'] == 'bwd_small'
    _lib.query('gx_gn_relu_bwd_proj_fuses_wgrad', 16, 64, 128, 4, 4)
    _lib.query('gx_gn_relu_bwd_proj_ws_bytes', 1, 16, 64, 128, 4, 4)
    assert hip_ops.gn_last_plan() == before
    assert 'gx_gn_fwd_plan' in _lib.declarations() and 'gx_gn_bwd_plan' in _lib.declarations()
