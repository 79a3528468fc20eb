"""The case tables of tests/test_conv_plans_gpu.py against a written enumeration of the plan classes each conv kernel's host planner
can pick, the gx_conv_last_plan record before any launch, and the refusals the host decides -- all without a GPU.

The enumeration is derived from the planners (cited per block) and written out here; the tables must cover it, so a deleted or
re-pointed row fails on the CPU.  A class is (form, lTH, lTW, lG, nq or NPOS) of a family; a tail is one of the names
tests/test_conv_plans_gpu.py's tails_of() computes from a recorded plan (the GPU test asserts every declared set against it)."""
import ctypes
import threading

import pytest

from genesis_amd._lib import GenesisHipError
from tests import test_conv_plans_gpu as T

# family -> (classes that must be declared by some row, tails that must be declared by some row of the family)
REQUIRED = {
    # q_plan (gx_kq.hip): TW = min(Wb, 64), TH = min(256 / TW, Hb), G = 256 / (TW TH); CHS = G (TH + 2) (TW + 2), refused when
    # 2 CHS > 1024 (4 x 4), nq = 3 when 2 CHS <= 768 (16 x 16: 648, 8 x 32: 680) else 4 (8 x 8: 800, 4 x 8: 960, 4 x 64 / 64 x 4 /
    # 64 x 64: 792); q_split_tail: ptiles > 256, r = ptiles % 256 in (0, 128], M % 64 == 0 or > 32
    'kq_c3': ([('fp32', 3, 3, 2, 4), ('fp32', 2, 3, 3, 4), ('fp32', 4, 4, 0, 3), ('fp32', 3, 5, 0, 3), ('fp32', 2, 6, 0, 4),
               ('fp32', 6, 2, 0, 4)], ['image_tail', 'm_tail', 'split_tail', 'split_refused']),
    # ... the transposed conv's fp32 kernels run with the 16-bit pipe off, for K % 16 != 0, and for the tiles whose three piece
    # planes qh_lds refuses (4 x 16 / 16 x 4: CHS = 432, 3 * 2 * 432 * 16 + 36864 > 80 KiB)
    'kq_dt': ([('fp32', 3, 3, 2, 4), ('fp32', 2, 4, 2, 4), ('fp32', 4, 4, 0, 3)], ['image_tail', 'stats', 'split_tail', 'm_tail']),
    'kq_dg': ([('fp32', 4, 2, 2, 4), ('fp32', 4, 4, 0, 3), ('fp32', 3, 3, 2, 4)], ['image_tail', 'split_tail', 'm_tail']),
    # gx_kq_deconv_fwd_h_launch / _dgrad_h_launch: the same q_plan tiles in the three 16-bit forms; grid.y == 1 interleaves the row
    # parities along x (g.ilv); st = stats && lG == 0 && M % 8 == 0
    'kq_dth': ([(f, 3, 3, 2, 4) for f in ('bf16x6', 'fp16x3')] + [(f, 4, 4, 0, 3) for f in ('bf16x6', 'fp16x3')]
               + [(f, 3, 5, 0, 3) for f in ('bf16x6', 'fp16x3')], ['image_tail', 'ilv', 'stats', 'm_tail', 'split_tail']),
    'kq_dgh': ([(f, 3, 3, 2, 4) for f in ('bf16x6', 'fp16x3')] + [(f, 4, 4, 0, 3) for f in ('bf16x6', 'fp16x3')]
               + [(f, 3, 5, 0, 3) for f in ('bf16x6', 'fp16x3')], ['image_tail', 'split_tail', 'm_tail']),
    # q_plan_c3h: the largest power-of-two divisors of W (<= 64) and H, images fill the rest; TW < W, TW < 32, W <= 128: whole rows
    # (rt_th = 256 / W: 10 at W = 24, 3 at W = 72, 42 at W = 6), tiles_h = ceil(H / rt_th); grid.x capped at 768 / grid.y
    'kq_c3h': ([(f, 3, 3, 2, 4) for f in ('bf16x6', 'fp16x3')] + [(f, 4, 5, 0, 3) for f in ('bf16x6', 'fp16x3')]
               + [(f, 2, 7, 0, 3) for f in ('bf16x6', 'fp16x3')] + [(f, 6, 3, 0, 3) for f in ('bf16x6', 'fp16x3')]
               + [(f, 2, 6, 0, 4) for f in ('bf16x6', 'fp16x3')] + [('fp16x3', 4, 4, 0, 3)],
               ['image_tail', 'ragged_h', 'tile_taller', 'second_round', 'm_tail']),
    # q_plan_c5h: one plan (16 x 16 tiles, one image, four staging rounds)
    'kq_c5h': ([('bf16x6', 4, 4, 0, 4), ('fp16x3', 4, 4, 0, 4)], ['m_tail']),
    # pick_tile / plan_tapconv / plan_c3: NPOS = LO (2; 8 for M_DG) when ceil(CHS / 256) <= LO else 2 LO; 128-pixel tiles when the
    # 256-pixel plan splits the reduction (or cannot hold its halos: 1 x 4); nsplit = min(ceil(512 / base), nchunks, 64)
    'tap_c3': ([('fp32', 3, 3, 2, 2), ('fp32', 2, 2, 4, 4), ('fp32', 0, 2, 5, 4), ('fp32', 1, 1, 5, 2), ('fp32', 3, 4, 0, 2),
                ('fp32', 1, 2, 5, 4), ('fp32', 2, 1, 5, 4)],
               ['image_tail', 'ragged_h', 'ragged_w', 'k_pad', 'm_tail', 'm_low', 'splitk', 'splitk_uneven', 'splitk_capped', 'px128']),
    'tap_c5': ([('fp32', 2, 2, 4, 4), ('fp32', 3, 3, 2, 4), ('fp32', 4, 4, 0, 2), ('fp32', 4, 1, 3, 4)],
               ['image_tail', 'ragged_h', 'ragged_w', 'k_pad', 'm_tail', 'm_low', 'splitk', 'splitk_capped']),
    'tap_dt': ([('fp32', 0, 2, 5, 4), ('fp32', 3, 3, 1, 2), ('fp32', 1, 1, 5, 2), ('fp32', 4, 4, 0, 2), ('fp32', 2, 2, 4, 4),
                ('fp32', 1, 2, 5, 4)], ['image_tail', 'ragged_h', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128', 'stats']),
    'tap_dg': ([('fp32', 0, 2, 5, 16), ('fp32', 3, 3, 1, 8), ('fp32', 1, 1, 5, 8), ('fp32', 2, 2, 4, 16), ('fp32', 2, 1, 5, 16)],   # (0, 2, 5, 16): 9 x 12 and 1 x 4
               ['image_tail', 'ragged_w', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128']),
    # wino_shape_ok: one tile plan (8 x 16 output pixels per workgroup), the fp32 and the 16-bit operand forms
    'wino': ([('fp32', 0, 0, 0, 0), ('bf16x6', 0, 0, 0, 0)], ['k_pad', 'm_tail']),
    # smallcin_fwd_ok: no tile; SC_COB = 8 output channels per workgroup row
    'smallcin': ([('fp32', 0, 0, 0, 0)], ['m_tail']),
}
ROWS = {'kq_c3': 12, 'kq_deconv': 28, 'kq_c3h': 19, 'kq_c5h': 8, 'tap': 31, 'wino': 8, 'smallcin': 5}


def test_every_row_states_its_plan_class_and_ids_are_unique():
    ids = [r['id'] for r in T.ALL_CASES]
    assert len(ids) == len(set(ids))
    for r in T.ALL_CASES:
        assert all(k in r['plan'] for k in T.PLAN_KEYS), r['id']
        assert r['plan']['family'] in REQUIRED, r['id']
        assert set(r['plan']) <= {'family', 'form', 'lTH', 'lTW', 'lG', 'nq', 'pixels', 'rt_th', 'rt_tw', 'tiles_h', 'tiles_w', 'grid_x',
                                  'grid_y', 'grid_z', 'nsplit', 'chunks_per_split', 'nfull', 'stats'}, r['id']


def test_no_row_was_removed():
    assert {k: len(v) for k, v in T.TABLES.items()} == ROWS


@pytest.mark.parametrize('family', sorted(REQUIRED))
def test_the_tables_cover_the_enumerated_plan_classes(family):
    rows = [r for r in T.ALL_CASES if r['plan']['family'] == family]
    have = {tuple(r['plan'][k] for k in T.PLAN_KEYS[1:]) for r in rows}
    tails = set().union(*[r['tails'] for r in rows]) if rows else set()
    classes, need_tails = REQUIRED[family]
    assert not [c for c in classes if c not in have], 'no row declares these %s classes: %s' % (family, [c for c in classes if c not in have])
    assert not [t for t in need_tails if t not in tails], 'no %s row declares these tails: %s' % (family, [t for t in need_tails if t not in tails])


def test_the_tables_cover_what_the_issue_names():
    """The shapes and counts the classes were asked for, by geometry."""
    geo = {(r['plan']['family'],) + T.geometry(r) for r in T.ALL_CASES}

    def has(fam, N=None, K=None, M=None, H=None, W=None):
        return any(g[0] == fam and all(v is None or g[i + 1] == v for i, v in enumerate((N, K, M, H, W))) for g in geo)
    for M in (40, 72, 130):
        assert has('kq_c3', M=M)
    assert has('kq_c3', K=8) and has('kq_c3', K=24) and has('kq_c3', N=5, H=8, W=8) and has('kq_c3', H=64, W=64)
    assert has('kq_dth', N=5, H=8, W=8) and has('kq_dgh', N=7, H=8, W=8) and has('kq_dt', N=7, K=24)
    assert has('kq_dth', K=48) and has('kq_dgh', K=48) and has('kq_dth', M=20) and has('kq_dgh', H=32) and has('kq_dth', H=32)
    assert any(r.get('cin_out') and r['plan']['family'] == 'kq_dgh' for r in T.ALL_CASES)
    for M in (7, 24, 32):
        assert has('kq_c3h', M=M)
    assert has('kq_c3h', K=48) and has('kq_c3h', N=200, H=40, W=24) and has('kq_c3h', H=6, W=6) and has('kq_c3h', H=4, W=128)
    assert any(r.get('tap') for r in T.KQ_C3H_CASES)
    assert {r['op'] for r in T.KQ_C3H_CASES if r['plan']['family'] == 'kq_c3h'} == {'c3_fwd', 'c3_act', 'c3_dgrad', 'c3_dgrad_act'}
    for M in (24, 64, 72):
        assert has('kq_c5h', M=M)
    assert has('kq_c5h', N=1) and has('kq_c5h', N=3) and has('kq_c5h', K=48) and has('kq_c5h', H=16, W=48) and has('kq_c5h', H=48, W=16)
    assert {r['op'] for r in T.KQ_C5H_CASES} == {'c5_0', 'c5_1'}
    for fam in ('tap_c3', 'tap_dt', 'tap_dg'):
        assert has(fam, H=72, W=72) and has(fam, H=2, W=2), fam
    assert has('tap_c3', H=1, W=4) and has('tap_dt', H=1, W=4) and has('tap_dg', H=1, W=4) and has('tap_c3', H=12, W=20) and has('tap_c5', H=72, W=72)
    for K in (3, 12, 66):
        assert has('tap_c3', K=K)
    assert has('tap_c3', M=1) and has('tap_c3', M=65)
    assert {'c3_fwd_parts', 'c3_dgrad_parts', 'dt_parts'} <= {r['op'] for r in T.TAP_CASES}
    assert has('wino', H=8, W=16) and has('wino', H=8, W=256) and has('wino', H=128, W=16) and has('wino', K=17) and has('wino', M=65)
    assert has('wino', N=1) and has('wino', M=16) and has('wino', K=16)
    assert {'wino0', 'wino1', 'c3_fwd', 'c3_dgrad'} <= {r['op'] for r in T.WINO_CASES}
    assert has('smallcin', M=1) and has('smallcin', M=9)
    # one step outside every eligibility boundary: the declared family is the fallback
    out = {r['id']: r['plan']['family'] for r in T.ALL_CASES if '-out-' in r['id']}
    assert len(out) >= 14 and all(f.startswith('tap_') or f == 'kq_c3' for f in out.values()), out


def test_the_one_bf16_rows_are_the_rows_of_the_families_that_have_the_form():
    assert len(T.B1_KQ) >= 18 and len(T.B1_WINO) >= 3 and len(T.B1_TAP) == len(T.TAP_CASES) - 1          # (tap-dg-1x4 has no one-bf16 plan)
    assert {r['plan']['family'] for r in T.B1_KQ} == {'kq_dth', 'kq_dgh', 'kq_c3h', 'kq_c5h'}


def test_tails_of_on_hand_made_records():
    """tails_of() itself, on records written by hand from the planners' rules."""
    row = T.R('x', 'c3_fwd', (1028, 8, 40, 8, 8), T.P('kq_c3', 'fp32', 3, 3, 2, 4))
    rec = dict(family='kq_c3', form='fp32', lTH=3, lTW=3, lG=2, nq=4, pixels=256, rt_th=0, rt_tw=0, tiles_h=1, tiles_w=1, grid_x=258,
               grid_y=1, grid_z=1, nsplit=1, chunks_per_split=1, nfull=256, stats=0)
    assert T.tails_of(row, rec) == {'split_tail', 'm_tail'}
    assert T.tails_of(row, dict(rec, nfull=257, grid_x=257)) == {'split_refused', 'm_tail'}
    row = T.R('y', 'c3_dgrad', (3, 24, 16, 16, 24), T.P('kq_c3h', 'bf16x6'))
    rec = dict(rec, family='kq_c3h', lTH=4, lTW=5, lG=0, nq=3, rt_th=10, rt_tw=24, tiles_h=2, nfull=6, grid_x=6)
    assert T.tails_of(row, rec) == {'ragged_h', 'm_tail'}
    assert T.tails_of(row, dict(rec, nfull=800, grid_x=768)) == {'ragged_h', 'm_tail', 'second_round'}
    row = T.R('z', 'c3_fwd', (64, 40, 64, 16, 16), T.P('tap_c3', 'fp32'))
    rec = dict(rec, family='tap_c3', lTH=3, lTW=4, lG=0, nq=2, pixels=128, rt_th=0, rt_tw=0, tiles_h=2, nsplit=3, chunks_per_split=2)
    assert T.tails_of(row, rec) == {'splitk', 'splitk_uneven', 'px128'}


def test_last_plan_is_none_before_any_launch():
    """The record is per thread: a thread that never launched a conv reads family 'none' and zeros."""
    from genesis_amd import _lib, hip_ops
    assert 'gx_conv_last_plan' in _lib.declarations()
    got = {}

    def read():
        got['plan'] = hip_ops.conv_last_plan()
        buf = (ctypes.c_int * 4)(7, 7, 7, 7)
        got['n'] = int(_lib.load().gx_conv_last_plan(buf, 2))           # a short buffer: only n fields are written
        got['buf'] = list(buf)
    t = threading.Thread(target=read)
    t.start()
    t.join()
    assert got['plan']['family'] == 'none' and got['plan']['form'] == 'fp32'
    assert all(v == 0 for k, v in got['plan'].items() if k not in ('family', 'form')), got
    assert set(got['plan']) == set(hip_ops.PLAN_FIELDS)
    assert got['n'] == len(hip_ops.PLAN_FIELDS) and got['buf'] == [0, 0, 7, 7]
    assert int(_lib.load().gx_conv_last_plan(None, 0)) == len(hip_ops.PLAN_FIELDS)


@pytest.mark.parametrize('name,kind,dims,message', T.REFUSALS, ids=['%s-%s' % (r[0], 'x'.join(map(str, r[2]))) for r in T.REFUSALS])
def test_refusals_raise_without_a_gpu(name, kind, dims, message):
    """check_dims is the first check of these entry points: every pointer is NULL, so a refusal that stopped refusing would meet
    the null-pointer check behind it (another message: this test fails) and never a launch."""
    import re
    from genesis_amd import _lib
    N, a, b, H, W = dims
    with pytest.raises(GenesisHipError, match=re.escape(message)):
        if kind == 'c3':
            _lib.call(name, None, None, None, N, a, b, H, W, None, 0, None)
        elif kind == 'c3_dgrad_act':
            _lib.call(name, None, None, None, 1, None, None, N, a, b, H, W, None, 0, None)
        elif kind == 'dt':
            _lib.call(name, None, None, None, None, N, a, b, H, W, None, 0, None)
        else:
            assert kind == 'dg'
            _lib.call(name, None, None, None, N, a, a, b, H, W, None, 0, None)


@pytest.mark.parametrize('name,args', T.UNSUPPORTED, ids=['%s-%s' % (u[0], 'x'.join(map(str, u[1]))) for u in T.UNSUPPORTED])
def test_supported_queries_answer_no(name, args):
    from genesis_amd import _lib
    assert _lib.query(name, *args) == 0


def test_one_by_four_grid_has_a_tap_conv_plan():
    """1 x 4 (the smallest grid check_dims admits): 64 images per 256-pixel tile do not fit their halos, so plan_tapconv falls back
    to 128-pixel tiles -- the workspace query must answer (and did before), and gx_conv5x5s1_supported keeps refusing H < 4."""
    from genesis_amd import _lib
    assert _lib.query('gx_conv3x3_ws_bytes', 3, 64, 64, 1, 4) > 0 and _lib.query('gx_deconv5x5s2_ws_bytes', 3, 64, 64, 1, 4) > 0
    # the split-K slabs of the 128-pixel plan are part of the workspace: packed weights (24 * 64 * 64 + 4096 floats), 8 chunks of 8
    # channels -> 8 slabs of 3 * 64 * 1 * 4 floats, the amax scratch (256 floats)
    assert _lib.query('gx_conv3x3_ws_bytes', 3, 64, 64, 1, 4) == (24 * 64 * 64 + 4096 + 8 * 3 * 64 * 4 + 256) * 4
    assert _lib.query('gx_conv5x5s1_supported', 3, 8, 8, 1, 4) == 0
