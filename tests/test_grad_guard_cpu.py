"""The gradient guard without a GPU: the constants against the header, the restated clip coefficient against
torch.nn.utils.clip_grad_norm_ run on the CPU in fp64 (finite, NaN and infinite norms, a parameter without a gradient), every refusal
of gx_grad_guard / gx_scale_multi_guarded / the guarded tail launches (raised from the host copy of the table, before any launch)
and of the Python layer (raised before the library is called)."""
import ctypes
import os.path as osp
import re

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd import grad_guard as gg
from genesis_amd._lib import GenesisHipError
from tests import grad_guard_restatement as R

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def test_constants_match_the_header():
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define GX_GUARD_(\w+) (\d+)', header)}
    assert sorted(defs) == sorted(['FP32', 'FP64', 'D_SRC', 'D_N', 'D_DTYPE', 'D_WORK', 'DESC_WORDS', 'CHUNK', 'MAX_GRID', 'MAX_CHECK',
                                   'R_S', 'R_NORM', 'R_COEF', 'R_SCALE', 'R_OK', 'R_SKIPPED', 'RECORD_BYTES'])
    for name, v in defs.items():
        assert getattr(gg, name) == v, name
    assert gg.R_SKIPPED + 8 == gg.RECORD_BYTES


# ---- the coefficient: the restatement against torch on the CPU in fp64 ----------------------------------------------------------
def _params(kind):
    gen = torch.Generator().manual_seed(3)
    shapes = [(7, 5), (33,), (1,), (4, 3, 3, 3)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    for i, p in enumerate(ps):
        p.grad = torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.5 + i)
    if kind == 'nan':
        ps[1].grad[4] = float('nan')
    if kind == 'inf':
        ps[3].grad[1, 2, 0, 1] = float('inf')
    ps.insert(2, torch.nn.Parameter(torch.randn(6, generator=gen, dtype=torch.float64)))      # no gradient: skipped
    return ps


@pytest.mark.parametrize('kind', ['finite', 'nan', 'inf'])
@pytest.mark.parametrize('max_norm', [0.25, 1e3, 'equal'])
def test_coefficient_formula_is_torchs(kind, max_norm):
    ps = _params(kind)
    before = [p.grad.clone() for p in ps if p.grad is not None]
    S = R.sum_squares([g.numpy() for g in before])
    if max_norm == 'equal':
        max_norm = float(np.sqrt(S)) if kind == 'finite' else 1.0
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, error_if_nonfinite=False)
    assert ps[2].grad is None
    # the norm: sqrt of the fp64 sum of squares against torch's norm of per-tensor norms
    if kind == 'finite':
        assert abs(float(total) - np.sqrt(S)) <= 8 * 2.0 ** -52 * np.sqrt(S)
    elif kind == 'nan':
        assert np.isnan(float(total)) and np.isnan(S)
    else:
        assert np.isinf(float(total)) and np.isinf(S)
    # the coefficient, from torch's own norm: the clipped gradients are g * coef bit for bit
    c = R.coef64(float(total), max_norm)
    if kind == 'nan':
        assert c != c
    if kind == 'inf':
        assert c == 0.0
    after = [p.grad for p in ps if p.grad is not None]
    for b, a in zip(before, after):
        want = b * c
        assert torch.equal(a.view(torch.int64), want.view(torch.int64))
    assert R.coef64(3.0, None) == 1.0


def test_record_restatement():
    n64, n32, c64, c32 = R.record_ref(4.0, 0.5, 0.25)
    assert n64 == 1.0 and n32 == np.float32(1.0) and c64 == 0.25 / (1.0 + 1e-6) and c32 == np.float32(c64)
    assert R.record_ref(4.0, 1.0, None)[2:] == (1.0, np.float32(1.0))
    assert R.record_ref(float('inf'), 1.0, 1.0)[2] == 0.0
    assert np.isnan(R.record_ref(float('nan'), 1.0, 1.0)[3])
    assert R.ulps32(np.float32(1.0), np.float32(1.0)) == 0.0 and R.ulps32(np.nextafter(np.float32(1), np.float32(2)), 1.0) == 1.0


# ---- gx_grad_guard / gx_scale_multi_guarded: refusals with fake device addresses (validation reads no device memory) --------------
FAKE = 4096


def _segment(**over):
    row = [0] * gg.DESC_WORDS
    fields = dict(SRC=FAKE, N=100, DTYPE=gg.FP32, WORK=0)
    fields.update(over)
    for k, v in fields.items():
        row[getattr(gg, 'D_' + k)] = v
    return row


def _guard(rows, n_segments=None, table_words=None, table_dev=FAKE, check=0, n_check=0, record=FAKE, ws=FAKE, ws_bytes=1 << 20):
    table = np.array([w for row in rows for w in row], np.int64)
    _lib.call('gx_grad_guard', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(table_dev),
              table.size if table_words is None else table_words, len(rows) if n_segments is None else n_segments,
              ctypes.c_void_p(check), n_check, 1.0, 1.0, 0, ctypes.c_void_p(record), ctypes.c_void_p(ws), ws_bytes, None)


def _scale(rows, table_dev=FAKE, record=FAKE):
    table = np.array([w for row in rows for w in row], np.int64)
    _lib.call('gx_scale_multi_guarded', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(table_dev), table.size, len(rows),
              ctypes.c_void_p(record), None)


@pytest.mark.parametrize('rows, kwargs, message', [
    ([_segment()], dict(table_dev=0), 'null descriptor table'),
    ([_segment()], dict(record=0), 'null record or workspace'),
    ([_segment()], dict(ws=0), 'null record or workspace'),
    ([_segment()], dict(record=FAKE + 4), '8-byte aligned'),
    ([_segment()], dict(table_dev=FAKE + 4), '8-byte aligned'),
    ([_segment()], dict(n_segments=0), 'n_segments = 0 below 1'),
    ([_segment(N=0)], {}, r'segment 0: N = 0 outside \[1, 2\^31\)'),
    ([_segment(N=-5)], {}, 'segment 0: N = -5 outside'),
    ([_segment(N=1 << 31)], {}, 'segment 0: N = 2147483648 outside'),
    ([_segment(DTYPE=2)], {}, 'segment 0: unknown dtype 2'),
    ([_segment(SRC=0)], {}, 'segment 0: null source'),
    ([_segment(SRC=FAKE + 2)], {}, 'segment 0: source 0x1002 is not aligned to its 4-byte elements'),
    ([_segment(SRC=FAKE + 4, DTYPE=1)], {}, 'segment 0: source 0x1004 is not aligned to its 8-byte elements'),
    ([_segment(WORK=1)], {}, 'segment 0: WORK = 1, the prefix is 0'),
    ([_segment(N=8193), _segment(WORK=1)], {}, 'segment 1: WORK = 1, the prefix is 2'),
    ([_segment(), _segment(WORK=1)], dict(table_words=7), '2 segments do not fit a table of 7 words'),
    ([_segment(N=8193)], dict(ws_bytes=8), 'workspace of 8 bytes, 16 needed'),
    ([_segment()], dict(n_check=2), 'n_check = 2'),
    ([_segment()], dict(n_check=9, check=FAKE), 'n_check = 9'),
    ([_segment()], dict(n_check=-1), 'n_check = -1'),
])
def test_grad_guard_refuses_before_launching(rows, kwargs, message):
    with pytest.raises(GenesisHipError, match=message):
        _guard(rows, **kwargs)


@pytest.mark.parametrize('rows, kwargs, message', [
    ([_segment()], dict(table_dev=0), 'null descriptor table'),
    ([_segment()], dict(record=0), 'null or misaligned record'),
    ([_segment()], dict(record=FAKE + 4), 'null or misaligned record'),
    ([_segment(N=0)], {}, 'segment 0: N = 0 outside'),
    ([_segment(SRC=FAKE + 1)], {}, 'not aligned to its 4-byte elements'),
])
def test_scale_multi_refuses_before_launching(rows, kwargs, message):
    with pytest.raises(GenesisHipError, match='gx_scale_multi_guarded.*' + message):
        _scale(rows, **kwargs)


def test_workspace_size_follows_the_grid_cap():
    q = lambda n: _lib.query('gx_grad_guard_ws_bytes', n)      # noqa: E731
    assert q(0) == 8 and q(1) == 8 and q(3) == 24 and q(gg.MAX_GRID) == 8 * gg.MAX_GRID and q(10 * gg.MAX_GRID) == 8 * gg.MAX_GRID
    # a 4-byte-aligned fp32 slice and an 8-byte-aligned fp64 slice are legal segments: the call gets past them to the next check
    with pytest.raises(GenesisHipError, match='workspace'):
        _guard([_segment(SRC=FAKE + 4), _segment(SRC=FAKE + 8, DTYPE=1, WORK=1)], ws_bytes=0)


def test_guarded_tail_refuses_a_missing_record():
    p = ctypes.c_void_p(FAKE)
    for name, args in (
            ('gx_step_increment_guarded', (p, None, None)),
            ('gx_geco_update_step_guarded', (p, p, 1.0, 1.0, 0.99, 0.0, 0, 1e-10, 1e10, p, None, None)),
            ('gx_adam_step_pair_guarded', (p, p, p, p, 8, None, None, None, None, 0, p, 1e-3, 0.9, 0.999, 1e-8, None, 1, None)),
            ('gx_optimiser_step_pair_guarded', (1, p, p, p, 8, None, None, None, 0, p, 1e-3, 0.99, 1e-8, None, 1, None))):
        with pytest.raises(GenesisHipError, match=name + ': null or misaligned guard record'):
            _lib.call(name, *args)
    with pytest.raises(GenesisHipError, match='kind must be 1'):
        _lib.call('gx_optimiser_step_pair_guarded', 3, p, p, p, 8, None, None, None, 0, p, 1e-3, 0.99, 1e-8, p, 1, None)
    with pytest.raises(GenesisHipError, match='empty fp32 group'):
        _lib.call('gx_adam_step_pair_guarded', p, p, p, p, 0, None, None, None, None, 0, p, 1e-3, 0.9, 0.999, 1e-8, p, 1, None)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [0, 0.0, -1.0, float('nan'), float('inf'), 'big', True, [1.0]])
def test_trainstep_refuses_a_bad_max_grad_norm(bad):
    from genesis_amd.trainer import TrainStep
    with pytest.raises(ValueError, match='max_grad_norm'):
        TrainStep(None, 64, max_grad_norm=bad)            # (refused before the model is looked at)
    with pytest.raises(ValueError, match='max_grad_norm'):
        gg.check_max_grad_norm(bad)
    assert gg.check_max_grad_norm(None) is None and gg.check_max_grad_norm(2) == 2.0 and gg.check_max_grad_norm(np.float32(0.5)) == 0.5


def test_drop_in_refusals_name_their_argument():
    import genesis_amd
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(GenesisHipError, match='norm_type'):
        genesis_amd.clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(GenesisHipError, match='norm_type'):
        genesis_amd.clip_grad_norm_([p], 1.0, norm_type=float('inf'))
    with pytest.raises(GenesisHipError, match='error_if_nonfinite'):
        genesis_amd.clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    for bad in (0.0, -2.0, float('nan'), 'x'):
        with pytest.raises(GenesisHipError, match='max_norm'):
            genesis_amd.clip_grad_norm_([p], bad)
    with pytest.raises(GenesisHipError, match='parameters: gradient 0 is on cpu'):
        genesis_amd.clip_grad_norm_([p], 1.0)
    with pytest.raises(GenesisHipError, match='parameters: gradient 0 is on cpu'):
        genesis_amd.clip_grad_norm_(p, 1.0)               # a single tensor, as torch accepts
    q = torch.nn.Parameter(torch.zeros(3))                # no gradient anywhere: torch's 0
    assert float(genesis_amd.clip_grad_norm_([q], 1.0)) == 0.0
    assert torch.equal(p.grad, torch.ones(4))
