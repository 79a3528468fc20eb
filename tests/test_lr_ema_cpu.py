"""Learning-rate schedules and averaged weights without a GPU: LRSchedule.value against torch's SequentialLR([LinearLR, X]) read from
param_groups[0]['lr'], every validation error by argument name, the constants Python uses against include/genesis_hip.h, and the
refusals of the three entry points (raised from host values, before any launch).

The bar on the rates is 1e-12 relative: torch's schedulers are recursive (lr_{k+1} from lr_k) and drift by rounding -- at most
4.8e-15 over 2000 cosine steps on torch 2.10 -- while `constant` and `step` without a warm-up are exact; 1e-12 leaves two orders of
magnitude above the measured drift and sits four orders below what an fp32 parameter can see."""
import ctypes
import math
import os.path as osp
import re
import warnings

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd import ema as E
from genesis_amd import schedule as SC
from genesis_amd._lib import GenesisHipError
from genesis_amd.schedule import LRSchedule

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))
BASE = 3e-4
RTOL = 1e-12
STEPS = 2000
T_COS = 1500

KINDS = {
    'constant': (dict(kind='constant'), lambda opt: torch.optim.lr_scheduler.ConstantLR(opt, factor=1.0, total_iters=0)),
    'cosine': (dict(kind='cosine', decay_iters=T_COS, min_lr=1e-6),
               lambda opt: torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_COS, eta_min=1e-6)),
    'exponential': (dict(kind='exponential', gamma=0.997), lambda opt: torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.997)),
    'step': (dict(kind='step', gamma=0.5, milestones=(1, 2, 40, 40, 700, 1999)),
             lambda opt: torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1, 2, 40, 40, 700, 1999], gamma=0.5)),
}


def torch_rates(make, W, s0, steps):
    """param_groups[0]['lr'] at last_epoch = 0 .. steps - 1 of SequentialLR([LinearLR(s0, 1, W), X], [W]) (W = 0: X alone)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if W:
            lin = torch.optim.lr_scheduler.LinearLR(opt, start_factor=s0, end_factor=1.0, total_iters=W)
            sched = torch.optim.lr_scheduler.SequentialLR(opt, [lin, make(opt)], milestones=[W])
        else:
            sched = make(opt)
        out = []
        for _ in range(steps):
            out.append(opt.param_groups[0]['lr'])
            opt.step()
            sched.step()
    return out


@pytest.mark.parametrize('W', [0, 7])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_value_is_torchs_sequential_lr(kind, W):
    kwargs, make = KINDS[kind]
    s0 = 0.25
    sch = LRSchedule(warmup_iters=W, warmup_start=s0, **kwargs)
    want = torch_rates(make, W, s0, STEPS)
    worst = 0.0
    for k, lr in enumerate(want):
        if kind == 'cosine' and k - W > T_COS:
            continue                                           # torch is periodic past T; this schedule holds eta_min (below)
        got = sch.value(k, BASE)
        if kind in ('constant', 'step') and W == 0:
            assert got == lr, (k, got, lr)                     # (gamma = 0.5: torch's running product is exact too)
        worst = max(worst, abs(got - lr) / abs(lr))
    print('%s W=%d: worst relative distance from torch %.3g' % (kind, W, worst))
    assert worst <= RTOL, worst
    if kind == 'constant' and W == 0:
        assert all(sch.value(k, BASE) == BASE for k in range(50))
    if kind == 'cosine':
        # after T the rate IS eta_min, exactly and for good (torch's climbs again)
        for k in (W + T_COS, W + T_COS + 1, W + T_COS + 5, W + 3 * T_COS, 2 ** 31 + 7):
            assert sch.value(k, BASE) == 1e-6
        assert want[W + T_COS + 5] > 1e-6 if W + T_COS + 5 < STEPS else True
    if W:
        assert sch.value(0, BASE) == BASE * s0 and sch.value(W, BASE) == want[W]


def test_value_edges():
    sch = LRSchedule('step', gamma=0.1, milestones=(0, 3))
    assert sch.value(0, 1.0) == 0.1 and sch.value(2, 1.0) == 0.1 and sch.value(3, 1.0) == 1.0 * math.pow(0.1, 2.0)
    assert LRSchedule('exponential', gamma=0.999).value(2 ** 31 + 6, 1.0) == 0.0
    assert LRSchedule('exponential', gamma=2.0).value(5000, 1.0) == math.inf
    assert LRSchedule('constant', warmup_iters=4, warmup_start=1.0).value(2, 0.5) == 0.5
    with pytest.raises(ValueError, match='device'):
        LRSchedule('device').value(0, 1.0)
    d = LRSchedule('cosine', warmup_iters=3, decay_iters=4, min_lr=1e-5).state_dict()
    assert LRSchedule(**d) == LRSchedule('cosine', warmup_iters=3, decay_iters=4, min_lr=1e-5)
    assert set(d) == {'kind', 'warmup_iters', 'warmup_start', 'decay_iters', 'min_lr', 'gamma', 'milestones'}
    assert all(isinstance(v, (str, int, float, list, type(None))) for v in d.values())
    assert SC.ema_decay_at(0.999, 1, True) == 2.0 / 11.0 and SC.ema_decay_at(0.999, 10 ** 6, True) == 0.999
    assert SC.ema_decay_at(0.9, 1, False) == 0.9


@pytest.mark.parametrize('kwargs, name', [
    (dict(kind='linear'), 'kind'),
    (dict(warmup_iters=-1), 'warmup_iters'),
    (dict(warmup_iters=2.5), 'warmup_iters'),
    (dict(warmup_iters=True), 'warmup_iters'),
    (dict(warmup_start=0.0), 'warmup_start'),
    (dict(warmup_start=1.5), 'warmup_start'),
    (dict(warmup_start=float('nan')), 'warmup_start'),
    (dict(warmup_start='x'), 'warmup_start'),
    (dict(kind='cosine'), 'decay_iters'),
    (dict(kind='cosine', decay_iters=0), 'decay_iters'),
    (dict(kind='cosine', decay_iters=-3), 'decay_iters'),
    (dict(kind='cosine', decay_iters=10.0), 'decay_iters'),
    (dict(kind='cosine', decay_iters=10, min_lr=float('inf')), 'min_lr'),
    (dict(kind='exponential', gamma=0.0), 'gamma'),
    (dict(kind='exponential', gamma=-0.5), 'gamma'),
    (dict(kind='exponential', gamma=float('nan')), 'gamma'),
    (dict(kind='step', milestones=(5, 3)), 'milestones'),
    (dict(kind='step', milestones=tuple(range(9))), 'milestones'),
    (dict(kind='step', milestones=(1.5,)), 'milestones'),
    (dict(kind='step', milestones=(-1,)), 'milestones'),
    (dict(kind='step', milestones=4), 'milestones'),
    (dict(kind='device', warmup_iters=3), 'warmup_iters'),
])
def test_schedule_validation_names_the_argument(kwargs, name):
    with pytest.raises(ValueError, match=name):
        LRSchedule(**kwargs)


@pytest.mark.parametrize('bad', [1.0, -0.1, 1.5, float('nan'), 'x', True, [0.5]])
def test_trainstep_refuses_a_bad_ema_decay(bad):
    from genesis_amd.trainer import TrainStep
    with pytest.raises(ValueError, match='ema_decay'):
        TrainStep(None, 64, ema_decay=bad)                    # (refused before the model is looked at)
    with pytest.raises(ValueError, match='ema_decay'):
        SC.check_ema_decay(bad)
    assert SC.check_ema_decay(None) is None and SC.check_ema_decay(0) == 0.0 and SC.check_ema_decay(np.float32(0.5)) == 0.5


def test_trainstep_refuses_bad_schedule_arguments():
    from genesis_amd.trainer import TrainStep
    with pytest.raises(ValueError, match='lr_schedule'):
        TrainStep(None, 64, lr_schedule='cosine')
    with pytest.raises(ValueError, match='ema_warmup'):
        TrainStep(None, 64, ema_warmup=True)


def test_constants_match_the_header():
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    sched = {k: int(v) for k, v in re.findall(r'#define GX_SCHED_(\w+) (\d+)', header)}
    assert sorted(sched) == sorted(['CONSTANT', 'COSINE', 'EXPONENTIAL', 'STEP', 'DEVICE', 'KIND', 'BASE', 'WARMUP', 'START', 'T', 'ETA_MIN',
                                    'GAMMA', 'N_MILESTONES', 'MILESTONE0', 'MAX_MILESTONES', 'WORDS'])
    for name, v in sched.items():
        assert getattr(SC, name) == v, name
    assert SC.MILESTONE0 + SC.MAX_MILESTONES == SC.WORDS
    assert SC.KINDS == {'constant': SC.CONSTANT, 'cosine': SC.COSINE, 'exponential': SC.EXPONENTIAL, 'step': SC.STEP, 'device': SC.DEVICE}
    tail = {k: int(v) for k, v in re.findall(r'#define GX_TAIL_(\w+) (\d+)', header)}
    assert tail == {'LR': SC.TAIL_LR, 'DECAY': SC.TAIL_DECAY, 'BYTES': SC.TAIL_BYTES} and SC.TAIL_DECAY + 8 == SC.TAIL_BYTES
    ema = {k: int(v) for k, v in re.findall(r'#define GX_EMA_(\w+) (\d+)', header)}
    assert sorted(ema) == sorted(['FP32', 'FP64', 'D_SRC', 'D_DST', 'D_N', 'D_DTYPE', 'D_WORK', 'DESC_WORDS', 'CHUNK', 'MAX_GRID'])
    for name, v in ema.items():
        assert getattr(E, name) == v, name
    # the words as the launch receives them
    w = LRSchedule('step', warmup_iters=7, warmup_start=0.25, gamma=0.5, milestones=(3, 9)).words(BASE)
    assert w.dtype == np.float64 and w.shape == (SC.WORDS,)
    assert (w[SC.KIND], w[SC.BASE], w[SC.WARMUP], w[SC.START], w[SC.GAMMA], w[SC.N_MILESTONES]) == (SC.STEP, BASE, 7.0, 0.25, 0.5, 2.0)
    assert list(w[SC.MILESTONE0:SC.MILESTONE0 + 3]) == [3.0, 9.0, 0.0]
    w = LRSchedule('cosine', decay_iters=11, min_lr=1e-6).words(1.0)
    assert (w[SC.KIND], w[SC.T], w[SC.ETA_MIN]) == (SC.COSINE, 11.0, 1e-6)
    table, work = E.make_table([(4096, 8192, 1, E.FP32), (4096, 8192, E.CHUNK + 1, E.FP64), (4096, 8192, 5, E.FP32)])
    assert work == 4 and [int(x) for x in table[:, E.D_WORK]] == [0, 1, 3] and table.shape == (3, E.DESC_WORDS)


# ---- refusals of the entry points, with fake device addresses (validation reads no device memory) --------------------------------
FAKE = 4096
P = ctypes.c_void_p(FAKE)


def _words(**over):
    w = LRSchedule('constant').words(1e-3)
    for k, v in over.items():
        w[getattr(SC, k)] = v
    return w


def _adam_ex(w=None, lr_dev=None, record=None, ema32=None, ema64=None, decay=0.9, tail=P, n32=8, n64=0, p64=None, step=P, p32=P):
    w = _words() if w is None else w
    _lib.call('gx_adam_step_pair_ex', p32, P, P, P, n32, p64, p64, p64, p64, n64, step, ctypes.c_void_p(w.ctypes.data), lr_dev, 0.9, 0.999,
              1e-8, 1.0, record, ema32, ema64, decay, 0, tail, 1, None)


def _opt_ex(w=None, lr_dev=None, record=None, ema32=None, ema64=None, decay=0.9, tail=P, n32=8, n64=0, p64=None, step=P, p32=P, kind=1):
    w = _words() if w is None else w
    _lib.call('gx_optimiser_step_pair_ex', kind, p32, P, P, n32, p64, p64, p64, n64, step, ctypes.c_void_p(w.ctypes.data), lr_dev, 0.99,
              1e-8, 1.0, record, ema32, ema64, decay, 0, tail, 1, None)


EX_REFUSALS = [
    (dict(p32=None), 'null pointer / empty fp32 group'),
    (dict(n32=0), 'null pointer / empty fp32 group'),
    (dict(step=None), 'null pointer'),
    (dict(n64=4), 'null fp64 pointer'),
    (dict(tail=None), 'null or misaligned tail record'),
    (dict(tail=ctypes.c_void_p(FAKE + 4)), 'null or misaligned tail record'),
    (dict(record=ctypes.c_void_p(FAKE + 4)), 'misaligned guard record'),
    (dict(ema32=P, decay=1.0), r'decay = 1 outside \[0, 1\)'),
    (dict(ema32=P, decay=-0.1), r'decay = -0.1 outside \[0, 1\)'),
    (dict(ema32=P, decay=float('nan')), 'decay = nan outside'),
    (dict(ema32=P, n64=4, p64=P), 'null ema64 with an fp64 group of 4 elements'),
    (dict(ema64=P), 'ema64 without ema32'),
    (dict(w=_words(KIND=7)), 'unknown schedule kind 7'),
    (dict(w=_words(WARMUP=-1)), 'W = -1'),
    (dict(w=_words(WARMUP=2.5)), 'W = 2.5'),
    (dict(w=_words(KIND=SC.COSINE, T=0)), 'T = 0'),
    (dict(w=_words(KIND=SC.COSINE, T=-4)), 'T = -4'),
    (dict(w=_words(KIND=SC.EXPONENTIAL, GAMMA=0)), 'gamma = 0'),
    (dict(w=_words(KIND=SC.STEP, GAMMA=-2)), 'gamma = -2'),
    (dict(w=_words(KIND=SC.STEP, N_MILESTONES=9)), '9 milestones, at most 8'),
    (dict(w=LRSchedule('step', milestones=(1, 5, 9)).words(1.0)[[0, 1, 2, 3, 4, 5, 6, 7, 9, 8, 10, 11, 12, 13, 14, 15]].copy()),
     'milestones are not in ascending order'),
    (dict(w=_words(START=0)), r's0 = 0 outside \(0, 1\]'),
    (dict(w=_words(START=1.25)), r's0 = 1.25 outside \(0, 1\]'),
    (dict(w=_words(KIND=SC.DEVICE)), 'device schedule needs an 8-byte aligned lr_dev'),
    (dict(w=_words(KIND=SC.DEVICE), lr_dev=ctypes.c_void_p(FAKE + 4)), 'device schedule needs an 8-byte aligned lr_dev'),
    (dict(w=_words(BASE=float('inf'))), 'base rate inf is not finite'),
    (dict(w=_words(BASE=float('nan'))), 'base rate nan is not finite'),
]


@pytest.mark.parametrize('kwargs, message', EX_REFUSALS)
def test_ex_entry_points_refuse_before_launching(kwargs, message):
    with pytest.raises(GenesisHipError, match='gx_adam_step_pair_ex.*' + message):
        _adam_ex(**kwargs)
    with pytest.raises(GenesisHipError, match='gx_optimiser_step_pair_ex.*' + message):
        _opt_ex(**kwargs)


def test_optimiser_ex_refuses_an_unknown_kind():
    with pytest.raises(GenesisHipError, match='kind must be 1'):
        _opt_ex(kind=3)
    with pytest.raises(GenesisHipError, match='null schedule descriptor'):
        _lib.call('gx_adam_step_pair_ex', P, P, P, P, 8, None, None, None, None, 0, P, None, None, 0.9, 0.999, 1e-8, 1.0, None, None, None,
                  0.9, 0, P, 1, None)


def _segment(**over):
    row = [0] * E.DESC_WORDS
    fields = dict(SRC=FAKE, DST=2 * FAKE, N=100, DTYPE=E.FP32, WORK=0)
    fields.update(over)
    for k, v in fields.items():
        row[getattr(E, 'D_' + k)] = v
    return row


def _ema(rows, n_segments=None, table_words=None, table_dev=FAKE, step=FAKE, decay=0.9, used=0):
    table = np.array([w for row in rows for w in row], np.int64)
    _lib.call('gx_ema_multi', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(table_dev),
              table.size if table_words is None else table_words, len(rows) if n_segments is None else n_segments, ctypes.c_void_p(step),
              decay, 0, ctypes.c_void_p(used), None)


@pytest.mark.parametrize('rows, kwargs, message', [
    ([_segment()], dict(table_dev=0), 'null descriptor table'),
    ([_segment()], dict(table_dev=FAKE + 4), '8-byte aligned'),
    ([_segment()], dict(n_segments=0), 'n_segments = 0 below 1'),
    ([_segment()], dict(step=0), 'null or misaligned step counter'),
    ([_segment()], dict(step=FAKE + 4), 'null or misaligned step counter'),
    ([_segment()], dict(used=FAKE + 4), 'misaligned decay_used'),
    ([_segment()], dict(decay=1.0), r'decay = 1 outside \[0, 1\)'),
    ([_segment()], dict(decay=-1e-3), r'decay = -0.001 outside'),
    ([_segment()], dict(decay=float('nan')), 'decay = nan outside'),
    ([_segment(N=0)], {}, r'segment 0: N = 0 outside \[1, 2\^31\)'),
    ([_segment(N=1 << 31)], {}, 'segment 0: N = 2147483648 outside'),
    ([_segment(DTYPE=2)], {}, 'segment 0: unknown dtype 2'),
    ([_segment(SRC=0)], {}, 'segment 0: null source or destination'),
    ([_segment(DST=0)], {}, 'segment 0: null source or destination'),
    ([_segment(SRC=FAKE + 2)], {}, 'not aligned to its 4-byte elements'),
    ([_segment(DST=2 * FAKE + 4, DTYPE=1)], {}, 'not aligned to its 8-byte elements'),
    ([_segment(WORK=1)], {}, 'segment 0: WORK = 1, the prefix is 0'),
    ([_segment(N=8193), _segment(WORK=1)], {}, 'segment 1: WORK = 1, the prefix is 2'),
    ([_segment(), _segment(WORK=1)], dict(table_words=9), '2 segments do not fit a table of 9 words'),
])
def test_ema_multi_refuses_before_launching(rows, kwargs, message):
    with pytest.raises(GenesisHipError, match='gx_ema_multi: .*' + message):
        _ema(rows, **kwargs)


def test_model_ema_refusals_name_their_argument():
    import genesis_amd
    model = torch.nn.Linear(3, 2)
    for bad in (1.0, -0.5, float('nan'), 'x', None):
        with pytest.raises(GenesisHipError, match='decay'):
            genesis_amd.ModelEMA(model, bad)
    with pytest.raises(GenesisHipError, match='parameter weight is on cpu'):
        genesis_amd.ModelEMA(model, 0.99)
    with pytest.raises(GenesisHipError, match='no parameters'):
        genesis_amd.ModelEMA(torch.nn.ReLU(), 0.99)
