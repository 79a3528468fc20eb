"""Learning-rate schedules and averaged weights on the GPU: the _ex forms of the two optimiser launches against the existing entry
points bit for bit, the recorded rate against LRSchedule.value, the EMA against the numpy recurrence e + w (p' - e) in the group's
dtype bit for bit, gx_ema_multi, TrainStep(lr_schedule=, ema_decay=, ema_warmup=) on the tiny model and ModelEMA in an eager loop.

Bounds.  The recorded rate: the device's cos / pow are a few ulp of fp64 off Python's, 1e-12 relative (tests/test_lr_ema_cpu.py holds
the closed form to torch's schedulers with the same bar).  Everything else is compared bit for bit: p, m, v are adam_body /
simple_opt_body called with the rate the launch computed, so the existing entry point called with the RECORDED rate must reproduce
them, and the EMA is three roundings in the parameter's type.

What each test would catch (one-line mistakes):

  a rate computed in fp32, or from t instead of k = t - 1       test_ex_schedule_rate_and_update at t = 1, W, W + 1
  the cosine not held after T / the ramp applied to 'device'     test_ex_schedule_rate_and_update at W + T, W + T + 5
  the EMA as one fma, or w formed in fp32                        test_ex_ema_is_the_recurrence (decay 0.9999: 1 - decay in fp32 is 1e-4 off)
  16-byte accesses on an EMA view that is not 16-byte aligned     test_ex_ema_is_the_recurrence (the views start 4 / 8 bytes past one)
  a skipped step that still averages or writes the record        test_ex_not_ok_changes_nothing_but_the_gradients
  a grid-stride loop of the EMA that stops after one trip        test_ex_not_ok / test_ex_constant at one past both grid caps
  EMA / record missing from the capture warm-up's snapshot       test_trainstep_warmup_cosine_eager_equals_graph
  set_lr dropping the captured graph                             test_trainstep_device_rate_under_graph_replay
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import grad_guard_restatement as R
from tests import step_tail_restatement as S
from tests.common import Golden
from tests.test_model_gpu import build

pytestmark = pytest.mark.gpu

hip = pytest.importorskip('genesis_amd.hip_ops')
from genesis_amd import _lib  # noqa: E402
from genesis_amd import ema as E  # noqa: E402
from genesis_amd import grad_guard as gg  # noqa: E402
from genesis_amd import schedule as SC  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.schedule import LRSchedule  # noqa: E402

DEV = 'cuda'
F32, F64 = torch.float32, torch.float64
RTOL = 1e-12
SMALL = ((1, 0), (1023, 1), (1025, 33), (5, 3 * 1024))
BIG = (2048 * 1024 + 1027, 256 * 1024 + 5)                   # one past both grid caps of the optimiser launch
assert BIG in S.PAIR_SIZES and all(s in S.PAIR_SIZES for s in SMALL)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_groups(n32, n64, k, seed):
    b32 = S.GuardedBuffers(n32, F32, k, DEV, seed=seed)
    b64 = S.GuardedBuffers(n64, F64, k, DEV, seed=seed + 1)
    for b in (b32, b64):
        for i in range(2, k):
            b.views[i].abs_()                                  # (moments / square averages: non-negative)
    return b32, b64


def call_plain(opt, b32, b64, n32, n64, step, lr, scale_or_record, zero, guarded):
    """The existing entry point on (p, g, m[, v]) = views 0..3."""
    v32, v64 = b32.views, (b64.views if n64 else [None] * 4)
    arg = P(scale_or_record) if guarded else scale_or_record
    sfx = '_guarded' if guarded else ''
    if opt == 'adam':
        _lib.call('gx_adam_step_pair' + sfx, P(v32[0]), P(v32[1]), P(v32[2]), P(v32[3]), n32, P(v64[0]), P(v64[1]), P(v64[2]),
                  P(v64[3]), n64, P(step), lr, S.BETA1, S.BETA2, S.ADAM_EPS, arg, zero, stream())
    else:
        kind, hp, eps = (1, S.RMS_ALPHA, S.RMS_EPS) if opt == 'rmsprop' else (2, S.SGD_MOMENTUM, 0.0)
        _lib.call('gx_optimiser_step_pair' + sfx, kind, P(v32[0]), P(v32[1]), P(v32[2]), n32, P(v64[0]), P(v64[1]), P(v64[2]), n64,
                  P(step), lr, hp, eps, arg, zero, stream())


def call_ex(opt, b32, b64, n32, n64, step, words, tail, zero, gscale=1.0, record=None, lr_dev=None, ema=(None, None), decay=0.0,
            warm=0):
    """The _ex entry point on the same views; words: LRSchedule.words (kept alive by the caller)."""
    v32, v64 = b32.views, (b64.views if n64 else [None] * 4)
    tail_args = (gscale, P(record), P(ema[0]), P(ema[1]) if n64 else None, decay, warm, P(tail), zero, stream())
    sched = ctypes.c_void_p(words.ctypes.data)
    if opt == 'adam':
        _lib.call('gx_adam_step_pair_ex', P(v32[0]), P(v32[1]), P(v32[2]), P(v32[3]), n32, P(v64[0]), P(v64[1]), P(v64[2]), P(v64[3]),
                  n64, P(step), sched, P(lr_dev), S.BETA1, S.BETA2, S.ADAM_EPS, *tail_args)
    else:
        kind, hp, eps = (1, S.RMS_ALPHA, S.RMS_EPS) if opt == 'rmsprop' else (2, S.SGD_MOMENTUM, 0.0)
        _lib.call('gx_optimiser_step_pair_ex', kind, P(v32[0]), P(v32[1]), P(v32[2]), n32, P(v64[0]), P(v64[1]), P(v64[2]), n64,
                  P(step), sched, P(lr_dev), hp, eps, *tail_args)


def new_tail():
    return torch.full((2,), -7.0, dtype=F64, device=DEV)


def whole_equal(A, B):
    return all(torch.equal(a.whole.view(a.bits), b.whole.view(b.bits)) for a, b in zip(A, B))


def ema_ref(e, p, decay_t):
    """e + w (p - e), every operation rounded in the arrays' dtype (numpy does not contract)."""
    w = e.dtype.type(1.0 - decay_t)
    d = p - e
    return e + w * d


def close(got, want):
    return abs(got - want) <= RTOL * abs(want)


# ------------------------------------------------------------------------------------------------- 1. the _ex launches
CASES = [(n32, n64, zero, opt) for (n32, n64) in SMALL for zero in (0, 1) for opt in ('adam', 'rmsprop', 'sgd')] + \
    [BIG + (1, 'adam')]


@pytest.mark.parametrize('guarded', [False, True])
@pytest.mark.parametrize('n32,n64,zero,opt', CASES)
def test_ex_constant_without_ema_matches_the_existing_entry_point(n32, n64, zero, opt, guarded):
    """Three steps: the _ex launch with a constant schedule on one set of buffers, the existing entry point (guarded against guarded,
    unguarded against unguarded) on a twin: the same bits in p, m, v and g, guard bands untouched, the counter left alone."""
    p32, p64, grads = S.optimiser_inputs(n32, n64, 3)
    A, B = make_groups(n32, n64, 4, 21), make_groups(n32, n64, 4, 21)
    for (a32, a64) in (A, B):
        a32.views[0].copy_(p32); a64.views[0].copy_(p64)
    guard = gg.GradGuard([A[0].views[1]] + ([A[1].views[1]] if n64 else [])) if guarded else None
    words = LRSchedule('constant').words(S.LR)
    tail = new_tail()
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    for it, (g32, g64) in enumerate(grads):
        for (a32, a64) in (A, B):
            a32.views[1].copy_(g32); a64.views[1].copy_(g64)
        snaps = [b.snapshot() for b in A + B]
        gs = S.GRAD_SCALES[it + 1]
        _lib.call('gx_step_increment', P(step), stream())
        if guarded:
            guard.run(gs, 0.5 * gs * np.sqrt(R.sum_squares([g32.numpy(), g64.numpy()])))
            call_ex(opt, A[0], A[1], n32, n64, step, words, tail, zero, gscale=123.0, record=guard.record)      # (gscale: ignored)
            call_plain(opt, B[0], B[1], n32, n64, step, S.LR, guard.record, zero, True)
        else:
            call_ex(opt, A[0], A[1], n32, n64, step, words, tail, zero, gscale=gs)
            call_plain(opt, B[0], B[1], n32, n64, step, S.LR, gs, zero, False)
        assert int(step) == it + 1
        assert whole_equal(A, B), 'step %d: the buffers differ' % (it + 1)
        for b, snap in zip(A + B, snaps):
            assert b.guards_unchanged(snap)
        assert tail.cpu().tolist() == [S.LR, 0.0]
        if zero:
            assert S.same_bits(A[0].views[1], torch.zeros_like(A[0].views[1]))
        else:
            assert S.same_bits(A[0].views[1].cpu(), g32)


W_, T_ = 7, 20
SCHEDULES = {
    'warmup': LRSchedule('constant', warmup_iters=W_, warmup_start=0.25),
    'cosine': LRSchedule('cosine', warmup_iters=W_, warmup_start=0.25, decay_iters=T_, min_lr=1e-6),
    'exponential': LRSchedule('exponential', warmup_iters=W_, warmup_start=0.25, gamma=0.97),
    'step': LRSchedule('step', warmup_iters=W_, warmup_start=0.25, gamma=0.5, milestones=(0, 1, T_, T_, T_ + 5)),
    'device': LRSchedule('device'),
}
TS = (1, W_, W_ + 1, W_ + T_, W_ + T_ + 5, 2 ** 31 + 7)


@pytest.mark.parametrize('opt', ['adam', 'rmsprop', 'sgd'])
@pytest.mark.parametrize('kind', sorted(SCHEDULES))
def test_ex_schedule_rate_and_update(kind, opt):
    """At every t of TS (the counter set to it): the recorded rate within 1e-12 of LRSchedule.value(t - 1), and p, m, v, g the bits of
    the existing entry point called with the recorded rate."""
    n32, n64 = 1025, 33
    sch = SCHEDULES[kind]
    words = sch.words(S.LR)
    lr_dev = torch.tensor(7.5e-4, dtype=F64, device=DEV)
    p32, p64, grads = S.optimiser_inputs(n32, n64, 1)
    A, B = make_groups(n32, n64, 4, 41), make_groups(n32, n64, 4, 41)
    tail = new_tail()
    seen = []
    for t in TS:
        step = torch.full((), t, dtype=torch.int64, device=DEV)
        for (a32, a64) in (A, B):
            a32.views[0].copy_(p32); a64.views[0].copy_(p64)
            a32.views[1].copy_(grads[0][0]); a64.views[1].copy_(grads[0][1])
        call_ex(opt, A[0], A[1], n32, n64, step, words, tail, 1, gscale=0.5, lr_dev=lr_dev)
        lr, dec = tail.cpu().tolist()
        want = 7.5e-4 if kind == 'device' else sch.value(t - 1, S.LR)
        print('%s t=%d: lr %r, closed form %r' % (kind, t, lr, want))
        assert close(lr, want), (kind, t, lr, want)
        if kind == 'device':
            assert lr == 7.5e-4
        assert dec == 0.0 and int(step) == t
        call_plain(opt, B[0], B[1], n32, n64, step, lr, 0.5, 1, False)
        assert whole_equal(A, B), '%s t=%d: not the existing launch at the recorded rate' % (kind, t)
        seen.append(lr)
    if kind == 'cosine':
        # t = W + T is j = T - 1, the last step of the descent; from j = T on the rate is held at eta_min, exactly
        assert seen[3] > 1e-6 and seen[4] == 1e-6 and seen[5] == 1e-6
        assert seen[0] == S.LR * 0.25 and seen[2] > seen[1]
    if kind == 'warmup':
        assert seen[0] == S.LR * 0.25 and seen[2:] == [S.LR] * 4 and seen[1] < S.LR


EMA_CASES = [(0.0, 0, 3), (0.9, 0, 3), (0.9999, 0, 3), (0.9999, 1, 1), (0.9999, 1, 50), (0.9999, 1, 10 ** 6)]


@pytest.mark.parametrize('opt', ['adam', 'rmsprop', 'sgd'])
@pytest.mark.parametrize('decay,warm,t', EMA_CASES)
def test_ex_ema_is_the_recurrence(decay, warm, t, opt):
    """e' = e + w (p' - e) in the group's dtype, bit for bit, on EMA views that start 4 (fp32) / 8 (fp64) bytes past a 16-byte
    boundary; decay_t in the record exact; p, m, v, g the bits of the existing entry point."""
    n32, n64 = 1025, 33
    p32, p64, grads = S.optimiser_inputs(n32, n64, 1)
    A, B = make_groups(n32, n64, 4, 51), make_groups(n32, n64, 4, 51)
    e32b, e64b = S.GuardedBuffers(n32 + 1, F32, 1, DEV, seed=53), S.GuardedBuffers(n64 + 1, F64, 1, DEV, seed=54)
    e32, e64 = e32b.views[0][1:], e64b.views[0][1:]
    assert e32.data_ptr() % 16 == 4 and e64.data_ptr() % 16 == 8
    for (a32, a64) in (A, B):
        a32.views[0].copy_(p32); a64.views[0].copy_(p64)
        a32.views[1].copy_(grads[0][0]); a64.views[1].copy_(grads[0][1])
    before = (e32.cpu().numpy().copy(), e64.cpu().numpy().copy())
    snaps = (e32b.snapshot(), e64b.snapshot())
    step = torch.full((), t, dtype=torch.int64, device=DEV)
    tail = new_tail()
    words = LRSchedule('constant').words(S.LR)
    call_ex(opt, A[0], A[1], n32, n64, step, words, tail, 1, gscale=0.5, ema=(e32, e64), decay=decay, warm=warm)
    call_plain(opt, B[0], B[1], n32, n64, step, S.LR, 0.5, 1, False)
    assert whole_equal(A, B)
    lr, dec = tail.cpu().tolist()
    decay_t = SC.ema_decay_at(decay, t, warm)
    assert lr == S.LR and dec == decay_t, (dec, decay_t)
    if warm:
        assert decay_t == (min(decay, 2.0 / 11.0) if t == 1 else min(decay, (1.0 + t) / (10.0 + t)))
    for e, was, p, bits in ((e32, before[0], A[0].views[0], np.int32), (e64, before[1], A[1].views[0], np.int64)):
        want = ema_ref(was, p.cpu().numpy(), decay_t)
        assert want.dtype == was.dtype
        assert np.array_equal(e.cpu().numpy().view(bits), want.view(bits)), 'the %s EMA is not the recurrence' % was.dtype
        if decay == 0.0:
            assert np.array_equal(e.cpu().numpy().view(bits), (was + (p.cpu().numpy() - was)).view(bits))
    for b, snap in ((e32b, snaps[0]), (e64b, snaps[1])):
        assert b.guards_unchanged(snap)
        assert S.same_bits(b.views[0][:1], snap[S.GUARD:S.GUARD + 1])      # the element in front of the view


@pytest.mark.parametrize('opt', ['adam', 'rmsprop', 'sgd'])
@pytest.mark.parametrize('zero', [0, 1])
def test_ex_not_ok_changes_nothing_but_the_gradients(zero, opt):
    """A NaN among the gradients, one past both grid caps: p, m, v, the EMA, the tail record and the counter keep their bits; g is all
    +0 with the zeroing flag and bit-unchanged without it."""
    n32, n64 = BIG
    b32, b64 = make_groups(n32, n64, 5, 31)                    # view 4: the EMA
    b32.views[1][n32 - 2] = float('nan')
    step = torch.full((), 2 ** 31 + 7, dtype=torch.int64, device=DEV)
    guard = gg.GradGuard([b32.views[1], b64.views[1]])
    guard.run(0.5, 1.0)
    assert int(guard.ok) == 0
    tail = new_tail()
    words = SCHEDULES['cosine'].words(S.LR)
    before = [b.snapshot() for b in (b32, b64)]
    call_ex(opt, b32, b64, n32, n64, step, words, tail, zero, record=guard.record, ema=(b32.views[4], b64.views[4]), decay=0.9, warm=1)
    assert int(step) == 2 ** 31 + 7 and tail.cpu().tolist() == [-7.0, -7.0]
    for b, snap in ((b32, before[0]), (b64, before[1])):
        assert b.guards_unchanged(snap)
        stride = b.n + 2 * S.GUARD
        for i in range(5):
            got, was = b.views[i], snap[i * stride + S.GUARD:i * stride + S.GUARD + b.n]
            if i == 1 and zero:
                assert S.same_bits(got, torch.zeros_like(got)), 'gradients not all +0'
            else:
                assert S.same_bits(got, was), 'buffer %d changed in a skipped step' % i
    # the same launch with a record that is ok: the EMA of the whole group moves (every thread's strided second trip included)
    b32.views[1].normal_(); b64.views[1].normal_()
    guard.run(0.5, None)
    assert int(guard.ok) == 1
    e_was = (b32.views[4].cpu().numpy().copy(), b64.views[4].cpu().numpy().copy())
    call_ex(opt, b32, b64, n32, n64, step, words, tail, zero, record=guard.record, ema=(b32.views[4], b64.views[4]), decay=0.9, warm=1)
    lr, dec = tail.cpu().tolist()
    assert lr == 1e-6 and dec == 0.9
    for b, was, bits in ((b32, e_was[0], np.int32), (b64, e_was[1], np.int64)):
        want = ema_ref(was, b.views[0].cpu().numpy(), 0.9)
        assert np.array_equal(b.views[4].cpu().numpy().view(bits), want.view(bits))


# ------------------------------------------------------------------------------------------------- 2. gx_ema_multi
def test_ema_multi_mixed_segments():
    """fp32 and fp64 segments: one element, one past a chunk, one that starts 4 bytes past a 16-byte boundary; the same bits as the
    recurrence, decay_t exact, the bytes around every destination untouched, the sources unchanged."""
    lens = [(1, F32, 0), (E.CHUNK + 1, F64, 0), (2 * E.CHUNK + 5, F32, 1), (33, F64, 1), (E.CHUNK, F32, 0)]
    srcs = [S.GuardedBuffers(n + sh, dt, 1, DEV, seed=60 + i) for i, (n, dt, sh) in enumerate(lens)]
    dsts = [S.GuardedBuffers(n + sh, dt, 1, DEV, seed=70 + i) for i, (n, dt, sh) in enumerate(lens)]
    sv = [b.views[0][sh:] for b, (_, _, sh) in zip(srcs, lens)]
    dv = [b.views[0][sh:] for b, (_, _, sh) in zip(dsts, lens)]
    assert dv[2].data_ptr() % 16 == 4 and dv[3].data_ptr() % 16 == 8 and dv[0].numel() == 1
    table, work = E.make_table([(s.data_ptr(), d.data_ptr(), s.numel(), E.FP32 if s.dtype == F32 else E.FP64) for s, d in zip(sv, dv)])
    assert work == 1 + 2 + 3 + 1 + 1
    table_dev = torch.from_numpy(table).to(DEV)
    step = torch.full((), 48, dtype=torch.int64, device=DEV)
    used = torch.full((), -1.0, dtype=F64, device=DEV)
    for decay, warm in ((0.9, False), (0.9999, True), (0.0, False)):
        was = [d.cpu().numpy().copy() for d in dv]
        snaps = [b.snapshot() for b in srcs + dsts]
        _lib.call('gx_step_increment', P(step), stream())
        E.ema_multi(table, table_dev, step, decay, warm, used)
        t = int(step)
        decay_t = SC.ema_decay_at(decay, t, warm)
        assert float(used) == decay_t and (not warm or decay_t == (1.0 + t) / (10.0 + t))
        for s, d, w in zip(sv, dv, was):
            bits = np.int32 if w.dtype == np.float32 else np.int64
            want = ema_ref(w, s.cpu().numpy(), decay_t)
            assert np.array_equal(d.cpu().numpy().view(bits), want.view(bits)), 'segment of %d %s' % (w.size, w.dtype)
        for b, snap in zip(srcs + dsts, snaps):
            assert b.guards_unchanged(snap)
        for b, snap, (_, _, sh) in zip(dsts, snaps[len(srcs):], lens):
            assert S.same_bits(b.views[0][:sh], snap[S.GUARD:S.GUARD + sh])
        for b, snap in zip(srcs, snaps):
            assert torch.equal(b.whole.view(b.bits), snap.view(b.bits))
    # refusals arrive before any launch: the destinations and the decay word keep their bits
    snaps = [b.snapshot() for b in dsts]
    used_was = float(used)

    def row(**over):
        tab = table.copy()
        for k, v in over.items():
            tab[1, getattr(E, 'D_' + k)] = v
        return tab

    for tab, decay, message in ((table, 1.0, 'decay = 1 outside'), (table, -0.5, 'decay = -0.5 outside'), (row(N=0), 0.5, 'segment 1: N = 0'),
                                (row(DST=0), 0.5, 'segment 1: null source or destination'), (row(DTYPE=3), 0.5, 'unknown dtype 3'),
                                (row(DST=int(table[1, E.D_DST]) + 4), 0.5, 'not aligned to its 8-byte elements'),
                                (row(WORK=5), 0.5, 'segment 1: WORK = 5')):
        with pytest.raises(GenesisHipError, match=message):
            E.ema_multi(tab, table_dev, step, decay, False, used)
    with pytest.raises(GenesisHipError, match='null or misaligned step counter'):
        _lib.call('gx_ema_multi', ctypes.c_void_p(table.ctypes.data), P(table_dev), table.size, table.shape[0], None, 0.5, 0, P(used), stream())
    torch.cuda.synchronize()
    assert float(used) == used_was
    for b, snap in zip(dsts, snaps):
        assert torch.equal(b.whole.view(b.bits), snap.view(b.bits))


def test_ex_refusals_leave_the_buffers_alone():
    n32, n64 = 1025, 33
    b32, b64 = make_groups(n32, n64, 5, 81)
    step = torch.full((), 3, dtype=torch.int64, device=DEV)
    tail = new_tail()
    before = [b.snapshot() for b in (b32, b64)]
    good = LRSchedule('constant').words(S.LR)

    def words(**over):
        w = good.copy()
        for k, v in over.items():
            w[getattr(SC, k)] = v
        return w

    ema = (b32.views[4], b64.views[4])
    for opt in ('adam', 'sgd'):
        for kwargs, message in ((dict(words=words(KIND=SC.DEVICE)), 'needs an 8-byte aligned lr_dev'),
                                (dict(words=words(KIND=SC.COSINE, T=0)), 'T = 0'), (dict(words=words(START=0.0)), 's0 = 0 outside'),
                                (dict(words=words(BASE=float('nan'))), 'not finite'), (dict(words=words(WARMUP=-2)), 'W = -2'),
                                (dict(words=good, ema=ema, decay=1.0), 'decay = 1 outside'),
                                (dict(words=good, ema=(ema[0], None)), 'null ema64 with an fp64 group of 33 elements')):
            with pytest.raises(GenesisHipError, match=message):
                call_ex(opt, b32, b64, n32, n64, step, tail=tail, zero=1, **kwargs)
    torch.cuda.synchronize()
    assert tail.cpu().tolist() == [-7.0, -7.0]
    for b, snap in zip((b32, b64), before):
        assert torch.equal(b.whole.view(b.bits), snap.view(b.bits))


# ------------------------------------------------------------------------------------------------- 3. TrainStep on the tiny model
LR0 = 1e-3


def _seed(s=5):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def cosine():
    return LRSchedule('cosine', warmup_iters=3, warmup_start=0.25, decay_iters=4, min_lr=1e-6)


def bits_of(ts):
    """Parameters and averaged weights (when kept) as host clones."""
    out = [ts.flat_p.clone().cpu(), ts.flat_p64.clone().cpu()]
    if ts.ema32 is not None:
        out += [ts.ema32.clone().cpu(), ts.ema64.clone().cpu()]
    return out


def all_same(a, b):
    return len(a) == len(b) and all(S.same_bits(u, v) for u, v in zip(a, b))


def run(ts, xs, lrs=None, before=None):
    """step() over xs -> (outputs [n, 4] on the host, current_lr after each step as Python floats or None)."""
    outs, seen = [], []
    for i, x in enumerate(xs):
        if before is not None:
            before(i)
        outs.append(ts.step(x).clone())
        seen.append(float(ts.current_lr) if ts.current_lr is not None else None)
    torch.cuda.synchronize()
    return torch.stack(outs).cpu(), seen


@pytest.fixture(scope='module')
def tiny():
    """The tiny model's input and the six-step trajectories of plain eager TrainSteps (computed once, read only): at the default rate
    and at LR0."""
    from genesis_amd.trainer import TrainStep
    gold = Golden('tiny')
    x, _, _ = gold.inputs()
    xd = x.to(DEV)
    ref = {}
    for lr in (1e-4, LR0):
        plain = TrainStep(build(gold), gold.S, lr=lr, graph=False)
        _seed()
        out, _ = run(plain, [xd] * 6)
        ref[lr] = (out, plain.flat_p.clone().cpu(), plain.flat_p64.clone().cpu())
        keys = set(plain.state_dict(5))
        plain.close()
    return dict(gold=gold, xd=xd, ref=ref, keys=keys)


@pytest.mark.parametrize('graph', [False, True])
def test_trainstep_defaults_issue_the_launches_they_always_have(tiny, graph, monkeypatch):
    from genesis_amd.trainer import TrainStep
    names = []
    orig = _lib.call

    def spy(name, *args):
        names.append(name)
        return orig(name, *args)
    monkeypatch.setattr(_lib, 'call', spy)
    ts = TrainStep(build(tiny['gold']), tiny['gold'].S, graph=graph)
    _seed()
    out, lrs = run(ts, [tiny['xd']] * 6)
    new = ('gx_adam_step_pair_ex', 'gx_optimiser_step_pair_ex', 'gx_ema_multi')
    assert 'gx_adam_step_pair' in names and not [n for n in names if n in new]
    assert torch.equal(out, tiny['ref'][1e-4][0]) and S.same_bits(ts.flat_p.cpu(), tiny['ref'][1e-4][1])
    assert ts.current_lr is None and ts.ema_decay_used is None and lrs == [None] * 6 and ts.ema32 is None
    assert set(ts.state_dict(5)) == tiny['keys'] == {'model_state_dict', 'optimiser_state_dict', 'beta', 'err_ema', 'iter_idx'}
    assert 'initial_lr' not in ts.state_dict(5)['optimiser_state_dict']['param_groups'][0]
    for call in (ts.ema_weights, ts.ema_state_dict, lambda: ts.set_lr(1e-3)):
        with pytest.raises(GenesisHipError):
            call()
    ts.close()


@pytest.mark.parametrize('graph', [False, True])
def test_trainstep_constant_schedule_with_ema_keeps_the_trajectory(tiny, graph, monkeypatch):
    """Outputs and parameters: the plain trajectory's bits.  The EMA after every step: the recurrence over that step's parameters, fp32
    group and the fp64 log_sigma group alike.  One _ex launch per step, no other optimiser launch."""
    from genesis_amd.trainer import TrainStep
    names = []
    orig = _lib.call

    def spy(name, *args):
        names.append(name)
        return orig(name, *args)
    ts = TrainStep(build(tiny['gold']), tiny['gold'].S, lr=LR0, graph=graph, lr_schedule=LRSchedule('constant'), ema_decay=0.99)
    assert ts.n64 > 0 and all_same(bits_of(ts)[:2], bits_of(ts)[2:])      # the EMA starts as a copy of the parameters
    _seed()
    outs = []
    for it in range(6):
        e32, e64 = ts.ema32.cpu().numpy().copy(), ts.ema64.cpu().numpy().copy()
        if it == 5 and not graph:
            monkeypatch.setattr(_lib, 'call', spy)
        outs.append(ts.step(tiny['xd']).clone())
        w32, w64 = ema_ref(e32, ts.flat_p.cpu().numpy(), 0.99), ema_ref(e64, ts.flat_p64.cpu().numpy(), 0.99)
        assert np.array_equal(ts.ema32.cpu().numpy().view(np.int32), w32.view(np.int32)), 'step %d, fp32' % (it + 1)
        assert np.array_equal(ts.ema64.cpu().numpy().view(np.int64), w64.view(np.int64)), 'step %d, fp64' % (it + 1)
        assert float(ts.current_lr) == LR0 and float(ts.ema_decay_used) == 0.99
    monkeypatch.setattr(_lib, 'call', orig)
    if not graph:
        opt = [n for n in names if 'adam' in n or 'optimiser' in n or 'ema' in n]
        assert opt == ['gx_adam_step_pair_ex'], opt
    assert torch.equal(torch.stack(outs).cpu(), tiny['ref'][LR0][0])
    assert S.same_bits(ts.flat_p.cpu(), tiny['ref'][LR0][1]) and S.same_bits(ts.flat_p64.cpu(), tiny['ref'][LR0][2])
    assert not S.same_bits(ts.ema32.cpu(), ts.flat_p.cpu())
    assert ts.current_lr.dtype == F64 and ts.current_lr.is_cuda and ts.current_lr.dim() == 0 and ts.ema_decay_used.dtype == F64
    ts.close()


@pytest.mark.parametrize('guard', [False, True])
@pytest.mark.parametrize('opt', ['rmsprop', 'sgd'])
def test_trainstep_other_optimisers_take_the_ex_form_too(tiny, opt, guard):
    """RMSprop / SGD, with and without the gradient guard in front: a constant schedule with an EMA keeps the plain run's bits, the
    EMA is the recurrence, and the schedule's rate reaches the launch (a second run at half the rate through warmup_start)."""
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    kw = dict(lr=1e-5, graph=False, optimiser=opt, skip_nonfinite=guard)
    plain = TrainStep(build(gold), gold.S, **kw)
    ts = TrainStep(build(gold), gold.S, lr_schedule=LRSchedule('constant'), ema_decay=0.9, **kw)
    half = TrainStep(build(gold), gold.S, lr_schedule=LRSchedule('constant', warmup_iters=10 ** 6, warmup_start=0.5), **kw)
    twin = TrainStep(build(gold), gold.S, **dict(kw, lr=0.5e-5))
    _seed()
    outs = [run(t, [xd] * 2)[0] for t in (plain, half, twin)]
    for it in range(2):
        e32, e64 = ts.ema32.cpu().numpy().copy(), ts.ema64.cpu().numpy().copy()
        ts.step(xd)
        w32, w64 = ema_ref(e32, ts.flat_p.cpu().numpy(), 0.9), ema_ref(e64, ts.flat_p64.cpu().numpy(), 0.9)
        assert np.array_equal(ts.ema32.cpu().numpy().view(np.int32), w32.view(np.int32))
        assert np.array_equal(ts.ema64.cpu().numpy().view(np.int64), w64.view(np.int64))
    assert all_same(bits_of(ts)[:2], bits_of(plain)) and float(ts.current_lr) == 1e-5 and float(ts.ema_decay_used) == 0.9
    assert close(float(half.current_lr), 1e-5 * (0.5 + (0.5 * 1.0) / 1e6))
    # (the second step's outputs come from the parameters the first update left: half the rate, exactly the twin's)
    assert torch.equal(outs[1][1], outs[2][1]) and not torch.equal(outs[1][1], outs[0][1])
    assert not all_same(bits_of(half), bits_of(plain))
    if guard:
        assert int(ts.skipped_steps) == 0 and int(half.skipped_steps) == 0
    for t in (plain, ts, half, twin):
        t.close()


def test_trainstep_warmup_cosine_eager_equals_graph(tiny):
    """Warm-up 3 + cosine 4 with a warmed-up EMA: eager and graph replay agree bit for bit (the capture's warm-up iterations leaked
    nothing into the EMA, the counter or the record), current_lr is the closed form, and a plain eager twin whose lr is SET to the
    recorded rate before every step ends with the same parameters."""
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    runs = []
    for graph in (False, True):
        ts = TrainStep(build(gold), gold.S, lr=LR0, graph=graph, lr_schedule=cosine(), ema_decay=0.99, ema_warmup=True)
        _seed()
        out, lrs = run(ts, [xd] * 9)
        runs.append((out, lrs, bits_of(ts), float(ts.ema_decay_used), int(ts.step_t)))
        ts.close()
    (a, la, ba, da, sa), (b, lb, bb, db, sb) = runs
    assert torch.equal(a, b) and la == lb and all_same(ba, bb) and da == db == 10.0 / 19.0 and sa == sb == 9
    for k, lr in enumerate(la):
        want = cosine().value(k, LR0)
        print('k=%d: current_lr %r, closed form %r' % (k, lr, want))
        assert close(lr, want), (k, lr, want)
    assert la[0] == LR0 * 0.25 and close(la[3], LR0) and la[7] == la[8] == 1e-6
    twin = TrainStep(build(gold), gold.S, graph=False)
    _seed()
    out_t, _ = run(twin, [xd] * 9, before=lambda i: setattr(twin, 'lr', la[i]))
    assert torch.equal(out_t, a) and all_same(bits_of(twin), ba[:2])
    twin.close()


@pytest.mark.parametrize('graph', [False, True])
def test_trainstep_skipped_step_advances_neither_schedule_nor_average(tiny, graph):
    """A NaN batch in the middle: parameters, EMA, step counter and current_lr keep their bits over the skipped step; the run then
    continues exactly like a twin that never saw the batch (the noise is keyed by the counter, so it draws the same)."""
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    kw = dict(lr=LR0, graph=graph, skip_nonfinite=True, lr_schedule=cosine(), ema_decay=0.9, ema_warmup=True)
    ts, twin = TrainStep(build(gold), gold.S, **kw), TrainStep(build(gold), gold.S, **kw)
    _seed()
    for t in (ts, twin):
        t.step(xd); t.step(xd)
    state = lambda t: bits_of(t) + [t.m32.cpu(), t.v32.cpu(), t.m64.cpu(), t.v64.cpu(), t.geco.state.cpu(), t._tail.clone().cpu()]      # noqa: E731
    before = state(ts)
    bad = xd.clone()
    bad[0, 0, 0, 0] = float('nan')
    ts.step(bad)
    assert int(ts.skipped_steps) == 1 and int(ts.step_t) == 2
    assert all_same(before, state(ts))
    assert float(ts.current_lr) == cosine().value(1, LR0) or close(float(ts.current_lr), cosine().value(1, LR0))
    x2 = xd.flip(0).contiguous()
    for x in (x2, xd, x2):
        a, b = ts.step(x).clone(), twin.step(x).clone()
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert all_same(state(ts), state(twin))
    assert int(ts.skipped_steps) == 1 and int(twin.skipped_steps) == 0 and int(ts.step_t) == int(twin.step_t) == 5
    assert close(float(ts.current_lr), cosine().value(4, LR0))
    ts.close(); twin.close()


def test_trainstep_device_rate_under_graph_replay(tiny):
    """kind='device': set_lr between replays leaves the captured graph in place, and the result is that of a plain eager twin given
    the same rates."""
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    rates = [1e-3, 5e-4, 2e-3, 1e-4, 1e-4, 7.5e-4]
    ts = TrainStep(build(gold), gold.S, lr=rates[0], graph=True, lr_schedule=LRSchedule('device'), ema_decay=0.9)
    twin = TrainStep(build(gold), gold.S, graph=False)
    _seed()
    graphs = []
    out, lrs = run(ts, [xd] * 6, before=lambda i: (ts.set_lr(rates[i]), graphs.append(ts.graph)))
    assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[1:]) and ts.graph is graphs[1]
    assert lrs == rates
    _seed()
    out_t, _ = run(twin, [xd] * 6, before=lambda i: setattr(twin, 'lr', rates[i]))
    assert torch.equal(out, out_t) and all_same(bits_of(ts)[:2], bits_of(twin))
    sd = ts.state_dict(5)
    g0 = sd['optimiser_state_dict']['param_groups'][0]
    assert g0['lr'] == rates[5] and g0['initial_lr'] == rates[0] and sd['lr_schedule']['kind'] == 'device'
    with pytest.raises(ValueError, match='finite'):
        ts.set_lr(float('nan'))
    ts.close(); twin.close()
    other = TrainStep(build(gold), gold.S, lr_schedule=cosine())
    with pytest.raises(GenesisHipError, match='device'):
        other.set_lr(1e-3)
    other.close()


def test_trainstep_schedule_and_ema_under_a_forced_collective(tiny, monkeypatch):
    """World size 1 with the collective forced into the step: the two-graph (or collective-in-graph) form equals the single-graph run
    bit for bit, EMA and rates included."""
    import torch.distributed as dist
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    kw = dict(lr=LR0, graph=True, lr_schedule=cosine(), ema_decay=0.99, ema_warmup=True)
    single = TrainStep(build(gold), gold.S, **kw)
    _seed()
    want = run(single, [xd] * 6) + (bits_of(single),)
    assert single.graph is not None and single.graph2 is None
    single.close()
    monkeypatch.setenv('GENESIS_FORCE_ALLREDUCE', '1')
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:29548', rank=0, world_size=1)
    try:
        ts = TrainStep(build(gold), gold.S, **kw)
        _seed()
        got = run(ts, [xd] * 6) + (bits_of(ts),)
        assert ts.collective_in_graph or (ts._split and ts.graph2 is not None)
        ts.close()
    finally:
        dist.destroy_process_group()
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and all_same(got[2], want[2])


def test_trainstep_checkpoint_round_trip(tiny):
    """Save after step 3, load into a fresh TrainStep, three more steps == six uninterrupted ones in parameters, EMA and current_lr;
    'lr' / 'initial_lr' as torch's schedulers leave them; a checkpoint without ema_state_dict seeds the EMA from the loaded
    parameters."""
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    xs = [xd, xd.flip(0).contiguous(), xd, xd, xd.flip(0).contiguous(), xd]
    kw = dict(lr=LR0, graph=False, lr_schedule=cosine(), ema_decay=0.9, ema_warmup=True)
    whole = TrainStep(build(gold), gold.S, **kw)
    _seed()
    out_w, lr_w = run(whole, xs)
    first = TrainStep(build(gold), gold.S, **kw)
    _seed()
    out_a, lr_a = run(first, xs[:3])
    sd = first.state_dict(2)
    assert set(sd) == tiny['keys'] | {'ema_state_dict', 'lr_schedule'}
    assert sd['lr_schedule'] == cosine().state_dict() and LRSchedule(**sd['lr_schedule']) == cosine()
    g0 = sd['optimiser_state_dict']['param_groups'][0]
    assert g0['initial_lr'] == LR0 and g0['lr'] == cosine().value(3, LR0) and close(g0['lr'], LR0)
    assert list(sd['ema_state_dict']) == list(sd['model_state_dict'])
    for name, p in first.model.named_parameters():
        assert S.same_bits(sd['ema_state_dict'][name], first._ema_slice(p)) and not sd['ema_state_dict'][name].data_ptr() == first._ema_slice(p).data_ptr()
    sd = {k: (v if k != 'model_state_dict' else {n: t.clone() for n, t in v.items()}) for k, v in sd.items()}
    # resumed with another base rate: the checkpoint's initial_lr wins
    second = TrainStep(build(gold), gold.S, **dict(kw, lr=123.0))
    assert second.load_state_dict(sd) == 3 and second.lr == LR0 and int(second.step_t) == 3
    assert all_same(bits_of(second), bits_of(first))
    _seed()
    out_b, lr_b = run(second, xs[3:])
    assert torch.equal(torch.cat((out_a, out_b)), out_w) and lr_a + lr_b == lr_w
    assert all_same(bits_of(second), bits_of(whole))
    # no averaged weights in the checkpoint: the average starts from the loaded parameters
    third = TrainStep(build(gold), gold.S, **kw)
    _seed()
    run(third, xs[:1])
    bare = {k: v for k, v in sd.items() if k != 'ema_state_dict'}
    third.load_state_dict(bare)
    assert all_same(bits_of(third)[:2], bits_of(first)[:2]) and all_same(bits_of(third)[2:], bits_of(first)[:2])
    for t in (whole, first, second, third):
        t.close()


def test_trainstep_ema_weights_context(tiny):
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    rp, eps = gold.noise(1)
    rp, eps = rp.to(DEV), torch.stack(eps).to(DEV)
    kw = dict(lr=LR0, graph=False, lr_schedule=LRSchedule('constant'), ema_decay=0.9)
    ts, never = TrainStep(build(gold), gold.S, **kw), TrainStep(build(gold), gold.S, **kw)
    _seed()
    out_n, _ = run(never, [xd] * 6)
    _seed()
    out_a, _ = run(ts, [xd] * 3)
    live, avg = bits_of(ts)[:2], bits_of(ts)[2:]
    assert not S.same_bits(live[0], avg[0])
    esd = ts.ema_state_dict()

    def forward(model):
        with torch.no_grad():
            recon, losses, _, _, _ = model(xd, rp, eps)
        return recon.clone(), losses.err.clone()

    live_fwd = forward(ts.model)
    with ts.ema_weights() as m:
        assert m is ts.model and all_same(bits_of(ts)[:2], avg) and all_same(bits_of(ts)[2:], live)
        for name, p in ts.model.named_parameters():
            assert S.same_bits(p.detach(), esd[name])
        inside = forward(ts.model)
        again = ts.ema_state_dict()                            # (asked for inside the block: still the average)
        assert list(again) == list(esd) and all(S.same_bits(again[k], esd[k]) for k in esd if esd[k].is_floating_point())
        with pytest.raises(GenesisHipError, match='ema_weights'):
            ts.step(xd)
        with pytest.raises(GenesisHipError, match='ema_weights'):
            ts.state_dict(2)
    assert all_same(bits_of(ts), live + avg)
    # a freshly built model loaded with ema_state_dict(): the same forward, bit for bit (nothing packed from the live weights was
    # served to the forward inside the block)
    fresh = build(gold)
    fresh.load_state_dict(esd)
    outside = forward(fresh)
    assert S.same_bits(inside[0], outside[0]) and S.same_bits(inside[1], outside[1])
    assert not S.same_bits(inside[0], live_fwd[0])
    after = forward(ts.model)
    assert S.same_bits(after[0], live_fwd[0]) and S.same_bits(after[1], live_fwd[1])
    with pytest.raises(RuntimeError, match='boom'):
        with ts.ema_weights():
            raise RuntimeError('boom')
    assert all_same(bits_of(ts), live + avg) and not ts._in_ema
    _seed()
    out_b, _ = run(ts, [xd] * 3)
    assert torch.equal(torch.cat((out_a, out_b)), out_n) and all_same(bits_of(ts), bits_of(never))
    ts.close(); never.close()


# ------------------------------------------------------------------------------------------------- 4. ModelEMA in an unchanged loop
def test_model_ema_in_an_eager_loop():
    import genesis_amd
    gold = Golden('tiny')
    x, _, _ = gold.inputs()
    model = build(gold)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    ema = genesis_amd.ModelEMA(model, 0.9, warmup=True)
    names = [n for n, _ in model.named_parameters()]
    assert ema.names == names and {p.dtype for p in ema.params} == {F32, F64}
    shadow = [p.detach().cpu().numpy().copy() for p in model.parameters()]
    for it in range(3):
        rp, eps = gold.noise(it + 1)
        opt.zero_grad()
        recon, losses, stats, att, comp = model(x.to(DEV), rp.to(DEV), torch.stack(eps).to(DEV))
        (losses.err.mean(0) + torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()).backward()
        opt.step()
        ema.update()
        decay_t = SC.ema_decay_at(0.9, it + 1, True)
        assert float(ema.decay_used) == decay_t and int(ema.updates) == it + 1
        shadow = [ema_ref(e, p.detach().cpu().numpy(), decay_t) for e, p in zip(shadow, model.parameters())]
        for n, e, want in zip(names, ema.shadow, shadow):
            bits = np.int32 if want.dtype == np.float32 else np.int64
            assert np.array_equal(e.cpu().numpy().view(bits), want.view(bits)), 'update %d: %s' % (it + 1, n)
    live = [p.detach().clone() for p in model.parameters()]
    avg = [e.clone() for e in ema.shadow]
    assert not S.same_bits(live[0], avg[0])
    with pytest.raises(RuntimeError, match='boom'):
        with ema.applied() as m:
            assert m is model
            assert all(S.same_bits(p.detach(), a) for p, a in zip(model.parameters(), avg))
            with pytest.raises(GenesisHipError, match='applied'):
                ema.update()
            raise RuntimeError('boom')
    assert all(S.same_bits(p.detach(), l) for p, l in zip(model.parameters(), live))
    assert all(S.same_bits(e, a) for e, a in zip(ema.shadow, avg))
    sd = ema.state_dict()
    assert list(sd['ema_state_dict']) == names and sd['updates'] == 3 and sd['decay'] == 0.9 and sd['warmup'] is True
    other = genesis_amd.ModelEMA(model, 0.9, warmup=True)
    other.load_state_dict(sd)
    assert int(other.updates) == 3 and all(S.same_bits(e, a) for e, a in zip(other.shadow, avg))
    # refusals
    lin = torch.nn.Linear(4, 6).to(DEV)
    lin.weight.data = torch.zeros(4, 6, device=DEV).t()
    with pytest.raises(GenesisHipError, match='parameter weight .* is not contiguous'):
        genesis_amd.ModelEMA(lin, 0.9)
    with pytest.raises(GenesisHipError, match='parameter weight is torch.float16'):
        genesis_amd.ModelEMA(torch.nn.Linear(4, 6).to(DEV).half(), 0.9)
    with pytest.raises(GenesisHipError, match='parameter weight is on cpu'):
        genesis_amd.ModelEMA(torch.nn.Linear(4, 6), 0.9)
    lin = torch.nn.Linear(4, 6).to(DEV)
    e2 = genesis_amd.ModelEMA(lin, 0.9)
    e2.update()
    lin.extra = torch.nn.Parameter(torch.zeros(3, device=DEV))
    with pytest.raises(GenesisHipError, match='not the ones seen at construction'):
        e2.update()
    del lin.extra
    e2.update()
    lin.weight.data = lin.weight.data.clone()
    with pytest.raises(GenesisHipError, match='not the ones seen at construction'):
        with e2.applied():
            pass
