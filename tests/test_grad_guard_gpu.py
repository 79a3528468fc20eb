"""The gradient guard on the GPU: gx_grad_guard against numpy in fp64 on the same values, the guarded tail launches against the
unguarded entry points bit for bit, TrainStep(max_grad_norm=, skip_nonfinite=) on the tiny model, and the clip_grad_norm_ drop-in
against torch's function (tests/grad_guard_restatement.py restates the record; tests/test_grad_guard_cpu.py pins it to torch).

Bounds.  S: two summation orders of N non-negative fp64 terms differ by at most N * 2^-52 relative.  norm, coef: the fp32 rounding
of the fp64 formula may fall either side of a rounding boundary when S moves in its last bits: 1 ulp of fp32.  Everything else is
compared bit for bit.

What each test would catch (one-line mistakes):

  guard_scan without the element loads at the ragged ends      test_guard_record at every size that is no multiple of 4 / 2,
                                                               test_guard_segment_off_the_16_byte_boundary
  a grid-stride loop that stops after the first trip           test_guard_record[8388609-3] (one past the grid cap)
  guard_final_kernel adding only the first 256 partials        test_guard_record at every size above 256 chunks
  `c < 1 ? c : 1` for the clamp (a NaN norm gives coef 1)       test_guard_extremes, test_drop_in_non_finite_norm_is_torchs
  scale = (float)((double)gscale * c)                          check_record: scale must be the fp32 product of gscale and coef
  the guarded kernels taking gscale from anywhere else         test_guarded_tail_ok_matches_the_unguarded_entry_points
  a skipped step that still bumps the counter / GECO           test_guarded_tail_not_ok_changes_nothing_but_the_gradients
  a warm-up before the capture that leaves its skips counted   test_trainstep_skips_a_non_finite_batch[True]
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
from genesis_amd import grad_guard as gg  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

DEV = 'cuda'
F32, F64 = torch.float32, torch.float64
CHUNK, CAP = gg.CHUNK, gg.MAX_GRID
# the reduction's own seams: one element; one short of / exactly / one past a chunk (in either group); one past the grid cap (every
# workgroup takes a strided second trip)
SEAMS = ((1, 1), (CHUNK - 1, 0), (CHUNK, CHUNK - 1), (CHUNK + 1, CHUNK), (7, CHUNK + 1), (CAP * CHUNK + 1, 3))


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def read(guard):
    """The record on the host: dict of numpy scalars + the raw bytes."""
    raw = guard.record.cpu().numpy().view(np.uint8)
    f = lambda off, dt: raw[off:off + np.dtype(dt).itemsize].view(dt)[0]      # noqa: E731
    return dict(S=f(gg.R_S, np.float64), norm=f(gg.R_NORM, np.float32), coef=f(gg.R_COEF, np.float32), scale=f(gg.R_SCALE, np.float32),
                ok=int(f(gg.R_OK, np.int32)), skipped=int(f(gg.R_SKIPPED, np.int64)), raw=raw.tobytes())


def check_record(rec, S_ref, N, gscale, max_norm, what):
    assert abs(rec['S'] - S_ref) <= N * 2.0 ** -52 * S_ref, '%s: S %r against %r' % (what, rec['S'], S_ref)
    _, n32, _, c32 = R.record_ref(S_ref, gscale, max_norm)
    un, uc = R.ulps32(rec['norm'], n32), R.ulps32(rec['coef'], c32)
    assert un <= 1.0 and uc <= 1.0, '%s: norm %r (%r, %.2f ulp), coef %r (%r, %.2f ulp)' % (what, rec['norm'], n32, un, rec['coef'], c32, uc)
    assert rec['coef'] <= 1.0
    want = np.float32(gscale) * rec['coef']
    assert np.float32(rec['scale']).tobytes() == np.float32(want).tobytes(), '%s: scale %r is not gscale * coef = %r' % (what, rec['scale'], want)


def segments(n32, n64, seed=0, shift32=0):
    """The two gradient segments inside guard bands (shift32: the fp32 segment starts that many elements later)."""
    b32 = S.GuardedBuffers(n32 + shift32, F32, 1, DEV, seed=seed + 1)
    b64 = S.GuardedBuffers(n64, F64, 1, DEV, seed=seed + 2) if n64 else None
    segs = [b32.views[0][shift32:]] + ([b64.views[0]] if n64 else [])
    return b32, b64, segs


# ------------------------------------------------------------------------------------------------- 1. the guard reduction
@pytest.mark.parametrize('n32,n64', S.PAIR_SIZES + SEAMS)
def test_guard_record(n32, n64):
    b32, b64, segs = segments(n32, n64)
    snaps = [b.snapshot() for b in (b32, b64) if b is not None]
    N = n32 + n64
    S_ref = R.sum_squares([s.cpu().numpy() for s in segs])
    guard = gg.GradGuard(segs)
    for gs in S.GRAD_SCALES:
        norm = float(np.float32(gs)) * np.sqrt(S_ref)
        for max_norm in (0.37 * norm, 2.5 * norm, norm, None):
            guard.run(gs, max_norm)
            rec = read(guard)
            check_record(rec, S_ref, N, gs, max_norm, 'n = (%d, %d) gscale %g max_norm %r' % (n32, n64, gs, max_norm))
            assert rec['ok'] == 1 and rec['skipped'] == 0
            if max_norm is None or max_norm > norm:
                assert rec['coef'] == 1.0
            elif max_norm < norm:
                assert rec['coef'] < 1.0
    # the same input again: the same bits, whatever the workspace held before
    guard.run(S.GRAD_SCALES[3], 0.37 * norm)
    first = read(guard)['raw']
    guard.ws.fill_(float('nan'))
    guard.run(S.GRAD_SCALES[3], 0.37 * norm)
    assert read(guard)['raw'] == first
    for b, snap in zip([b for b in (b32, b64) if b is not None], snaps):
        assert b.guards_unchanged(snap) and torch.equal(b.whole.view(b.bits), snap.view(b.bits))


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, CHUNK + 2])
def test_guard_segment_off_the_16_byte_boundary(n):
    """An fp32 segment that starts 4 bytes past a 16-byte boundary (and a lone fp64 element 8 bytes past one)."""
    b32, b64, _ = segments(n, 2, seed=7, shift32=1)
    seg32, seg64 = b32.views[0][1:], b64.views[0][1:]
    assert seg32.data_ptr() % 16 == 4 and seg64.data_ptr() % 16 == 8 and seg32.numel() == n
    S_ref = R.sum_squares([seg32.cpu().numpy(), seg64.cpu().numpy()])
    guard = gg.GradGuard([seg32, seg64])
    guard.run(1.0, 0.5 * np.sqrt(S_ref))
    check_record(read(guard), S_ref, n + 1, 1.0, 0.5 * np.sqrt(S_ref), 'n = %d' % n)
    # the scale launch on the same ragged segments: g * coef in the element's type, the neighbours untouched
    snap32, snap64 = b32.snapshot(), b64.snapshot()
    coef = torch.tensor(read(guard)['coef'])
    want32, want64 = seg32.cpu() * coef, seg64.cpu() * coef
    guard.scale()
    assert S.same_bits(seg32.cpu(), want32) and S.same_bits(seg64.cpu(), want64)
    assert b32.guards_unchanged(snap32) and b64.guards_unchanged(snap64)
    assert S.same_bits(b32.views[0][:1].cpu(), snap32[S.GUARD:S.GUARD + 1].cpu())


def test_guard_extremes():
    """fp32 gradients of 1e-25 and +-3e38 next to ordinary ones are finite in fp64: ok, the norm to the same bound.  A planted NaN, a
    planted +inf, an fp64 gradient of 1e200 (S overflows) and a NaN in a checked tail scalar: not ok."""
    n32, n64 = CHUNK + 5, 33
    b32, b64, segs = segments(n32, n64, seed=11)
    g32, g64 = segs
    g32[3], g32[CHUNK + 1], g32[CHUNK - 1], g32[17] = 1e-25, 3e38, -3e38, 1e-25
    clean32, clean64 = g32.clone(), g64.clone()
    tail = torch.tensor([1234.5, 0.25], device=DEV)
    guard = gg.GradGuard(segs)
    S_ref = R.sum_squares([g32.cpu().numpy(), g64.cpu().numpy()])
    assert np.isfinite(S_ref) and S_ref > 1e76
    guard.run(0.5, 1e30, check=tail)                           # (a coefficient that is a normal fp32 number)
    rec = read(guard)
    assert rec['ok'] == 1
    check_record(rec, S_ref, n32 + n64, 0.5, 1e30, 'extremes')

    def verdict(force=False):
        guard.run(0.5, 1.0, check=tail, force_ok=force)       # (gscale 0.5: sqrt(S) = 4.2e38 is past fp32, half of it is not)
        return read(guard)

    g32[CHUNK + 2] = float('nan')
    rec = verdict()
    assert rec['ok'] == 0 and np.isnan(rec['S']) and np.isnan(rec['norm']) and np.isnan(rec['coef']) and np.isnan(rec['scale'])
    assert verdict(force=True)['ok'] == 1                      # max_grad_norm without skip_nonfinite: never skips
    g32.copy_(clean32)
    g32[0] = float('inf')
    rec = verdict()
    assert rec['ok'] == 0 and np.isinf(rec['S']) and rec['coef'] == 0.0
    g32.copy_(clean32)
    g64[32] = 1e200
    rec = verdict()
    assert rec['ok'] == 0 and np.isinf(rec['S'])
    g64.copy_(clean64)
    assert verdict()['ok'] == 1
    for k in (0, 1):
        tail[k] = float('nan') if k == 0 else float('-inf')
        rec = verdict()
        assert rec['ok'] == 0 and np.isfinite(rec['S']) and np.isfinite(rec['norm'])
        tail[k] = 1.0
    assert verdict()['ok'] == 1 and read(guard)['skipped'] == 0


def test_guard_refuses_before_any_launch():
    b32, _, segs = segments(100, 0, seed=13)
    guard = gg.GradGuard(segs)
    guard.run(1.0, None)
    before = read(guard)['raw']
    table = guard.table.copy()

    def call(tab=table, table_dev=guard.table_dev, record=guard.record, ws=guard.ws, ws_bytes=guard.ws_bytes):
        _lib.call('gx_grad_guard', ctypes.c_void_p(tab.ctypes.data), P(table_dev), tab.size, tab.shape[0], None, 0, 2.0, 1e-3, 0,
                  P(record), P(ws), ws_bytes, stream())

    def row(**over):
        t = table.copy()
        for k, v in over.items():
            t[0, getattr(gg, 'D_' + k)] = v
        return t

    for kwargs, message in ((dict(record=None), 'null record'), (dict(ws=None), 'null record or workspace'),
                            (dict(table_dev=None), 'null descriptor table'), (dict(tab=row(SRC=0)), 'null source'),
                            (dict(tab=row(SRC=int(table[0, 0]) + 2)), 'not aligned to its 4-byte elements'),
                            (dict(tab=row(N=0)), 'N = 0 outside'), (dict(tab=row(DTYPE=5)), 'unknown dtype 5'),
                            (dict(ws_bytes=4), 'workspace of 4 bytes, 8 needed')):
        with pytest.raises(GenesisHipError, match=message):
            call(**kwargs)
    assert read(guard)['raw'] == before                        # (gscale 2, max_norm 1e-3 would have changed it)


# ------------------------------------------------------------------------------------------------- 2. the guarded tail
def make_groups(n32, n64, k, seed):
    b32 = S.GuardedBuffers(n32, F32, k, DEV, seed=seed)
    b64 = S.GuardedBuffers(n64, F64, k, DEV, seed=seed + 1)
    for b in (b32, b64):
        for i in range(2, k):
            b.views[i].abs_()                                  # (moments / square averages: non-negative)
    return b32, b64


def call_tail(opt, b32, b64, n32, n64, step, scale_or_record, zero, guarded):
    """One optimiser launch on (p, g, m[, v]) = views 0..3; scale_or_record: the host float, or the record tensor."""
    v32, v64 = b32.views, (b64.views if n64 else [None] * 4)
    arg = P(scale_or_record) if guarded else scale_or_record
    sfx = '_guarded' if guarded else ''
    if opt == 'adam':
        _lib.call('gx_adam_step_pair' + sfx, P(v32[0]), P(v32[1]), P(v32[2]), P(v32[3]), n32, P(v64[0]), P(v64[1]), P(v64[2]),
                  P(v64[3]), n64, P(step), S.LR, S.BETA1, S.BETA2, S.ADAM_EPS, arg, zero, stream())
    else:
        kind, hp, eps = (1, S.RMS_ALPHA, S.RMS_EPS) if opt == 'rmsprop' else (2, S.SGD_MOMENTUM, 0.0)
        _lib.call('gx_optimiser_step_pair' + sfx, kind, P(v32[0]), P(v32[1]), P(v32[2]), n32, P(v64[0]), P(v64[1]), P(v64[2]), n64,
                  P(step), S.LR, hp, eps, arg, zero, stream())


@pytest.mark.parametrize('opt', ['adam', 'rmsprop', 'sgd'])
@pytest.mark.parametrize('zero', [0, 1])
@pytest.mark.parametrize('n32,n64', S.PAIR_SIZES)
def test_guarded_tail_ok_matches_the_unguarded_entry_points(n32, n64, zero, opt):
    """Steps 1..3: the guard over the gradients with a binding clip, then the guarded launch on one set of buffers and the unguarded
    one, given the record's `scale` as its host grad_scale, on a twin: the same bits in p, m, v and g, the same step counter."""
    p32, p64, grads = S.optimiser_inputs(n32, n64, 3)
    A, B = make_groups(n32, n64, 4, 21), make_groups(n32, n64, 4, 21)
    for (a32, a64) in (A, B):
        a32.views[0].copy_(p32); a64.views[0].copy_(p64)
    guard = gg.GradGuard([A[0].views[1]] + ([A[1].views[1]] if n64 else []))
    step_a = torch.zeros((), dtype=torch.int64, device=DEV)
    step_b = torch.zeros((), dtype=torch.int64, device=DEV)
    for it, (g32, g64) in enumerate(grads):
        for (a32, a64) in (A, B):
            a32.views[1].copy_(g32); a64.views[1].copy_(g64)
        snaps = [b.snapshot() for b in A + B]
        gs = S.GRAD_SCALES[it + 1]
        norm = gs * np.sqrt(R.sum_squares([g32.numpy(), g64.numpy()]))
        guard.run(gs, 0.5 * norm)
        rec = read(guard)
        assert rec['ok'] == 1 and 0.49 < rec['coef'] < 0.51
        _lib.call('gx_step_increment_guarded', P(step_a), P(guard.record), stream())
        _lib.call('gx_step_increment', P(step_b), stream())
        call_tail(opt, A[0], A[1], n32, n64, step_a, guard.record, zero, True)
        call_tail(opt, B[0], B[1], n32, n64, step_b, float(rec['scale']), zero, False)
        assert int(step_a) == int(step_b) == it + 1 and read(guard)['skipped'] == 0
        for a, b, name in ((A[0], B[0], 'fp32'), (A[1], B[1], 'fp64')):
            assert torch.equal(a.whole.view(a.bits), b.whole.view(b.bits)), 'step %d: the %s buffers differ' % (it + 1, name)
        for b, snap in zip(A + B, snaps):
            assert b.guards_unchanged(snap)
        if zero:
            assert S.same_bits(A[0].views[1], torch.zeros_like(A[0].views[1]))
        else:
            assert S.same_bits(A[0].views[1].cpu(), g32)


@pytest.mark.parametrize('opt', ['adam', 'rmsprop', 'sgd'])
@pytest.mark.parametrize('zero', [0, 1])
@pytest.mark.parametrize('t0', [0, 2 ** 31 + 7])
def test_guarded_tail_not_ok_changes_nothing_but_the_gradients(t0, zero, opt):
    """A NaN among the gradients: p, m, v, the step counter and the GECO state keep their bits over three steps, g is all +0 with
    the zeroing flag and bit-unchanged without it, `skipped` grows by one per step, the guard bands stay."""
    n32, n64 = 2048 * 1024 + 1027, 256 * 1024 + 5              # one past both grid caps of the optimiser launch
    b32, b64 = make_groups(n32, n64, 4, 31)
    b32.views[1][n32 - 2] = float('nan')
    geco = S.GuardedBuffers(3, F32, 1, DEV, seed=33)
    err = torch.tensor([3.5], device=DEV)
    step = torch.full((), t0, dtype=torch.int64, device=DEV)
    guard = gg.GradGuard([b32.views[1], b64.views[1]])
    for it in range(3):
        before = [b.snapshot() for b in (b32, b64, geco)]
        guard.run(0.5, 1.0, check=err)
        assert read(guard)['ok'] == 0
        if it % 2 == 0:
            _lib.call('gx_geco_update_step_guarded', P(geco.views[0]), P(err), 10.0, 1e-2, 0.99, 10.0, 1, 1e-10, 1e10, P(step),
                      P(guard.record), stream())
        else:
            _lib.call('gx_step_increment_guarded', P(step), P(guard.record), stream())
        call_tail(opt, b32, b64, n32, n64, step, guard.record, zero, True)
        assert int(step) == t0 and read(guard)['skipped'] == it + 1
        assert torch.equal(geco.whole.view(geco.bits), before[2].view(geco.bits))
        for b, snap in ((b32, before[0]), (b64, before[1])):
            assert b.guards_unchanged(snap)
            stride = b.n + 2 * S.GUARD
            for i in range(4):
                got, was = b.views[i], snap[i * stride + S.GUARD:i * stride + S.GUARD + b.n]
                if i == 1 and zero:
                    assert S.same_bits(got, torch.zeros_like(got)), 'gradients not all +0'
                else:
                    assert S.same_bits(got, was), 'buffer %d changed in a skipped step' % i
        if zero:                                               # the next step's gradients: not finite again
            b32.views[1][5] = float('inf')


@pytest.mark.parametrize('speedup', [None, 10.0])
def test_guarded_geco_matches_gx_geco_update_step(speedup):
    """ok: the same bits as gx_geco_update_step over a short series (first call included), the counter advanced."""
    errs = torch.tensor([3.0, 9.5, 12.0, 7.0, 10.0], device=DEV)
    a, b = (torch.tensor([1.0, 0.0, 0.0], device=DEV) for _ in range(2))
    sa, sb = (torch.full((), 41, dtype=torch.int64, device=DEV) for _ in range(2))
    g = torch.ones(64, device=DEV)
    guard = gg.GradGuard([g])
    guard.run(1.0, None)
    args = (10.0, 1e-2, 0.99, float(speedup or 0.0), int(speedup is not None), 1e-10, 1e10)
    for i in range(errs.numel()):
        _lib.call('gx_geco_update_step_guarded', P(a), P(errs[i:i + 1]), *args, P(sa), P(guard.record), stream())
        _lib.call('gx_geco_update_step', P(b), P(errs[i:i + 1]), *args, P(sb), stream())
        assert S.same_bits(a, b) and int(sa) == int(sb) == 42 + i
    assert float(a[0]) != 1.0 and read(guard)['skipped'] == 0


# ------------------------------------------------------------------------------------------------- 3. TrainStep on the tiny model
def _seed(s=5):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _trajectory(ts, xd, steps=6):
    _seed()
    vals = [ts.step(xd).clone() for _ in range(steps)]
    torch.cuda.synchronize()
    return torch.stack(vals).cpu(), ts.flat_p.clone().cpu()


@pytest.fixture(scope='module')
def tiny():
    """The tiny model's input, the six-step trajectory of an unguarded eager TrainStep (computed once, read only) and the first
    step's measured gradient norm."""
    from genesis_amd.trainer import TrainStep
    gold = Golden('tiny')
    x, _, _ = gold.inputs()
    xd = x.to(DEV)
    plain = TrainStep(build(gold), gold.S, graph=False)
    ref = _trajectory(plain, xd)
    plain.close()                                              # (a library context each: released as the tests go)
    ts = TrainStep(build(gold), gold.S, graph=False, skip_nonfinite=True)
    _seed()
    ts.step(xd)
    norm = float(ts.grad_norm)
    assert np.isfinite(norm) and norm > 0 and float(ts.clip_coef) == 1.0
    ts.close()
    return dict(gold=gold, xd=xd, ref=ref, norm=norm)


@pytest.mark.parametrize('graph', [False, True])
def test_trainstep_with_a_clip_that_never_binds_keeps_the_trajectory(tiny, graph):
    from genesis_amd.trainer import TrainStep
    ts = TrainStep(build(tiny['gold']), tiny['gold'].S, graph=graph, max_grad_norm=1e6 * tiny['norm'], skip_nonfinite=True)
    out, p = _trajectory(ts, tiny['xd'])
    assert torch.equal(out, tiny['ref'][0]) and S.same_bits(p, tiny['ref'][1])
    assert int(ts.skipped_steps) == 0 and int(ts.step_t) == 6
    n = float(ts.grad_norm)
    assert np.isfinite(n) and n > 0 and float(ts.clip_coef) == 1.0
    assert ts.grad_norm.dtype == F32 and ts.clip_coef.dtype == F32 and ts.skipped_steps.dtype == torch.int64
    assert ts.grad_norm.is_cuda and ts.grad_norm.dim() == 0
    off = TrainStep(build(tiny['gold']), tiny['gold'].S)
    assert off.grad_norm is None and off.clip_coef is None and off.skipped_steps is None and off._guard is None
    ts.close(); off.close()


def _spy_update(ts, saved):
    """Clones the step's buffers between the backward half and _update (an instance attribute: trainer.py is not edited)."""
    orig = ts._update

    def spy(st, gscale):
        saved.update(p=ts.flat_p.clone(), g=ts.flat_g[:ts.n32].clone(), m=ts.m32.clone(), v=ts.v32.clone(), p64=ts.flat_p64.clone(),
                     g64=ts.flat_g64.clone(), m64=ts.m64.clone(), v64=ts.v64.clone(), step=ts.step_t.clone(), gscale=gscale)
        return orig(st, gscale)
    ts._update = spy


@pytest.mark.parametrize('opt', ['adam', 'rmsprop', 'sgd'])
def test_trainstep_clipped_step_is_the_unguarded_launch_with_the_record_scale(tiny, opt):
    from genesis_amd.trainer import TrainStep
    half = 0.5 * tiny['norm']
    ts = TrainStep(build(tiny['gold']), tiny['gold'].S, graph=False, optimiser=opt, max_grad_norm=half)
    saved = {}
    _spy_update(ts, saved)
    _seed()
    ts.step(tiny['xd'])
    rec = read(ts._guard)
    assert saved['gscale'] == 1.0 and rec['ok'] == 1 and int(ts.skipped_steps) == 0
    # (the first step's gradient does not depend on the optimiser: the measured norm holds for all three)
    assert abs(float(ts.grad_norm) - tiny['norm']) <= 1e-5 * tiny['norm']
    want = np.float32(half / (np.sqrt(rec['S']) + 1e-6))
    assert R.ulps32(float(ts.clip_coef), want) <= 1.0 and 0.49 < float(ts.clip_coef) < 0.51
    assert np.float32(rec['scale']).tobytes() == np.float32(rec['coef']).tobytes()      # gscale 1
    step = saved['step'] + 1
    n32, n64 = ts.n32, ts.n64
    if opt == 'adam':
        _lib.call('gx_adam_step_pair', P(saved['p']), P(saved['g']), P(saved['m']), P(saved['v']), n32, P(saved['p64']), P(saved['g64']),
                  P(saved['m64']), P(saved['v64']), n64, P(step), ts.lr, ts.betas[0], ts.betas[1], ts.eps, float(rec['scale']), 1, stream())
    else:
        kind, hp, eps = (1, 0.99, 1e-8) if opt == 'rmsprop' else (2, 0.9, 0.0)
        _lib.call('gx_optimiser_step_pair', kind, P(saved['p']), P(saved['g']), P(saved['m']), n32, P(saved['p64']), P(saved['g64']),
                  P(saved['m64']), n64, P(step), ts.lr, hp, eps, float(rec['scale']), 1, stream())
    assert n64 > 0 and int(ts.step_t) == int(step) == 1
    for name, got in (('p', ts.flat_p), ('m', ts.m32), ('v', ts.v32), ('p64', ts.flat_p64), ('m64', ts.m64), ('v64', ts.v64)):
        assert S.same_bits(got, saved[name]), name
    assert S.same_bits(ts.flat_g[:n32], torch.zeros_like(ts.flat_g[:n32])) and S.same_bits(ts.flat_g64, torch.zeros_like(ts.flat_g64))
    ts.close()


def test_trainstep_clipped_graph_replay_equals_eager(tiny):
    from genesis_amd.trainer import TrainStep
    runs = []
    for graph in (False, True):
        ts = TrainStep(build(tiny['gold']), tiny['gold'].S, graph=graph, max_grad_norm=0.5 * tiny['norm'])
        runs.append(_trajectory(ts, tiny['xd']) + (float(ts.clip_coef), float(ts.grad_norm)))
        ts.close()
    (a, pa, ca, na), (b, pb, cb, nb) = runs
    assert torch.equal(a, b) and S.same_bits(pa, pb) and ca == cb and na == nb and ca < 1.0
    assert not S.same_bits(pa, tiny['ref'][1])


@pytest.mark.parametrize('graph', [False, True])
def test_trainstep_skips_a_non_finite_batch(tiny, graph):
    """A batch whose first pixel is NaN: the step returns, is counted, leaves parameters, moments, step counter and GECO state alone
    and the gradients zeroed (the bucket's tail scalars, err and kl, are rewritten by every step and hold this step's NaN); the next
    clean batch then gives the step of a twin that never saw the bad one."""
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    ts = TrainStep(build(gold), gold.S, graph=graph, skip_nonfinite=True)
    twin = TrainStep(build(gold), gold.S, graph=graph, skip_nonfinite=True)
    _seed()
    ts.step(xd)
    twin.step(xd)
    state = lambda t: [t.flat_p, t.flat_p64, t.m32, t.v32, t.m64, t.v64, t.geco.state]      # noqa: E731
    before = [s.clone() for s in state(ts)]
    bad = xd.clone()
    bad[0, 0, 0, 0] = float('nan')
    out = ts.step(bad)
    assert out.shape == (4,) and int(ts.skipped_steps) == 1 and int(ts.step_t) == 1
    assert not bool(torch.isfinite(ts.grad_norm))
    for was, now in zip(before, state(ts)):
        assert S.same_bits(was, now)
    assert S.same_bits(ts.flat_g[:ts.n32], torch.zeros_like(ts.flat_g[:ts.n32]))
    assert S.same_bits(ts.flat_g64, torch.zeros_like(ts.flat_g64))
    x2 = xd.flip(0).contiguous()
    a, b = ts.step(x2).clone(), twin.step(x2).clone()
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    for u, v in zip(state(ts), state(twin)):
        assert S.same_bits(u, v)
    assert int(ts.skipped_steps) == 1 and int(twin.skipped_steps) == 0 and int(ts.step_t) == int(twin.step_t) == 2
    ts.close(); twin.close()
    if graph:
        # the bad batch as the very FIRST one: the capture's warm-up iterations see it too, and must not stay counted
        fresh = TrainStep(build(gold), gold.S, graph=True, skip_nonfinite=True)
        p0 = fresh.flat_p.clone()
        fresh.step(bad)
        assert int(fresh.skipped_steps) == 1 and int(fresh.step_t) == 0 and S.same_bits(fresh.flat_p, p0)
        fresh.close()


def test_trainstep_guard_under_a_forced_collective(tiny, monkeypatch):
    """World size 1 with the collective forced into the step (as test_rccl_allreduce_in_the_step_matches_single_graph sets it up):
    with a clip that never binds the guarded step reproduces the single-graph trajectory bit for bit."""
    import torch.distributed as dist
    from genesis_amd.trainer import TrainStep
    gold, xd = tiny['gold'], tiny['xd']
    monkeypatch.setenv('GENESIS_FORCE_ALLREDUCE', '1')
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:29547', rank=0, world_size=1)
    try:
        ts = TrainStep(build(gold), gold.S, graph=True, max_grad_norm=1e6 * tiny['norm'], skip_nonfinite=True)
        got = _trajectory(ts, xd)
        assert ts.collective_in_graph or (ts._split and ts.graph2 is not None)
        skipped, coef = int(ts.skipped_steps), float(ts.clip_coef)
        ts.close()
    finally:
        dist.destroy_process_group()
    assert torch.equal(got[0], tiny['ref'][0]) and S.same_bits(got[1], tiny['ref'][1])
    assert skipped == 0 and coef == 1.0


@pytest.mark.parametrize('bad', [0.0, -3.0, float('inf'), float('nan'), '1'])
def test_trainstep_bad_max_grad_norm(tiny, bad):
    from genesis_amd.trainer import TrainStep
    with pytest.raises(ValueError, match='max_grad_norm'):
        TrainStep(build(tiny['gold']), tiny['gold'].S, max_grad_norm=bad)


# ------------------------------------------------------------------------------------------------- 4. the drop-in
def _yardstick(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on the CPU in fp64 -> its norm."""
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=F64)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.detach().cpu().to(F64).clone()             # (its own copy: torch clips in place)
    return float(torch.nn.utils.clip_grad_norm_(ps, max_norm))


def _mixed_parameters(flat):
    """fp32 and fp64 gradients, as views of ONE flat buffer per dtype (gaps between them hold other numbers) or separately
    allocated; one is a 1-element tensor at an odd 4-byte offset."""
    gen = torch.Generator().manual_seed(17)
    shapes = [((3, 5), F32), ((1,), F32), ((CHUNK + 3,), F32), ((2, 2), F64), ((7,), F64), ((4, 3, 3, 3), F32)]
    ps = [torch.nn.Parameter(torch.zeros(s, dtype=dt, device=DEV)) for s, dt in shapes]
    ps.insert(3, torch.nn.Parameter(torch.zeros(5, device=DEV)))                 # no gradient: skipped
    bufs = {F32: torch.randn(3 * CHUNK, generator=gen).to(DEV), F64: torch.randn(64, generator=gen, dtype=F64).to(DEV)}
    offs = {F32: 0, F64: 0}
    for p, (s, dt) in zip([p for i, p in enumerate(ps) if i != 3], shapes):
        n = int(np.prod(s))
        if flat:
            o = offs[dt]
            if s == (1,):
                o += (1 - o) % 4                               # 4 bytes past a 16-byte boundary
            p.grad = bufs[dt][o:o + n].view(s)
            offs[dt] = o + n + 2
        else:
            p.grad = (torch.randn(n + 1, generator=gen, dtype=dt).to(DEV))[1:].view(s) if s == (1,) else \
                torch.randn(s, generator=gen, dtype=dt).to(DEV)
    one = ps[1].grad
    assert one.numel() == 1 and one.data_ptr() % 16 == 4
    return ps, bufs


@pytest.mark.parametrize('flat', [True, False])
@pytest.mark.parametrize('clip', ['binds', 'equal', 'loose'])
def test_drop_in_against_torch_on_the_cpu(flat, clip):
    import genesis_amd
    ps, bufs = _mixed_parameters(flat)
    grads = [p.grad for p in ps if p.grad is not None]
    before = [g.detach().cpu().clone() for g in grads]
    whole = {dt: b.clone() for dt, b in bufs.items()}
    norm64 = np.sqrt(R.sum_squares([g.numpy() for g in before]))
    max_norm = {'binds': 0.3 * norm64, 'equal': norm64, 'loose': 4.0 * norm64}[clip]
    want_norm = _yardstick(before, max_norm)
    got = genesis_amd.clip_grad_norm_(ps, max_norm)
    assert got.is_cuda and got.dtype == F32 and got.dim() == 0
    assert R.ulps32(float(got), np.float32(want_norm)) <= 1.0
    guard = next(reversed(gg._CACHE.values()))
    assert guard.table.shape[0] == len(grads)                  # not the unchanged loop's flat buffers: one segment per gradient
    rec = read(guard)
    assert R.ulps32(rec['coef'], np.float32(R.coef64(want_norm, max_norm))) <= 1.0
    coef = torch.tensor(rec['coef'])
    assert ps[3].grad is None
    if clip == 'loose':
        assert rec['coef'] == 1.0
    for g, b in zip(grads, before):
        want = b if clip == 'loose' else b * coef              # coef == 1: bit-unchanged
        assert want.dtype == b.dtype and S.same_bits(g.cpu(), want)
    if clip == 'binds':
        assert rec['coef'] < 0.31
    if flat:                                                   # what lies between the views is not the call's to touch
        for dt, b in bufs.items():
            mask = torch.ones(b.numel(), dtype=torch.bool, device=DEV)
            for g in grads:
                if g.dtype == dt:
                    o = (g.data_ptr() - b.data_ptr()) // b.element_size()
                    mask[o:o + g.numel()] = False
            bits = torch.int32 if dt == F32 else torch.int64
            assert torch.equal(b.view(bits)[mask], whole[dt].view(bits)[mask])
    # the table is cached while the addresses stay the same; the returned norm is the caller's own tensor
    again = genesis_amd.clip_grad_norm_(ps, max_norm)
    assert next(reversed(gg._CACHE.values())) is guard and again.data_ptr() != got.data_ptr()


def test_drop_in_non_finite_norm_is_torchs():
    import genesis_amd
    ps, _ = _mixed_parameters(False)
    ps[0].grad[1, 2] = float('nan')
    got = genesis_amd.clip_grad_norm_(ps, 1.0)
    assert bool(torch.isnan(got))
    assert all(bool(torch.isnan(p.grad).all()) for p in ps if p.grad is not None)      # torch: every gradient times NaN
    ps, _ = _mixed_parameters(False)
    ps[4].grad[0, 1] = float('inf')
    before = [p.grad.cpu().clone() for p in ps if p.grad is not None]
    got = genesis_amd.clip_grad_norm_(ps, 1.0)
    assert bool(torch.isinf(got))
    for p, b in zip([p for p in ps if p.grad is not None], before):
        assert S.same_bits(p.grad.cpu(), b * torch.tensor(0.0))                        # coef 0: zeros, inf * 0 = NaN


def test_drop_in_refusals_on_the_device():
    import genesis_amd
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    p.grad = torch.ones(6, 4, device=DEV).t()
    with pytest.raises(GenesisHipError, match='parameters: gradient 0 .* is not contiguous'):
        genesis_amd.clip_grad_norm_([p], 1.0)
    p.grad = None
    q = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    q.grad = torch.ones(4, device=DEV, dtype=torch.float16)
    with pytest.raises(GenesisHipError, match='parameters: gradient 0 is torch.float16'):
        genesis_amd.clip_grad_norm_([p, q], 1.0)
    r = torch.nn.Parameter(torch.zeros(4))
    r.grad = torch.ones(4)
    with pytest.raises(GenesisHipError, match='parameters: gradient 0 is on cpu'):
        genesis_amd.clip_grad_norm_([r], 1.0)
    with pytest.raises(GenesisHipError, match='norm_type'):
        genesis_amd.clip_grad_norm_([p], 1.0, norm_type=3)
    with pytest.raises(GenesisHipError, match='error_if_nonfinite'):
        genesis_amd.clip_grad_norm_([p], 1.0, error_if_nonfinite=True)


def test_drop_in_in_the_unchanged_loop():
    """One iteration of the unchanged loop on the tiny model with the drop-in where torch's function stood: the parameters after
    optimiser.step() within test_adam_kernel_matches_torch's tolerance, the norms within 1e-6 relative (torch sums per-tensor fp32
    norms), and -- every .grad a view of the loop's flat buffers -- one segment per flat buffer."""
    import genesis_amd
    gold = Golden('tiny')
    x, _, _ = gold.inputs()
    rp, eps = gold.noise(1)

    def iteration(clip):
        model = build(gold)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        opt.zero_grad()
        recon, losses, stats, att, comp = model(x.to(DEV), rp.to(DEV), torch.stack(eps).to(DEV))
        err = losses.err.mean(0)
        kl = torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()
        (err + kl).backward()
        norm = clip(list(model.parameters()))
        opt.step()
        return float(norm), {n: p.detach().cpu().clone() for n, p in model.named_parameters()}

    n0, _ = iteration(lambda ps: torch.nn.utils.clip_grad_norm_(ps, 1e30))
    max_norm = 0.5 * n0
    nt, pt = iteration(lambda ps: torch.nn.utils.clip_grad_norm_(ps, max_norm))
    ng, pg = iteration(lambda ps: genesis_amd.clip_grad_norm_(ps, max_norm))
    guard = next(reversed(gg._CACHE.values()))
    assert guard.table.shape[0] == 2 and {int(d) for d in guard.table[:, gg.D_DTYPE]} == {gg.FP32, gg.FP64}
    assert abs(ng - nt) <= 1e-6 * nt and abs(nt - n0) <= 1e-6 * n0
    for n in pt:
        np.testing.assert_allclose(pg[n].numpy(), pt[n].numpy(), rtol=2e-6, atol=1e-7, err_msg=n)
