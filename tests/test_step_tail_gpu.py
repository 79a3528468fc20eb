"""The tail of a training step and cross-replica BatchNorm, one kernel at a time: what TrainStep._forward_backward and
TrainStep._update launch after the backward pass (gx_elbo_fwd_grads, gx_mse_rmse, gx_beta_warmup, gx_geco_update[_step],
gx_adam_step_pair) and the four entry points behind hip_ops.gated_bn_sync_fwd / _bwd, each against a float64 restatement
(tests/step_tail_restatement.py; tests/test_step_tail_cpu.py pins those to torch.optim and to the reference's GECO class and
measures the float32 bounds used here), with guard bands around every destination.

What each test would catch (one-line mistakes):

  adam_pair_kernel without `- nb32`           test_adam_pair (every size with an fp64 group): the fp64 blocks start nb32 blocks in
  adam_body without `if (ZERO_G)`             test_adam_pair[... zero_grads = 0]: the gradients are no longer bit-unchanged
  geco_update_kernel ignoring use_speedup     test_geco_series_takes_both_branches (speedup = None: the factor becomes exp(0))
                                              (`constraint >= 0.f` for `> 0.f` is no mistake: at 0 both branches give exp(0) = 1)
  d_kl = beta / (B R)                         test_elbo_fwd_grads at every R > 1
  gx_gated_bn_bwd_apply given N H W for m     test_sync_batchnorm_shards at world 2 and 3 (dy), test_sync_batchnorm_hard_operands
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_tail_restatement as S
from tests.test_kernel_edges_gpu import Arena, close, finite, gated_operands, gated_ref, leaf, to

pytestmark = pytest.mark.gpu

hip = pytest.importorskip('genesis_amd.hip_ops')
from genesis_amd import _lib  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

DEV = 'cuda'
F32, F64 = torch.float32, torch.float64


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------- 1. Adam on the flat buffers
def call_adam_pair(b32, b64, n32, n64, step, gs, zero):
    v32, v64 = b32.views, (b64.views if n64 else [None] * 4)
    _lib.call('gx_adam_step_pair', P(v32[0]), P(v32[1]), P(v32[2]), P(v32[3]), n32, P(v64[0]), P(v64[1]), P(v64[2]), P(v64[3]),
              n64, P(step), S.LR, S.BETA1, S.BETA2, S.ADAM_EPS, gs, zero, stream())


def adam_alone(before, is_f64, step, gs):
    """gx_adam_step on copies of (p, g, m, v) -> (p, m, v)."""
    p, g, m, v = (t.clone() for t in before)
    _lib.call('gx_adam_step', P(p), P(g), P(m), P(v), p.numel(), is_f64, P(step), S.LR, S.BETA1, S.BETA2, S.ADAM_EPS, gs, stream())
    return p, m, v


def check_f32(got, ref, scales, what):
    r = S.adam_f32_ratios(got, ref, scales)
    print('%s: p %.3e m %.3e v %.3e (allowed %g x %s)' % (what, r['p'], r['m'], r['v'], S.ADAM_GPU_MARGIN, S.ADAM_F32_ERR))
    for k in r:
        assert r[k] <= S.ADAM_GPU_MARGIN * S.ADAM_F32_ERR[k], '%s: %s is %.3e of its scale' % (what, k, r[k])


def check_f64(got, ref, what):
    for a, b, name in zip(got, ref, 'pmv'):
        np.testing.assert_allclose(a.cpu().numpy(), b.numpy(), rtol=1e-12, atol=1e-14, err_msg='%s: %s' % (what, name))


def run_adam_pair(n32, n64, zero, gs, t0, grads, p32, p64):
    """One gx_adam_step_pair launch per entry of `grads` from step counter t0 and zero moments; after every launch: p, m, v of
    both groups against adam_ref on the values the launch started from (fp32: every element against its own scale), the same
    bits as gx_adam_step on each group alone, the gradients zeroed / bit-unchanged, every guard band bit-unchanged."""
    b32 = S.GuardedBuffers(n32, F32, 4, DEV, seed=1)
    b64 = S.GuardedBuffers(n64, F64, 4, DEV, seed=2)
    for b, p in ((b32, p32), (b64, p64)):
        b.views[0].copy_(p)
        b.views[2].zero_(); b.views[3].zero_()
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    for it, (g32, g64) in enumerate(grads):
        t = t0 + it + 1
        step.fill_(t)
        b32.views[1].copy_(g32); b64.views[1].copy_(g64)
        before32, before64 = [v.clone() for v in b32.views], [v.clone() for v in b64.views]
        snap32, snap64 = b32.snapshot(), b64.snapshot()
        alone32 = adam_alone(before32, 0, step, gs)
        alone64 = adam_alone(before64, 1, step, gs) if n64 else None
        call_adam_pair(b32, b64, n32, n64, step, gs, zero)
        assert int(step) == t, 'the launch changed the step counter'
        assert b32.guards_unchanged(snap32), 'step %d: a guard band of the fp32 group changed' % t
        assert b64.guards_unchanged(snap64), 'step %d: a guard band of the fp64 group changed' % t
        for b, before, alone, name in ((b32, before32, alone32, 'fp32'), (b64, before64, alone64, 'fp64')):
            if b.n == 0:
                continue
            if zero:
                assert S.same_bits(b.views[1], torch.zeros_like(b.views[1])), 'step %d: %s gradients not all +0' % (t, name)
            else:
                assert S.same_bits(b.views[1], before[1]), 'step %d: %s gradients changed' % (t, name)
            for a, c, nm in zip((b.views[0], b.views[2], b.views[3]), alone, 'pmv'):
                assert S.same_bits(a, c), 'step %d: %s %s differs from gx_adam_step on the group alone' % (t, name, nm)
        cpu32 = [v.cpu() for v in before32]
        ref32 = S.adam_ref(*cpu32, t, gs)
        got32 = [b32.views[i].cpu() for i in (0, 2, 3)]
        check_f32(got32, ref32, S.adam_scales(*cpu32, t, gs), 'step %d fp32' % t)
        if n64:
            check_f64([b64.views[i] for i in (0, 2, 3)], S.adam_ref(*[v.cpu() for v in before64], t, gs), 'step %d fp64' % t)
    return b32, b64


@pytest.mark.parametrize('gs', S.GRAD_SCALES, ids=lambda g: 'gs%.4g' % g)
@pytest.mark.parametrize('zero', [0, 1])
@pytest.mark.parametrize('n32,n64', S.PAIR_SIZES)
def test_adam_pair(n32, n64, zero, gs):
    """gx_adam_step_pair, steps 1..5 on N(0, (0.1 + it)^2) gradients.  Sizes: see PAIR_SIZES; (2048 * 1024 + 1027,
    256 * 1024 + 5) is one past both grid caps.  grad_scale travels through the ABI as a float: for 1 / 3 the reference uses the
    float32-rounded value 0.3333333432674408, widened to the group's type (fp64 group: g * (double)(float)(1 / 3), as
    adam_body's `(T)gscale` has it).  fp64 group: rtol 1e-12, atol 1e-14; fp32 group: every element within 4 x the measured
    per-element error of torch's own float32 Adam (step_tail_restatement.ADAM_F32_ERR)."""
    p32, p64, grads = S.optimiser_inputs(n32, n64, 5)
    run_adam_pair(n32, n64, zero, gs, 0, grads, p32, p64)


@pytest.mark.parametrize('t0', [99999, 2 ** 31 + 6])
def test_adam_pair_late_counters(t0):
    """Two steps from a preset counter: 100000, where pow(b2, t) has underflowed towards bc2 = 1 (and pow(b1, t) to 0), and
    2^31 + 7: the counter is int64, a 32-bit read would see 7 (bc1 = 0.52, an update twice as large)."""
    n32, n64 = 1025, 33
    p32, p64, grads = S.optimiser_inputs(n32, n64, 2, seed=5)
    run_adam_pair(n32, n64, 1, 1.0, t0, grads, p32, p64)


def test_adam_pair_zero_gradient():
    """An all-zero gradient at step 1: m = v = 0, the update is exactly 0, p keeps its bits."""
    n32, n64 = 1025, 33
    p32, p64, _ = S.optimiser_inputs(n32, n64, 0, seed=6)
    b32, b64 = run_adam_pair(n32, n64, 0, 1.0, 0, [(torch.zeros(n32), torch.zeros(n64, dtype=F64))], p32, p64)
    for b, p in ((b32, p32), (b64, p64)):
        assert S.same_bits(b.views[0].cpu(), p)
        assert S.same_bits(b.views[2], torch.zeros_like(b.views[2])) and S.same_bits(b.views[3], torch.zeros_like(b.views[3]))


@pytest.mark.parametrize('gs', [1.0, S.GRAD_SCALES[3]], ids=['gs1', 'gs0.3333'])
def test_adam_pair_extreme_gradients(gs):
    """Three steps with a block of 1e-25 gradients (g * g = 1e-50 flushes to 0 in float32: v stays 0, the denominator is eps)
    and a block of 1e15 gradients (v = 1e27) next to ordinary ones; the bounds are per element, so each entry is held to its own
    scale."""
    n32, n64 = 1025, 33
    p32, p64, grads = S.optimiser_inputs(n32, n64, 3, seed=7)
    for g32, g64 in grads:
        g32[0:64] = 1e-25; g32[64:128] = 1e15; g32[64:128:2] *= -1
        g64[0:8] = 1e-25; g64[8:16] = 1e15; g64[8:16:2] *= -1
    run_adam_pair(n32, n64, 1, gs, 0, grads, p32, p64)


# ------------------------------------------------------------------------------------------------- 2. GECO
@pytest.fixture(scope='module')
def series():
    import os.path as osp
    return dict(np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'geco_series.npz')))


def make_geco(s, speedup, step_size=None, **kw):
    from genesis_amd.geco import GECO
    return GECO(float(s['goal']), float(s['step_size']) if step_size is None else step_size, float(s['alpha']), speedup=speedup,
                device=DEV, **kw)


def drive(geco, errs):
    """geco.update over a device series -> float64 arrays (beta [T], ema [T]); one host read at the end."""
    e = torch.as_tensor(errs, dtype=F32).to(DEV)
    states = []
    for i in range(e.numel()):
        geco.update(e[i])
        states.append(geco.state.clone())
    st = torch.stack(states).cpu().double().numpy()
    assert (st[:, 2] == 1.0).all()
    return st[:, 0], st[:, 1]


def test_geco_series_takes_both_branches(series):
    """The recorded 300-step series (3 x goal, below the goal near step 100, a shrinking oscillation around it: the moving
    average crosses the goal eleven times) through GECO.update with speedup = 10 and with speedup = None.  Each curve against
    geco_ref on the same series within 4 x the drift of a float32 transcription (GECO_F32_DRIFT, per speedup setting); the two beta curves are the same up to the first crossing and differ at every step after it."""
    s = series
    prm = dict(goal=float(s['goal']), step_size=float(s['step_size']), alpha=float(s['alpha']))
    curves = {}
    for case, speedup in (('main_su10', 10), ('main_none', None)):
        beta, ema = drive(make_geco(s, speedup), s['main_err'])
        rb, re_ = S.geco_ref_series(s['main_err'], speedup=speedup, **prm)
        db, de = S.rel_dist(beta, rb), S.rel_dist(ema, re_)
        print('%s: beta %.3e, moving average %.3e from geco_ref (allowed %g x %s)' % (case, db, de, S.GECO_GPU_MARGIN,
                                                                                     S.GECO_F32_DRIFT[case]))
        assert db <= S.GECO_GPU_MARGIN * S.GECO_F32_DRIFT[case]['beta'], (case, db)
        assert de <= S.GECO_GPU_MARGIN * S.GECO_F32_DRIFT[case]['ema'], (case, de)
        curves[case] = (beta, rb, re_)
    first = int(np.argmax(float(s['goal']) - curves['main_su10'][2] > 0))
    assert first > 0 and np.array_equal(curves['main_su10'][0][:first], curves['main_none'][0][:first])
    assert (curves['main_su10'][0][first:] != curves['main_none'][0][first:]).all()
    assert S.rel_dist(curves['main_su10'][1][first:], curves['main_none'][1][first:]) > 1e-2     # (not a close call)


@pytest.mark.parametrize('speedup', [10, None])
def test_geco_at_the_goal_and_on_the_clamps(series, speedup):
    """err = goal at the first call: constraint exactly 0, factor 1, beta keeps its bits.  Lower clamp: beta_init 1e-9, the error
    1e6 x goal at step size 1, the factor underflows to 0: beta = float32(1e-10) exactly.  Upper clamp (with speedup): error 0
    at step size 1, the factor overflows to inf: beta = float32(1e10) exactly, and again after each of 3 further updates."""
    s = series
    goal = float(s['goal'])
    assert float(np.float32(goal)) == goal
    g = make_geco(s, speedup, beta_init=0.37)
    g.update(torch.tensor(goal, device=DEV))
    assert S.same_bits(g.state.cpu(), torch.tensor([0.37, goal, 1.0])), g.state
    g = make_geco(s, speedup, step_size=1.0, beta_init=1e-9)
    beta, ema = drive(g, s['lo_clamp_err'])
    assert (beta.astype(np.float32) == np.float32(1e-10)).all() and ema[0] == s['lo_clamp_err'][0], beta
    if speedup is not None:
        beta, _ = drive(make_geco(s, speedup, step_size=1.0), s['hi_clamp_err'])
        assert beta.shape == (4,) and np.isfinite(beta).all() and (beta.astype(np.float32) == np.float32(1e10)).all(), beta


@pytest.mark.parametrize('speedup', [10, None])
@pytest.mark.parametrize('ema0,err', [(1700.0, 1600.0), (1800.5, 1900.0)])
def test_geco_resume(series, speedup, ema0, err):
    """beta and err_ema set through the property setters (the checkpoint path), then ONE update against geco_ref continued from
    that state: relative 1e-6 (two float32 roundings and one expf; |step_size * constraint| < 0.02).  The moving average ends
    below the goal in the first case (the speedup branch) and above it in the second.  err_ema reads None before the first
    update and after err_ema = None, and the update after that starts the average afresh."""
    s = series
    prm = dict(goal=float(s['goal']), step_size=float(s['step_size']), alpha=float(s['alpha']), speedup=speedup)
    g = make_geco(s, speedup)
    assert g.err_ema is None
    g.beta = 0.0123
    g.err_ema = ema0
    assert float(g.beta) == S.f32(0.0123) and float(g.err_ema) == ema0
    g.update(torch.tensor(err, device=DEV))
    rb, re_ = S.geco_ref(S.f32(0.0123), ema0, err, **prm)
    assert (prm['goal'] - re_ > 0) == (ema0 < 1750)
    assert abs(float(g.beta) - rb) <= S.GECO_SINGLE_RTOL * rb, (float(g.beta), rb)
    assert abs(float(g.err_ema) - re_) <= S.GECO_SINGLE_RTOL * re_, (float(g.err_ema), re_)
    g.err_ema = None
    assert g.err_ema is None
    before = float(g.beta)
    g.update(torch.tensor(err, device=DEV))
    rb, _ = S.geco_ref(before, None, err, **prm)
    assert float(g.err_ema) == err and abs(float(g.beta) - rb) <= S.GECO_SINGLE_RTOL * rb


@pytest.mark.parametrize('t0', [0, 2 ** 31 + 7])
def test_geco_update_step_counter_and_neighbours(series, t0):
    """gx_geco_update_step adds exactly 1 to the int64 counter per call (from 0 and from 2^31 + 7) and computes what
    gx_geco_update computes; gx_geco_update leaves the counter alone; the 64 floats before and after the 3-float state and the
    64 int64 words around the counter keep their bits."""
    s = series
    goal, step_size, alpha = float(s['goal']), float(s['step_size']), float(s['alpha'])
    errs = torch.as_tensor(s['main_err'][95:101].copy()).to(DEV)          # (around the first crossing)
    fl = S.GuardedBuffers(3, F32, 2, DEV, seed=3)
    words = torch.arange(1, 2 * S.GUARD + 2, dtype=torch.int64, device=DEV) * 0x0101010101
    counter = words[S.GUARD:S.GUARD + 1]
    counter.fill_(t0)
    for st in fl.views:
        st.copy_(torch.tensor([1.0, 0.0, 0.0]))
    snap, wsnap = fl.snapshot(), words.clone()
    args = (goal, step_size, alpha, 10.0, 1, S.GECO_BETA_MIN, S.GECO_BETA_MAX)
    for i in range(errs.numel()):
        _lib.call('gx_geco_update_step', P(fl.views[0]), P(errs[i:i + 1]), *args, P(counter), stream())
        assert int(counter) == t0 + i + 1
        _lib.call('gx_geco_update', P(fl.views[1]), P(errs[i:i + 1]), *args, stream())
        assert int(counter) == t0 + i + 1
        assert S.same_bits(fl.views[0], fl.views[1])
    assert fl.guards_unchanged(snap)
    wsnap[S.GUARD] = t0 + errs.numel()
    assert torch.equal(words, wsnap)
    rb, re_ = S.geco_ref_series(errs.cpu().numpy(), goal, step_size, alpha, 10)
    got = fl.views[0].cpu().double()
    assert abs(float(got[0]) - rb[-1]) <= 6 * S.GECO_SINGLE_RTOL * rb[-1] and abs(float(got[1]) - re_[-1]) <= 6 * S.GECO_SINGLE_RTOL * re_[-1]


def test_geco_loss_uses_the_beta_from_before_the_update(series):
    g = make_geco(series, 10, beta_init=0.25)
    err, kld = torch.tensor(3000.0, device=DEV), torch.tensor(8.0, device=DEV)
    loss = g.loss(err, kld)
    assert float(loss) == 3000.0 + 0.25 * 8.0
    assert float(g.beta) < 0.25 and float(g.err_ema) == 3000.0


# ------------------------------------------------------------------------------------------------- 3. gx_beta_warmup
@pytest.mark.parametrize('beta', [0.5, 0.0])
@pytest.mark.parametrize('warm', [4.0, 0.2 * 500000])
def test_beta_warmup_direct(warm, beta):
    """gx_beta_warmup at step 0, 1, warm - 1, warm, warm + 1 and 2^40 (an int64 counter) against clamp(beta step / warm, 0, beta)
    in float64: relative 1e-6, exact at step 0 and from step = warm on; the floats around *out keep their bits."""
    buf = S.GuardedBuffers(1, F32, 1, DEV, seed=4)
    snap = buf.snapshot()
    step = torch.zeros((), dtype=torch.int64, device=DEV)
    for t in (0, 1, int(warm) - 1, int(warm), int(warm) + 1, 2 ** 40):
        step.fill_(t)
        _lib.call('gx_beta_warmup', P(step), beta, warm, P(buf.views[0]), stream())
        got, want = float(buf.views[0]), S.beta_warmup_ref(beta, t, warm)
        if t == 0 or t >= warm:
            assert got == want == (0.0 if t == 0 else beta), (t, got, want)
        else:
            assert abs(got - want) <= 1e-6 * want, (t, got, want)
        assert int(step) == t
    assert buf.guards_unchanged(snap)


def test_beta_warmup_refuses_zero_warm_iters():
    step, out = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(GenesisHipError, match='gx_beta_warmup'):
        _lib.call('gx_beta_warmup', P(step), 0.5, 0.0, P(out), stream())


# ------------------------------------------------------------------------------------------------- 4. gx_elbo_fwd_grads
@pytest.mark.parametrize('beta', [1.0, 1e-10, 1e10])
@pytest.mark.parametrize('with_tail', [True, False])
@pytest.mark.parametrize('B,R', [(1, 0), (1, 1), (3, 9), (65, 1), (1, 65), (257, 3), (32, 18)])
def test_elbo_fwd_grads(B, R, with_tail, beta):
    """gx_elbo_fwd_grads (what the trainer launches; its d_err / d_kl start the backward pass).  (257, 3): R B > 256, the strided
    loops; (32, 18): MONet / GENESIS-style stacked KL rows; R = 0: kl = None.  err has mean 3000 and spread 1 (a float32
    accumulation of 257 of them is 1e-6 off).  out[0:5] and tail against float64 means: relative 2e-7 (the means are rounded to
    float once; loss = e + beta k rounds a product and a sum of them: 3 x 2^-24 = 1.8e-7); d_err = float32(1) / B and
    d_kl = beta / B exactly; everything bit-identical to elbo_fwd followed by elbo_bwd(g = 1); written through the C entry point
    into slices of one sentinel-filled buffer, nothing outside them changes."""
    g = torch.Generator().manual_seed(40 + B + R)
    err = (torch.randn(B, generator=g) + 3000).to(DEV)
    kl = (torch.rand(R, B, generator=g) * 10).to(DEV) if R else None
    bt = torch.tensor([beta], dtype=F32, device=DEV)
    tail = torch.full((2,), -7.0, device=DEV) if with_tail else None
    out, d_err, d_kl = hip.elbo_fwd_grads(err, kl, bt, tail)
    ref, ge, gk = S.elbo_ref(err, kl, S.f32(beta))
    finite(out, d_err, d_kl)
    o = out.cpu().double()
    assert bool(((o - ref).abs() <= 2e-7 * ref.abs()).all()), (o, ref)
    if R == 0:
        assert float(out[3]) == 0.0 and d_kl is None
    assert float(out[4]) == S.f32(beta)
    assert bool((d_err == float(ge)).all()) and float(ge) == float(np.float32(1) / np.float32(B))
    if R:
        assert d_kl.shape == (R, B) and bool((d_kl == float(gk)).all()), (d_kl.flatten()[:3], gk)
    if with_tail:
        assert S.same_bits(tail, out[2:4])
    # the two-launch form
    tail2 = torch.full((2,), -7.0, device=DEV) if with_tail else None
    loss, out2 = hip.elbo_fwd(err, kl, bt, tail2)
    e2, k2 = hip.elbo_bwd(torch.ones(1, device=DEV), bt, B, R)
    assert S.same_bits(out, out2) and S.same_bits(loss, out[0:1]) and S.same_bits(d_err, e2)
    assert (k2 is None and d_kl is None) or S.same_bits(d_kl, k2)
    if with_tail:
        assert S.same_bits(tail, tail2)
    # destinations inside one sentinel-filled buffer
    ar = Arena(B + R * B + 7 + 64)
    a_err, a_kl = ar.take(B), (ar.take(R, B) if R else None)
    a_out, a_tail = ar.take(5), (ar.take(2) if with_tail else None)
    _lib.call('gx_elbo_fwd_grads', P(err), P(kl), P(bt), B, R, P(a_out), P(a_tail), None, P(a_err), P(a_kl), stream())
    ar.untouched()
    assert S.same_bits(a_out, out) and S.same_bits(a_err, d_err) and (not R or S.same_bits(a_kl, d_kl))
    assert not with_tail or S.same_bits(a_tail, tail)


# ------------------------------------------------------------------------------------------------- 5. gx_mse_rmse
def call_mse(x, r, out, ws, ws_bytes=None):
    B = x.shape[0]
    _lib.call('gx_mse_rmse', P(x), P(r), B, x[0].numel(), P(out), P(ws), ws.numel() * 4 if ws_bytes is None else ws_bytes, stream())


@pytest.mark.parametrize('B,n', [(1, 1), (1, 255), (3, 257), (65, 105), (5, 3072)])
def test_mse_rmse_shapes(B, n):
    """gx_mse_rmse: n = 1 and 255 leave the 256-thread loop partly filled, 257 gives thread 0 a second trip; B = 65 puts the
    final average over more images than a wave.  Two launches on ONE workspace with different inputs: the second result is that
    of the second inputs (the completion counter re-arms itself); x == r: both outputs exactly 0; float64 reference, rtol 2e-6;
    out sits in a guarded buffer; a workspace one float short is refused."""
    g = torch.Generator().manual_seed(50 + B + n)
    xs = [torch.rand(B, n, generator=g) for _ in range(3)]
    buf = S.GuardedBuffers(2, F32, 1, DEV, seed=5)
    snap, out = buf.snapshot(), buf.views[0]
    ws = torch.zeros(B + 4, device=DEV)
    for x, r in ((xs[0], xs[1]), (xs[2] * 3, xs[0]), (xs[1], xs[1])):
        call_mse(x.to(DEV), r.to(DEV), out, ws)
        want = S.mse_rmse_ref(x, r)
        if x is r:
            assert float(out[0]) == 0.0 and float(out[1]) == 0.0
        else:
            np.testing.assert_allclose(out.cpu().numpy(), want, rtol=2e-6)
    assert buf.guards_unchanged(snap)
    assert _lib.query('gx_mse_rmse_ws_bytes', B) == 4 * (B + 4)
    with pytest.raises(GenesisHipError, match='workspace too small'):
        call_mse(xs[0].to(DEV), xs[1].to(DEV), out, ws, ws_bytes=4 * (B + 4) - 4)


# ------------------------------------------------------------------------------------------------- 6. cross-replica BatchNorm
def sync_emulated(ys, bias, prm, douts, out_dst=None):
    """`world` = len(ys) ranks on one device through hip.gated_bn_sync_fwd / _bwd: a first pass per rank records the rank's
    pack / sums (its all-reduce callable keeps a copy and leaves the tensor alone; what that pass goes on to compute is dropped),
    the copies are added on the device in rank order, and a second pass per rank gets the total from its callable.
    out_dst(k, r): the `out=` destinations of rank r's backward call in pass k (0: recording, 1: replaying).
    -> per rank (out, stats, dy, dgh, dbh, dgg, dbg, dbias), m."""
    world = len(ys)
    args = [to(t) for t in prm]

    def two_pass(call):
        packs = []
        for r in range(world):
            call(r, lambda t: packs.append(t.clone()), 0)
        assert len(packs) == world
        total = packs[0].clone()
        for q in packs[1:]:
            total += q
        return [call(r, lambda t: t.copy_(total), 1) for r in range(world)]

    fwd = two_pass(lambda r, red, k: hip.gated_bn_sync_fwd(ys[r], bias, *args, red, world))
    m = fwd[0][2]
    assert all(f[2] == m for f in fwd) and m == float(ys[0].numel() // ys[0].shape[1] * world)
    bwd = two_pass(lambda r, red, k: hip.gated_bn_sync_bwd(ys[r], bias, *args, fwd[r][1], douts[r], m, red,
                                                           out=None if out_dst is None else out_dst(k, r)))
    return [(fwd[r][0], fwd[r][1]) + tuple(bwd[r]) for r in range(world)], m


def global_stats(y, bias):
    """{mean, rstd} per unit [2C][2] of float32(y + bias) over the whole batch, in float64."""
    t = (y + bias.view(1, -1, 1, 1)).double()
    mean = t.mean((0, 2, 3))
    var = ((t - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    return torch.stack((mean, 1.0 / torch.sqrt(var + 1e-5)), 1).flatten()


def check_sync(y, bias, prm, g, world, dy_tol=(1e-4, 1e-5), single_dy_err=None):
    """y, g: the GLOBAL batch (world * N_shard images), split into equal shards.  Against gated_ref in float64 on the global
    batch and against hip.gated_norm_fwd / _bwd('bn') on it, at run_gated's tolerances."""
    C = y.shape[1] // 2
    b0 = bias if bias is not None else torch.zeros(2 * C)
    yr, br, pr = leaf(y), leaf(b0), [leaf(t) for t in prm]
    ref = gated_ref(yr, br, 'bn', pr)
    grads = torch.autograd.grad((ref * g.double()).sum(), [yr] + pr)
    yd, gd, bd = to(y), to(g), to(bias)
    ys, gs = list(yd.chunk(world)), list(gd.chunk(world))
    ys, gs = [t.contiguous() for t in ys], [t.contiguous() for t in gs]
    res, _ = sync_emulated(ys, bd, prm, gs)
    stats_ref = global_stats(y, b0)
    for r, (out, stats, dy, dgh, dbh, dgg, dbg, dbias) in enumerate(res):
        finite(out, stats, dy, dgh, dbh, dgg, dbg, dbias)
        close(out, ref.chunk(world)[r], 1e-5, 1e-5, 'rank %d fwd' % r)
        s = stats.cpu().double()
        assert s.numel() == 4 * C and bool(((s - stats_ref).abs() <= 1e-5 * stats_ref.abs()).all()), 'rank %d stats' % r
        close(dy, grads[0].chunk(world)[r], *dy_tol, msg='rank %d dy' % r)
        if bias is None:
            assert dbias is None
        else:
            assert S.same_bits(dbias, torch.zeros_like(dbias)), 'rank %d dbias' % r
    for i, nm in enumerate(('dgamma_h', 'dbeta_h', 'dgamma_g', 'dbeta_g')):
        close(sum(r_[3 + i].double() for r_ in res), grads[1 + i], 1e-4, 1e-4, nm)
    # the single-device kernels on the whole batch
    args = [to(t) for t in prm]
    out1, stats1 = hip.gated_norm_fwd(yd, bd, 'bn', *args)
    one = hip.gated_norm_bwd(yd, bd, 'bn', *args, stats1, gd)
    close(torch.cat([r_[0] for r_ in res]), out1, 1e-5, 1e-5, 'fwd against gated_norm_fwd')
    for r_ in res:
        s1 = stats1[:4 * C].cpu().double()
        assert bool(((r_[1].cpu().double() - s1).abs() <= 1e-5 * s1.abs()).all()), 'stats against gated_norm_fwd'
    close(torch.cat([r_[2] for r_ in res]), one[0], *dy_tol, msg='dy against gated_norm_bwd')
    for i, nm in enumerate(('dgamma_h', 'dbeta_h', 'dgamma_g', 'dbeta_g')):
        close(sum(r_[3 + i].double() for r_ in res), one[1 + i], 1e-4, 1e-4, nm + ' against gated_norm_bwd')
    if single_dy_err is not None:
        single_dy_err.append(float((one[0].cpu().double() - grads[0]).abs().max()))
        single_dy_err.append(float((torch.cat([r_[2] for r_ in res]).cpu().double() - grads[0]).abs().max()))
        single_dy_err.append(float(grads[0].abs().max()))


SYNC_SHAPES = [(1, 5, 1, 1), (2, 6, 5, 7), (2, 4, 3, 3), (3, 342, 2, 2), (5, 256, 1, 3), (2, 3, 33, 33), (1, 1100, 1, 1)]


@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('N,C,H,W', SYNC_SHAPES)
def test_sync_batchnorm_shards(N, C, H, W, world, with_bias):
    """`world` ranks with N images each, emulated on one device (sync_emulated).  Shapes, from nchunks = min(N, 2048 / (2 C)) of
    the local-sums kernels and the gx_ceil_div(HW, 1024) grid of the two apply kernels:
    (1,5,1,1): one value per plane and rank; (2,6,5,7), (2,4,3,3): HW = 35, 9, the scalar paths; (3,342,2,2): nchunks = 2 does not
    divide 3; (5,256,1,3): nchunks = 4, per = 2, an empty last chunk; (2,3,33,33): HW = 1089 > 1024, grid.y = 2 in both apply
    kernels; (1,1100,1,1): 2048 / (2 C) = 0, clamped to 1.  Every rank's out / dy against the matching slice of the float64
    reference on the global batch, its stats against the global {mean, rstd}, the affine gradients SUMMED over the ranks against
    the reference's, dbias exactly 0; the same against gated_norm_fwd / _bwd('bn') on the concatenated batch.

    (1,1100,1,1) at ONE rank is a batch of one value per channel: zero variance, rstd = 1 / sqrt(eps) = 316, and the reference dy
    is identically 0, so the bound is the bare atol 1e-5.  It caught gated_bwd_apply_kernel fusing dout * sig into the
    subtraction of S1 / m, which is that product ROUNDED: the half ulp left over, times rstd gamma = 411, was 1.138e-05
    (gated_dA in gx_gated.hip now rounds dA once for both passes)."""
    y, bias, prm, g = gated_operands(N * world, C, H, W)
    check_sync(y, bias if with_bias else None, prm, g, world)


HARD_DY_TOL = (1e-4, 1e-5)


def test_sync_batchnorm_hard_operands():
    """Channel means near 30 with a standard deviation of 1e-2, two ranks of (2, 4, 5, 7): a float32 sum of squares (900 per
    value, spacing 6e-5) could not hold a variance of 1e-4; the float64 {sum, sum of squares} do, and rstd = 100 must come out
    to 1e-5.  The values are built so that the question is the sums and nothing else: y + bias and the channel means are exact
    in float32 (multiples of 2^-19 in [16, 32), deviations in +- pairs scattered over both ranks), because a mean rounded to
    float (2e-6 at 30) is 2e-4 standard deviations whatever kernel normalises with it.  dout is scaled by 1e-2, so dy is O(1).
    dy keeps run_gated's 1e-4 / 1e-5: gated_norm_bwd('bn') on the same concatenated data stays far inside it against the same
    reference, so twice its error is no looser bound and none is taken.  The test prints both errors."""
    N, C, H, W, world = 2, 4, 5, 7, 2
    n = N * world * H * W
    gen = torch.Generator().manual_seed(60)
    q = 2.0 ** -19
    y = torch.empty(N * world, 2 * C, H, W)
    bias = torch.tensor([(ch % 5 - 2) / 16.0 for ch in range(2 * C)])
    for ch in range(2 * C):
        z = (torch.randn(n // 2, generator=gen).abs() * 1e-2 / q).round() * q
        z = torch.cat((z, -z))[torch.randperm(n, generator=gen)]
        y[:, ch] = ((30.0 + ch / 64.0 - float(bias[ch])) + z).view(N * world, H, W)
    t = (y + bias.view(1, -1, 1, 1))
    assert torch.equal(t.double(), y.double() + bias.double().view(1, -1, 1, 1))                       # y + bias is exact
    assert torch.equal(t.double().mean((0, 2, 3)), torch.tensor([30.0 + ch / 64.0 for ch in range(2 * C)], dtype=F64))
    assert not torch.equal(t[:N].double().mean((0, 2, 3)), t[N:].double().mean((0, 2, 3)))             # the ranks differ
    _, _, prm, g = gated_operands(N * world, C, H, W)
    errs = []
    check_sync(y, bias, prm, g * 1e-2, world, dy_tol=HARD_DY_TOL, single_dy_err=errs)
    print('hard operands: dy max error %.3e (gated_norm_bwd on the whole batch), %.3e (two ranks), reference max %.3e' % tuple(errs))


@pytest.mark.parametrize('N,C,H,W', [(2, 6, 5, 7), (2, 4, 4, 4)])
def test_sync_batchnorm_bwd_destinations(N, C, H, W):
    """gated_bn_sync_bwd(out=): each rank's five parameter-gradient destinations as slices of one sentinel-filled buffer (two
    ranks; a ragged and an aligned plane): nothing outside them changes, and they hold what the call without `out` returns."""
    world = 2
    y, bias, prm, g = gated_operands(N * world, C, H, W)
    ys, gs = [t.contiguous() for t in to(y).chunk(world)], [t.contiguous() for t in to(g).chunk(world)]
    plain, _ = sync_emulated(ys, to(bias), prm, gs)
    ar = Arena(world * 2 * (6 * C + 25) + 64)          # (both passes of sync_emulated write: every rank gets two sets)
    first = [[ar.take(C) for _ in range(4)] + [ar.take(2 * C)] for _ in range(world)]
    dst = [[ar.take(C) for _ in range(4)] + [ar.take(2 * C)] for _ in range(world)]
    res, _ = sync_emulated(ys, to(bias), prm, gs, out_dst=lambda k, r: tuple((first, dst)[k][r]))
    ar.untouched()
    for r in range(world):
        assert S.same_bits(res[r][2], plain[r][2])
        for d, got, want in zip(dst[r], res[r][3:], plain[r][3:]):
            assert got.data_ptr() == d.data_ptr() and S.same_bits(d, want)
        for d, e in zip(dst[r][:5], first[r][:5]):
            assert S.same_bits(d, e)                   # (the rank's own sums do not depend on the all-reduce)


def run_gated_fn(y, bias, prm, g, sync, direct, monkeypatch):
    """sylvester.GatedNormFn on the 'bn' path -> (out, dy, [dgh, dbh, dgg, dbg, dbias]); direct: the parameter gradients go
    straight into preallocated p.grad buffers (functions._gout), the Function returns None for them."""
    from genesis_amd import functions as fn, sylvester
    monkeypatch.setitem(sylvester._SYNC, 'on', sync)
    monkeypatch.setattr(sylvester, '_world', lambda: 1)
    monkeypatch.setattr(sylvester, '_all_reduce_sum', lambda t, info=None: None)
    st = fn.step_state()
    monkeypatch.setattr(st, 'direct_param_grads', direct)
    fn.begin_direct_grads()
    yd = to(y).requires_grad_()
    params = [torch.nn.Parameter(to(t)) for t in [bias] + list(prm)]
    if direct:
        for p in params:
            p.grad = torch.full_like(p, float('nan'))
    out, stats = sylvester.GatedNormFn.apply(yd, params[0], 'bn', *params[1:])
    assert not stats.requires_grad
    (out * to(g)).sum().backward()
    fn.begin_direct_grads()
    return out.detach(), yd.grad, [params[i].grad for i in (1, 2, 3, 4, 0)]


@pytest.mark.parametrize('direct', [False, True])
@pytest.mark.parametrize('N,C,H,W', [(2, 6, 5, 7), (2, 3, 33, 33)])
def test_gated_norm_fn_sync_branch_on_one_rank(N, C, H, W, direct, monkeypatch):
    """GatedNormFn.forward / backward with cross-replica statistics switched on, a world of one and an identity all-reduce (no
    process group): the same output and the same gradients -- y, bias, the four affine parameters; direct: through the deferred
    p.grad destinations -- as with the switch off, at run_gated's tolerances, and both against gated_ref in float64."""
    y, bias, prm, g = gated_operands(N, C, H, W)
    yr, br, pr = leaf(y), leaf(bias), [leaf(t) for t in prm]
    ref = gated_ref(yr, br, 'bn', pr)
    grads = torch.autograd.grad((ref * g.double()).sum(), [yr] + pr + [br])
    off = run_gated_fn(y, bias, prm, g, False, direct, monkeypatch)
    on = run_gated_fn(y, bias, prm, g, True, direct, monkeypatch)
    for res, which in ((off, 'off'), (on, 'on')):
        finite(res[0], res[1], *res[2])
        close(res[0], ref, 1e-5, 1e-5, 'fwd, sync ' + which)
        close(res[1], grads[0], 1e-4, 1e-5, 'dy, sync ' + which)
        for got, want, nm in zip(res[2], grads[1:], ('dgamma_h', 'dbeta_h', 'dgamma_g', 'dbeta_g')):
            close(got, want, 1e-4, 1e-4, '%s, sync %s' % (nm, which))
        assert S.same_bits(res[2][4], torch.zeros_like(res[2][4])), 'dbias, sync ' + which
    close(on[0], off[0], 1e-5, 1e-5, 'fwd, on against off')
    close(on[1], off[1], 1e-4, 1e-5, 'dy, on against off')
    for a, b in zip(on[2][:4], off[2][:4]):
        close(a, b, 1e-4, 1e-4, 'affine gradients, on against off')


def test_sync_batchnorm_refusals():
    """A workspace one byte smaller than gx_gated_bn_sums_ws_bytes (both local-sums entry points) and m < 1 (both apply entry
    points) are refused."""
    N, C, H, W = 2, 4, 3, 3
    y, bias, prm, g = gated_operands(N, C, H, W)
    yd, bd, gd = to(y), to(bias), to(g)
    a = [to(t) for t in prm]
    nb = _lib.query('gx_gated_bn_sums_ws_bytes', N, C)
    assert nb == 4 * 2 * C * min(N, 2048 // (2 * C)) * 4
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    pack, sums, stats = torch.zeros(4 * C, dtype=F64, device=DEV), torch.zeros(4 * C, device=DEV), torch.zeros(4 * C, device=DEV)
    out, dy, d = torch.zeros(N, C, H, W, device=DEV), torch.zeros_like(yd), [torch.zeros(C, device=DEV) for _ in range(4)]
    with pytest.raises(GenesisHipError, match='gx_gated_bn_local_sums: workspace too small'):
        _lib.call('gx_gated_bn_local_sums', P(yd), P(bd), N, C, H, W, P(pack), P(ws), nb - 1, stream())
    with pytest.raises(GenesisHipError, match='gx_gated_bn_bwd_local_sums: workspace too small'):
        _lib.call('gx_gated_bn_bwd_local_sums', P(yd), P(bd), *[P(t) for t in a], P(stats), P(gd), N, C, H, W, P(sums),
                  *[P(t) for t in d], None, P(ws), nb - 1, stream())
    for m in (0.0, 0.5):
        with pytest.raises(GenesisHipError, match='gx_gated_bn_apply'):
            _lib.call('gx_gated_bn_apply', P(yd), P(bd), P(pack), m, *[P(t) for t in a], N, C, H, W, 1e-5, P(out), P(stats), stream())
        with pytest.raises(GenesisHipError, match='gx_gated_bn_bwd_apply'):
            _lib.call('gx_gated_bn_bwd_apply', P(yd), P(bd), *[P(t) for t in a], P(stats), P(gd), P(sums), m, N, C, H, W, P(dy),
                      stream())
