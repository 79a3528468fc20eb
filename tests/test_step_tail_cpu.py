"""The restatements of tests/step_tail_restatement.py against what they restate, and the float32 bounds they carry -- no GPU:
  * adam_ref / rmsprop_ref / sgd_ref against torch.optim.Adam / RMSprop / SGD(momentum 0.9) in float64: 1e-14;
  * torch.optim.Adam in float32 against adam_ref: the measured one-step error, printed, inside ADAM_F32_ERR (the kernels are
    held to ADAM_GPU_MARGIN times that by tests/test_step_tail_gpu.py);
  * geco_ref against the reference's own GECO class as recorded in tests/golden/geco_series.npz, and the drift of a float32
    transcription over the 300-step series, printed, inside GECO_F32_DRIFT;
  * the small formulas (warm-up, ELBO aggregation, mse / rmse) against the expressions of the reference's training loop."""
import os.path as osp

import numpy as np
import pytest
import torch

from tests import step_tail_restatement as S

F64 = torch.float64
GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'geco_series.npz')


def _adam(params, t0):
    """torch.optim.Adam(lr) whose state starts at step counter t0 with zero moments."""
    opt = torch.optim.Adam(params, S.LR, betas=(S.BETA1, S.BETA2), eps=S.ADAM_EPS)
    for p in params:
        opt.state[p] = {'step': torch.tensor(float(t0), dtype=F64), 'exp_avg': torch.zeros_like(p),
                        'exp_avg_sq': torch.zeros_like(p)}
    return opt


@pytest.mark.parametrize('t0', [0, 99999, 2 ** 31 + 6])
def test_adam_restatement_is_torch_adam_in_float64(t0):
    """Five steps from counter t0 (0; 99999: pow(b2, t) has underflowed towards bc2 = 1; 2^31 + 6: past int32)."""
    _, p, grads = S.optimiser_inputs(33, 10007, 5, seed=1)
    ref = p.clone().requires_grad_()
    opt = _adam([ref], t0)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for it, (_, g) in enumerate(grads):
        ref.grad = g.clone()
        opt.step()
        p, m, v = S.adam_ref(p, g, m, v, t0 + it + 1)
        st = opt.state[ref]
        assert float(st['step']) == t0 + it + 1
        for got, want, name in ((p, ref.detach(), 'p'), (m, st['exp_avg'], 'm'), (v, st['exp_avg_sq'], 'v')):
            np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-14, atol=1e-14, err_msg='%s, step %d' % (name, it + 1))
    if t0:
        assert S.adam_scalars(t0 + 1) == (S.LR, 1.0)


@pytest.mark.parametrize('kind', ['rmsprop', 'sgd'])
def test_rmsprop_and_sgd_restatements_are_torch_in_float64(kind):
    _, p, grads = S.optimiser_inputs(33, 10007, 5, seed=2)
    ref = p.clone().requires_grad_()
    opt = torch.optim.RMSprop([ref], S.LR) if kind == 'rmsprop' else torch.optim.SGD([ref], S.LR, S.SGD_MOMENTUM)
    m = torch.zeros_like(p)
    for it, (_, g) in enumerate(grads):
        ref.grad = g.clone()
        opt.step()
        p, m = S.rmsprop_ref(p, g, m) if kind == 'rmsprop' else S.sgd_ref(p, g, m)
        state = opt.state[ref]['square_avg' if kind == 'rmsprop' else 'momentum_buffer']
        np.testing.assert_allclose(p.numpy(), ref.detach().numpy(), rtol=1e-14, atol=1e-14, err_msg='p, step %d' % (it + 1))
        np.testing.assert_allclose(m.numpy(), state.numpy(), rtol=1e-14, atol=1e-14, err_msg='state, step %d' % (it + 1))


def test_grad_scale_multiplies_the_gradient_first():
    """adam_ref(g, grad_scale) is adam_ref(g * grad_scale): the scale is the float32-rounded value, widened."""
    _, p, grads = S.optimiser_inputs(1, 257, 1, seed=3)
    g, z = grads[0][1], torch.zeros_like(p)
    third = S.GRAD_SCALES[3]
    assert third == float(np.float32(1.0 / 3.0)) and third != 1.0 / 3.0
    for a, b in zip(S.adam_ref(p, g, z, z, 1, third), S.adam_ref(p, g * third, z, z, 1)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n32,n64', S.PAIR_SIZES)
def test_float32_adam_stays_inside_the_bound(n32, n64):
    """torch.optim.Adam in float32 on the CPU over the inputs of the GPU test (every size, every gradient scale, five steps):
    its one-step error against adam_ref on the float32 state it started the step from, in the three figures of
    step_tail_restatement's docstring.  Prints the maxima; they lie inside ADAM_F32_ERR, the kernels are allowed
    ADAM_GPU_MARGIN (4) times ADAM_F32_ERR."""
    p0, _, grads = S.optimiser_inputs(n32, n64, 5)
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for gs in S.GRAD_SCALES:
        ref = p0.clone().requires_grad_()
        opt = _adam([ref], 0)
        for it, (g, _) in enumerate(grads):
            st = opt.state[ref]
            before = (ref.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone())
            ref.grad = g * np.float32(gs)                  # (float32 times float32, rounded: what a float32 implementation holds)
            opt.step()
            want = S.adam_ref(before[0], g, before[1], before[2], it + 1, gs)
            r = S.adam_f32_ratios((ref.detach(), st['exp_avg'], st['exp_avg_sq']), want,
                                  S.adam_scales(before[0], g, before[1], before[2], it + 1, gs))
            worst = {k: max(worst[k], r[k]) for k in worst}
    print('\nfloat32 torch.optim.Adam against adam_ref at (n32 = %d): p %.3e (past one ulp of p), m %.3e, '
          'v %.3e; recorded bound p %.1e m %.1e v %.1e, kernels allowed %g x' %
          (n32, worst['p'], worst['m'], worst['v'], S.ADAM_F32_ERR['p'], S.ADAM_F32_ERR['m'], S.ADAM_F32_ERR['v'],
           S.ADAM_GPU_MARGIN))
    for k in worst:
        assert worst[k] <= S.ADAM_F32_ERR[k], (k, worst[k])


# ------------------------------------------------------------------------------------------------- GECO
@pytest.fixture(scope='module')
def series():
    return dict(np.load(GOLDEN))


def _prm(s):
    return dict(goal=float(s['goal']), step_size=float(s['step_size']), alpha=float(s['alpha']))


def test_the_recorded_series_takes_every_branch(series):
    """The fixture is what the issue asks for: 300 steps from 3 x goal, the moving average crosses the goal many times in both
    directions, and the two speedup settings part after the first crossing."""
    s = series
    goal, err = float(s['goal']), s['main_err'].astype(np.float64)
    assert err.shape == (300,) and err[0] == np.float32(3 * goal) and err[99] > 0.8 * goal > err[100] * 0.999
    c = goal - s['main_su10_ema'].astype(np.float64)
    first = int(np.argmax(c > 0))
    assert 90 < first < 130 and (c[:first] < 0).all()
    flips = np.diff(np.sign(c))
    assert (flips > 0).sum() >= 4 and (flips < 0).sum() >= 4
    assert np.array_equal(s['main_su10_beta'][:first], s['main_none_beta'][:first])
    assert (s['main_su10_beta'][first:] != s['main_none_beta'][first:]).all()


@pytest.mark.parametrize('case,speedup', [('main_su10', 10), ('main_none', None)])
def test_float32_geco_drift_on_the_series(series, case, speedup):
    """geco_ref (float64) over the recorded series against (a) the reference's own class as recorded and (b) a float32 torch
    transcription run here: the relative distance of beta and of the moving average, printed.  (b) lies inside GECO_F32_DRIFT,
    the kernel is allowed GECO_GPU_MARGIN (4) times GECO_F32_DRIFT over the curve -- and so is the recording, which is another
    machine's float32 exp."""
    s = series
    if speedup is not None:
        assert float(s['speedup']) == speedup
    beta, ema = S.geco_ref_series(s['main_err'], speedup=speedup, **_prm(s))
    b32, e32 = S.geco_f32_series(s['main_err'], speedup=speedup, **_prm(s))
    here = {'beta': S.rel_dist(b32, beta), 'ema': S.rel_dist(e32, ema)}
    rec = {'beta': S.rel_dist(s[case + '_beta'], beta), 'ema': S.rel_dist(s[case + '_ema'], ema)}
    bound = S.GECO_F32_DRIFT[case]
    print('\nGECO %s: float32 transcription against geco_ref: beta %.3e, ema %.3e; the recorded reference: beta %.3e, ema %.3e; '
          'recorded bound beta %.1e ema %.1e, kernel allowed %g x' %
          (case, here['beta'], here['ema'], rec['beta'], rec['ema'], bound['beta'], bound['ema'], S.GECO_GPU_MARGIN))
    for k in here:
        assert here[k] <= bound[k], (k, here[k])
        assert rec[k] <= S.GECO_GPU_MARGIN * bound[k], (k, rec[k])


def test_geco_restatement_on_the_clamps_and_at_the_goal(series):
    s = series
    prm = dict(goal=float(s['goal']), alpha=float(s['alpha']), speedup=float(s['speedup']))
    beta, _ = S.geco_ref_series(s['lo_clamp_err'], step_size=1.0, beta_init=1e-9, **prm)
    assert (beta == S.GECO_BETA_MIN).all() and (s['lo_clamp_beta'] == np.float32(1e-10)).all()
    beta, _ = S.geco_ref_series(s['hi_clamp_err'], step_size=1.0, **prm)
    assert (beta == S.GECO_BETA_MAX).all() and (s['hi_clamp_beta'] == np.float32(1e10)).all()
    # err = goal at the first call: constraint 0, factor exp(0) = 1
    assert S.geco_ref(0.37, None, prm['goal'], prm['goal'], 4e-5, 0.9, 10) == (0.37, prm['goal'])
    # the branch: a positive constraint is sped up, a negative one is not, and without speedup neither is
    up = S.geco_ref(1.0, None, 90.0, 100.0, 1e-3, 0.9, 10)[0]
    assert up == pytest.approx(np.exp(10 * 1e-3 * 10.0), rel=1e-15)
    assert S.geco_ref(1.0, None, 110.0, 100.0, 1e-3, 0.9, 10)[0] == pytest.approx(np.exp(-1e-3 * 10.0), rel=1e-15)
    assert S.geco_ref(1.0, None, 90.0, 100.0, 1e-3, 0.9, None)[0] == pytest.approx(np.exp(1e-3 * 10.0), rel=1e-15)
    # a resumed moving average: (1 - alpha) err + alpha ema
    assert S.geco_ref(1.0, 120.0, 100.0, 100.0, 1e-3, 0.9, None)[1] == pytest.approx(0.1 * 100.0 + 0.9 * 120.0, rel=1e-15)


# ------------------------------------------------------------------------------------------------- the small formulas
def test_small_restatements():
    # the reference's loop: beta = beta * iter / (0.2 * train_iter) clamped to [0, beta]
    for beta in (0.5, 0.0):
        for warm in (4.0, 0.2 * 500000):
            for step in (0, 1, int(warm) - 1, int(warm), int(warm) + 1, 2 ** 40):
                want = float(torch.tensor(beta * step / warm, dtype=F64).clamp(0.0, beta))
                assert S.beta_warmup_ref(beta, step, warm) == want
            assert S.beta_warmup_ref(beta, 0, warm) == 0.0 and S.beta_warmup_ref(beta, 2 ** 40, warm) == beta
    g = torch.Generator().manual_seed(4)
    err, kl = torch.randn(7, generator=g) + 3000, torch.rand(3, 7, generator=g)
    out, d_err, d_kl = S.elbo_ref(err, kl, 0.25)
    e, k = err.double().mean(), torch.stack(list(kl.double()), dim=1).mean(dim=0).sum()       # train.py's aggregation
    np.testing.assert_allclose(out.numpy(), [e + 0.25 * k, e + k, e, k, 0.25], rtol=1e-15)
    assert d_err == np.float32(1) / np.float32(7) and d_kl == np.float32(0.25) / np.float32(7)
    assert float(S.elbo_ref(err, None, 0.25)[0][3]) == 0.0
    x, r = torch.rand(3, 50, generator=g), torch.rand(3, 50, generator=g)
    mse = ((x.double() - r.double()) ** 2).mean(1)
    assert S.mse_rmse_ref(x, r) == (float(mse.mean()), float(mse.sqrt().mean()))
