"""The gradient contract of the models' OUTPUTS, not only of their loss terms: a loss term on any forward output a user can
differentiate (comp_stats.mu_k, z_k, q_z_k, stats.log_m_k, x_r_k, log_m_r_k, recon) must reach the parameters -- eagerly and in the
unchanged loop's replayed form (genesis_amd/autostep.py), where the captured forward's static tensors come back through one autograd
node -- and agree with the fp64 oracle on the same weights, input and noise (the budget of tests/test_error_budget_gpu.py).
Settings a captured forward bakes in (a frozen parameter, model.std, pixel_bound, detach_mr_in_klm, autoreg_prior, the attention
kernel) changed after the capture must give what the eager loop gives; outputs without a backward kernel (log_s_k, colour, seeds)
must raise when a gradient reaches them instead of dropping it."""
import functools

import pytest
import torch

from tests.test_autostep_gpu import _state_is_clean
from tests.test_error_budget_gpu import grads_of, hip_grads, judge, relerr, to_dtype

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K, S, D, B = 4, 32, 16, 2         # the 'tiny' golden configuration
TOL = 5e-5                       # eager vs replayed gradients (the bar of test_graph_loop_falls_back_and_stays_correct)
WARM = 4                         # standard iterations before the measured one: by then the loop replays
MEASURED_SEED = 5

CONFIGS = {'tiny': {}, 'klm_nodetach': dict(klm_loss=True, detach_mr_in_klm=False)}


def _fixed(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


_V = _fixed((K, B, D), 17)       # the fixed point at which q_z_k is evaluated


def _sq(t):
    return t.pow(2).sum() / t.shape[-4 if t.dim() >= 4 else -2]


def _stack(l):
    return torch.stack(list(l))


def _log_prob(mu, sigma, v):
    return (-((v - mu) ** 2) / (2 * sigma ** 2) - sigma.log()).sum() / mu.shape[-2]


# output name -> (term on the model's five return values, term on the oracle's, parameter prefix upstream of it).  Each term is a
# smooth function summed over the output and divided by B: the scale of err, so that it moves the upstream gradients visibly.
OUTPUTS = {
    'mu_k': (lambda r: _sq(_stack(r[4].mu_k)), lambda o: _sq(_stack(o[4]['mu_k'])), 'z_head.'),
    'sigma_k': (lambda r: _sq(_stack(r[4].sigma_k)), lambda o: _sq(_stack(o[4]['sigma_k'])), 'z_head.'),
    'z_k': (lambda r: _sq(_stack(r[4].z_k)), lambda o: _sq(_stack(o[4]['z_k'])), 'z_head.'),
    'q_z_k': (lambda r: sum(q.log_prob(_V[k].float().to(DEV)).sum() for k, q in enumerate(r[4].q_z_k)) / B,
              lambda o: _log_prob(_stack(o[4]['mu_k']), _stack(o[4]['sigma_k']), _V.to(o[4]['mu_k'][0].dtype)), 'z_head.'),
    'log_m_k': (lambda r: _sq(_stack(r[2].log_m_k)), lambda o: _sq(_stack(o[2]['log_m_k'])), 'seg_head.'),
    'x_r_k': (lambda r: _sq(_stack(r[2].x_r_k)), lambda o: _sq(_stack(o[2]['x_r_k'])), 'decoder_module.'),
    'log_m_r_k': (lambda r: _sq(_stack(r[2].log_m_r_k)), lambda o: _sq(_stack(o[2]['log_m_r_k'])), 'decoder_module.'),
    'recon': (lambda r: _sq(r[0]), lambda o: _sq(o[0]), 'decoder_module.'),
}


def _v2_cfg(**over):
    from oracle import v2_oracle as O
    return O.make_cfg(K_steps=K, img_size=S, feat_dim=D, **over)


def _v2_model(cfg):
    """test_error_budget_gpu.py::test_genesis_v2's setup: default initialisation under seed 7, the semiconv gate opened."""
    import genesis_amd.genesisv2_config as G
    from genesis_amd.compat.attrdict import AttrDict
    torch.manual_seed(7)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    with torch.no_grad():
        model.att_process.colour_head.gate.gate.fill_(0.2)
    return model


@functools.lru_cache(maxsize=None)
def _input():
    from genesis_amd import testing as T
    return T.make_input(99, B, S)


def _noise(seed):
    """What the model's forward draws after torch.manual_seed(seed), in _compute's order: the uniform seed-pixel draw, then eps."""
    torch.manual_seed(seed)
    rp = torch.rand(B, 1, S, S, device=DEV)
    eps = torch.randn(K, B, D, device=DEV)
    return rp.cpu(), list(eps.cpu().unbind(0))


def _base_loss(r):
    losses = r[1]
    loss = losses.err.mean(0) + torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()
    if 'kl_m' in losses:
        loss = loss + losses.kl_m.mean(0)
    return loss


def _oracle(sd, cfg, noise, term, dtype):
    from oracle import v2_oracle as O
    rp, eps = noise
    p = to_dtype(sd, dtype)
    out = O.v2_forward(p, _input().to(dtype), cfg, rp.to(dtype), [e.to(dtype) for e in eps], reference_form=False)
    e, kl, klm = O.aggregate_losses(out[1])
    loss = e + kl + klm.to(dtype)
    if term is not None:
        loss = loss + term(out)
    loss.backward()
    return out, grads_of(p)


def _grads(model):
    return {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in model.named_parameters()}


def _rel(a, b, big):
    return float((a.double() - b.double()).norm()) / (float(b.double().norm()) + 1e-6 * big)


def _assert_same_grads(got, want, what, tol=TOL):
    big = max(float(v.double().norm()) for v in want.values())
    for n in want:
        e = _rel(got[n], want[n], big)
        assert e <= tol, (what, n, e)


def _standard_iteration(model, opt, xd, seed):
    opt.zero_grad()
    torch.manual_seed(seed)
    r = model(xd)
    loss = _base_loss(r)
    loss.backward()
    opt.step()
    return r


def _measured(model, graph, term):
    """WARM standard iterations (SGD at lr 0: the parameters stay the initial ones), the measured one with `term` added to the
    loss, three standard ones.  -> (gradients and err of the measured iteration, graph_stats before / after it / at the end)."""
    from genesis_amd import autostep
    autostep.GRAPH = graph
    xd = _input().to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    for it in range(WARM):
        _standard_iteration(model, opt, xd, 1 + it)
    s0 = autostep.graph_stats(model)
    opt.zero_grad()
    torch.manual_seed(MEASURED_SEED)
    r = model(xd)
    (_base_loss(r) + term(r)).backward()
    s1 = autostep.graph_stats(model)
    g, err = _grads(model), r[1].err.detach().clone()
    for it in range(3):
        _standard_iteration(model, opt, xd, 10 + it)
    s2 = autostep.graph_stats(model)
    _state_is_clean()
    return g, err, (s0, s1, s2)


@functools.lru_cache(maxsize=None)
def _oracle_base(config):
    cfg = _v2_cfg(**CONFIGS[config])
    sd = {k: v.clone() for k, v in _v2_model(cfg).state_dict().items()}
    return cfg, sd, _oracle(sd, cfg, _noise(MEASURED_SEED), None, torch.float64)[1]


def _delta(s1, s0):
    return tuple(a - b for a, b in zip(s1, s0))


@pytest.fixture
def autostep_on():
    from genesis_amd import autostep
    prev = (autostep.ENABLED, autostep.GRAPH)
    autostep.ENABLED = True
    try:
        yield autostep
    finally:
        autostep.ENABLED, autostep.GRAPH = prev


# ------------------------------------------------------------------------------------------------ A. a loss on each output
@pytest.mark.parametrize('out', list(OUTPUTS))
@pytest.mark.parametrize('config', list(CONFIGS))
def test_loss_on_an_output_eager_and_replayed_equals_fp64(config, out, autostep_on):
    term, oterm, upstream = OUTPUTS[out]
    cfg, sd, g64_base = _oracle_base(config)
    g_eager, err_eager, _ = _measured(_v2_model(cfg).to(DEV), False, term)
    g_graph, err_graph, (s0, s1, s2) = _measured(_v2_model(cfg).to(DEV), True, term)
    noise = _noise(MEASURED_SEED)
    o64, g64 = _oracle(sd, cfg, noise, oterm, torch.float64)
    o32, g32 = _oracle(sd, cfg, noise, oterm, torch.float32)
    # (err at fp32 tolerance: the noise drawn here is the noise the model drew)
    assert relerr(err_eager, o64[1]['err']) <= 2e-5 and relerr(err_graph, o64[1]['err']) <= 2e-5
    fwd = [('err', err_eager, o32[1]['err'], o64[1]['err'])]
    for what, g in (('eager', g_eager), ('replayed', g_graph)):
        bad = judge(fwd, list(g.items()), g32, g64, 'V2 %s, loss on %s, %s' % (config, out, what))
        assert not bad, (what, bad)
    _assert_same_grads(g_graph, g_eager, (config, out, 'replayed vs eager'))
    # the measured iteration was a forward replay whose backward took the retained-graph fallback; the loop replays on after it
    assert _delta(s1, s0) == (1, 0, 1), (s0, s1)
    assert _delta(s2, s1) == (3, 3, 0), (s1, s2)
    # not vacuous: the term moves the gradients upstream of the output by far more than the tolerance
    names = [n for n in g64 if n.startswith(upstream)]
    moved = float(torch.cat([(g64[n] - g64_base[n]).flatten() for n in names]).norm()) \
        / float(torch.cat([g64_base[n].flatten() for n in names]).norm())
    assert moved > 100 * TOL, (out, moved)


def test_adam_loop_with_a_latent_term_in_every_iteration(autostep_on):
    """A loss on z_k in EVERY iteration: the backward graph is captured for that set of outputs and replayed; the trajectory is
    the eager one (tolerances of test_unchanged_loop_as_two_replayed_graphs_equals_the_eager_loop)."""
    term = OUTPUTS['z_k'][0]
    cfg = _v2_cfg()
    xd = _input().to(DEV)

    def run(graph):
        autostep_on.GRAPH = graph
        model = _v2_model(cfg).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        hist = []
        for it in range(6):
            opt.zero_grad()
            torch.manual_seed(100 + it)
            r = model(xd)
            err = r[1].err.mean(0)
            kl = torch.stack(r[1].kl_l_k, dim=1).mean(dim=0).sum()
            (err + kl + term(r)).backward()
            opt.step()
            hist.append((float(err.detach()), float(kl.detach())))
        return hist, model
    h0, _ = run(False)
    h1, model = run(True)
    assert autostep_on.graph_stats(model) == (4, 4, 0), autostep_on.graph_stats(model)
    for a, b in zip(h0, h1):
        assert abs(a[0] - b[0]) <= 2e-4 * abs(a[0]) and abs(a[1] - b[1]) <= 2e-3 * abs(a[1]) + 1e-4, (h0, h1)
    _state_is_clean()


def _monet_setup():
    from oracle import monet_oracle as O
    import genesis_amd.monet_config as G
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd import testing as T
    Km, Sm, Bm = 4, 32, 2
    cfg = O.make_cfg(K_steps=Km, img_size=Sm)
    torch.manual_seed(11)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    x = T.make_input(98, Bm, Sm)
    eps = torch.randn(Km * Bm, cfg['comp_ldim'], generator=torch.Generator().manual_seed(5))
    run = lambda m: m(x.to(DEV), eps.to(DEV))                                                       # noqa: E731
    oracle = lambda p, dt: O.monet_forward(p, x.to(dt), cfg, eps.to(dt))                            # noqa: E731
    return model, run, oracle, O.aggregate_losses


def _genesis_setup():
    from oracle import genesis_oracle as O
    import genesis_amd.genesis_config as G
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd import testing as T
    Kg, Sg, Bg = 3, 32, 2
    cfg = O.make_cfg(K_steps=Kg, img_size=Sg)
    torch.manual_seed(13)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    x = T.make_input(97, Bg, Sg)
    gen = torch.Generator().manual_seed(6)
    eps_m = [torch.randn(Bg, cfg['attention_latents'], generator=gen) for _ in range(Kg)]
    eps_c = torch.randn(Kg * Bg, cfg['comp_ldim'], generator=gen)
    run = lambda m: m(x.to(DEV), [e.to(DEV) for e in eps_m], eps_c.to(DEV))                        # noqa: E731
    oracle = lambda p, dt: O.genesis_forward(p, x.to(dt), cfg, [e.to(dt) for e in eps_m], eps_c.to(dt))   # noqa: E731
    return model, run, oracle, O.aggregate_losses


@pytest.mark.parametrize('out', ['recon', 'x_r_k'])
@pytest.mark.parametrize('family', ['monet', 'genesis'])
def test_mixture_w_outputs_are_differentiable(family, out):
    """MONet / GENESIS (MixtureWFn: the attention masks as mixing weights): a loss on recon or x_r_k, eagerly, against fp64."""
    model, run, oracle, agg = (_monet_setup if family == 'monet' else _genesis_setup)()
    term = (lambda r: _sq(r[0])) if out == 'recon' else (lambda r: _sq(_stack(r[2]['x_r_k'])))
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def ref(dtype, with_term=True):
        p = to_dtype(sd, dtype)
        o = oracle(p, dtype)
        e, kl_l, kl_m = agg(o[1])
        loss = e + kl_l + kl_m
        if with_term:
            loss = loss + term(o)
        loss.backward()
        return o, grads_of(p)
    o64, g64 = ref(torch.float64)
    o32, g32 = ref(torch.float32)
    _, g64_base = ref(torch.float64, False)
    model = model.to(DEV).train()
    r = run(model)
    losses = r[1]
    kl_l = torch.stack(list(losses.kl_l_k), 1).mean(0).sum()
    kl_m = losses.kl_m.mean(0) if 'kl_m' in losses else torch.stack(list(losses.kl_m_k), 1).mean(0).sum()
    (losses.err.mean(0) + kl_l + kl_m + term(r)).backward()
    fwd = [('recon', r[0], o32[0], o64[0]), ('err', losses.err, o32[1]['err'], o64[1]['err'])]
    bad = judge(fwd, hip_grads(model), g32, g64, '%s, loss on %s' % (family, out))
    assert not bad, bad
    names = [n for n in g64 if n.startswith('comp_vae.decoder_module.')]
    moved = float(torch.cat([(g64[n] - g64_base[n]).flatten() for n in names]).norm()) \
        / float(torch.cat([g64_base[n].flatten() for n in names]).norm())
    assert moved > 100 * TOL, moved


# ------------------------------------------------------------------------------------------------ B. settings changed after capture
def _freeze(m, on):
    m.encoder.down[1][0].weight.requires_grad_(not on)


def _set(attr, value, sub=None):
    def f(m, on):
        obj = getattr(m, sub) if sub else m
        if on:
            f.saved = getattr(obj, attr)
            setattr(obj, attr, value(f.saved))
        else:
            setattr(obj, attr, f.saved)
    return f


SETTINGS = {
    'requires_grad': ('tiny', _freeze),
    'std': ('tiny', _set('std', lambda v: 0.5)),
    'pixel_bound': ('tiny', _set('pixel_bound', lambda v: not v)),
    'detach_mr_in_klm': ('klm_nodetach', _set('detach_mr_in_klm', lambda v: not v)),
    'autoreg_prior': ('tiny', _set('autoreg_prior', lambda v: not v)),
    'kernel': ('tiny', _set('kernel', lambda v: 'laplacian', 'att_process')),
}
AFTER = 4        # iterations with the change: the first replays the old capture if the key misses it, the fourth a new one


@pytest.mark.parametrize('setting', list(SETTINGS))
def test_setting_changed_after_capture(setting, autostep_on):
    config, change = SETTINGS[setting]
    cfg = _v2_cfg(**CONFIGS[config])
    xd = _input().to(DEV)

    def run(graph):
        autostep_on.GRAPH = graph
        model = _v2_model(cfg).to(DEV)
        opt = torch.optim.SGD(model.parameters(), lr=1e-6)      # (small: a frozen parameter that got a gradient would move)
        for it in range(3):
            _standard_iteration(model, opt, xd, 1 + it)        # captured by the third (graph on)
        change(model, True)
        frozen = model.encoder.down[1][0].weight
        w0 = frozen.detach().clone()
        sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        out = []
        for it in range(AFTER):
            r = _standard_iteration(model, opt, xd, 20 + it)
            if setting == 'requires_grad':
                assert frozen.grad is None, (graph, it)
            out.append((r[1].err.detach().clone(), torch.stack(list(r[1].kl_l_k)).detach().clone(), _grads(model)))
        if setting == 'requires_grad':
            assert torch.equal(frozen.detach(), w0), graph
        change(model, False)
        s0 = autostep_on.graph_stats(model)
        for it in range(autostep_on._STABLE_ITERS + 1):
            _standard_iteration(model, opt, xd, 30 + it)
        s1 = autostep_on.graph_stats(model)
        _state_is_clean()
        return out, sd0, _delta(s1, s0)
    eager, _, _ = run(False)
    graph, sd0, d = run(True)
    for it, ((e0, k0, g0), (e1, k1, g1)) in enumerate(zip(eager, graph)):
        assert relerr(e1, e0) <= 1e-5 and relerr(k1, k0) <= 1e-4, (setting, it, e0, e1, k0, k1)
        _assert_same_grads(g1, g0, (setting, it))
    if setting == 'std':
        cfg = dict(cfg, pixel_std1=0.5, pixel_std2=0.5)
        o64, g64 = _oracle(sd0, cfg, _noise(20), None, torch.float64)
        o32, g32 = _oracle(sd0, cfg, _noise(20), None, torch.float32)
        e1, _, g1 = graph[0]
        assert relerr(e1, o64[1]['err']) <= 2e-5
        bad = judge([('err', e1, o32[1]['err'], o64[1]['err'])], list(g1.items()), g32, g64, 'V2 std 0.5 after capture')
        assert not bad, bad
    assert d == (1, 1, 0), d          # after the undo: eager for _STABLE_ITERS iterations, then captured and replayed again


# ------------------------------------------------------------------------------------------------ C. outputs without a backward
NO_GRAD = {'log_s': lambda r: _sq(_stack(r[2].log_s_k)), 'colour': lambda r: _sq(r[3]['colour']),
           'seeds': lambda r: _sq(_stack(r[3]['seeds']))}


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('out', list(NO_GRAD))
def test_gradient_on_an_output_without_backward_raises(out, graph, autostep_on):
    cfg = _v2_cfg()
    model = _v2_model(cfg).to(DEV)
    autostep_on.GRAPH = graph
    xd = _input().to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    for it in range(WARM):
        _standard_iteration(model, opt, xd, 1 + it)
    opt.zero_grad()
    torch.manual_seed(MEASURED_SEED)
    r = model(xd)
    loss = _base_loss(r) + NO_GRAD[out](r)
    with pytest.raises(RuntimeError, match="'%s'" % out):
        loss.backward()
    # the loop goes on
    r = _standard_iteration(model, opt, xd, 9)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    _state_is_clean()
