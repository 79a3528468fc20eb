"""Opt-in bf16 products for the tap-conv kernels and the strip weight gradient (gx_tapconv_precision(3) /
genesis_amd.set_tapconv_precision('medium')): every operand rounded ONCE to bf16 (round to nearest even), one bf16 product per
fp32 product, fp32 accumulation.

Per layer the yardstick is fp64 arithmetic on the bf16-ROUNDED operands, judged element by element against S = sum |a * b| (the
same conv on |a| and |b|): what is left is fp32 accumulation, |mode 3 - ref| <= ACC_BAR * S.  Each call must also report mode 3
through gx_tapconv_last_mode() (the path that ran), and mode 0 of the same call must differ from it (the bf16 path really rounded)
while staying within 2^-8 * S of it (two roundings of 2^-9 per product).  Model level: the fp64 oracle against the same oracle with
every conv operand rounded to bf16, judged by tests/test_error_budget_gpu.py's rule (as tests/test_matmul_precision_gpu.py does for
'medium')."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ACC_BAR = 1e-5           # max over elements of |mode 3 - fp64(bf16 operands)| / S   (fp32 accumulation of <= 1600 products)
ACC_MEAN_BAR = 1e-6      # ... and its mean over elements
BF16_BAR = 2.0 ** -8 * (1 + 2.0 ** -9)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def bf(t):
    """fp64 copy of t rounded to bf16 (round to nearest even: torch's conversion)."""
    return t.float().to(torch.bfloat16).double()


def _L():
    from genesis_amd import _lib
    return _lib.load()


class tap_mode(object):
    """with tap_mode(m): gx_tapconv_precision(m), the previous mode restored afterwards (and the kq / Winograd dispatch set to
    `policy`: 0 sends every shape of the conv3x3 / transposed-conv / 5x5 entry points to the tap-conv kernels)."""

    def __init__(self, m, policy=None):
        self.m, self.policy = m, policy

    def __enter__(self):
        self.prev = int(_L().gx_tapconv_precision(self.m))
        assert self.prev >= 0
        if self.policy is not None:
            from genesis_amd import _lib
            _lib.call('gx_kq_policy', self.policy)
            _lib.call('gx_conv3x3_wino_policy', self.policy)

    def __exit__(self, *a):
        _L().gx_tapconv_precision(self.prev)
        if self.policy is not None:
            from genesis_amd import _lib
            _lib.call('gx_kq_policy', 1)
            _lib.call('gx_conv3x3_wino_policy', 1)


def run_modes(fn, policy=None):
    """{0: fn(), 3: fn()}, each asserting that the tap-conv / strip launches of fn ran in that mode."""
    out = {}
    for m in (3, 0):
        with tap_mode(m, policy):
            r = fn()
            torch.cuda.synchronize()
            assert int(_L().gx_tapconv_last_mode()) == m, ('the call did not reach the tap-conv kernels in mode %d' % m)
        out[m] = r
    return out


def judge(name, got, ref, S):
    g3, g0 = got[3].detach().double().cpu(), got[0].detach().double().cpu()
    S = S.detach().double().cpu()
    assert torch.isfinite(g3).all(), name
    r = (g3 - ref).abs() / S.clamp_min(1e-30)
    d = (g3 - g0).abs() / S.clamp_min(1e-30)
    print('%-48s mode 3 vs fp64(bf16 operands) / S: max %.2e mean %.2e;  mode 3 vs mode 0 / S: max %.2e'
          % (name, float(r.max()), float(r.mean()), float(d.max())))
    assert float(r.max()) <= ACC_BAR and float(r.mean()) <= ACC_MEAN_BAR, name
    assert not torch.equal(got[3], got[0]), name + ': mode 3 is bit-equal to mode 0 -- no bf16 rounding happened'
    assert float(d.max()) <= BF16_BAR, name


# ---------------------------------------------------------------- conv3x3 forward (+ bias + act) and data gradient
# MONet's recurrent attention UNet at B = 64 (the first two: its small levels, which the default dispatch sends to
# tapconv_kernel<M_C3>), a <= 32-output-channel layer, layers whose grid splits the channel reduction, odd H / W -- the others with
# the 16-bit-pipe kernels and Winograd switched off (policy 0), so every shape reaches the tap-conv kernels.
C3_SHAPES = [(64, 64, 64, 8, 8, None), (64, 128, 64, 4, 4, None), (64, 64, 64, 16, 16, 0), (64, 128, 32, 16, 16, 0),
             (64, 64, 32, 8, 8, 0), (2, 256, 64, 4, 4, 0), (1, 320, 96, 8, 8, 0), (3, 40, 24, 9, 12, 0), (2, 24, 70, 7, 20, 0)]


@pytest.mark.parametrize('N,Cin,Cout,H,W,policy', C3_SHAPES)
def test_conv3x3_in_tap_mode_3(N, Cin, Cout, H, W, policy):
    from genesis_amd import hip_ops as hip
    x, w, b = rnd(N, Cin, H, W, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=1.0 / np.sqrt(9 * Cin)), rnd(Cout, seed=3, scale=0.3)
    dy = rnd(N, Cout, H, W, seed=4)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    ref = F.conv2d(bf(x), bf(w), None, padding=1)
    S = F.conv2d(bf(x).abs(), bf(w).abs(), None, padding=1)
    judge('conv3x3 fwd N=%d %d->%d %dx%d' % (N, Cin, Cout, H, W), run_modes(lambda: hip.conv3x3_fwd(xd, wd), policy), ref, S)
    for act in ('relu', 'elu'):
        refa = ref + b.double().view(1, -1, 1, 1)
        refa = F.relu(refa) if act == 'relu' else F.elu(refa)
        got = run_modes(lambda: hip.conv3x3_bias_act_fwd(xd, wd, bd, act), policy)
        # (the activation is 1-Lipschitz: the bound on its argument holds for its value; S includes the bias)
        judge('conv3x3 bias+%s fwd N=%d %d->%d %dx%d' % (act, N, Cin, Cout, H, W), got, refa, S + b.double().abs().view(1, -1, 1, 1))
    dref = F.conv_transpose2d(bf(dy), bf(w), None, padding=1)
    dS = F.conv_transpose2d(bf(dy).abs(), bf(w).abs(), None, padding=1)
    judge('conv3x3 dgrad N=%d %d->%d %dx%d' % (N, Cin, Cout, H, W), run_modes(lambda: hip.conv3x3_dgrad(dyd, wd), policy), dref, dS)


def test_conv3x3_dgrad_act_is_not_a_tap_conv_entry():
    """gx_conv3x3_dgrad_act runs on the 16-bit pipe only (gx_kq.hip's kq_c3h, gx_matmul_precision's switch): it launches no tap-conv
    kernel, so the tap-conv mode leaves its result and gx_tapconv_last_mode() untouched."""
    from genesis_amd import hip_ops as hip, _lib
    N, Cin, Cout, H, W = 16, 32, 32, 72, 72
    dy, w = rnd(N, Cout, H, W, seed=5).to(DEV), rnd(Cout, Cin, 3, 3, seed=6, scale=0.1).to(DEV)
    xout = torch.relu(rnd(N, Cin, H, W, seed=7)).to(DEV)
    res = {}
    for m in (0, 3, 0):
        with tap_mode(m):
            hip.conv3x3_fwd(rnd(2, 8, 4, 4, seed=8).to(DEV), rnd(8, 8, 3, 3, seed=9).to(DEV))     # a tap-conv launch: last mode = m
            torch.cuda.synchronize()
            assert int(_L().gx_tapconv_last_mode()) == m
            _lib.call('gx_kq_policy', 2)             # every eligible shape (the default asks for a chip-filling grid)
            try:
                assert hip.conv3x3_dgrad_act_supported(N, Cin, Cout, H, W)
                r = hip.conv3x3_dgrad_act(dy, w, xout, 'relu')
            finally:
                _lib.call('gx_kq_policy', 1)
            r = r[0] if isinstance(r, tuple) else r
            torch.cuda.synchronize()
            assert int(_L().gx_tapconv_last_mode()) == m
        if m in res:
            assert torch.equal(res[m], r)
        res[m] = r.clone()
    assert torch.equal(res[0], res[3])


# ---------------------------------------------------------------- the transposed conv (k5 s2): forward, with GroupNorm statistics, data gradient
DT_SHAPES = [(64, 64, 64, 4, 4, 0), (64, 64, 32, 8, 8, 0), (64, 32, 64, 8, 8, 0), (2, 128, 64, 4, 4, 0), (3, 24, 40, 7, 4, 0),
             (8, 64, 64, 16, 16, 0)]


@pytest.mark.parametrize('N,Cin,Cout,Hin,Win,policy', DT_SHAPES)
def test_transposed_conv_in_tap_mode_3(N, Cin, Cout, Hin, Win, policy):
    from genesis_amd import hip_ops as hip
    x, w, b = rnd(N, Cin, Hin, Win, seed=11), rnd(Cin, Cout, 5, 5, seed=12, scale=0.05), rnd(Cout, seed=13, scale=0.3)
    dy = rnd(N, Cout, 2 * Hin, 2 * Win, seed=14)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    ref = F.conv_transpose2d(bf(x), bf(w), b.double(), 2, 2, 1)
    S = F.conv_transpose2d(bf(x).abs(), bf(w).abs(), b.double().abs(), 2, 2, 1)
    tag = 'N=%d %d->%d %dx%d' % (N, Cin, Cout, Hin, Win)
    judge('deconv fwd ' + tag, run_modes(lambda: hip.deconv5x5s2_fwd(xd, wd, bd), policy), ref, S)
    if Cout % 8 == 0 and Hin & (Hin - 1) == 0 and Win & (Win - 1) == 0:      # (gx_deconv5x5s2_gn_stats_fwd's shapes)
        groups = Cout // 8
        gamma, beta = torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)
        got = run_modes(lambda: hip.deconv5x5s2_gn_stats_fwd(xd, wd, bd, gamma, beta, groups, 1e-5), policy)
        judge('deconv+gn stats fwd ' + tag, {m: got[m][0] for m in got}, ref, S)
        for m in (0, 3):       # the statistics belong to the output this mode computed
            y = got[m][0].double().view(N, groups, -1)
            assert torch.allclose(got[m][1].double().view(N, groups), y.mean(2), rtol=1e-4, atol=1e-5), m
    dref = F.conv2d(bf(dy), bf(w), None, 2, 2)
    dS = F.conv2d(bf(dy).abs(), bf(w).abs(), None, 2, 2)
    judge('deconv dgrad ' + tag, run_modes(lambda: hip.deconv5x5s2_dgrad(dyd, wd), policy), dref, dS)


# ---------------------------------------------------------------- the stride-1 5x5 conv (the gated stacks)
@pytest.mark.parametrize('N,K,M,S', [(16, 32, 64, 16), (32, 64, 32, 8), (3, 48, 40, 12), (2, 64, 64, 4)])
def test_conv5x5_stride1_in_tap_mode_3(N, K, M, S):
    from genesis_amd import hip_ops as hip
    x, w0, w1 = rnd(N, K, S, S, seed=21), rnd(M, K, 5, 5, seed=22, scale=0.1), rnd(K, M, 5, 5, seed=23, scale=0.1)
    xd, w0d, w1d = x.to(DEV), w0.to(DEV), w1.to(DEV)
    if not hip.conv5x5s1_supported(N, K, M, S, S):
        pytest.skip('gx_conv5x5s1 does not take %s' % ((N, K, M, S),))
    tag = 'N=%d %d->%d @%d' % (N, K, M, S)
    judge('conv5x5 ' + tag, run_modes(lambda: hip.conv5x5s1(xd, w0d, M, False), 0),
          F.conv2d(bf(x), bf(w0), None, 1, 2), F.conv2d(bf(x).abs(), bf(w0).abs(), None, 1, 2))
    judge('conv5x5 flipped ' + tag, run_modes(lambda: hip.conv5x5s1(xd, w1d, M, True), 0),
          F.conv_transpose2d(bf(x), bf(w1), None, 1, 2), F.conv_transpose2d(bf(x).abs(), bf(w1).abs(), None, 1, 2))


# ---------------------------------------------------------------- the strip weight gradient (gx_wstrip.hip: the 72 x 72 canvas)
@pytest.mark.parametrize('N,H,W', [(32, 72, 72), (8, 40, 24)])
def test_strip_weight_gradient_in_tap_mode_3(N, H, W):
    from genesis_amd import hip_ops as hip
    C = 32
    x, dy = rnd(N, C, H, W, seed=31), rnd(N, C, H, W, seed=32)
    xd, dyd = x.to(DEV), dy.to(DEV)
    wz = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(bf(x), wz, None, 1, 1) * bf(dy)).sum().backward()
    ref = wz.grad.clone()
    wz.grad = None
    (F.conv2d(bf(x).abs(), wz, None, 1, 1) * bf(dy).abs()).sum().backward()
    S = wz.grad
    db = {}

    def run():
        db_ = torch.empty(C, device=DEV)
        r = hip.conv3x3_wgrad_quad(xd, dyd, dbias_out=db_)
        db[int(_L().gx_tapconv_precision_get())] = db_
        return r
    got = run_modes(run)
    judge('strip wgrad N=%d %dx%d' % (N, H, W), got, ref, S)
    assert torch.equal(db[0], db[3])          # the bias gradient is a sum of dy: no product, the same bits in both modes


# ---------------------------------------------------------------- switching
def test_mode_0_after_a_round_trip_through_mode_3_is_bit_identical():
    from genesis_amd import hip_ops as hip
    x, w, b = rnd(64, 64, 8, 8, seed=41).to(DEV), rnd(64, 64, 3, 3, seed=42, scale=0.05).to(DEV), rnd(64, seed=43).to(DEV)
    xt, wt = rnd(64, 64, 8, 8, seed=44).to(DEV), rnd(64, 32, 5, 5, seed=45, scale=0.05).to(DEV)
    xs, dys = rnd(8, 32, 72, 72, seed=46).to(DEV), rnd(8, 32, 72, 72, seed=47).to(DEV)

    def calls():
        return [hip.conv3x3_bias_act_fwd(x, w, b, 'relu'), hip.conv3x3_dgrad(x, w), hip.deconv5x5s2_fwd(xt, wt, b[:32]),
                hip.deconv5x5s2_dgrad(hip.deconv5x5s2_fwd(xt, wt, b[:32]), wt), hip.conv3x3_wgrad_quad(xs, dys)]
    with tap_mode(0, 0):
        before = [t.clone() for t in calls()]
    with tap_mode(3, 0):
        mid = calls()
    with tap_mode(0, 0):
        after = calls()
    for i, (p, q, r) in enumerate(zip(before, mid, after)):
        assert torch.equal(p, r), i
        assert not torch.equal(p, q), i


def _v2_tiny():
    from tests.test_matmul_precision_gpu import _v2_tiny as tiny
    return tiny()


def test_a_tap_mode_change_between_forward_and_backward_raises():
    import genesis_amd
    from genesis_amd import testing as T
    model = _v2_tiny()
    x = T.make_input(5, 4, 32).to(DEV)
    with tap_mode(0):
        recon, losses, _, _, _ = model(x)
        genesis_amd.set_tapconv_precision('medium')
        with pytest.raises(RuntimeError, match='between a forward'):      # (GenesisHipError, through the autograd engine)
            losses.err.mean().backward()
        genesis_amd.set_tapconv_precision('default')       # back at the forward's mode: the same graph runs
        recon, losses, _, _, _ = model(x)
        losses.err.mean().backward()


def test_unchanged_loop_graphs_are_keyed_by_the_tap_mode():
    import genesis_amd
    from genesis_amd import autostep
    from genesis_amd import testing as T
    model = _v2_tiny()
    opt = torch.optim.Adam(model.parameters(), 1e-4)
    x = T.make_input(6, 8, 32).to(DEV)
    keys = []
    with tap_mode(0):
        for m in ('default', 'medium', 'default'):
            genesis_amd.set_tapconv_precision(m)
            keys.append(autostep._graph_key(model, x))
            for _ in range(4):
                opt.zero_grad()
                recon, losses, _, _, _ = model(x)
                loss = losses.err.mean() + torch.stack(list(losses.kl_l_k), 1).mean(0).sum()
                loss.backward()
                opt.step()
                assert torch.isfinite(loss.detach()).all()
    assert keys[0] != keys[1] and keys[0][:-1] == keys[1][:-1] and keys[0] == keys[2]
    assert keys[0][-1][1] == 0 and keys[1][-1][1] == 3


def _full(case):
    from tests.test_fullbatch_gpu import Full
    return Full(case)


def test_trainstep_round_trip_default_tap_medium_default():
    """GENESIS-V2 (metric configuration; its step is a function of the restored state -- MONet's draws from the generator),
    TrainStep(graph=True): default, two steps in tap 'medium', default again -- all in one TrainStep.  After each switch the next
    step() re-captures: its output and parameters equal an eager step in the new mode from the same state, bit for bit; after the
    round trip a step in the default is bit-identical to one before any switch."""
    import genesis_amd
    from genesis_amd.trainer import TrainStep
    from tests.test_matmul_precision_gpu import _snap, _restore, _eager_step
    gold = _full('v2_metric_b32')
    x = gold.x().to(DEV)
    with tap_mode(0):
        torch.manual_seed(0)
        ts = TrainStep(gold.build(), gold.S, graph=True)
        s0 = _snap(ts)
        before = ts.step(x).clone()
        p_before = ts.flat_p.clone()
        _restore(ts, s0)
        ts.step(x)                                    # captured in the default
        for i, m in enumerate(['medium', 'medium', 'default']):
            genesis_amd.set_tapconv_precision(m)
            s = _snap(ts)
            g_out = ts.step(x).clone()
            g_p = ts.flat_p.clone()
            assert torch.isfinite(g_out).all()
            if i != 1:                                # (the steps right after a switch)
                _restore(ts, s)
                e_out = _eager_step(ts, x).clone()
                assert torch.equal(g_out, e_out), (m, g_out, e_out)
                assert torch.equal(g_p, ts.flat_p), m
        _restore(ts, s0)
        after = ts.step(x).clone()
        assert torch.equal(before, after), (before, after)
        assert torch.equal(p_before, ts.flat_p)
        ts.close()


# ---------------------------------------------------------------- model level
@pytest.mark.parametrize('case', ['monet_cfg4_b32', 'genesis_cfg3_b32', 'v2_metric_b32'])
def test_model_in_medium_plus_tap_medium_within_the_bf16_error_budget(case):
    """'medium' and tap-conv 'medium' together, at B = 32: the HIP forward and gradients against the fp64 oracle, with the fp64
    oracle on bf16-rounded conv operands as the yardstick (tests/test_error_budget_gpu.py's rule, as in
    tests/test_matmul_precision_gpu.py::test_model_in_medium_within_the_bf16_error_budget)."""
    import genesis_amd
    from genesis_amd import _lib
    from tests.test_error_budget_gpu import judge as budget, to_dtype, grads_of, hip_grads
    from tests.test_matmul_precision_gpu import _rounded_convs
    gold = _full(case)
    model = gold.build()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x = gold.x()
    nz = gold.noise()
    fam, cfg = gold.fam, gold.cfg

    def oracle(rounded, seed_idx=None):
        p = to_dtype(sd, torch.float64)
        r2, rt, c2, ct = _rounded_convs()
        if rounded:
            F.conv2d, F.conv_transpose2d = r2, rt
        try:
            if fam == 'v2':
                from oracle import v2_oracle as O
                out = O.v2_forward(p, x.double(), cfg, nz[0].double(), [e.double() for e in nz[1:]], seed_idx=seed_idx,
                                   reference_form=False)
            elif fam == 'monet':
                from oracle import monet_oracle as O
                out = O.monet_forward(p, x.double(), cfg, nz[0].double())
            else:
                from oracle import genesis_oracle as O
                out = O.genesis_forward(p, x.double(), cfg, [e.double() for e in nz[:gold.K]], nz[gold.K].double())
            e, kl = gold.aggregate(out[1])
            (e + kl).backward()
        finally:
            F.conv2d, F.conv_transpose2d = c2, ct
        return out, grads_of(p)
    o64, g64 = oracle(False)
    seeds = list(torch.stack(o64[3]['seed_idx']).unbind(0)) if fam == 'v2' else None
    ob, gb = oracle(True, seeds)
    with tap_mode(3):
        try:
            genesis_amd.set_matmul_precision('medium')
            if fam == 'v2':
                out = model(x.to(DEV), nz[0].to(DEV), torch.stack(nz[1:]).to(DEV), torch.stack(seeds).to(DEV))
            else:
                out = gold.forward(model, x, nz)
            e, kl = gold.aggregate(out[1])
            (e + kl).backward()
        finally:
            _lib.load().gx_matmul_precision(-1)
    s = lambda l: torch.stack(list(l))   # noqa: E731
    fwd = [('recon', out[0], ob[0], o64[0]), ('err', out[1]['err'], ob[1]['err'], o64[1]['err']),
           ('log_m', s(out[2]['log_m_k']), s(ob[2]['log_m_k']), s(o64[2]['log_m_k']))]
    bad = budget(fwd, hip_grads(model), gb, g64, '%s medium + tap medium (column 2: fp64 with bf16 conv operands)' % case)
    assert not bad, bad


# ---------------------------------------------------------------- training
ELBO_GAP_BAR = 4e-4      # relative |ELBO(both medium) - ELBO(default)| per step over 50 steps: 2.2 x the measured maximum (1.78e-4)


@pytest.mark.parametrize('case', ['monet_cfg4_b32'])
def test_fifty_training_steps_with_both_switches_track_the_default(case):
    import genesis_amd
    from genesis_amd import _lib
    from genesis_amd.trainer import TrainStep
    gold = _full(case)
    x = gold.x().to(DEV)
    elbo = {}
    try:
        for on in (False, True):
            genesis_amd.set_matmul_precision('medium' if on else 'high')
            genesis_amd.set_tapconv_precision('medium' if on else 'default')
            torch.manual_seed(0)
            ts = TrainStep(gold.build(), gold.S, graph=True)
            elbo[on] = torch.stack([ts.step(x)[0].clone() for _ in range(50)]).double().cpu()
            ts.close()
    finally:
        _lib.load().gx_matmul_precision(-1)
        _L().gx_tapconv_precision(-1)
    assert torch.isfinite(elbo[False]).all() and torch.isfinite(elbo[True]).all()
    gap = (elbo[True] - elbo[False]).abs() / elbo[False].abs()
    print('%s: relative ELBO gap (medium + tap medium) vs default over 50 steps: max %.3e (step %d), mean %.3e; bar %.1e'
          % (case, float(gap.max()), int(gap.argmax()), float(gap.mean()), ELBO_GAP_BAR))
    assert float(gap.max()) <= ELBO_GAP_BAR
