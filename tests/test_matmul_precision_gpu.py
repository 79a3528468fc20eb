"""Opt-in bf16 matmul precision (gx_matmul_precision / genesis_amd.set_matmul_precision, 'medium' = mode 3 of the three 16-bit-pipe
conv families): every operand of those layers rounded ONCE to bf16 (round to nearest even), one bf16 product per fp32 product,
fp32 accumulation.

Per family the yardstick is fp64 arithmetic on the bf16-ROUNDED operands: what is left is the fp32 accumulation (and, for
Winograd, the fp32 output transform) -- bar 2e-5 relative L2 per tensor, 1e-4 per output channel.  The same results must differ
from mode 2 (fp32-equivalent pieces) by more than 1e-4 relative in some output channel: together the two prove that the
one-piece path ran and that it rounded the right operands to nearest even (a truncation, or a rounding of a third operand, is
off the yardstick by ~1e-3).  A layer that runs on the fp32 pipe in the default (mode 2 bit-equal to mode 0: channel counts the
16-bit kernels do not take) must stay there in mode 3, bit for bit: mode 3 covers exactly the default's 16-bit-pipe layers.
Model level: the fp64 oracle against the same oracle with every conv operand rounded to bf16 (F.conv2d / conv_transpose2d
wrapped here; oracle/ untouched), judged by tests/test_error_budget_gpu.py's rule."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TENSOR_BAR, CHANNEL_BAR, DIFF_MIN = 2e-5, 1e-4, 1e-4


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def bf(t):
    """fp64 copy of t rounded to bf16 (round to nearest even: torch's conversion)."""
    return t.float().to(torch.bfloat16).double()


def rel(a, ref):
    ref = ref.detach().double().cpu()
    return float((a.detach().double().cpu() - ref).norm()) / float(ref.norm())


def per_channel(a, ref, dim):
    """Largest per-channel relative L2 error along `dim`."""
    a, ref = a.detach().double().cpu().movedim(dim, 0), ref.detach().double().cpu().movedim(dim, 0)
    e = (a - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1).clamp_min(1e-300)
    return float(e.max())


def check(name, got, ref, dim, k=None):
    """got: {mode: result} (modes 0, 2, 3), k: index into tuple results."""
    pick = (lambda m: got[m]) if k is None else (lambda m: got[m][k])  # noqa: E731
    got3, got2, got0 = pick(3), pick(2), pick(0)
    assert torch.isfinite(got3).all(), name
    if torch.equal(got2, got0):
        print('%-40s on the fp32 pipe in the default: mode 3 bit-equal to it: %s' % (name, torch.equal(got3, got0)))
        assert torch.equal(got3, got0), name
        return
    e, ec, d = rel(got3, ref), per_channel(got3, ref, dim), per_channel(got3, got2, dim)
    print('%-40s mode 3 vs fp64(bf16 operands): %.2e (worst channel %.2e); mode 3 vs mode 2 (largest channel): %.2e' % (name, e, ec, d))
    assert e <= TENSOR_BAR and ec <= CHANNEL_BAR, (name, e, ec)
    assert d > DIFF_MIN, (name, d)


def modes(family, fn):
    """{0: fn(), 2: fn(), 3: fn()} with gx_<family>_precision set, the default restored afterwards."""
    from genesis_amd import _lib
    out = {}
    try:
        for m in (0, 2, 3):
            _lib.call('gx_%s_precision' % family, m)
            out[m] = fn()
    finally:
        _lib.call('gx_%s_precision' % family, -1)
    return out


def stress(kind, shape, seed):
    """The hard operand sets of tests/test_kernels_gpu.py: relu_like (x >= 0 with half of it zero / heavy-tailed), one_outlier
    (one element 2^20 times the rest), big / small (scaled by 2^30 / 2^-30)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(*shape, generator=g) * 2 - 1
    if kind == 'relu_like':
        return torch.relu(t) if seed % 2 else t ** 3
    if kind == 'one_outlier':
        t.view(-1)[t.numel() // 3] = 2.0 ** 20
        return t
    return t * (2.0 ** 30 if kind == 'big' else 2.0 ** -30)


# ---------------------------------------------------------------- gx_wgq.hip: weight gradients (stream-K launch)
def _wgrad_case(kind, x, dy):
    from genesis_amd import hip_ops as hip
    if kind == 'conv3x3':
        w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
        (F.conv2d(bf(x), w, None, 1, 1) * bf(dy)).sum().backward()
        run = lambda: hip.conv3x3_wgrad(x.to(DEV), dy.to(DEV))  # noqa: E731
    else:
        w = torch.zeros(x.shape[1], dy.shape[1], 5, 5, dtype=torch.float64, requires_grad=True)
        (F.conv_transpose2d(bf(x), w, None, 2, 2, 1) * bf(dy)).sum().backward()
        run = lambda: hip.deconv5x5s2_wgrad(x.to(DEV), dy.to(DEV))  # noqa: E731
    return w.grad, modes('wgq', run)


@pytest.mark.parametrize('kind,N,Cin,Cout,S', [('conv3x3', 32, 64, 64, 64), ('conv3x3', 8, 128, 64, 32), ('conv3x3', 4, 40, 72, 16),
                                                ('deconv', 56, 64, 64, 32), ('deconv', 16, 64, 64, 16), ('deconv', 9, 24, 40, 8)])
def test_weight_gradients_in_mode_3_are_fp32_sums_of_bf16_products(kind, N, Cin, Cout, S):
    """Row-ring tiles (64 / 32 / 16-pixel rows) and the LDS-DMA tiles (8-pixel rows) of the stream-K launch: the shapes of
    tests/test_kernels_gpu.py::test_weight_gradients_on_the_bf16_pipe_keep_fp32_accuracy."""
    s = 2 if kind == 'deconv' else 1
    x, dy = rnd(N, Cin, S, S, seed=1), rnd(N, Cout, s * S, s * S, seed=2)
    ref, got = _wgrad_case(kind, x, dy)
    check('%s wgrad N=%d %d->%d @%d' % (kind, N, Cin, Cout, S), got, ref, 0)


@pytest.mark.parametrize('case', ['relu_like', 'one_outlier', 'big', 'small'])
def test_weight_gradients_in_mode_3_on_hard_operands_need_no_scale(case):
    """No amax hint is armed (gx_wgq_operand_amax): mode 3 needs none -- bf16 has fp32's exponent range."""
    x, dy = stress(case, (32, 64, 64, 64), 1), stress(case if case != 'one_outlier' else 'relu_like', (32, 64, 64, 64), 2)
    if case == 'one_outlier':
        dy = stress('one_outlier', (32, 64, 64, 64), 2)
    ref, got = _wgrad_case('conv3x3', x, dy)
    check('conv3x3 wgrad, %s operands' % case, got, ref, 0)


# ---------------------------------------------------------------- gx_kq.hip: transposed conv, conv3x3 <= 32 channels, conv5x5
def _deconv_case(x, w, b, dy):
    from genesis_amd import hip_ops as hip
    xr = bf(x).requires_grad_()
    ref = F.conv_transpose2d(xr, bf(w), b.double(), 2, 2, 1)
    ref.backward(bf(dy))
    got = modes('kq', lambda: (hip.deconv5x5s2_fwd(x.to(DEV), w.to(DEV), b.to(DEV)), hip.deconv5x5s2_dgrad(dy.to(DEV), w.to(DEV))))
    return ref.detach(), xr.grad, got


@pytest.mark.parametrize('N,Cin,Cout,Hin', [(56, 64, 64, 32), (70, 64, 64, 32), (224, 64, 64, 16), (60, 32, 64, 32),
                                            (56, 64, 40, 32), (52, 48, 72, 32), (13, 64, 64, 64), (16, 32, 64, 64)])
def test_transposed_conv_in_mode_3(N, Cin, Cout, Hin):
    """Q_DT0H / Q_DT1H (forward) and Q_DGH (data gradient) with one input plane and one-piece weight taps: the shapes of
    tests/test_kernels_gpu.py::test_transposed_conv_on_the_bf16_pipe_keeps_fp32_accuracy."""
    x, w, b = rnd(N, Cin, Hin, Hin, seed=71), rnd(Cin, Cout, 5, 5, seed=72, scale=0.05), rnd(Cout, seed=73, scale=0.3)
    dy = rnd(N, Cout, 2 * Hin, 2 * Hin, seed=76)
    ref, dref, got = _deconv_case(x, w, b, dy)
    check('deconv fwd N=%d %d->%d @%d' % (N, Cin, Cout, Hin), got, ref, 1, 0)
    check('deconv dgrad N=%d %d->%d @%d' % (N, Cin, Cout, Hin), got, dref, 1, 1)


@pytest.mark.parametrize('case', ['relu_like', 'one_outlier', 'big', 'small'])
def test_transposed_conv_in_mode_3_on_hard_operands_need_no_scale(case):
    x, w = stress(case, (56, 64, 32, 32), 3), rnd(64, 64, 5, 5, seed=72, scale=0.05)
    dy = stress(case, (56, 64, 64, 64), 4)
    ref, dref, got = _deconv_case(x, w, torch.zeros(64), dy)
    check('deconv fwd, %s operands' % case, got, ref, 1, 0)
    check('deconv dgrad, %s operands' % case, got, dref, 1, 1)


@pytest.mark.parametrize('N,Cin,Cout,H,W', [(16, 32, 32, 72, 72), (5, 16, 24, 40, 24), (4, 32, 7, 16, 16), (9, 48, 32, 8, 64)])
def test_conv3x3_to_32_channels_in_mode_3(N, Cin, Cout, H, W):
    """Q_C3H (kq_c3h: the BroadcastDecoder's canvas convs of MONet / GENESIS), forward (+ bias + ELU) and data gradient."""
    from genesis_amd import hip_ops as hip, _lib
    x, w, b = rnd(N, Cin, H, W, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=1.0 / np.sqrt(9 * Cin)), rnd(Cout, seed=3)
    dy = rnd(N, Cout, H, W, seed=4)
    ref = F.elu(F.conv2d(bf(x), bf(w), b.double(), padding=1))
    dref = F.conv_transpose2d(bf(dy), bf(w), None, padding=1)
    _lib.call('gx_kq_policy', 2)                  # every eligible shape (the default asks for a chip-filling grid)
    try:
        got = modes('kq', lambda: (hip.conv3x3_bias_act_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 'elu'),
                                   hip.conv3x3_dgrad(dy.to(DEV), w.to(DEV))))
    finally:
        _lib.call('gx_kq_policy', 1)
    check('conv3x3 -> %d fwd %dx%d' % (Cout, H, W), got, ref, 1, 0)
    check('conv3x3 -> %d dgrad %dx%d' % (Cout, H, W), got, dref, 1, 1)


@pytest.mark.parametrize('N,K,M,S', [(16, 32, 64, 64), (52, 64, 128, 32), (200, 64, 64, 16), (13, 48, 64, 64)])
def test_conv5x5_stride1_in_mode_3(N, K, M, S):
    """Q_C5H (kq_c5h: the gated stacks of MONet / GENESIS), both weight roles."""
    from genesis_amd import hip_ops as hip
    x, w0, w1 = rnd(N, K, S, S, seed=1), rnd(M, K, 5, 5, seed=2, scale=0.1), rnd(K, M, 5, 5, seed=3, scale=0.1)
    r0, r1 = F.conv2d(bf(x), bf(w0), None, 1, 2), F.conv_transpose2d(bf(x), bf(w1), None, 1, 2)
    got = modes('kq', lambda: (hip.conv5x5s1(x.to(DEV), w0.to(DEV), M, False), hip.conv5x5s1(x.to(DEV), w1.to(DEV), M, True)))
    check('conv5x5 N=%d %d->%d @%d' % (N, K, M, S), got, r0, 1, 0)
    check('conv5x5 flipped N=%d %d->%d @%d' % (N, K, M, S), got, r1, 1, 1)


# ---------------------------------------------------------------- gx_wino.hip: Winograd F(2x2, 3x3)
AT = torch.tensor([[1., 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def _g_rows(g, dim):
    """G applied along `dim` (3 -> 4), in fp32 in the kernel's order: g0 | 0.5 ((g0 + g1) + g2) | 0.5 ((g0 - g1) + g2) | g2."""
    g0, g1, g2 = g.unbind(dim)
    return torch.stack((g0, 0.5 * ((g0 + g1) + g2), 0.5 * ((g0 - g1) + g2), g2), dim)


def _bt_rows(d, dim):
    """B^T applied along `dim` (4 -> 4), in fp32: d0 - d2 | d1 + d2 | d2 - d1 | d1 - d3."""
    d0, d1, d2, d3 = d.unbind(dim)
    return torch.stack((d0 - d2, d1 + d2, d2 - d1, d1 - d3), dim)


def wino_ref(x, w):
    """conv3x3 (pad 1) by F(2x2, 3x3): U = G g G^T and V = B^T d B rounded to bf16 in the Winograd domain, everything after that
    in fp64.  The transforms themselves are formed in fp32 in the order the kernel forms them (wino_pack_h_kernel: U, rows then
    columns; wino_conv_h_kernel: V in registers, rows then columns): the kernel's operands are fp32 values rounded once to bf16,
    and an fp64 transform rounded instead differs from them wherever the fp32 value lies next to a bf16 tie (~2^-16 of the
    values) -- one such U value moves a whole output channel by ~1e-4 and would measure the yardstick, not the kernel."""
    N, K, H, W = x.shape
    U = bf(_g_rows(_g_rows(w.float(), 2), 3))                                  # [M, K, 4, 4]
    xp = F.pad(x.float(), (1, 1, 1, 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                     # [N, K, H/2, W/2, 4 rows, 4 cols]
    V = bf(_bt_rows(_bt_rows(d, 4), 5))
    Mt = torch.einsum('mkab,nkijab->nmijab', U, V)
    Y = AT @ Mt @ AT.t()                                                       # [N, M, H/2, W/2, 2, 2]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(N, w.shape[0], H, W)


@pytest.mark.parametrize('N,Cin,Cout,H,W', [(2, 16, 16, 8, 16), (3, 24, 40, 32, 32), (2, 64, 64, 64, 64),
                                            (1, 128, 72, 16, 48), (2, 70, 130, 24, 32)])
def test_conv3x3_winograd_in_mode_3(N, Cin, Cout, H, W):
    """wino_conv_h_kernel with U packed as one bf16 plane (wino_pack_h_kernel) and V rounded in registers: forward and data
    gradient (the flipped, transposed weights) -- the shapes of tests/test_kernels_gpu.py::test_conv3x3_winograd."""
    from genesis_amd import hip_ops as hip
    x, w, dy = rnd(N, Cin, H, W, seed=61), rnd(Cout, Cin, 3, 3, seed=62, scale=0.1), rnd(N, Cout, H, W, seed=63)
    got = modes('wino', lambda: (hip.conv3x3_wino(x.to(DEV), w.to(DEV), 0), hip.conv3x3_wino(dy.to(DEV), w.to(DEV), 1)))
    check('winograd fwd %d->%d %dx%d' % (Cin, Cout, H, W), got, wino_ref(x, w), 1, 0)
    check('winograd dgrad %d->%d %dx%d' % (Cin, Cout, H, W), got, wino_ref(dy, w.flip(2, 3).transpose(0, 1)), 1, 1)


@pytest.mark.parametrize('case', ['relu_like', 'one_outlier', 'big', 'small'])
def test_conv3x3_winograd_in_mode_3_on_hard_operands_with_a_hint_armed(case):
    """An armed gx_conv_input_amax hint (what the norm kernels hand the next conv) is ignored in mode 3 -- and cleared."""
    from genesis_amd import hip_ops as hip, _lib
    x, w = stress(case, (2, 64, 64, 64), 5), rnd(64, 64, 3, 3, seed=62, scale=0.1)
    parts = torch.full((16,), float(x.abs().max()) / 1e6, device=DEV)       # a deliberately WRONG maximum: must not be read
    xd = x.to(DEV)

    def run():
        _lib.call('gx_conv_input_amax', parts.data_ptr(), 16, None, 0)
        return hip.conv3x3_wino(xd, w.to(DEV), 0)
    from genesis_amd import _lib as L
    got = {}
    try:
        L.call('gx_wino_precision', 3)
        got[3] = run()
        _lib.call('gx_conv_input_amax', None, 0, None, 0)
        for m in (0, 2):
            L.call('gx_wino_precision', m)
            got[m] = hip.conv3x3_wino(xd, w.to(DEV), 0)
    finally:
        L.call('gx_wino_precision', -1)
        _lib.call('gx_conv_input_amax', None, 0, None, 0)
    check('winograd fwd, %s operands, hint armed' % case, got, wino_ref(x, w), 1)


# ---------------------------------------------------------------- API, switching
def test_api_default_set_get_and_invalid_level():
    import genesis_amd
    from genesis_amd import _lib
    out = subprocess.run([sys.executable, '-c', 'import genesis_amd; print(genesis_amd.get_matmul_precision())'], cwd=ROOT,
                         env={k: v for k, v in os.environ.items() if not k.startswith('GENESIS_')}, capture_output=True, text=True)
    assert out.stdout.strip().splitlines()[-1] == 'high', out
    try:
        for lv in ('highest', 'medium', 'high', 'medium'):
            genesis_amd.set_matmul_precision(lv)
            assert genesis_amd.get_matmul_precision() == lv
        with pytest.raises(ValueError):
            genesis_amd.set_matmul_precision('low')
        assert genesis_amd.get_matmul_precision() == 'medium'
        _lib.call('gx_wgq_precision', 1)                # one family by hand: no common level
        assert genesis_amd.get_matmul_precision() is None
        assert _lib.load().gx_matmul_precision(7) < 0
    finally:
        _lib.load().gx_matmul_precision(-1)
    assert genesis_amd.get_matmul_precision() == 'high'


def test_environment_variable_decides_a_fresh_process(tmp_path):
    """GENESIS_MATMUL_PRECISION in a fresh child process: the level it names, ahead of the per-family variables (set here to the
    fp32 pipe / six bf16 pieces: the level wins), and the transposed conv computes at that level."""
    code = ('import torch, genesis_amd; from genesis_amd import hip_ops as hip\n'
            'g = torch.Generator().manual_seed(1)\n'
            'x = torch.rand(56, 64, 32, 32, generator=g).cuda(); w = (torch.rand(64, 64, 5, 5, generator=g) * 0.05).cuda()\n'
            'y = hip.deconv5x5s2_fwd(x, w, torch.zeros(64, device="cuda"))\n'
            'torch.save(y.cpu(), %r)\nprint(genesis_amd.get_matmul_precision())')
    res = {}
    for lv in ('highest', 'high', 'medium'):
        path = str(tmp_path / ('y_%s.pt' % lv))
        env = dict(os.environ, GENESIS_MATMUL_PRECISION=lv, GENESIS_KQ_F16X3='0', GENESIS_KQ_BF16X6='0')
        out = subprocess.run([sys.executable, '-c', code % path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip().splitlines()[-1] == lv
        res[lv] = torch.load(path)
    assert not torch.equal(res['medium'], res['high']) and not torch.equal(res['high'], res['highest'])
    d_med, d_high = rel(res['medium'], res['highest']), rel(res['high'], res['highest'])
    print('fresh process: high vs highest %.2e, medium vs highest %.2e' % (d_high, d_med))
    assert d_high < 2e-6 and 1e-4 < d_med < 2e-2


def _v2_tiny():
    from oracle import v2_oracle as O
    import genesis_amd.genesisv2_config as G
    from genesis_amd.compat.attrdict import AttrDict
    cfg = O.make_cfg(K_steps=3, img_size=32, feat_dim=16)     # (small layers: what matters here is the autograd / graph bookkeeping)
    torch.manual_seed(3)
    return G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False))).to(DEV).train()


def test_a_level_change_between_forward_and_backward_raises():
    import genesis_amd
    from genesis_amd import _lib, testing as T
    model = _v2_tiny()
    x = T.make_input(5, 4, 32).to(DEV)
    try:
        genesis_amd.set_matmul_precision('high')
        recon, losses, _, _, _ = model(x)
        genesis_amd.set_matmul_precision('medium')
        with pytest.raises(RuntimeError, match='between a forward'):      # (GenesisHipError, through the autograd engine)
            losses.err.mean().backward()
        genesis_amd.set_matmul_precision('high')      # back at the forward's level: the same graph runs
        recon, losses, _, _, _ = model(x)
        losses.err.mean().backward()
    finally:
        _lib.load().gx_matmul_precision(-1)


def _full(case):
    from tests.test_fullbatch_gpu import Full
    return Full(case)


def _snap(ts):
    return [t.clone() for t in ts._train_state()]


def _restore(ts, snap):
    with torch.no_grad():
        for t, s in zip(ts._train_state(), snap):
            t.copy_(s)


def _eager_step(ts, x):
    ts.use_graph = False
    try:
        return ts.step(x)
    finally:
        ts.use_graph = True


def test_trainstep_round_trip_high_medium_high():
    """'high', three TrainStep(graph=True) steps in 'medium', 'high' again.  After every switch the next step() re-captures:
    its output and parameters equal an eager step at the new level from the same state, bit for bit; after the round trip a
    forward + backward + update in 'high' is bit-identical to one before any switch."""
    import genesis_amd
    from genesis_amd import _lib
    from genesis_amd.trainer import TrainStep
    gold = _full('v2_metric_b32')
    model = gold.build()
    x = gold.x().to(DEV)
    kw = gold.forward_kwargs(gold.noise())
    try:
        genesis_amd.set_matmul_precision('high')
        ts = TrainStep(model, gold.S, graph=True)
        s0 = _snap(ts)
        before = ts.step(x, **kw).clone()
        p_before = ts.flat_p.clone()
        _restore(ts, s0)
        ts.step(x)                                   # captured at 'high'
        outs = {}
        for i, lv in enumerate(['medium', 'medium', 'medium', 'high']):
            switched = i == 0 or lv != 'medium'
            genesis_amd.set_matmul_precision(lv)
            s = _snap(ts)
            g_out = ts.step(x).clone()
            g_p = ts.flat_p.clone()
            if switched:
                _restore(ts, s)
                e_out = _eager_step(ts, x).clone()
                assert torch.equal(g_out, e_out), (lv, g_out, e_out)
                assert torch.equal(g_p, ts.flat_p), lv
            outs.setdefault(lv, []).append(g_out)
            assert torch.isfinite(g_out).all()
        _restore(ts, s0)
        after = ts.step(x, **kw).clone()
        assert torch.equal(before, after), (before, after)
        assert torch.equal(p_before, ts.flat_p)
        print('ELBO high %.6f, medium %s' % (float(before[0]), ['%.6f' % float(o[0]) for o in outs['medium']]))
        ts.close()
    finally:
        _lib.load().gx_matmul_precision(-1)


def test_unchanged_loop_graphs_are_keyed_by_the_level():
    """The unchanged train.py loop (autostep): its captured graphs and its packed-weight cache are keyed by the level, so a
    switch re-captures instead of replaying the other level's kernels; every loss stays finite and the medium one moves."""
    import genesis_amd
    from genesis_amd import _lib, autostep
    from genesis_amd import testing as T
    model = _v2_tiny()
    opt = torch.optim.Adam(model.parameters(), 1e-4)
    x = T.make_input(6, 8, 32).to(DEV)
    keys, replays = [], []
    try:
        for lv in ('high', 'medium', 'high'):
            genesis_amd.set_matmul_precision(lv)
            keys.append(autostep._graph_key(model, x))
            for _ in range(5):
                opt.zero_grad()
                recon, losses, _, _, _ = model(x)
                loss = losses.err.mean() + torch.stack(list(losses.kl_l_k), 1).mean(0).sum()
                loss.backward()
                opt.step()
                assert torch.isfinite(loss.detach()).all()
            replays.append(autostep.graph_stats(model))
    finally:
        _lib.load().gx_matmul_precision(-1)
    assert keys[0] != keys[1] and keys[0][:-1] == keys[1][:-1] and keys[0] == keys[2]
    print('autostep (forward replays, backward replays, fallbacks) after each level:', replays)


# ---------------------------------------------------------------- model level
def _rounded_convs():
    """F.conv2d / F.conv_transpose2d with both operands rounded to bf16 in the forward, and the incoming gradient rounded in the
    backward (what the data- and weight-gradient kernels multiply): fp64 arithmetic otherwise."""
    c2, ct = F.conv2d, F.conv_transpose2d

    def make(orig):
        class Fn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, w, b, args):
                ctx.save_for_backward(x, w)
                ctx.args, ctx.has_b = args, b is not None
                return orig(x.to(torch.bfloat16).to(x.dtype), w.to(torch.bfloat16).to(w.dtype), b, *args)

            @staticmethod
            def backward(ctx, g):
                x, w = ctx.saved_tensors
                with torch.enable_grad():
                    xr = x.detach().to(torch.bfloat16).to(x.dtype).requires_grad_()
                    wr = w.detach().to(torch.bfloat16).to(w.dtype).requires_grad_()
                    y = orig(xr, wr, None, *ctx.args)
                    gx, gw = torch.autograd.grad(y, (xr, wr), g.to(torch.bfloat16).to(g.dtype))
                return gx, gw, (g.sum((0, 2, 3)) if ctx.has_b else None), None

        def call(x, w, b=None, *args):
            return Fn.apply(x, w, b, args)
        return call
    return make(c2), make(ct), c2, ct


@pytest.mark.parametrize('case', ['v2_metric_b32', 'monet_cfg4_b32', 'genesis_cfg3_b32'])
def test_model_in_medium_within_the_bf16_error_budget(case):
    """GENESIS-V2 (metric configuration), MONet (cfg 4) and GENESIS (cfg 3) at B = 32 -- the chip-filling dispatch -- in 'medium',
    with the fixture's noise (and, for GENESIS-V2, the fp64 run's seed pixels) injected.  Yardstick: the fp64 oracle against the
    same oracle with every conv's operands rounded to bf16 (a superset of the layers 'medium' rounds: the fp32-pipe layers stay
    exact in the HIP path).  Bar (tests/test_error_budget_gpu.py): HIP error <= 4 x the yardstick's error + floor."""
    import genesis_amd
    from genesis_amd import _lib
    from tests.test_error_budget_gpu import judge, to_dtype, grads_of, hip_grads
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
    bad = judge(fwd, hip_grads(model), gb, g64, '%s medium (column 2: fp64 with bf16 conv operands)' % case)
    assert not bad, bad


# ---------------------------------------------------------------- training
ELBO_GAP_BAR = 2e-5      # relative |ELBO(medium) - ELBO(high)| per step: 2.5 x the measured maximum over the 50 steps (8.1e-6)


def test_fifty_training_steps_in_medium_track_high():
    """50 TrainStep(graph=True) steps from the full_v2_metric_b32 weights and inputs at 'medium' and at 'high': every ELBO
    finite, the relative gap at every step within ELBO_GAP_BAR (>= 2 x the measured maximum; both printed)."""
    import genesis_amd
    from genesis_amd import _lib
    from genesis_amd.trainer import TrainStep
    gold = _full('v2_metric_b32')
    x = gold.x().to(DEV)
    elbo = {}
    try:
        for lv in ('high', 'medium'):
            genesis_amd.set_matmul_precision(lv)
            torch.manual_seed(0)
            ts = TrainStep(gold.build(), gold.S, graph=True)
            elbo[lv] = torch.stack([ts.step(x)[0].clone() for _ in range(50)]).double().cpu()
            ts.close()
    finally:
        _lib.load().gx_matmul_precision(-1)
    assert torch.isfinite(elbo['high']).all() and torch.isfinite(elbo['medium']).all()
    gap = ((elbo['medium'] - elbo['high']).abs() / elbo['high'].abs())
    print('relative ELBO gap medium vs high over 50 steps: max %.3e (step %d), mean %.3e; bar %.1e; ELBO high %.4f -> %.4f'
          % (float(gap.max()), int(gap.argmax()), float(gap.mean()), ELBO_GAP_BAR, float(elbo['high'][0]), float(elbo['high'][-1])))
    assert float(gap.max()) <= ELBO_GAP_BAR
