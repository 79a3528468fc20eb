"""The partial-maxima hand-over behind the fp16-piece convs (gx_amax_tap / gx_kq_amax_link, hip_ops.take_amax): every producer
leaves one partial maximum per workgroup whose maximum IS the stored tensor's largest magnitude, writes every one of the n
slots it reports, and declines where it must; every consumer reads all n partials (the last one, both arrays of a pair, across
the fold / Winograd thresholds); and a real training step hands each operand its own maxima.

A wrong maximum is silent (a hi piece that overflows fp16, or lost low bits), so these tests pin the number itself, bit for bit,
not only the conv results at a tolerance."""
import inspect
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

from genesis_amd import _lib
from genesis_amd import hip_ops as hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)


def _arena():
    hip.amax_fill(NAN)
    return hip._ARENA[torch.cuda.current_device()][0]


def _tapped(fn):
    """fn() after the whole arena was set to NaN (and no handle is pending) -> (result, handle take_amax() returns)."""
    _arena()
    hip.take_amax()
    r = fn()
    return r, hip.take_amax()


def _check_parts(h, t, what=''):
    """h: the launch's handle; t: the tensor it stored (or a list of the tensors that hold the same values)."""
    assert h is not None and h.n > 0, '%s: the launch did not serve the tap' % what
    assert h.n <= hip._TAP_CAP, (what, h.n)
    v = hip.amax_values(h).clone()
    assert bool(torch.isfinite(v).all()), '%s: %d of %d partials never written' % (what, int((~torch.isfinite(v)).sum()), h.n)
    assert float(v.min()) >= 0.0, (what, float(v.min()))
    ts = t if isinstance(t, (list, tuple)) else [t]
    for tt in ts:
        assert float(v.max()) == float(tt.abs().max()), (what, float(v.max()), float(tt.abs().max()), h.n)
    return h.n


def _plant(t, where, value):
    """t[N, C, H, W]: one element set to `value` -- first / last element, last image, last channel, last row and column."""
    N, C, H, W = t.shape
    idx = {'first': (0, 0, 0, 0), 'last': (N - 1, C - 1, H - 1, W - 1), 'last_image': (N - 1, C // 2, H // 2, 1),
           'last_channel': (N // 2, C - 1, 1, W // 2), 'tile_edge': (N - 1, C // 3, H - 1, W - 2)}[where]
    t[idx] = value
    return t


PLANTS = ['first', 'last', 'last_image', 'last_channel', 'tile_edge']


@pytest.fixture
def kq_every_shape():
    """The <= 32-channel kernel (and its tap) at the tests' small batches, not only where it fills the chip."""
    _lib.call('gx_kq_policy', 2)
    yield
    _lib.call('gx_kq_policy', 1)


# ============================================================================== 1. producers
# --- kq_c3h (conv3x3 of <= 32 output channels, fp16 x 3 form) through conv3x3_bias_act_fwd / conv3x3_dgrad_act
KQ_SHAPES = {           # (N, K reduction channels, M output channels, H, W): the epilogue each reaches
    'row_tiles_partial': (4, 16, 32, 40, 40),         # whole-row tiles (6 rows of 40), the last tile 4 rows
    'full_tile': (4, 32, 32, 64, 64),                 # power-of-two grid, all 32 channels: the unguarded store
    'partial_channels': (4, 16, 20, 64, 64),          # M < 32: the guarded store
    'partial_image_group': (5, 16, 32, 8, 8),         # 8 x 8 tiles of G = 4 images: the last group holds one
}


@pytest.mark.parametrize('act', ['relu', 'elu', 'none'])
@pytest.mark.parametrize('shape', sorted(KQ_SHAPES))
@pytest.mark.usefixtures('kq_every_shape')
def test_kq_c3h_forward_tap_is_exact_and_complete(shape, act):
    N, K, M, H, W = KQ_SHAPES[shape]
    w = rnd(M, K, 3, 3, seed=2, scale=0.2)
    b = rnd(M, seed=3, scale=0.1)
    for i, where in enumerate(PLANTS):
        x = _plant(rnd(N, K, H, W, seed=10 + i), where, -40.0 if act == 'none' else 40.0)
        y, h = _tapped(lambda: hip.conv3x3_bias_act_fwd(x, w, b, act, tap=True))
        _check_parts(h, y, '%s %s %s' % (shape, act, where))
        assert torch.equal(y, hip.conv3x3_bias_act_fwd(x, w, b, act))
    if act == 'relu':          # a dead ReLU: all-zero output, all-zero partials
        y, h = _tapped(lambda: hip.conv3x3_bias_act_fwd(x, w, torch.full_like(b, -1e4), act, tap=True))
        assert float(y.abs().max()) == 0.0
        _check_parts(h, y, 'dead relu')


@pytest.mark.parametrize('act', ['relu', 'elu', 'none'])
@pytest.mark.parametrize('shape', sorted(KQ_SHAPES))
@pytest.mark.usefixtures('kq_every_shape')
def test_kq_c3h_masked_data_gradient_tap_is_exact_and_complete(shape, act):
    """conv3x3_dgrad_act: the data gradient with act'(xout) (the MONet mask) in the epilogue -- signed values."""
    N, K, M, H, W = KQ_SHAPES[shape]          # (K: dy's channels, M: dx's)
    assert hip.conv3x3_dgrad_act_supported(N, M, K, H, W)
    w = rnd(K, M, 3, 3, seed=4, scale=0.2)
    pre = rnd(N, M, H, W, seed=5)
    xout = F.relu(pre) if act == 'relu' else (F.elu(pre) if act == 'elu' else pre)
    xout = xout.contiguous()
    for i, where in enumerate(PLANTS):
        dy = _plant(rnd(N, K, H, W, seed=20 + i), where, -50.0)
        (dxa, _), h = _tapped(lambda: hip.conv3x3_dgrad_act(dy, w, xout, act, want_dbias=False, tap=True))
        _check_parts(h, dxa, '%s %s %s' % (shape, act, where))
        assert torch.equal(dxa, hip.conv3x3_dgrad_act(dy, w, xout, act, want_dbias=False)[0])


# --- GroupNorm + ReLU forward: register / small / two-pass forms, concat slices, resampled copies, the conv epilogue
GN_FWD = {       # (N, C, S, groups)
    'register_64': (8, 64, 64, 8), 'register_32': (6, 32, 32, 8), 'register_16': (7, 32, 16, 8), 'two_pass_128': (3, 32, 128, 8),
}


@pytest.mark.parametrize('form', sorted(GN_FWD))
def test_groupnorm_forward_tap_is_exact_and_complete(form):
    N, C, S, G = GN_FWD[form]
    gamma, beta = 1 + 0.3 * rnd(C, seed=1), 0.2 * rnd(C, seed=2)
    for i, where in enumerate(PLANTS):
        y = _plant(rnd(N, C, S, S, seed=30 + i), where, 30.0)
        out = torch.empty_like(y)
        _, h = _tapped(lambda: hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (out, 0, 0)))
        _check_parts(h, out, '%s %s' % (form, where))
    # a channel slice of a concat buffer + the downsampled second copy (the UNet's skip buffer and next input)
    y = _plant(rnd(N, C, S, S, seed=40), 'last_channel', 30.0)
    cat = torch.zeros(N, C + 16, S, S, device=DEV)
    nxt = torch.empty(N, C, S // 2, S // 2, device=DEV)
    _, h = _tapped(lambda: hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (cat, 16, 0), (nxt, 0, 2)))
    _check_parts(h, cat[:, 16:], form + ' concat slice')
    assert float(nxt.abs().max()) <= float(cat.abs().max())
    # a dead ReLU everywhere
    out = torch.empty_like(y)
    _, h = _tapped(lambda: hip.gn_relu_fwd(y, gamma, torch.full_like(beta, -1e3), G, 1e-5, (out, 0, 0)))
    assert float(out.abs().max()) == 0.0
    _check_parts(h, out, form + ' dead relu')


@pytest.mark.parametrize('S', [16, 32, 64])
def test_conv_groupnorm_epilogue_tap_is_exact_and_complete(S):
    N, Cin, C, G = 6, 32, 64, 8
    w = rnd(C, Cin, 3, 3, seed=3, scale=0.1)
    gamma, beta = 1 + 0.3 * rnd(C, seed=4), 0.2 * rnd(C, seed=5)
    for i, where in enumerate(PLANTS):
        x = _plant(rnd(N, Cin, S, S, seed=50 + i), where, 25.0)
        cat = torch.zeros(N, C + 8, S, S, device=DEV)
        up = torch.empty(N, C, 2 * S, 2 * S, device=DEV)
        _, h = _tapped(lambda: hip.conv3x3_gn_relu_fwd(x, w, gamma, beta, G, 1e-5, (cat, 8, 0), (up, 0, 1)))
        _check_parts(h, cat[:, 8:], 'S=%d %s' % (S, where))
        assert float(up.abs().max()) <= float(cat.abs().max())


# --- GroupNorm + ReLU backward (plain, and with the 1x1 conv's data gradient formed on load)
@pytest.mark.parametrize('N,C,S,G', [(8, 64, 64, 8), (7, 32, 16, 8), (3, 32, 128, 8), (6, 32, 32, 8)])
def test_groupnorm_backward_tap_is_exact_and_complete(N, C, S, G):
    gamma, beta = 1 + 0.3 * rnd(C, seed=1), 0.2 * rnd(C, seed=2)
    y = rnd(N, C, S, S, seed=3, scale=2.0) + 0.3
    mean, rstd = hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (torch.empty_like(y), 0, 0))
    for i, where in enumerate(PLANTS):
        g = _plant(rnd(N, C, S, S, seed=60 + i), where, -200.0)
        (dy, _, _, _), h = _tapped(lambda: hip.gn_relu_bwd(y, gamma, beta, mean, rstd, G, (g, 0, 0), None, True))
        _check_parts(h, dy, where)


@pytest.mark.parametrize('N,C,Cout,S', [(200, 32, 4, 64), (3, 64, 4, 64), (2, 32, 7, 128), (14, 32, 4, 128)])
def test_groupnorm_projected_backward_tap_is_exact_and_complete(N, C, Cout, S):
    """gn_relu_bwd_proj (the decoder head): 200 x 8 = 1600 workgroups on the register kernel (beyond 1536), and the chunked
    128 x 128 form (its apply kernel covers the whole tensor: it serves)."""
    G = 8
    gamma, beta = 1 + 0.3 * rnd(C, seed=1), 0.2 * rnd(C, seed=2)
    y = rnd(N, C, S, S, seed=3, scale=2.0) + 0.3
    w = rnd(Cout, C, seed=4, scale=0.3)
    mean, rstd = hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, None)
    ns = set()
    for i, where in enumerate(['first', 'last', 'last_image']):
        g = _plant(rnd(N, Cout, S, S, seed=70 + i), where, -300.0)
        (dy, _, _, _), h = _tapped(lambda: hip.gn_relu_bwd_proj(y, gamma, beta, mean, rstd, G, g, w, True))
        ns.add(_check_parts(h, dy, where))
    if N * G > 1536:
        assert min(ns) > 1536, ns


# --- gated units (GENESIS / BaselineVAE)
@pytest.mark.parametrize('norm', ['bn', 'in', None])
@pytest.mark.parametrize('N,C,S', [(6, 32, 32), (4, 32, 16), (3, 64, 64)])
def test_gated_unit_taps_are_exact_and_complete(norm, N, C, S):
    assert hip.GATED_AMAX
    bias = rnd(2 * C, seed=1, scale=0.5)
    prm = [1 + 0.3 * rnd(C, seed=2), 0.2 * rnd(C, seed=3), 1 + 0.3 * rnd(C, seed=4), 0.2 * rnd(C, seed=5)] if norm else [None] * 4
    for i, where in enumerate(['first', 'last', 'last_channel']):
        y = _plant(rnd(N, 2 * C, S, S, seed=80 + i, scale=2.0), where, -40.0)
        (out, stats), h = _tapped(lambda: hip.gated_norm_fwd(y, bias, norm, *prm))
        _check_parts(h, out, 'fwd %s' % where)
        g = _plant(rnd(N, C, S, S, seed=90 + i), where, -60.0)
        res, h = _tapped(lambda: hip.gated_norm_bwd(y, bias, norm, *prm, stats, g))
        _check_parts(h, res[0], 'bwd %s' % where)


# --- the BroadcastDecoder chain's first layer and the 1 x 1 data gradient (40 x 40 and 72 x 72 planes: partial last blocks)
@pytest.mark.parametrize('act', ['relu', 'elu'])
@pytest.mark.parametrize('d', [40, 72])      # (40 x 40 and 72 x 72 planes: not multiples of 256)
@pytest.mark.usefixtures('kq_every_shape')
def test_broadcast_chain_producers_tap_exact_and_complete(act, d):
    N, L, C = 24, 16, 32
    w0, b0 = rnd(C, L + 2, 3, 3, seed=1, scale=0.2), rnd(C, seed=2, scale=0.1)
    lin = torch.linspace(-1, 1, d, device=DEV)
    z = rnd(N, L, seed=3)
    z[N - 1, L - 1] = 30.0
    y, h = _tapped(lambda: hip.bcast_conv3x3_fwd(z, w0, b0, lin, lin, act, tap=True))
    _check_parts(h, y, 'bcast')
    ow, ob = rnd(4, C, seed=4, scale=0.3), rnd(4, seed=5, scale=0.1)
    for i, where in enumerate(PLANTS):
        g = _plant(rnd(N, 4, d, d, seed=100 + i), where, -80.0)
        (dxa, _, _, _), h = _tapped(lambda: hip.conv1x1_bwd_act(y, g, ow, ob, act, tap=True))
        _check_parts(h, dxa, 'conv1x1_bwd_act %s' % where)


# --- declining: a chunked launch, a launch beyond the request's capacity, and every wrapper that does not tap
def _producers():
    """(name, call with the tap armed by its wrapper, the tensor it stores) -- one per producer entry point."""
    C, S, G = 32, 32, 8
    y = rnd(4, C, S, S, seed=1, scale=2.0)
    gamma, beta = 1 + 0.3 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    out = torch.empty_like(y)
    mean, rstd = hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (out, 0, 0))
    g = rnd(4, C, S, S, seed=4)
    w3 = rnd(C, C, 3, 3, seed=5, scale=0.1)
    b3 = rnd(C, seed=6, scale=0.1)
    yg = rnd(4, 2 * C, S, S, seed=7)
    bg = rnd(2 * C, seed=8)
    ow, ob = rnd(4, C, seed=9), rnd(4, seed=10)
    g4 = rnd(4, 4, S, S, seed=11)
    z, lin = rnd(4, 16, seed=12), torch.linspace(-1, 1, S, device=DEV)
    w0 = rnd(C, 18, 3, 3, seed=13, scale=0.2)
    o2, o3 = torch.empty_like(y), torch.empty_like(y)
    _, stats = hip.gated_norm_fwd(yg, bg, None, None, None, None, None)
    hip.take_amax()

    def gn_fwd():
        hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (o2, 0, 0))
        return o2

    def conv_gn_fwd():
        hip.conv3x3_gn_relu_fwd(y, w3, gamma, beta, G, 1e-5, (o3, 0, 0))
        return o3
    return [
        ('gn_relu_fwd', gn_fwd),
        ('conv3x3_gn_relu_fwd', conv_gn_fwd),
        ('gn_relu_bwd', lambda: hip.gn_relu_bwd(y, gamma, beta, mean, rstd, G, (g, 0, 0))[0]),
        ('gn_relu_bwd_proj', lambda: hip.gn_relu_bwd_proj(y, gamma, beta, mean, rstd, G, g4, ow)[0]),
        ('gated_norm_fwd', lambda: hip.gated_norm_fwd(yg, bg, None, None, None, None, None)[0]),
        ('gated_norm_bwd', lambda: hip.gated_norm_bwd(yg, bg, None, None, None, None, None, stats, g)[0]),
        ('conv3x3_bias_act_fwd', lambda: hip.conv3x3_bias_act_fwd(y, w3, b3, 'relu', tap=True)),
        ('conv3x3_dgrad_act', lambda: hip.conv3x3_dgrad_act(g, w3, out, 'relu', want_dbias=False, tap=True)[0]),
        ('conv1x1_bwd_act', lambda: hip.conv1x1_bwd_act(out, g4, ow, ob, 'relu', tap=True)[0]),
        ('bcast_conv3x3_fwd', lambda: hip.bcast_conv3x3_fwd(z, w0, b3, lin, lin, 'relu', tap=True)),
    ]


@pytest.mark.usefixtures('kq_every_shape')
def test_every_producer_declines_a_chunked_launch_and_one_beyond_the_capacity(monkeypatch):
    served = {}
    for name, run in _producers():
        t, h = _tapped(run)
        served[name] = _check_parts(h, t, name)
    real_begin = hip._tap_begin
    # a launch that covers another count than the request's (what a chunked producer is): no handle, nothing written
    with monkeypatch.context() as m:
        m.setattr(hip, '_tap_begin', lambda dev, hw, numel: real_begin(dev, hw, numel + 4))
        for name, run in _producers():
            arena = _arena()
            hip.take_amax()
            run()
            assert hip.take_amax() is None, name
            assert bool(torch.isnan(arena).all()), '%s wrote partials for a launch that did not serve' % name
    # a request one slot short of the launch's workgroups: declined, the arena beyond (and inside) the reservation untouched
    for name, run in _producers():
        if served[name] < 2:
            continue
        with monkeypatch.context() as m:
            m.setattr(hip, '_TAP_CAP', served[name] - 1)
            arena = _arena()
            hip.take_amax()
            run()
            assert hip.take_amax() is None, name
            assert bool(torch.isnan(arena).all()), '%s wrote beyond its request' % name
    # the same request with room for exactly n: served again, the same count
    for name, run in _producers():
        with monkeypatch.context() as m:
            m.setattr(hip, '_TAP_CAP', served[name])
            t, h = _tapped(run)
            assert _check_parts(h, t, name) == served[name]


@pytest.mark.usefixtures('kq_every_shape')
def test_a_wrapper_that_does_not_tap_leaves_no_earlier_handle(monkeypatch):
    """take_amax() after a launch that did not tap is None -- never the handle an earlier tapped launch left untaken."""
    C, S, G = 32, 32, 8
    y = rnd(4, C, S, S, seed=1, scale=2.0)
    gamma, beta = 1 + 0.3 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    out = torch.empty_like(y)
    g, g4 = rnd(4, C, S, S, seed=4), rnd(4, 4, S, S, seed=5)
    w3, b3 = rnd(C, C, 3, 3, seed=6, scale=0.1), rnd(C, seed=7, scale=0.1)
    ow, ob = rnd(4, C, seed=8), rnd(4, seed=9)
    z, lin = rnd(4, 16, seed=10), torch.linspace(-1, 1, S, device=DEV)
    w0 = rnd(C, 18, 3, 3, seed=11, scale=0.2)
    yg, bg = rnd(4, 2 * C, S, S, seed=12), rnd(2 * C, seed=13)
    _, stats = hip.gated_norm_fwd(yg, bg, None, None, None, None, None)
    hip.take_amax()

    def leave_a_handle():
        hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (out, 0, 0))      # tapped, not taken
        assert hip._LAST.amax is not None, 'no handle pending: the test would pass vacuously'
    untapped = [
        ('gn_relu_fwd(dst0=None)', lambda: hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, None)),
        ('conv1x1_bwd_act', lambda: hip.conv1x1_bwd_act(out, g4, ow, ob, 'relu')),
        ('bcast_conv3x3_fwd', lambda: hip.bcast_conv3x3_fwd(z, w0, b3, lin, lin, 'relu')),
        ('conv3x3_bias_act_fwd', lambda: hip.conv3x3_bias_act_fwd(y, w3, b3, 'relu')),
        ('conv3x3_dgrad_act', lambda: hip.conv3x3_dgrad_act(g, w3, out, 'relu')),
    ]
    for name, run in untapped:
        leave_a_handle()
        run()
        assert hip.take_amax() is None, name
    with monkeypatch.context() as m:
        m.setattr(hip, 'GATED_AMAX', False)
        for name, run in (('gated_norm_fwd', lambda: hip.gated_norm_fwd(yg, bg, None, None, None, None, None)),
                          ('gated_norm_bwd', lambda: hip.gated_norm_bwd(yg, bg, None, None, None, None, None, stats, g))):
            leave_a_handle()
            run()
            assert hip.take_amax() is None, name + ' (GATED_AMAX off)'


def test_link_route_partials_are_exact_and_complete(monkeypatch):
    """gx_kq_amax_link on its own (the tap declined): the projected GroupNorm backward writes n partials into the link's buffer --
    the same n the tap reports, all finite, their maximum dy's -- and nothing behind them; the transposed conv that reads dy
    next is bit-identical with and without the hand-over."""
    N, C, Co, S, G = 56, 64, 4, 64, 8
    gamma, beta = 1 + 0.3 * rnd(C, seed=1), 0.2 * rnd(C, seed=2)
    y = rnd(N, C, S, S, seed=3, scale=2.0) + 0.3
    w, g = rnd(Co, C, seed=4, scale=0.2), _plant(rnd(N, Co, S, S, seed=5), 'last', -90.0)
    wd = rnd(C, C, 5, 5, seed=6, scale=0.05)
    mean, rstd = hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, None)
    (dy0, _, _, _), h = _tapped(lambda: hip.gn_relu_bwd_proj(y, gamma, beta, mean, rstd, G, g, w, True))
    n = _check_parts(h, dy0, 'tap')
    dx0 = hip.deconv5x5s2_dgrad(dy0, wd)
    hits = lambda: int(_lib.query('gx_kq_amax_link_hits'))      # noqa: E731
    try:
        with monkeypatch.context() as m:
            m.setattr(hip, '_TAP_CAP', 4)          # the tap declines: the link's own buffer takes the partials
            buf = hip.amax_link(y.device, y.numel())
            buf.fill_(NAN)
            h0 = hits()
            dy = hip.gn_relu_bwd_proj(y, gamma, beta, mean, rstd, G, g, w, True)[0]
            assert hip.take_amax() is None
            v = buf[:n].clone()
            assert bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0 and float(v.max()) == float(dy.abs().max())
            assert bool(torch.isnan(buf[n:]).all())
            dx = hip.deconv5x5s2_dgrad(dy, wd)
            assert hits() == h0 + 1
            assert torch.equal(dy, dy0) and torch.equal(dx, dx0)
            del buf
    finally:
        _lib.call('gx_kq_amax_link', None, 0, 0)


# ============================================================================== 2. consumers
LAYOUTS = [      # (n0, n1, where the maximum sits): around kFoldPartsAbove = 1024 and kWinoAmaxMax = 1536
    (1, 0, 'first'), (256, 0, 'last'), (1024, 0, 'last'), (1025, 0, 'last'), (1536, 0, 'first'), (1536, 0, 'last'),
    (1537, 0, 'last'), (16384, 0, 'last'), (768, 768, 'second'), (768, 769, 'second'), (1024, 1, 'second'),
    (700, 836, 'first'),
]
WINO_MAX = 1536


def _synthetic(top, n0, n1, where, seed, drop=False):
    """Handles whose partials lie in [0, top / 16) except ONE equal to `top` (the operand's true maximum) at `where`.  A consumer
    that misses the slot holding `top` takes a power-of-two scale at least four binades too large: the operand's largest values
    no longer fit an fp16 hi piece, and the result changes.  (One binade is not enough to show it: the hi / lo split of x * 2^e
    is exact under a power of two, so a scale one binade off gives the same bits -- measured.)  drop: that slot holds 0 instead
    (the handle a consumer that skips it effectively reads)."""
    g = torch.Generator().manual_seed(seed)
    v0 = torch.rand(n0, generator=g) * top / 16
    v1 = torch.rand(n1, generator=g) * top / 16 if n1 else None
    m = 0.0 if drop else top
    if where == 'first':
        v0[0] = m
    elif where == 'last':
        v0[n0 - 1] = m
    else:
        v1[n1 - 1] = m
    h0 = hip.amax_handle(v0)
    return h0 if v1 is None else [h0, hip.amax_handle(v1)]


def _chan_err(got, ref, dim=1):
    dims = [d for d in range(got.dim()) if d != dim]
    return ((got.double().cpu() - ref).pow(2).sum(dims).sqrt() / ref.pow(2).sum(dims).sqrt().clamp_min(1e-300))


def _fp32_pipe(setter, fn):
    _lib.call(setter, 0)
    try:
        return fn()
    finally:
        _lib.call(setter, -1)


_CONSUMERS = {}
_DGRAD_ACT = []


def _c5_every_size(fn):
    with pytest.MonkeyPatch.context() as m:
        m.setenv('GENESIS_C5_FAST', '2')          # (conv5x5_wgrad on the row-ring tiles at the test's small size, as test_kernels_gpu)
        return fn()


def _wino_f16_share():
    return float(_lib.load().gx_wino_f16_share())


def _consumer(name):
    """(operand tensors, call(handles), fp64 reference, output-channel dim, precision switch, kernel family) per consumer."""
    if name in _CONSUMERS:
        return _CONSUMERS[name]
    if name in ('conv3x3_fwd', 'conv3x3_wino_fwd', 'kq_c3h_fwd', 'kq_c3h_dgrad', 'conv3x3_dgrad', 'conv3x3_wino_dgrad',
                'kq_c3h_bias_act', 'kq_c3h_dgrad_act'):
        small = name.startswith('kq')
        N, Cin, Cout, S = (4, 32, 32, 40) if small else (16, 64, 64, 32)
        w = rnd(Cout, Cin, 3, 3, seed=2, scale=0.1)
        fwd = name.endswith('fwd') or name == 'kq_c3h_bias_act'
        x = rnd(N, Cin if fwd else Cout, S, S, seed=1)
        xd = x.double().cpu()
        b = rnd(Cout, seed=3, scale=0.1)
        xout = F.relu(rnd(N, Cin, S, S, seed=4)).contiguous()
        if fwd:
            ref = F.conv2d(xd, w.double().cpu(), None, 1, 1)
        else:
            ref = F.conv_transpose2d(xd, w.double().cpu(), None, 1, 1)
        if name == 'kq_c3h_bias_act':
            ref = F.relu(ref + b.double().cpu().view(1, -1, 1, 1))
            call = lambda hs: hip.conv3x3_bias_act_fwd(x, w, b, 'relu', amax_in=hs)       # noqa: E731
        elif name == 'kq_c3h_dgrad_act':
            ref = ref * (xout.double().cpu() > 0)
            _DGRAD_ACT[:] = [w, xout]
            call = lambda hs: hip.conv3x3_dgrad_act(x, w, xout, 'relu', want_dbias=False, amax_in=hs)[0]      # noqa: E731
        elif name in ('conv3x3_wino_fwd', 'conv3x3_wino_dgrad'):
            call = lambda hs: hip.conv3x3_wino(x, w, 0 if fwd else 1, amax_in=hs)       # noqa: E731
        elif fwd:
            call = lambda hs: hip.conv3x3_fwd(x, w, amax_in=hs)       # noqa: E731
        else:
            call = lambda hs: hip.conv3x3_dgrad(x, w, amax_in=hs)       # noqa: E731
        c = ([x], call, ref, 1, 'gx_kq_precision' if small else 'gx_wino_precision', 'kq' if small else 'wino')
    elif name == 'conv3x3_pair_fwd':
        N, Cin, Co1, Co2, S = 4, 64, 64, 32, 32
        x = rnd(N, Cin, S, S, seed=1)
        w1, w2 = rnd(Co1, Cin, 3, 3, seed=2, scale=0.1), rnd(Co2, Cin, 3, 3, seed=3, scale=0.1)
        ref = torch.cat([F.conv2d(x.double().cpu(), w.double().cpu(), None, 1, 1) for w in (w1, w2)], 1)
        c = ([x], lambda hs: torch.cat(hip.conv3x3_pair_fwd(x, w1, w2, amax_in=hs)[:2], 1), ref, 1, 'gx_wino_precision', 'wino')
    elif name == 'conv3x3_pair_dgrad':
        N, Cin, Co1, Co2, S = 4, 64, 64, 32, 32
        d1, d2 = rnd(N, Co1, S, S, seed=1), rnd(N, Co2, S, S, seed=2, scale=0.5)
        w1, w2 = rnd(Co1, Cin, 3, 3, seed=3, scale=0.1), rnd(Co2, Cin, 3, 3, seed=4, scale=0.1)
        ref = sum(F.conv_transpose2d(d.double().cpu(), w.double().cpu(), None, 1, 1) for d, w in ((d1, w1), (d2, w2)))
        c = ([d1, d2], lambda hs: hip.conv3x3_pair_dgrad(d1, d2, w1, w2, None, amax_in=hs), ref, 1, 'gx_wino_precision', 'wino')
    elif name in ('conv3x3_wgrad', 'deconv5x5s2_wgrad', 'conv5x5_wgrad'):
        N, Cin, Cout, S = (8, 64, 64, 32) if name != 'deconv5x5s2_wgrad' else (8, 64, 64, 16)
        x = rnd(N, Cin, S, S, seed=1)
        dy = rnd(N, Cout, 2 * S if name == 'deconv5x5s2_wgrad' else S, 2 * S if name == 'deconv5x5s2_wgrad' else S, seed=2)
        if name == 'conv3x3_wgrad':
            ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (Cout, Cin, 3, 3), dy.double().cpu(), padding=1)
            call, cdim = (lambda am: hip.conv3x3_wgrad(x, dy, amax=am)), 0
        elif name == 'deconv5x5s2_wgrad':
            wv = torch.zeros(Cin, Cout, 5, 5, dtype=torch.float64, requires_grad=True)
            F.conv_transpose2d(x.double().cpu(), wv, None, 2, 2, 1).backward(dy.double().cpu())
            ref = wv.grad
            call, cdim = (lambda am: hip.deconv5x5s2_wgrad(x, dy, amax=am)), 1
        else:
            ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (Cout, Cin, 5, 5), dy.double().cpu(), padding=2)
            call, cdim = (lambda am: _c5_every_size(lambda: hip.conv5x5_wgrad(dy, x, amax=am))), 0
        c = ([dy, x], call, ref, cdim, 'gx_wgq_precision', 'wgq')
    else:
        raise KeyError(name)
    _CONSUMERS[name] = c
    return c


INPUT_CONSUMERS = ['conv3x3_wino_fwd', 'conv3x3_wino_dgrad', 'conv3x3_pair_fwd', 'kq_c3h_fwd',
                   'kq_c3h_dgrad', 'kq_c3h_bias_act', 'kq_c3h_dgrad_act']


INPUT_CASES = [(n, l) for n in INPUT_CONSUMERS for l in LAYOUTS] + \
              [('conv3x3_pair_dgrad', l) for l in LAYOUTS if l[1] > 0]        # (one array per tensor: pairs only)


@pytest.mark.parametrize('name,layout', INPUT_CASES, ids=['%s-%d+%d@%s' % ((n,) + l) for n, l in INPUT_CASES])
@pytest.mark.usefixtures('kq_every_shape')
def test_input_hint_consumers_read_every_partial(name, layout):
    n0, n1, where = layout
    ops, call, ref, cdim, setter, fam = _consumer(name)
    top = max(float(t.abs().max()) for t in ops)
    hs = _synthetic(top, n0, n1, where, seed=n0 + 7 * n1)
    own = [hip.amax_of(t) for t in ops] if len(ops) > 1 else hip.amax_of(ops[0])
    s0 = _wino_f16_share()
    got = call(hs)
    s1 = _wino_f16_share()
    assert bool(torch.isfinite(got).all())
    with_own, without = call(own), call(None)
    f16 = fam == 'kq' or n0 + n1 <= WINO_MAX
    if name in ('conv3x3_wino_fwd', 'conv3x3_wino_dgrad'):
        # the form the launch took, as the library counts it (the share of Winograd flops on fp16 pieces since the process started)
        if f16:
            assert s1 > s0 or s1 == 1.0, ('expected the fp16-piece form', layout, s0, s1)
        else:
            assert s1 < s0 or s1 == 0.0, ('expected the bf16-piece form', layout, s0, s1)
    if f16:
        assert torch.equal(got, with_own), (name, layout)
        if fam == 'wino':        # (the <= 32-channel kernel makes a pass of its own without the hint: the same scale)
            assert not torch.equal(got, without), 'the hint was not taken'
        e = _chan_err(got, ref, cdim)
        if name == 'kq_c3h_dgrad_act':      # (the fused epilogue exists on the bf16 pipe only: the fp32 data gradient, masked)
            x, w, xout = ops[0], _DGRAD_ACT[0], _DGRAD_ACT[1]
            y32 = _fp32_pipe(setter, lambda: hip.conv3x3_dgrad(x, w) * (xout > 0))
        else:
            y32 = _fp32_pipe(setter, lambda: call(None))
        e32 = _chan_err(y32, ref, cdim)
        assert float((e / (1.5 * e32 + 1e-7)).max()) <= 1.0, (float(e.max()), float(e32.max()))
    else:        # (more partials than the Winograd kernel's workgroups reduce: the bf16-piece form, as without a hint)
        assert torch.equal(got, without), (name, layout)
    # the same handle without its maximum (that slot 0) gives other bits: the equality above depends on reading that slot
    if f16 and n0 + n1 > 1:       # (one partial of 0 is an all-zero tensor's handle: scale 2^0, exact for these values too)
        missing = _synthetic(top, n0, n1, where, seed=n0 + 7 * n1, drop=True)
        assert not torch.equal(call(missing), got), 'the slot holding the maximum was not read'


WGRAD_LAYOUTS = [(1, 0, 'first'), (1024, 0, 'last'), (1025, 0, 'last'), (1537, 0, 'last'), (16384, 0, 'last'),
                 (768, 769, 'second'), (1024, 1, 'second')]


@pytest.mark.parametrize('layout', WGRAD_LAYOUTS, ids=['%d+%d@%s' % l for l in WGRAD_LAYOUTS])
@pytest.mark.parametrize('name', ['conv3x3_wgrad', 'deconv5x5s2_wgrad', 'conv5x5_wgrad'])
def test_weight_gradient_consumers_read_every_partial_of_both_operands(name, layout):
    n0, n1, where = layout
    (a, b), call, ref, cdim, setter, fam = _consumer(name)
    own = call((hip.amax_of(a), hip.amax_of(b)))
    without = call(None)
    assert not torch.equal(own, without)
    e32 = _chan_err(_fp32_pipe(setter, lambda: call(None)), ref, cdim)
    for which in (0, 1):          # the synthetic handles on one operand, the other's own
        hs = _synthetic(float((a, b)[which].abs().max()), n0, n1, where, seed=n0 + n1 + which)
        am = (hs, hip.amax_of(b)) if which == 0 else (hip.amax_of(a), hs)
        got = call(am)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, own), (name, layout, which)
        e = _chan_err(got, ref, cdim)
        assert float((e / (1.5 * e32 + 1e-7)).max()) <= 1.0, (float(e.max()), float(e32.max()))
        if n0 + n1 == 1:
            continue
        missing = _synthetic(float((a, b)[which].abs().max()), n0, n1, where, seed=n0 + n1 + which, drop=True)
        assert not torch.equal(call((missing, am[1]) if which == 0 else (am[0], missing)), own), 'the maximum\'s slot was not read'


@pytest.mark.parametrize('scale', [1e-30, 1e30])
@pytest.mark.usefixtures('kq_every_shape')
def test_consumers_follow_a_real_producers_maxima_at_extreme_scales(scale):
    """GroupNorm with gamma / beta scaled by 1e-30 / 1e30 writes the operand; its tap is the consumer's scale.  One operand at
    the extreme, the other at unit scale (fp32 products stay finite)."""
    N, C, S, G = 4, 64, 32, 8
    y = rnd(N, C, S, S, seed=1, scale=2.0)
    gamma, beta = (1 + 0.3 * rnd(C, seed=2)) * scale, 0.2 * rnd(C, seed=3) * scale
    x = torch.empty_like(y)
    _, h = _tapped(lambda: hip.gn_relu_fwd(y, gamma, beta, G, 1e-5, (x, 0, 0)))
    _check_parts(h, x, 'scaled groupnorm')
    xd = x.double().cpu()
    for Cout, setter in ((64, 'gx_wino_precision'), (32, 'gx_kq_precision')):
        w = rnd(Cout, C, 3, 3, seed=4, scale=0.1)
        ref = F.conv2d(xd, w.double().cpu(), None, 1, 1)
        got = hip.conv3x3_fwd(x, w, amax_in=h)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, hip.conv3x3_fwd(x, w, amax_in=hip.amax_of(x)))
        e = _chan_err(got, ref)
        e32 = _chan_err(_fp32_pipe(setter, lambda: hip.conv3x3_fwd(x, w)), ref)
        assert float((e / (1.5 * e32 + 1e-7)).max()) <= 1.0, (Cout, float(e.max()), float(e32.max()))
    dy = rnd(N, 64, S, S, seed=5)
    ref = torch.nn.grad.conv2d_weight(xd, (64, C, 3, 3), dy.double().cpu(), padding=1)
    got = hip.conv3x3_wgrad(x, dy, amax=(hip.amax_of(dy), h))
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, hip.conv3x3_wgrad(x, dy, amax=(hip.amax_of(dy), hip.amax_of(x))))
    e = _chan_err(got, ref, 0)
    e32 = _chan_err(_fp32_pipe('gx_wgq_precision', lambda: hip.conv3x3_wgrad(x, dy)), ref, 0)
    assert float((e / (1.5 * e32 + 1e-7)).max()) <= 1.0, (float(e.max()), float(e32.max()))


# ============================================================================== 3. whole steps
# entry point -> (operand arguments, hint argument, kind): 'in' -- one tensor (a list of handles: the halves of one concat
# buffer, their union is the tensor's); 'pair' -- handle i belongs to tensor i; 'wgrad' -- (handles of a, handles of b)
AUDITED = {
    'conv3x3_fwd': (('x',), 'amax_in', 'in'), 'conv3x3_dgrad': (('dy',), 'amax_in', 'in'),
    'conv3x3_dgrad_parts': (('dy',), 'amax_in', 'in'), 'conv3x3_gn_relu_fwd': (('x',), 'amax_in', 'in'),
    'conv3x3_bias_act_fwd': (('x',), 'amax_in', 'in'), 'conv3x3_dgrad_act': (('dy',), 'amax_in', 'in'),
    'conv3x3_pair_fwd': (('x',), 'amax_in', 'in'), 'conv3x3_wino': (('x',), 'amax_in', 'in'),
    'conv3x3_pair_dgrad': (('dy1', 'dy2'), 'amax_in', 'pair'),
    'conv3x3_wgrad': (('dy', 'x'), 'amax', 'wgrad'), 'deconv5x5s2_wgrad': (('dy', 'x'), 'amax', 'wgrad'),
    'conv5x5_wgrad': (('a', 'b'), 'amax', 'wgrad'),
}
# consumer entry points each family must hand at least one handle to
EXPECT_HANDED = {
    'v2_metric_b32': ('conv3x3_gn_relu_fwd', 'conv3x3_wgrad', 'deconv5x5s2_wgrad', 'conv3x3_pair_dgrad'),
    'v2_cfg5_b32': ('conv3x3_gn_relu_fwd', 'conv3x3_wgrad', 'deconv5x5s2_wgrad', 'conv3x3_pair_dgrad'),
    'genesis_cfg3_b32': ('conv5x5_wgrad',),
    'monet_cfg4_b32': ('conv3x3_bias_act_fwd', 'conv3x3_dgrad_act', 'conv3x3_wgrad'),
}


def _union_max(hs):
    vs = [hip.amax_values(h) for h in hs]
    for v in vs:
        assert bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0, 'a handed partial is not a written maximum'
    return max(float(v.max()) for v in vs)


@pytest.mark.parametrize('case', sorted(EXPECT_HANDED))
def test_a_training_step_hands_every_operand_its_own_maxima(case, monkeypatch):
    from tests.test_fullbatch_gpu import Full
    took, own = defaultdict(int), defaultdict(int)
    floats = [0]

    def audited(fname, fn):
        names, hint, kind = AUDITED[fname]
        sig = inspect.signature(fn)

        def wrapper(*a, **k):
            ba = sig.bind(*a, **k)
            h = ba.arguments.get(hint)
            ops = [ba.arguments[n] for n in names]
            groups = None
            if h is not None:
                if kind == 'in':
                    hs = list(h) if isinstance(h, (list, tuple)) else [h]
                    groups = [(hs, ops[0])]
                elif kind == 'pair':
                    groups = [([h[0]], ops[0]), ([h[1]], ops[1])]
                else:
                    groups = [(list(x) if isinstance(x, (list, tuple)) else [x], t) for x, t in zip(h, ops)]
                if any(x is None for hs, _ in groups for x in hs):
                    groups = None
            if groups is None:
                own[fname] += 1
            else:
                took[fname] += 1
                for hs, t in groups:
                    assert _union_max(hs) == float(t.abs().max()), (case, fname, [x.n for x in hs])
            return fn(*a, **k)
        return wrapper
    for fname in AUDITED:
        monkeypatch.setattr(hip, fname, audited(fname, getattr(hip, fname)))
    real_scratch, real_end = hip._amax_scratch, hip._tap_end

    def scratch(device, n):
        floats[0] += (n + 3) & ~3
        return real_scratch(device, n)

    def tap_end(tap):
        if tap is None:
            return real_end(tap)
        a, before = tap[1], tap[1][2]
        real_end(tap)
        floats[0] += a[2] - before          # (the unused part of the request goes back)
    monkeypatch.setattr(hip, '_amax_scratch', scratch)
    monkeypatch.setattr(hip, '_tap_end', tap_end)
    gold = Full(case)
    model = gold.build()
    x, nz = gold.x(), gold.noise()
    hip.take_amax()
    out = gold.forward(model, x, nz)
    err, kl = gold.aggregate(out[1])
    (err + kl).backward()
    hip.defer_flush()
    torch.cuda.synchronize()
    print('%s: arena floats per step %d of %d' % (case, floats[0], hip._ARENA_FLOATS))
    for fname in sorted(set(took) | set(own)):
        print('%s: %-22s handed %4d, own pass %4d' % (case, fname, took[fname], own[fname]))
    assert floats[0] < hip._ARENA_FLOATS // 4, floats[0]
    for fname in EXPECT_HANDED[case]:
        assert took[fname] > 0, (case, fname, dict(took), dict(own))
