"""The packed-weight cache serves what a call would have packed itself, for every pack descriptor (genesis_amd/csrc/gx_pack.h).

Per case: the conv entry points are called once with no cache (each packs its weights into its workspace:
pack_weights_kernel), then again on the same inputs with a cache recorded, refreshed and active (every packing made by
ONE launch of pack_weights_batch_kernel, the trailers by pack_amax_batch_kernel).  The outputs must be bit-equal and the
cache must hold exactly the distinct (weight, view, form) packings of the calls.  The settings walk the forms: the three
levels of gx_matmul_precision and the 16-bit families' six-bf16-product mode, gx_tapconv_precision 0 and 3, and the Winograd
layer with and without its input's maxima handed in (gx_conv_input_amax: two fp16 pieces).  The dispatch policies send the
small shapes of tests/test_matmul_precision_gpu.py / test_tapconv_precision_gpu.py to each kernel family."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) * 2 - 1) * scale).to(DEV)


def _amax_parts(t):
    """16 partial maxima of t, as a norm kernel would hand them to the next conv."""
    return t.abs().max().reshape(1).repeat(16).contiguous()


def _conv3x3(N, Cin, Cout, H, W, armed=False, bias_act=True, dgrad_act=False):
    """forward, bias + ELU forward (not in the Winograd cases: the Winograd kernel has no epilogue, so that call would pack a third
    form), data gradient (and the data gradient through a ReLU layer where the 16-bit pipe takes it): two packings -- the forward
    view and the data-gradient view of w."""
    from genesis_amd import hip_ops as hip, _lib
    x, w, b = rnd(N, Cin, H, W, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=0.1), rnd(Cout, seed=3)
    dy, xout = rnd(N, Cout, H, W, seed=4), torch.relu(rnd(N, Cin, H, W, seed=5))
    px, pdy = _amax_parts(x), _amax_parts(dy)

    def arm(p):
        if armed:
            _lib.call('gx_conv_input_amax', p.data_ptr(), 16, None, 0)

    def run():
        out = []
        arm(px); out.append(hip.conv3x3_fwd(x, w))
        if bias_act:
            out.append(hip.conv3x3_bias_act_fwd(x, w, b, 'elu'))
        arm(pdy); out.append(hip.conv3x3_dgrad(dy, w))
        if dgrad_act and hip.conv3x3_dgrad_act_supported(N, Cin, Cout, H, W):
            out.append(hip.conv3x3_dgrad_act(dy, w, xout, 'relu')[0])
        _lib.call('gx_conv_input_amax', None, 0, None, 0)
        return out
    return run, 2


def _deconv(N, Cin, Cout, Hin, Win):
    """forward (two packings: the row parities) and data gradient (one)."""
    from genesis_amd import hip_ops as hip
    x, w, b = rnd(N, Cin, Hin, Win, seed=11), rnd(Cin, Cout, 5, 5, seed=12, scale=0.05), rnd(Cout, seed=13, scale=0.3)
    dy = rnd(N, Cout, 2 * Hin, 2 * Win, seed=14)
    return (lambda: [hip.deconv5x5s2_fwd(x, w, b), hip.deconv5x5s2_dgrad(dy, w)]), 3


def _conv5x5(N, K, M, S):
    """flip 0 and flip 1, each with a weight of its own: two packings."""
    from genesis_amd import hip_ops as hip
    x, w0, w1 = rnd(N, K, S, S, seed=21), rnd(M, K, 5, 5, seed=22, scale=0.1), rnd(K, M, 5, 5, seed=23, scale=0.1)
    return (lambda: [hip.conv5x5s1(x, w0, M, False), hip.conv5x5s1(x, w1, M, True)]), 2


# (kq policy, Winograd policy): 0 off, 2 every eligible shape
KQ, WINO, TAP = (2, 0), (0, 2), (0, 0)
MATMUL = [('matmul', 0), ('matmul', 1), ('matmul', 2), ('kq', 1)]
CASES = {
    # the <= 32-output-channel kernel (level 0: the fp32 k-quad or tap kernels)
    'conv3x3_kq': (lambda: _conv3x3(4, 32, 7, 16, 16, dgrad_act=True), KQ, MATMUL),
    # ... with both channel counts multiples of 16, so that the data gradient and gx_conv3x3_dgrad_act take it too
    'conv3x3_kq_16': (lambda: _conv3x3(5, 16, 16, 40, 24, dgrad_act=True), KQ, MATMUL),
    # Winograd: fp32 pipe, three bf16 pieces, one bf16 piece -- and two fp16 pieces with the input's maxima armed
    'conv3x3_wino': (lambda: _conv3x3(2, 16, 16, 8, 16, bias_act=False), WINO, [('matmul', 0), ('matmul', 1), ('matmul', 2)]),
    'conv3x3_wino_armed': (lambda: _conv3x3(2, 16, 16, 8, 16, armed=True, bias_act=False), WINO, [('matmul', 1)]),
    'conv3x3_wino_wide': (lambda: _conv3x3(3, 24, 40, 32, 32, bias_act=False), WINO, [('matmul', 1)]),
    # the tap-conv kernels: fp32 and one bf16 piece (odd H / W; a grid that splits the channel reduction)
    'conv3x3_tap': (lambda: _conv3x3(3, 40, 24, 9, 12), TAP, [('tap', 0), ('tap', 3)]),
    'conv3x3_tap_split': (lambda: _conv3x3(2, 256, 64, 4, 4), TAP, [('tap', 0), ('tap', 3)]),
    'deconv_kq': (lambda: _deconv(8, 64, 64, 16, 16), KQ, MATMUL),
    'deconv_tap': (lambda: _deconv(3, 24, 40, 7, 4), TAP, [('tap', 0), ('tap', 3)]),
    'conv5x5_kq': (lambda: _conv5x5(2, 32, 64, 16), KQ, MATMUL),
    'conv5x5_tap': (lambda: _conv5x5(2, 24, 40, 8), TAP, [('tap', 0), ('tap', 3)]),
}
PARAMS = [(name, s) for name in sorted(CASES) for s in CASES[name][2]]


class settings(object):
    """with settings(policy, (family, mode)): the dispatch policies and one precision switch set; everything restored."""

    def __init__(self, policy, setting):
        self.policy, self.setting = policy, setting

    def __enter__(self):
        from genesis_amd import _lib
        L = _lib.load()
        _lib.call('gx_kq_policy', self.policy[0])
        _lib.call('gx_conv3x3_wino_policy', self.policy[1])
        fam, mode = self.setting
        self.tap_prev = int(L.gx_tapconv_precision_get())
        if fam == 'tap':
            L.gx_tapconv_precision(mode)
        elif fam == 'matmul':
            L.gx_matmul_precision(mode)                  # (returns the previous level)
            assert int(L.gx_matmul_precision_get()) == mode
        else:
            _lib.call('gx_%s_precision' % fam, mode)

    def __exit__(self, *a):
        from genesis_amd import _lib
        L = _lib.load()
        L.gx_matmul_precision(-1)
        L.gx_tapconv_precision(self.tap_prev)
        _lib.call('gx_kq_policy', 1)
        _lib.call('gx_conv3x3_wino_policy', 1)
        _lib.call('gx_conv_input_amax', None, 0, None, 0)


def run_case(name, setting):
    """(outputs with no cache, outputs served from a refreshed cache, packings in the cache, packings expected)."""
    from genesis_amd import hip_ops as hip, _lib
    make, policy, _ = CASES[name]
    with settings(policy, setting):
        run, npack = make()
        plain = [t.clone() for t in run()]
        cid = int(_lib.query('gx_weight_cache_create'))
        try:
            _lib.call('gx_weight_cache_record', cid, 1)
            try:
                run()
            finally:
                _lib.call('gx_weight_cache_record', cid, 0)
            size = int(_lib.query('gx_weight_cache_size', cid))
            _lib.call('gx_weight_cache_refresh', cid, hip._stream())
            try:
                served = [t.clone() for t in run()]
            finally:
                _lib.call('gx_weight_cache_release')
            torch.cuda.synchronize()
        finally:
            _lib.call('gx_weight_cache_destroy', cid)
    return plain, served, size, npack


@pytest.mark.parametrize('name,setting', PARAMS, ids=['%s-%s%d' % (n, s[0], s[1]) for n, s in PARAMS])
def test_cache_served_packing_equals_per_call_packing(name, setting):
    plain, served, size, npack = run_case(name, setting)
    assert size == npack, (name, setting, size, npack)
    assert len(plain) == len(served) and len(plain) >= 2
    if name == 'conv3x3_kq_16' and setting != ('matmul', 0):
        assert len(plain) == 4, 'gx_conv3x3_dgrad_act did not take the shape'
    for i, (a, b) in enumerate(zip(plain, served)):
        assert torch.isfinite(a).all(), (name, setting, i)
        assert torch.equal(a, b), (name, setting, i, float((a - b).abs().max()))
