"""genesis_amd.image_quality on the device (gx_image_quality: MSE, RMSE, PSNR and Gaussian-window SSIM per image, one launch per
batch, fp64 throughout) against the fp64 numpy restatement in tests/image_quality_restatement.py, whose window is ONE 2-D
correlation (scipy), not the kernel's two separable passes.

Bars, derived: both sides are fp64 from the same fp32 values and differ only in summation order.
    mse (and rmse)  relative 1e-10: N <= 49 152 terms, worst case N 2^-53 ~ 5e-12.
    ssim            absolute 1e-10: reordering ~121 products of magnitude <= L^2 moves a variance term by <= ~1e-14 L^2 against
                    denominators >= C2 = 9e-4 L^2, ~1e-11.
    psnr            absolute 1e-9 dB.
The kernel's tile is 16 x 16 valid positions (include/genesis_hip.h); with the 11-tap window, valid extents of 16, 17 and 31 are
sides of 26, 27 and 41."""
import numpy as np
import pytest
import torch

from tests import image_quality_restatement as IR

pytestmark = pytest.mark.gpu

T = 16
KEYS = ('mse', 'rmse', 'psnr', 'ssim')
_cache = {}


def pair(shape, seed=0, kind='noisy'):
    """(pred, target) fp32 numpy, and their restated rows [B, 4] for the default window -- computed once per case, never changed."""
    key = (tuple(shape), seed, kind)
    if key not in _cache:
        pred, target = IR.make_pair(shape, seed) if kind == 'noisy' else IR.make_pair(shape, seed, noise=1e-3, clip=False)
        pred.setflags(write=False)
        target.setflags(write=False)
        _cache[key] = (pred, target, {})
    return _cache[key]


def want_rows(shape, seed=0, kind='noisy', L=1.0, win=11, sigma=1.5):
    pred, target, memo = pair(shape, seed, kind)
    k = (L, win, sigma)
    if k not in memo:
        memo[k] = IR.rows(pred, target, L, win, sigma)
        memo[k].setflags(write=False)
    return memo[k]


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def check_rows(got, want, what=''):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err = dict(mse=np.abs(got[:, 0] - want[:, 0]) / want[:, 0], rmse=np.abs(got[:, 1] - want[:, 1]) / want[:, 1],
               psnr=np.abs(got[:, 2] - want[:, 2]), ssim=np.abs(got[:, 3] - want[:, 3]))
    print(what, {k: float(v.max()) for k, v in err.items()})
    assert err['mse'].max() <= 1e-10, (what, err['mse'])
    assert err['rmse'].max() <= 1e-10, (what, err['rmse'])
    assert err['psnr'].max() <= 1e-9, (what, err['psnr'])
    assert err['ssim'].max() <= 1e-10, (what, err['ssim'])


def run_rows(pred, target, **kw):
    from genesis_amd.image_quality import image_quality
    rows = image_quality(pred, target, **kw)
    assert rows.dtype == torch.float64 and rows.is_cuda and rows.shape == (pred.shape[0], 4)
    return rows.cpu().numpy()


SHAPES = [(1, 1, 11, 11),                         # a single valid position
          (3, 3, 13, 29),                         # ragged, W % 4 != 0: the 4-byte loads
          (2, 3, 64, 64), (2, 3, 128, 128),       # the models' sizes
          (2, 1, 40, 76),
          (1, 2, T + 10, 12), (1, 2, T + 11, 12), (1, 2, 2 * T + 9, 12),       # valid extent T, T + 1, 2T - 1 in H
          (1, 2, 12, T + 10), (1, 2, 12, T + 11), (1, 2, 12, 2 * T + 9),       # ... and in W (the 16-byte loads at 12 x 28)
          (1, 1, 2 * T + 9, 2 * T + 10)]          # both at once: 2 x 2 tiles, the last ones ragged and full


@pytest.mark.parametrize('kind', ['noisy', 'near'])
@pytest.mark.parametrize('shape', SHAPES)
def test_rows_against_the_restatement(shape, kind):
    pred, target, _ = pair(shape, 3, kind)
    got = run_rows(dev(pred), dev(target))
    check_rows(got, want_rows(shape, 3, kind), '%s %s' % (shape, kind))
    if kind == 'near' and min(shape[2:]) >= 40:
        assert got[:, 3].min() > 0.9999                                   # the pair that stresses the cancellation in sigma


@pytest.mark.parametrize('win,sigma', [(3, 1.5), (7, 1.5), (11, 0.8), (5, 2.25)])
def test_window_sizes_and_sigma(win, sigma):
    shape = (2, 2, 8, 9) if win < 11 else (2, 2, 17, 20)
    pred, target, _ = pair(shape, 4)
    check_rows(run_rows(dev(pred), dev(target), win_size=win, sigma=sigma), want_rows(shape, 4, win=win, sigma=sigma),
               'win %d sigma %g' % (win, sigma))


def test_one_shot_psnr_and_ssim():
    from genesis_amd.image_quality import psnr, ssim
    shape = (3, 3, 13, 29)
    pred, target, _ = pair(shape, 3)
    want = want_rows(shape, 3)
    p, s = psnr(dev(pred), dev(target)), ssim(dev(pred), dev(target))
    assert p.shape == s.shape == (3,) and p.dtype == s.dtype == torch.float64 and p.is_cuda
    assert np.abs(p.cpu().numpy() - want[:, 2]).max() <= 1e-9 and np.abs(s.cpu().numpy() - want[:, 3]).max() <= 1e-10


def test_views_are_read_in_place_and_the_rest_is_copied():
    from genesis_amd.image_quality import _image_view
    shape = (3, 2, 16, 20)
    pred, target, _ = pair(shape, 5)
    want = want_rows(shape, 5)
    base = run_rows(dev(pred), dev(target))
    check_rows(base, want, 'contiguous')
    # images contiguous, image stride > C H W (a multiple of 4, then not): read in place
    for extra in (8, 3):
        big = torch.full((3, 2 * 16 * 20 + extra), float('nan'), device='cuda')
        view = big[:, :2 * 16 * 20].view(3, 2, 16, 20)
        view.copy_(dev(pred))
        assert view.stride(0) == 2 * 16 * 20 + extra and not view.is_contiguous()
        assert _image_view(view)[0] is view and _image_view(view)[1] == view.stride(0)
        assert np.array_equal(run_rows(view, dev(target)), base), extra
        assert np.array_equal(run_rows(dev(target), view), run_rows(dev(target), dev(pred))), extra
    # an odd element offset of a larger buffer: 4-byte loads, the same bits
    flat = torch.zeros(pred.size + 1, device='cuda')
    flat[1:].copy_(dev(pred).reshape(-1))
    assert np.array_equal(run_rows(flat[1:].view(shape), dev(target)), base)
    # not contiguous inside an image: the copy path
    wide = torch.zeros(3, 2, 16, 40, device='cuda')
    wide[:, :, :, ::2] = dev(pred)
    strided = wide[:, :, :, ::2]
    assert _image_view(strided)[0] is not strided
    assert np.array_equal(run_rows(strided, dev(target)), base)
    perm = dev(pred).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                  # channels last
    assert np.array_equal(run_rows(perm, dev(target)), base)
    expanded = dev(target)[:1].expand(3, -1, -1, -1)                                       # image stride 0
    assert np.array_equal(run_rows(dev(pred), expanded), run_rows(dev(pred), expanded.contiguous()))


def test_closed_forms_on_the_device():
    _, target, _ = pair((2, 3, 20, 24), 6)
    r = run_rows(dev(target), dev(target))
    assert np.abs(r[:, 3] - 1.0).max() <= 1e-12 and np.all(r[:, 0] == 0) and np.all(r[:, 1] == 0) and np.all(np.isposinf(r[:, 2]))
    c1, c2 = 0.25, 0.75
    a, b = torch.full((2, 2, 18, 21), c1, device='cuda'), torch.full((2, 2, 18, 21), c2, device='cuda')
    r = run_rows(a, b)
    want = (2 * c1 * c2 + 1e-4) / (c1 * c1 + c2 * c2 + 1e-4)
    assert np.abs(r[:, 3] - want).max() <= 1e-11
    assert np.all(r[:, 0] == 0.25) and np.all(r[:, 1] == 0.5) and np.abs(r[:, 2] - 10 * np.log10(4.0)).max() <= 1e-12
    # data_range = 2 with both images doubled (exact in fp32): the same ssim and psnr
    pred, target, _ = pair((2, 3, 20, 24), 6)
    one = run_rows(dev(pred), dev(target))
    two = run_rows(dev(pred) * 2, dev(target) * 2, data_range=2.0)
    assert np.abs(two[:, 3] - one[:, 3]).max() <= 1e-12
    assert np.abs(two[:, 2] - one[:, 2]).max() <= 1e-9
    np.testing.assert_allclose(two[:, 0], 4 * one[:, 0], rtol=1e-14)


def test_rows_are_deterministic_and_independent_of_the_batch():
    shape = (5, 3, 40, 44)
    pred, target, _ = pair(shape, 7)
    p, t = dev(pred), dev(target)
    first = run_rows(p, t)
    assert np.array_equal(first, run_rows(p, t))
    alone = run_rows(p[3:4].clone(), t[3:4].clone())
    assert np.array_equal(alone[0], first[3])
    assert np.array_equal(run_rows(p[3:4], t[3:4])[0], first[3])          # (the same image as a view at an offset)


def test_accumulation_over_batches():
    from genesis_amd._lib import GenesisHipError
    from genesis_amd.image_quality import ImageQuality
    shape = (8, 3, 18, 22)
    pred, target, _ = pair(shape, 8)
    want = want_rows(shape, 8)
    p, t = dev(pred), dev(target)
    iq = ImageQuality(keep_per_image=6)
    with pytest.raises(GenesisHipError, match='no batch was seen'):
        iq.compute()
    for lo, hi in ((0, 4), (4, 5), (5, 8)):
        iq.update(p[lo:hi], t[lo:hi])
    out = iq.compute()
    assert out['num_images'] == 8 and out['num_batches'] == 3
    assert all(isinstance(out[k], float) for k in KEYS)
    check_rows([[out[k] for k in KEYS]], [want.mean(0)], 'means over 8 images')
    per = np.stack([out['per_image'][k] for k in KEYS], 1)
    assert per.shape == (6, 4) and per.dtype == np.float64
    assert np.array_equal(per, run_rows(p, t)[:6])                        # the first six rows, in order, bit for bit
    iq.reset()
    with pytest.raises(GenesisHipError, match='no batch was seen'):
        iq.compute()
    iq.update(p[:2], t[:2])
    again = iq.compute()
    assert again['num_images'] == 2 and again['num_batches'] == 1 and len(again['per_image']['ssim']) == 2
    check_rows([[again[k] for k in KEYS]], [want[:2].mean(0)], 'after reset')
    plain = ImageQuality()
    plain.update(p, t)
    assert 'per_image' not in plain.compute()


def test_update_refuses_what_it_cannot_read():
    from genesis_amd._lib import GenesisHipError
    from genesis_amd.image_quality import ImageQuality
    a = torch.zeros(2, 3, 16, 16, device='cuda')
    iq = ImageQuality()
    for bad, match in (((a, a[:1]), 'differ in shape'), ((a.double(), a.double()), 'fp32'), ((a, a.cpu()), 'no CPU path'),
                       ((a[:, :, :10], a[:, :, :10]), 'below win_size')):
        with pytest.raises(GenesisHipError, match=match):
            iq.update(*bad)
    with pytest.raises(GenesisHipError, match='no batch was seen'):
        iq.compute()


def test_update_makes_no_host_read():
    """update() under torch's sync debug mode 'error', which turns every synchronising call into an exception (a build without
    that mode would capture one update in a graph instead: a capture admits no host read either)."""
    from genesis_amd.image_quality import ImageQuality
    shape = (3, 3, 16, 20)
    pred, target, _ = pair(shape, 9)
    p, t = dev(pred), dev(target)
    iq = ImageQuality(keep_per_image=6)
    iq.update(p, t)                                                      # (allocations made up front)
    iq.reset()
    torch.cuda.synchronize()
    supported = True
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()
            supported = False                                            # the mode did not catch a plain host read
        except RuntimeError:
            pass
        if supported:
            iq.update(p, t)
            iq.update(p[1:], t[1:])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not supported:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            iq.update(p, t)
        graph.replay()
        iq.update(p[1:], t[1:])
    out = iq.compute()
    assert out['num_batches'] == 2 and out['num_images'] == 5
    want = want_rows(shape, 9)
    check_rows([[out[k] for k in KEYS]], [np.concatenate([want, want[1:]]).mean(0)], 'two updates')


def test_nan_and_inf():
    from genesis_amd.image_quality import ImageQuality
    shape = (4, 2, 30, 33)
    pred, target, _ = pair(shape, 10)
    clean = run_rows(dev(pred), dev(target))
    bad = np.array(pred)
    bad[2, 1, 17, 29] = np.nan                                           # inside the second column of tiles
    r = run_rows(dev(bad), dev(target))
    assert np.all(np.isnan(r[2]))
    assert np.array_equal(r[[0, 1, 3]], clean[[0, 1, 3]])
    bad = np.array(pred)
    bad[0, 0, 29, 32] = np.nan                                           # the last pixel: under one window position only
    r = run_rows(dev(bad), dev(target))
    assert np.all(np.isnan(r[0])) and np.array_equal(r[1:], clean[1:])
    same = np.array(pred)
    same[1] = target[1]
    iq = ImageQuality(keep_per_image=4)
    iq.update(dev(same), dev(target))
    out = iq.compute()
    assert np.isposinf(out['per_image']['psnr'][1]) and out['per_image']['ssim'][1] == pytest.approx(1.0, abs=1e-12)
    assert np.array_equal(np.stack([out['per_image'][k] for k in KEYS], 1)[[0, 2, 3]], clean[[0, 2, 3]])
    assert np.isposinf(out['psnr']) and all(np.isfinite(out[k]) for k in ('mse', 'rmse', 'ssim'))


# ---- evaluation(): a stub model whose forward hands out recorded reconstructions and losses ------------------------------------
class QualityStub:
    def __init__(self, recons, losses):
        self.recons, self.losses, self.calls, self.training = recons, losses, 0, True
        self.param = torch.nn.Parameter(torch.zeros(1, device='cuda'))

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def parameters(self):
        return iter([self.param])

    def __call__(self, x):
        i, self.calls = self.calls, self.calls + 1
        return self.recons[i], {k: v[i] for k, v in self.losses.items()}, {}, None, None


def _eval_case():
    from tests import evaluation_stub as S
    shape = (8, 3, 16, 16)
    pred, target, _ = pair(shape, 11)
    g = torch.Generator().manual_seed(11)
    losses = {'err': (torch.rand(2, 4, generator=g) * 100).cuda(), 'kl_l': torch.rand(2, 4, generator=g).cuda()}
    recons = [dev(pred[:4]), dev(pred[4:])]
    loader = S.Loader([{'input': dev(target[:4])}, {'input': dev(target[4:])}], 4)
    return QualityStub(recons, losses), loader, want_rows(shape, 11).mean(0)


def test_evaluation_with_image_quality():
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd.evaluate import evaluation, reconstruction_quality_from_model
    from tests import evaluation_stub as S
    config = AttrDict(debug=False, gpu=True)
    model, loader, want = _eval_case()
    plain = evaluation(model, loader, None, config, 1)
    assert list(plain) == ['err', 'kl_l', 'elbo', 'err_element', 'duration', 'num_batches']       # exactly today's keys
    model, loader, want = _eval_case()
    writer = S.Writer()
    ret = evaluation(model, loader, writer, config, 1, image_quality=True)
    assert list(ret) == ['err', 'kl_l', 'elbo', 'err_element', 'mse', 'rmse', 'psnr', 'ssim', 'duration', 'num_batches']
    assert all(isinstance(v, float) for v in ret.values())
    for key in ('err', 'kl_l', 'elbo', 'err_element'):
        assert ret[key] == plain[key], key
    check_rows([[ret[k] for k in KEYS]], [want], 'evaluation')
    assert [c[0] for c in writer.calls] == ['val/' + k for k in ret]
    assert [c[1] for c in writer.calls] == [ret[k] for k in ret]
    assert model.training and model.calls == 2 and torch.is_grad_enabled()
    model, loader, want = _eval_case()
    out = reconstruction_quality_from_model(model, list(loader), keep_per_image=3)
    assert [out[k] for k in KEYS] == [ret[k] for k in KEYS]
    assert out['num_images'] == 8 and out['num_batches'] == 2 and len(out['per_image']['psnr']) == 3
    assert not model.training
    # data_range reaches the kernel: psnr moves by 20 log10(2), mse does not
    model, loader, want = _eval_case()
    wide = evaluation(model, loader, None, config, 1, image_quality=True, data_range=2.0)
    assert wide['mse'] == ret['mse'] and abs(wide['psnr'] - ret['psnr'] - 20 * np.log10(2.0)) <= 1e-9
