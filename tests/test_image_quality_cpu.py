"""Reconstruction quality without a GPU: the fp64 restatement (tests/image_quality_restatement.py) against a direct double loop and
against closed forms, genesis_amd.image_quality.gaussian_window against the formula, and every refusal of gx_image_quality and of
ImageQuality.update that is reachable before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd._lib import GenesisHipError
from tests import image_quality_restatement as IR


def test_restatement_agrees_with_the_double_loop():
    pred, target = IR.make_pair((12, 13), seed=1)
    got, want = IR.ssim_map(pred, target), IR.ssim_direct(pred, target)
    assert got.shape == want.shape == (2, 3)
    assert np.abs(got - want).max() <= 1e-13
    got, want = IR.ssim_map(pred, target, 1.0, 5, 0.8), IR.ssim_direct(pred, target, 1.0, 5, 0.8)
    assert got.shape == (8, 9) and np.abs(got - want).max() <= 1e-13


@pytest.mark.parametrize('n,sigma', [(11, 1.5), (3, 1.5), (7, 0.9), (5, 2.5)])
def test_gaussian_window(n, sigma):
    from genesis_amd.image_quality import gaussian_window
    g = gaussian_window(n, sigma)
    assert g.dtype == np.float64 and g.shape == (n,)
    assert abs(g.sum() - 1.0) <= 2.0 ** -52
    assert np.array_equal(g, g[::-1])
    raw = np.array([np.exp(-(i - (n - 1) / 2.0) ** 2 / (2.0 * sigma ** 2)) for i in range(n)])
    np.testing.assert_allclose(g, raw / raw.sum(), rtol=4e-16, atol=0)
    np.testing.assert_allclose(g, IR.window(n, sigma), rtol=4e-16, atol=0)


def test_gaussian_window_defaults_and_refusals():
    from genesis_amd.image_quality import gaussian_window
    assert np.array_equal(gaussian_window(), gaussian_window(11, 1.5))
    for bad in (2, 4, 1, 13, 5.5):
        with pytest.raises(GenesisHipError, match='win_size'):
            gaussian_window(bad)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(GenesisHipError, match='sigma'):
            gaussian_window(11, bad)


def test_closed_forms_through_the_restatement():
    _, target = IR.make_pair((2, 3, 14, 15), seed=2)
    r = IR.rows(target, target)
    assert np.abs(r[:, 3] - 1.0).max() <= 1e-12
    assert np.all(r[:, 0] == 0.0) and np.all(r[:, 1] == 0.0) and np.all(np.isposinf(r[:, 2]))
    c1, c2 = 0.25, 0.75
    a, b = np.full((1, 2, 12, 16), c1, np.float32), np.full((1, 2, 12, 16), c2, np.float32)
    for L in (1.0, 2.0):
        C1 = (0.01 * L) ** 2
        want = (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)
        assert abs(IR.ssim(a, b, L)[0] - want) <= 1e-11
    assert IR.mse(a, b)[0] == 0.25 and IR.rmse(a, b)[0] == 0.5
    assert abs(IR.psnr(a, b)[0] - 10.0 * np.log10(4.0)) <= 1e-12


P = ctypes.c_void_p(64)      # a non-null, aligned address: the refusals come before anything is dereferenced


def _call(**over):
    a = dict(pred=P, ps=3 * 16 * 16, target=P, ts=3 * 16 * 16, B=2, C=3, H=16, W=16,
             window=np.ascontiguousarray(IR.window()).ctypes.data_as(ctypes.c_void_p), win=11, L=1.0, rows=P, acc=P, state=P,
             log=None, cap=0, ws=P, ws_bytes=1 << 20)
    a.update(over)
    _lib.call('gx_image_quality', a['pred'], a['ps'], a['target'], a['ts'], a['B'], a['C'], a['H'], a['W'], a['window'], a['win'],
              ctypes.c_double(a['L']), a['rows'], a['acc'], a['state'], a['log'], a['cap'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('over,match', [
    (dict(pred=None), 'pred or target'), (dict(target=None), 'pred or target'), (dict(window=None), 'window'),
    (dict(rows=None), 'rows, acc or state'), (dict(acc=None), 'rows, acc or state'), (dict(state=None), 'rows, acc or state'),
    (dict(ws=None), 'ws is a null'),
    (dict(win=10), 'win = 10'), (dict(win=1), 'win = 1'), (dict(win=13, H=32, W=32), 'win = 13'),
    (dict(H=10), 'H = 10'), (dict(W=10), 'W = 10'), (dict(H=4097, ps=1 << 30, ts=1 << 30), 'H = 4097'),
    (dict(W=4097, ps=1 << 30, ts=1 << 30), 'W = 4097'),
    (dict(B=0), 'B = 0'), (dict(C=0), 'C = 0'),
    (dict(L=0.0), 'data_range'), (dict(L=-1.0), 'data_range'), (dict(L=float('inf')), 'data_range'),
    (dict(L=float('nan')), 'data_range'),
    (dict(ws_bytes=2 * 16 - 1), 'ws_bytes'),
    (dict(ps=3 * 16 * 16 - 1), 'pred_image_stride'), (dict(ts=3 * 16 * 16 - 1), 'target_image_stride'),
    (dict(log=P, cap=-1), 'log_capacity'),
])
def test_gx_image_quality_refusals_need_no_gpu(over, match):
    with pytest.raises(GenesisHipError, match=match):
        _call(**over)


def test_workspace_query():
    # two doubles per 16 x 16 tile of valid positions: 64 - 10 = 54 -> 4 x 4 tiles; 128 - 10 = 118 -> 8 x 8
    assert _lib.query('gx_image_quality_ws_bytes', 32, 3, 64, 64, 11) == 32 * 16 * 16
    assert _lib.query('gx_image_quality_ws_bytes', 32, 3, 128, 128, 11) == 32 * 64 * 16
    assert _lib.query('gx_image_quality_ws_bytes', 1, 1, 11, 11, 11) == 16
    assert _lib.query('gx_image_quality_ws_bytes', 1, 1, 26, 27, 11) == 2 * 16       # valid 16 x 17
    assert _lib.query('gx_image_quality_ws_bytes', 1, 1, 10, 11, 11) == 0            # refused shapes need nothing
    assert _lib.query('gx_image_quality_ws_bytes', 1, 1, 16, 16, 4) == 0


def test_update_refusals_on_host_tensors():
    from genesis_amd.image_quality import ImageQuality, image_quality
    a = torch.zeros(2, 3, 16, 16)
    iq = ImageQuality()
    with pytest.raises(GenesisHipError, match='differ in shape'):
        iq.update(a, a[:1])
    with pytest.raises(GenesisHipError, match=r'\[B, C, H, W\]'):
        iq.update(a[0], a[0])
    with pytest.raises(GenesisHipError, match='fp32'):
        iq.update(a.double(), a.double())
    with pytest.raises(GenesisHipError, match='fp32'):
        iq.update(a, a.half())
    with pytest.raises(GenesisHipError, match='below win_size'):
        iq.update(a[:, :, :10], a[:, :, :10])
    with pytest.raises(GenesisHipError, match='below win_size'):
        iq.update(a[:, :, :, :10], a[:, :, :, :10])
    with pytest.raises(GenesisHipError, match='no CPU path'):
        iq.update(a, a)                                                  # host tensors: the wrong device
    with pytest.raises(GenesisHipError, match='no CPU path'):
        image_quality(a, a)
    with pytest.raises(GenesisHipError, match='no batch was seen'):
        iq.compute()
    with pytest.raises(GenesisHipError, match='no CPU path'):
        ImageQuality(device='cpu')
    with pytest.raises(GenesisHipError, match='data_range'):
        ImageQuality(data_range=0.0)
    with pytest.raises(GenesisHipError, match='win_size'):
        ImageQuality(win_size=4)
    with pytest.raises(GenesisHipError, match='keep_per_image'):
        ImageQuality(keep_per_image=-1)
    with pytest.raises(GenesisHipError, match='no CPU path'):            # (a smaller window admits the 10-pixel side)
        ImageQuality(win_size=7).update(a[:, :, :10], a[:, :, :10])


def test_evaluation_signature_is_additive():
    import inspect
    from genesis_amd import evaluate as E
    p = inspect.signature(E.evaluation).parameters
    assert list(p)[:8] == ['model', 'data_loader', 'writer', 'config', 'iter_idx', 'N_eval', 'N_seg_metrics', 'max_labels']
    assert p['image_quality'].default is False and p['data_range'].default == 1.0
    q = inspect.signature(E.reconstruction_quality_from_model).parameters
    assert [(k, v.default) for k, v in list(q.items())[2:]] == [('data_range', 1.0), ('win_size', 11), ('sigma', 1.5),
                                                               ('keep_per_image', 0)]
