"""No-GPU checks of the feeder's crop / resample transforms (genesis_amd/feeder.py transform_frames / transform_labels):
Pillow's BILINEAR coefficient tables from the C ABI (gx_pil_bilinear_coeffs, the tables the device kernel is handed), run
through a numpy restatement of Pillow's two fixed-point passes, against Pillow itself and against tests/golden/feeder_pil.npz;
centre_box against the reference's centre-crop windows; argument checks that fail without a GPU."""
import ctypes
import os.path as osp
import sys

import numpy as np
import pytest
import torch

from genesis_amd import _lib

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_feeder as MG  # noqa: E402


def coeffs(n_in, n_out):
    """The tables through the bare C ABI, as a binding author would call it."""
    lib = _lib.load()
    k = lib.gx_pil_bilinear_ksize(n_in, n_out)
    bounds = np.zeros((n_out, 2), np.int32)
    weights = np.zeros((n_out, k), np.int32)
    rc = lib.gx_pil_bilinear_coeffs(n_in, n_out, k, bounds.ctypes.data_as(ctypes.c_void_p),
                                    weights.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, _lib.last_error()
    return bounds, weights


def resample_axis(a, bounds, weights, axis):
    """One of Pillow's 8-bit passes (ImagingResampleHorizontal / Vertical_8bpc): sum from 1 << 21, >> 22, clip to uint8."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + a.shape[1:], np.int64)
    for o, (first, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << 21, np.int64)
        for t in range(n):
            acc += a[first + t] * int(weights[o, t])
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def crop_resize(frames, box, size):
    """uint8 [B, Hs, Ws, C] -> uint8 [B, H, W, C]: the crop, then the horizontal pass, then the vertical pass."""
    top, left, h, w = box
    x = frames[:, top:top + h, left:left + w]
    x = resample_axis(x, *coeffs(w, size[1]), axis=2)
    return resample_axis(x, *coeffs(h, size[0]), axis=1)


def test_tables_are_pillows_layout():
    for n_in, n_out in ((196, 64), (64, 128), (512, 32), (7, 5), (100, 100)):
        bounds, weights = coeffs(n_in, n_out)
        scale = max(n_in / n_out, 1.0)
        assert weights.shape[1] == int(np.ceil(scale)) * 2 + 1
        assert (bounds[:, 0] >= 0).all() and (bounds.sum(1) <= n_in).all()
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()   # the kernel's band rows rely on it
        for (first, n), w in zip(bounds, weights):
            assert abs(int(w[:n].sum()) - (1 << 22)) <= n and not w[n:].any()
    b, w = coeffs(100, 100)                                                               # same size: the identity
    assert (b[:, 0] == np.arange(100)).all() and (w[:, 0] == 1 << 22).all()


@pytest.mark.parametrize('case', [c[0] for c in MG.CASES])
def test_two_pass_matches_the_fixture(case):
    _, shape, box, size = [c for c in MG.CASES if c[0] == case][0]
    g = np.load(osp.join(GOLDEN, 'feeder_pil.npz'))
    frames = MG.feeder_case_frames(case)
    assert MG.checksum(frames) == g[case + '_in_crc']
    assert np.array_equal(crop_resize(frames, box, size), g[case + '_out'])


@pytest.mark.parametrize('seed', range(6))
def test_two_pass_matches_live_pillow(seed):
    pytest.importorskip('PIL')
    rng = np.random.RandomState(seed)
    Hs, Ws = rng.randint(8, 400, 2)
    C = (1, 3)[seed % 2]
    h, w = rng.randint(4, Hs + 1), rng.randint(4, Ws + 1)
    box = (rng.randint(0, Hs - h + 1), rng.randint(0, Ws - w + 1), h, w)
    size = (max(1, h // rng.randint(1, 17)) if seed < 4 else rng.randint(h, 2 * h + 1),
            max(1, w // rng.randint(1, 17)) if seed < 4 else rng.randint(w, 2 * w + 1))
    frames = rng.randint(0, 256, (2, Hs, Ws, C)).astype(np.uint8)
    want = np.stack([MG.pil_crop_resize(f, box, size) for f in frames])
    assert np.array_equal(crop_resize(frames, box, size), want), (Hs, Ws, C, box, size)


def test_fixture_is_pillows_output():
    pytest.importorskip('PIL')
    g = np.load(osp.join(GOLDEN, 'feeder_pil.npz'))
    for name, _, box, size in MG.CASES:
        frames = MG.feeder_case_frames(name)
        assert np.array_equal(np.stack([MG.pil_crop_resize(f, box, size) for f in frames]), g[name + '_out']), name


# (Hs, Ws, crop) -> the centre window (top, left, h, w) the reference's datasets cut (utils/misc.py:45-56): the offsets
# are the floor of half the margin, worked out by hand
CENTRE_WINDOWS = [((224, 224, 196), (14, 14, 196, 196)), ((240, 320, 192), (24, 64, 192, 192)),
                  ((65, 64, 32), (16, 16, 32, 32)), ((7, 9, 3), (2, 3, 3, 3)), ((64, 64, 64), (0, 0, 64, 64)),
                  ((10, 11, (4, 6)), (3, 2, 4, 6))]


@pytest.mark.parametrize('args,window', CENTRE_WINDOWS)
def test_centre_box_is_the_references_window(args, window):
    from genesis_amd.feeder import centre_box
    Hs, Ws, crop = args
    assert centre_box(Hs, Ws, crop) == window
    top, left, h, w = window
    img = np.arange(Hs * Ws).reshape(Hs, Ws)
    block = img[top:top + h, left:left + w]
    # the window is the block whose margins above / below and left / right differ by at most one, the larger below / right
    assert block.shape == (h, w)
    assert 0 <= (Hs - top - h) - top <= 1 and 0 <= (Ws - left - w) - left <= 1
    assert block[0, 0] == top * Ws + left and block[-1, -1] == (top + h - 1) * Ws + left + w - 1


def test_bad_arguments_fail_without_a_gpu():
    from genesis_amd.feeder import centre_box, transform_frames, transform_labels
    lib = _lib.load()
    p = ctypes.c_void_p(8)
    assert lib.gx_pil_bilinear_ksize(0, 64) == 0 and lib.gx_pil_bilinear_ksize(196, 64) == 9
    with pytest.raises(_lib.GenesisHipError, match='ksize'):
        _lib.call('gx_pil_bilinear_coeffs', 196, 64, 7, p, p)
    with pytest.raises(_lib.GenesisHipError, match='null pointer'):
        _lib.call('gx_pil_bilinear_coeffs', 196, 64, 9, None, p)
    with pytest.raises(_lib.GenesisHipError, match='bad sizes'):
        _lib.call('gx_pil_bilinear_coeffs', 196, 0, 9, p, p)
    # (B, Hs, Ws, C, top, left, Hc, Wc, H, W): every launch argument check runs before anything touches the device
    for dims, msg in (((2, 224, 224, 3, 14, 14, 211, 196, 64, 64), 'outside'),
                      ((2, 224, 224, 3, -1, 14, 196, 196, 64, 64), 'outside'),
                      ((2, 224, 224, 3, 14, 14, 196, 196, 0, 64), 'bad dims'),
                      ((0, 224, 224, 3, 14, 14, 196, 196, 64, 64), 'bad dims')):
        with pytest.raises(_lib.GenesisHipError, match=msg):
            _lib.call('gx_u8hwc_resample_f32chw', p, p, *dims, 1, p, p, 9, p, p, 9, None)
    with pytest.raises(_lib.GenesisHipError, match='null pointer'):
        _lib.call('gx_u8hwc_resample_f32chw', None, p, 2, 224, 224, 3, 14, 14, 196, 196, 64, 64, 0, None, None, 0, None,
                  None, 0, None)
    with pytest.raises(_lib.GenesisHipError, match='coefficient tables'):
        _lib.call('gx_u8hwc_resample_f32chw', p, p, 2, 224, 224, 3, 14, 14, 196, 196, 64, 64, 1, None, None, 9, None,
                  None, 9, None)
    with pytest.raises(_lib.GenesisHipError, match='table ksize'):
        _lib.call('gx_u8hwc_resample_f32chw', p, p, 2, 224, 224, 3, 14, 14, 196, 196, 64, 64, 1, p, p, 7, p, p, 9, None)
    with pytest.raises(_lib.GenesisHipError, match='bad mode'):
        _lib.call('gx_u8hwc_resample_f32chw', p, p, 2, 224, 224, 3, 14, 14, 196, 196, 64, 64, 2, p, p, 9, p, p, 9, None)
    with pytest.raises(_lib.GenesisHipError, match='outside'):
        _lib.call('gx_labels_crop_nearest', p, 2, p, 2, 224, 224, 14, 30, 196, 196, 64, 64, None)
    with pytest.raises(_lib.GenesisHipError, match='bad dtype'):
        _lib.call('gx_labels_crop_nearest', p, 3, p, 2, 224, 224, 14, 14, 196, 196, 64, 64, None)
    with pytest.raises(_lib.GenesisHipError, match='null pointer'):
        _lib.call('gx_labels_crop_nearest', p, 0, None, 2, 224, 224, 14, 14, 196, 196, 64, 64, None)
    with pytest.raises(_lib.GenesisHipError, match='does not fit'):
        centre_box(64, 64, 65)
    with pytest.raises(_lib.GenesisHipError, match='no CPU path'):
        transform_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4)
    with pytest.raises(_lib.GenesisHipError, match='no CPU path'):
        transform_labels(torch.zeros(1, 8, 8, dtype=torch.int64), 4)
