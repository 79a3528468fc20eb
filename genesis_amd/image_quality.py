"""Reconstruction quality on the device: per-image MSE, RMSE, PSNR and the Gaussian-window SSIM of Wang et al. 2004, one
gx_image_quality launch per batch and fp64 from the fp32 load onwards (contract and tile plan: include/genesis_hip.h).

Definition, for pred / target fp32 [B, C, H, W], data range L, per image with N = C H W:
    mse  = (1 / N) sum (pred - target)^2        (train.py:244's mse_batched, in fp64)        rmse = sqrt(mse)
    psnr = 10 log10(L^2 / mse)                  (+inf when mse == 0; NaN inputs give NaN)
    ssim = mean over channels and valid window positions of
           ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)),  C1 = (0.01 L)^2, C2 = (0.03 L)^2,
           with mx = g * x, my = g * y, sx2 = g * x^2 - mx^2, sy2 = g * y^2 - my^2, sxy = g * (x y) - mx my and g the outer product
           of gaussian_window(win_size, sigma) with itself, "valid" correlation only ((H - n + 1) x (W - n + 1) positions, no padding).
This is the convention of tf.image.ssim, pytorch-msssim's ssim and skimage's structural_similarity(gaussian_weights=True,
use_sample_covariance=False) -- by definition; none of them was run against it.

`ImageQuality` mirrors genesis_amd.metrics.SegMetrics: the running sums stay on the device until `compute()`."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GenesisHipError

KEYS = ('mse', 'rmse', 'psnr', 'ssim')      # columns of a gx_image_quality row


def gaussian_window(win_size=11, sigma=1.5):
    """g[i] = exp(-(i - (n - 1) / 2)^2 / (2 sigma^2)), normalised to sum 1: float64 [win_size].  The one definition that the kernel's
    argument, the documents and the tests share."""
    n = int(win_size)
    if n != win_size or n % 2 == 0 or not 3 <= n <= 11:
        raise GenesisHipError('gaussian_window: win_size = %r is not an odd integer in [3, 11]' % (win_size,))
    sigma = float(sigma)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise GenesisHipError('gaussian_window: sigma = %r is not positive and finite' % (sigma,))
    d = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    g = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return g / g.sum()


def _image_view(t):
    """(tensor to read, image stride in floats): `t` itself when its images are contiguous C H W blocks one common stride apart,
    else a contiguous copy."""
    B, C, H, W = t.shape
    chw = C * H * W
    if t.stride()[1:] == (H * W, W, 1) and (B == 1 or t.stride(0) >= chw):
        return t, (t.stride(0) if B > 1 else chw)
    return t.contiguous(), chw


class _Launcher:
    """The checks, the window and the workspace that ImageQuality and the one-shot functions share.  Nothing here touches the
    device before check() has passed, so every refusal is raised on a machine without one too."""

    def __init__(self, data_range, win_size, sigma, device):
        self.data_range = float(data_range)
        if not (self.data_range > 0 and np.isfinite(self.data_range)):
            raise GenesisHipError('image quality: data_range = %r is not positive and finite' % (data_range,))
        self.window = np.ascontiguousarray(gaussian_window(win_size, sigma))
        self.win = int(win_size)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise GenesisHipError('image quality: the metrics run on the HIP device; there is no CPU path')
        self._ws = None

    def check(self, pred, target):
        if pred.shape != target.shape:
            raise GenesisHipError('image quality: pred %s and target %s differ in shape' % (tuple(pred.shape), tuple(target.shape)))
        if pred.dim() != 4:
            raise GenesisHipError('image quality: pred and target must be [B, C, H, W], got %s' % (tuple(pred.shape),))
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise GenesisHipError('image quality: pred (%s) and target (%s) must be fp32' % (pred.dtype, target.dtype))
        B, C, H, W = pred.shape
        if B < 1 or C < 1:
            raise GenesisHipError('image quality: empty batch or no channels: %s' % (tuple(pred.shape),))
        if H < self.win or W < self.win:
            raise GenesisHipError('image quality: H, W = %d, %d below win_size = %d' % (H, W, self.win))
        if not (pred.is_cuda and target.is_cuda):
            raise GenesisHipError('image quality: pred on %s and target on %s, the metrics on %s; there is no CPU path'
                                  % (pred.device, target.device, self.device))
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if pred.device != self.device or target.device != self.device:
            raise GenesisHipError('image quality: pred on %s and target on %s, the metrics on %s'
                                  % (pred.device, target.device, self.device))

    def launch(self, pred, target, rows, acc, state, log, capacity):
        B, C, H, W = pred.shape
        pred, ps = _image_view(pred)
        target, ts = _image_view(target)
        need = _lib.query('gx_image_quality_ws_bytes', B, C, H, W, self.win)
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        _lib.call('gx_image_quality', ctypes.c_void_p(pred.data_ptr()), ps, ctypes.c_void_p(target.data_ptr()), ts, B, C, H, W,
                  self.window.ctypes.data_as(ctypes.c_void_p), self.win, ctypes.c_double(self.data_range),
                  ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(state.data_ptr()),
                  ctypes.c_void_p(log.data_ptr()) if log is not None else None, capacity,
                  ctypes.c_void_p(self._ws.data_ptr()), self._ws.numel() * 8,
                  ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))


class ImageQuality:
    """MSE, RMSE, PSNR and SSIM of reconstructions, accumulated on the device: one gx_image_quality launch per `update`, no host
    read before `compute`.

    update(pred, target): fp32 [B, C, H, W] on the device, H, W >= win_size.  A view whose images are contiguous with one common
    image stride is read in place; anything else is made contiguous.
    compute(): the one host read.  dict of 'mse', 'rmse', 'psnr', 'ssim' as Python floats -- each the mean over the IMAGES seen
    ('mse' and 'rmse' are train.py:245-246's when all batches have one size; 'psnr' is inf as soon as one image is reproduced
    exactly, and a NaN pixel makes its image's values and the means NaN) --, 'num_images', 'num_batches', and with
    keep_per_image > 0 'per_image': the four keys as float64 arrays over the first keep_per_image images seen, in order.
    reset(): clears the accumulators.
    The accumulators are allocated by the first update that passes its checks."""

    def __init__(self, data_range=1.0, win_size=11, sigma=1.5, keep_per_image=0, device='cuda'):
        self.keep = int(keep_per_image)
        if self.keep < 0:
            raise GenesisHipError('ImageQuality: keep_per_image must be non-negative')
        self._launcher = _Launcher(data_range, win_size, sigma, device)
        self._acc = self._state = self._log = self._rows = None

    @property
    def device(self):
        return self._launcher.device

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()
            self._state.zero_()

    def update(self, pred, target):
        self._launcher.check(pred, target)
        if self._acc is None:
            self._acc = torch.zeros(4, dtype=torch.float64, device=self.device)
            self._state = torch.zeros(4, dtype=torch.int64, device=self.device)      # arrival counter, images, batches, log cursor
            self._log = torch.zeros(self.keep, 4, dtype=torch.float64, device=self.device) if self.keep else None
        B = pred.shape[0]
        if self._rows is None or self._rows.shape[0] < B:
            self._rows = torch.empty(B, 4, dtype=torch.float64, device=self.device)
        self._launcher.launch(pred, target, self._rows, self._acc, self._state, self._log, self.keep)

    def _parts(self):
        """What compute() needs on the host: 4 sums, 4 counters (exact in float64), the per-image log."""
        if self._acc is None:
            raise GenesisHipError('ImageQuality.compute: no batch was seen')
        return [self._acc, self._state] + ([self._log] if self.keep else [])

    def compute(self):
        return self._finish(torch.cat([t.reshape(-1).to(torch.float64) for t in self._parts()]).cpu().numpy())

    def _finish(self, host):
        """compute() on values already brought to the host (genesis_amd.evaluate fetches everything in one transfer)."""
        acc, (_, images, batches, cursor) = host[:4], (int(v) for v in host[4:8])
        if batches == 0:
            raise GenesisHipError('ImageQuality.compute: no batch was seen')
        with np.errstate(invalid='ignore'):
            out = {key: float(acc[c] / images) for c, key in enumerate(KEYS)}
        out['num_images'], out['num_batches'] = images, batches
        if self.keep:
            log = host[8:8 + 4 * self.keep].reshape(self.keep, 4)[:cursor]
            out['per_image'] = {key: log[:, c].copy() for c, key in enumerate(KEYS)}
        return out


def image_quality(pred, target, data_range=1.0, win_size=11, sigma=1.5):
    """fp64 [B, 4] on the device: the rows (mse, rmse, psnr, ssim) of one batch; one launch, no host read."""
    launcher = _Launcher(data_range, win_size, sigma, pred.device if pred.is_cuda else 'cuda')
    launcher.check(pred, target)
    rows = torch.empty(pred.shape[0], 4, dtype=torch.float64, device=pred.device)
    acc = torch.zeros(4, dtype=torch.float64, device=pred.device)
    state = torch.zeros(4, dtype=torch.int64, device=pred.device)
    launcher.launch(pred, target, rows, acc, state, None, 0)
    return rows


def psnr(pred, target, data_range=1.0):
    """fp64 [B] on the device (the same launch with the smallest window, so H, W >= 3)."""
    return image_quality(pred, target, data_range=data_range, win_size=3)[:, 2]


def ssim(pred, target, data_range=1.0, win_size=11, sigma=1.5):
    """fp64 [B] on the device."""
    return image_quality(pred, target, data_range=data_range, win_size=win_size, sigma=sigma)[:, 3]
