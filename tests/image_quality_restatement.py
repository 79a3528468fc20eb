"""fp64 numpy restatement of genesis_amd/image_quality.py, written from the definition: per image of pred / target [B, C, H, W]
with data range L and N = C H W,
    mse = (1 / N) sum (pred - target)^2,  rmse = sqrt(mse),  psnr = 10 log10(L^2 / mse) (+inf at mse == 0),
    ssim = mean over channels and valid positions of ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)),
    C1 = (0.01 L)^2, C2 = (0.03 L)^2, the moments taken with the 2-D outer-product Gaussian window.
The window goes through scipy.signal.correlate2d(mode='valid') as ONE 2-D correlation, so nothing here shares the kernel's
separable form; `ssim_direct` is a slow double loop over the positions for the CPU self-check.  Also the input pairs the tests
share."""
import numpy as np
from scipy.signal import correlate2d


def window(win_size=11, sigma=1.5):
    """Written out again from the formula (the tests compare genesis_amd.image_quality.gaussian_window with it)."""
    g = np.array([np.exp(-(i - (win_size - 1) / 2.0) ** 2 / (2.0 * sigma ** 2)) for i in range(win_size)], np.float64)
    return g / g.sum()


def _ssim_value(mx, my, mxx, myy, mxy, L):
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    vx, vy, cxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    return ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def ssim_map(x, y, L=1.0, win_size=11, sigma=1.5):
    """The SSIM map [H - n + 1, W - n + 1] of one channel."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    g = window(win_size, sigma)
    g2 = np.outer(g, g)
    f = lambda a: correlate2d(a, g2, mode='valid')      # noqa: E731
    return _ssim_value(f(x), f(y), f(x * x), f(y * y), f(x * y), L)


def ssim_direct(x, y, L=1.0, win_size=11, sigma=1.5):
    """The same map by a double loop over the positions, each moment a plain sum over the window."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    g = window(win_size, sigma)
    n = win_size
    out = np.empty((x.shape[0] - n + 1, x.shape[1] - n + 1), np.float64)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            m = [0.0] * 5
            for u in range(n):
                for v in range(n):
                    w, a, b = g[u] * g[v], x[i + u, j + v], y[i + u, j + v]
                    for q, val in enumerate((a, b, a * a, b * b, a * b)):
                        m[q] += w * val
            out[i, j] = _ssim_value(*m, L)
    return out


def mse(pred, target):
    """[B] fp64."""
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    return (d * d).reshape(d.shape[0], -1).mean(axis=1)


def rmse(pred, target):
    return np.sqrt(mse(pred, target))


def psnr(pred, target, L=1.0):
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10((L * L) / mse(pred, target))


def ssim(pred, target, L=1.0, win_size=11, sigma=1.5):
    """[B] fp64: the mean of the map over all channels and valid positions."""
    pred, target = np.asarray(pred), np.asarray(target)
    return np.array([np.mean([ssim_map(pred[b, c], target[b, c], L, win_size, sigma) for c in range(pred.shape[1])])
                     for b in range(pred.shape[0])], np.float64)


def rows(pred, target, L=1.0, win_size=11, sigma=1.5):
    """[B, 4] fp64: mse, rmse, psnr, ssim per image."""
    return np.stack([mse(pred, target), rmse(pred, target), psnr(pred, target, L), ssim(pred, target, L, win_size, sigma)], 1)


def make_pair(shape, seed, noise=0.1, clip=True):
    """target = rng.random(shape), pred = target + noise N(0, 1) (clipped to [0, 1] unless clip=False), both fp32."""
    rng = np.random.default_rng(seed)
    target = rng.random(shape).astype(np.float32)
    pred = target + np.float32(noise) * rng.standard_normal(shape).astype(np.float32)
    if clip:
        pred = np.clip(pred, 0.0, 1.0)
    return pred.astype(np.float32), target
