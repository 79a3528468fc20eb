"""A numpy restatement of "augment v1" (the normative text: include/genesis_hip.h, gx_cache_gather_aug), written from that text
and sharing no code with the kernel: Philox4x32-10 in Python integers, the parameters in integers and float32, the pixel
arithmetic in float32 with one numpy operation per rounding.  The plain gathers and the stores' layout come from
tests/data_cache_restatement.py."""
import numpy as np

from tests import data_cache_restatement as R

F32 = np.float32
M32 = 0xffffffff
CALL_A, CALL_B = 0xA06, 0xA07


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two -> four 32-bit words (Salmon et al. 2011)."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def words(seed, epoch, row):
    """r0 .. r7 of the frame in cache row `row` during resident epoch `epoch`."""
    seed, epoch, row = int(seed), int(epoch), int(row)
    key = (seed & M32, (seed >> 32) & M32)
    return (philox4x32_10((row & M32, (row >> 32) & M32, epoch & M32, CALL_A), key)
            + philox4x32_10((row & M32, (row >> 32) & M32, epoch & M32, CALL_B), key))


def t(x):
    return x >> 8


def u(x):
    return F32(t(x)) * F32(2.0 ** -24)


def gain(amount, word):
    """1 + amount * (2 u - 1), every operation in float32."""
    return F32(1.0) + F32(amount) * (F32(2.0) * u(word) - F32(1.0))


def params(seed, epoch, row, flip_t, wmin, brightness, colour, C, H, W):
    """-> (flip, x0, y0, w, h, [g_0, g_1, g_2] as float32; gains of channels the frame does not have are 1)."""
    r = words(seed, epoch, row)
    flip = int(t(r[0]) < flip_t)
    w = wmin + ((t(r[1]) * (W - wmin + 1)) >> 24)
    h = min(max((w * H + W // 2) // W, 1), H)
    x0 = (t(r[2]) * (W - w + 1)) >> 24
    y0 = (t(r[3]) * (H - h + 1)) >> 24
    g = gain(brightness, r[4])
    gains = [g * gain(colour, r[5 + ch]) if ch < C else F32(1.0) for ch in range(3)]
    return flip, x0, y0, w, h, gains


def params_row(p):
    """The int32 [8] row of params_out."""
    flip, x0, y0, w, h, gains = p
    return np.array([flip, x0, y0, w, h] + [int(np.array(g, dtype=F32).view(np.int32)) for g in gains], dtype=np.int32)


def taps(n, win, flipped):
    """Per output index 0 .. n - 1 of a window of `win` source values: (i0, i1, fraction float32, nearest index)."""
    o = np.arange(n, dtype=np.int64)
    if flipped:
        o = n - 1 - o
    s = (2 * o + 1) * win - n
    i0 = s // (2 * n)                                   # floor, also of the negative ones
    rem = s - i0 * 2 * n
    f = rem.astype(F32) / F32(2 * n)
    near = ((2 * o + 1) * win) // (2 * n)
    return np.clip(i0, 0, win - 1), np.clip(i0 + 1, 0, win - 1), f, near


def augment_frame(frame, p, mode):
    """frame uint8 [C, H, W] -> float32 [C, H, W]"""
    flip, x0, y0, w, h, gains = p
    C, H, W = frame.shape
    i0, i1, fx, _ = taps(W, w, flip)
    j0, j1, fy, _ = taps(H, h, False)
    win = frame[:, y0:y0 + h, x0:x0 + w].astype(F32)
    assert win.shape == (C, h, w)
    fx, fy = fx[None, None, :], fy[None, :, None]
    a00, a01 = win[:, j0][:, :, i0], win[:, j0][:, :, i1]
    a10, a11 = win[:, j1][:, :, i0], win[:, j1][:, :, i1]
    d = a01 - a00
    d = d * fx
    top = a00 + d
    d = a11 - a10
    d = d * fx
    bot = a10 + d
    d = bot - top
    d = d * fy
    v = top + d
    v = v * np.array(gains[:C], dtype=F32)[:, None, None]
    v = np.minimum(v, F32(255.0))
    assert v.dtype == F32
    return v / F32(255.0) if mode == 0 else v * R.ONE_OVER_255


def augment_labels(labels, p):
    """labels [H, W] -> the same dtype [H, W]: nearest, same window, no gain"""
    flip, x0, y0, w, h, _ = p
    H, W = labels.shape
    lx = taps(W, w, flip)[3]
    ly = taps(H, h, False)[3]
    return labels[y0:y0 + h, x0:x0 + w][ly][:, lx]


def gather(store, lstore, shape, rows, seed, epoch, flip_t, wmin, brightness, colour, mode):
    """The restated gx_cache_gather_aug over numpy stores (R.new_store): -> (float32 [B, C, H, W], int64 [B, 1, H, W] or None,
    int32 [B, 8])."""
    C, H, W = shape
    rows = [int(r) for r in rows]
    out = np.empty((len(rows), C, H, W), dtype=F32)
    out_labels = None if lstore is None else np.empty((len(rows), 1, H, W), dtype=np.int64)
    table = np.empty((len(rows), 8), dtype=np.int32)
    for b, row in enumerate(rows):
        p = params(seed, epoch, row, flip_t, wmin, brightness, colour, C, H, W)
        table[b] = params_row(p)
        out[b] = augment_frame(store[row, :C * H * W].reshape(C, H, W), p, mode)
        if lstore is not None:
            lab = np.ascontiguousarray(lstore[row, :2 * H * W]).view(np.int16).reshape(H, W)
            out_labels[b, 0] = augment_labels(lab, p).astype(np.int64)
    return out, out_labels, table
