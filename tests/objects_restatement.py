"""gx_object_table (include/genesis_hip.h) restated in numpy, and the one input maker both test files share.

restate(log_m, x): labels by np.argmax (ties: the lowest k; a NaN ranks above every number and the first one wins -- torch.argmax's
rule, which numpy shares), the integer table by np.bincount / np.minimum.at / plain loops, the fp64 sums with np.exp on float64.
Nothing here imports the package under test."""
import struct
import zlib

import numpy as np

from tests import png_restatement

GEOM_WORDS, SOFT_WORDS = 8, 6


def restate(log_m, x=None):
    """log_m float32 [K, B, H, W]; x float32 [B, C, H, W] or None -> (labels uint8 [B, H, W], geom int64 [B, K, 8],
    soft float64 [B, K, 6])."""
    log_m = np.asarray(log_m, dtype=np.float32)
    K, B, H, W = log_m.shape
    labels = np.argmax(log_m, axis=0).astype(np.uint8)
    geom = np.zeros((B, K, GEOM_WORDS), np.int64)
    soft = np.zeros((B, K, SOFT_WORDS), np.float64)
    py, px = np.divmod(np.arange(H * W), W)
    bits = ((px == 0) * 1 + (py == 0) * 2 + (px == W - 1) * 4 + (py == H - 1) * 8).astype(np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.exp(log_m.astype(np.float64)).reshape(K, B, H * W)
    for b in range(B):
        lab = labels[b].reshape(-1).astype(np.int64)
        geom[b, :, 0] = np.bincount(lab, minlength=K)
        lo_x, lo_y = np.full(K, W, np.int64), np.full(K, H, np.int64)
        hi_x, hi_y = np.full(K, -1, np.int64), np.full(K, -1, np.int64)
        np.minimum.at(lo_x, lab, px); np.minimum.at(lo_y, lab, py)
        np.maximum.at(hi_x, lab, px); np.maximum.at(hi_y, lab, py)
        geom[b, :, 1], geom[b, :, 2], geom[b, :, 3], geom[b, :, 4] = lo_x, lo_y, hi_x, hi_y
        for p in range(H * W):                  # plain loops for the sums and the border bits
            k = lab[p]
            geom[b, k, 5] += px[p]
            geom[b, k, 6] += py[p]
            geom[b, k, 7] |= bits[p]
        for k in range(K):
            own = lab == k
            soft[b, k, 0] = e[k, b].sum()
            soft[b, k, 1] = e[k, b][own].sum()
            if x is not None:
                for c in range(x.shape[1]):
                    soft[b, k, 2 + c] = x[b, c].reshape(-1).astype(np.float64)[own].sum()
    return labels, geom, soft


def make_inputs(B, K, H, W, seed=0, C=3):
    """(log_m float32 [K, B, H, W], x float32 [B, C, H, W] >= 0) with, wherever the shape has room for it:
      every image         exact ties between the planes 0 and 1 (both hold the pixel's largest value) at every 7th pixel;
      image 0             plane 0 wins the whole frame of border pixels -- an object that touches all four borders; (K >= 4, H, W >= 3)
                          plane 2 wins exactly one interior pixel and nothing else; plane K - 1 is the -1e10 padding of dynamic_K
                          (K >= 3): a slot that wins nowhere;
      image 1 (B >= 2)    plane K - 1 is -inf (K >= 3);
      the last image      NaNs in plane 1 at every 11th pixel, and at one of them in plane 2 as well (the first NaN wins).
    The planes are a log-softmax over k before these edits, so every exp is a mask value in [0, 1]."""
    rng = np.random.RandomState(seed + 1000 * B + 100 * K + 10 * H + W)
    z = rng.standard_normal((K, B, H, W)).astype(np.float64) * 2.0
    log_m = (z - np.log(np.exp(z).sum(0, keepdims=True))).astype(np.float32)
    flat = log_m.reshape(K, B, H * W)
    p = np.arange(H * W)
    if K >= 2:
        tie = p % 7 == 3
        top = flat.max(0)
        flat[0][:, tie] = top[:, tie]
        flat[1][:, tie] = top[:, tie]
    if K >= 3:
        flat[K - 1, 0] = -1e10
        if B >= 2:
            flat[K - 1, 1] = -np.inf
    if K >= 4 and H >= 3 and W >= 3:
        frame = ((p % W == 0) | (p % W == W - 1) | (p // W == 0) | (p // W == H - 1))
        flat[0, 0, frame] = 0.0                 # log 1: above every log-softmax value
        flat[1, 0, frame] = -3.0                # (no tie on the frame)
        centre = (H // 2) * W + W // 2
        flat[2, 0] = -30.0
        flat[2, 0, centre] = 0.5
    if K >= 2:
        nan = p % 11 == 5
        flat[1, B - 1, nan] = np.nan
        if K >= 3 and nan.any():
            flat[2, B - 1, np.flatnonzero(nan)[0]] = np.nan
    x = rng.random_sample((B, C, H, W)).astype(np.float32)
    return log_m, x


def read_grey_png(data):
    """An 8-bit greyscale, non-interlaced PNG -> uint8 [H, W]; every chunk's CRC is checked."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    w, h, depth, colour, comp, filt, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 0, 0, 0, 0)
    return png_restatement.unfilter(np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8), h, w, 1)[:, :, 0]
