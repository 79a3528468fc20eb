"""numpy restatement of the pixel half of baseline JPEG decoding as include/genesis_hip.h states it (libjpeg's default
path): dequantisation, the 13-bit fixed-point inverse DCT on columns then rows, triangle-filter chroma upsampling and the
16-bit fixed-point YCbCr -> RGB conversion.  Written from the definition, independently of gx_jpeg.hip; the tests feed it
the coefficients the C entropy decoder produces and compare with Pillow's pixels."""
import numpy as np


def plane_blocks_hw(H, W, sampling):
    """[(blocks high, blocks wide)] of the padded Y, Cb, Cr planes (whole MCUs)."""
    hs, vs = (2 if sampling else 1), (2 if sampling == 2 else 1)
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return [(my * vs, mx * hs), (my, mx), (my, mx)]


def idct_pass(v, shift):
    """The 8-point pass along the last axis of an int64 array, rounded by `shift` bits."""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., i] for i in range(8))
    z1 = (v2 + v6) * 4433
    t2 = z1 - v6 * 15137
    t3 = z1 + v2 * 6270
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = v7, v5, v3, v1
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * 9633
    a, b, c, d = a * 2446, b * 16819, c * 25172, d * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    out = np.stack([t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def component_planes(coef, qtab, H, W, sampling):
    """The three padded uint8-valued planes (int64 arrays) from the quantised coefficients (int16, planes one after the
    other, blocks in raster order, natural coefficient order) and the tables uint16 [3, 64]."""
    coef = np.asarray(coef).reshape(-1)
    qtab = np.asarray(qtab).reshape(3, 64)
    planes, at = [], 0
    for c, (bh, bw) in enumerate(plane_blocks_hw(H, W, sampling)):
        n = bh * bw
        blk = coef[at:at + n * 64].astype(np.int64).reshape(n, 8, 8) * qtab[c].astype(np.int64).reshape(8, 8)
        at += n * 64
        cols = idct_pass(blk.transpose(0, 2, 1), 11).transpose(0, 2, 1)     # along y for every column
        rows = idct_pass(cols, 18)                                          # along x for every row
        px = np.clip(rows + 128, 0, 255)
        planes.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes


def _h2(p, ra, rb):
    """Doubles the width of s-valued rows p: out[2i] = (3 p[i] + p[i-1] + ra) >> k, out[2i+1] = (3 p[i] + p[i+1] + rb) >> k
    with the edge sample as the missing neighbour (the caller shifts)."""
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    out[:, 0::2] = 3 * p + left + ra
    out[:, 1::2] = 3 * p + right + rb
    return out


def upsample(p, H, W, sampling):
    """A chroma plane (padded) -> [H, W]: the plane is first cut to its real extent ceil(W/2) x ceil(H/2)."""
    if sampling == 0:
        return p[:H, :W]
    cw = (W + 1) // 2
    if sampling == 1:
        return (_h2(p[:H, :cw], 1, 2) >> 2)[:, :W]
    ch = (H + 1) // 2
    p = p[:ch, :cw]
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    s = np.empty((2 * ch, cw), dtype=np.int64)
    s[0::2] = 3 * p + up
    s[1::2] = 3 * p + down
    return (_h2(s, 8, 7) >> 4)[:H, :W]


def decode_pixels(coef, qtab, H, W, sampling):
    """uint8 [H, W, 3] RGB."""
    y, cb, cr = component_planes(coef, qtab, H, W, sampling)
    y = y[:H, :W]
    cb = upsample(cb, H, W, sampling) - 128
    cr = upsample(cr, H, W, sampling) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)
