"""A NumPy restatement of PNG's five scanline filters (the PNG specification, section 9): test infrastructure, like
tests/jpeg_restatement.py.  It undoes the filters of an inflated frame as gx_png_inflate leaves it -- per row one filter
byte and W * C filtered bytes -- one row at a time, serial in x only where the filter needs it."""
import numpy as np


def unfilter(filtered, H, W, C):
    """filtered: uint8 [H * (1 + W * C)] -> uint8 [H, W, C].  Per byte: the left neighbour is C bytes back, bytes left of the
    row and above the first row are 0, Average is floor((a + b) / 2) on the 9-bit sum, Paeth breaks ties in the order a, b, c."""
    rows = np.asarray(filtered, dtype=np.uint8).reshape(H, 1 + W * C)
    out = np.zeros((H, W * C), dtype=np.int64)
    above = np.zeros(W * C, dtype=np.int64)
    for r in range(H):
        f, raw = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
        if f == 0:
            cur = raw
        elif f == 1:
            cur = raw.copy()
            for x in range(C, W * C):
                cur[x] = (cur[x] + cur[x - C]) & 255
        elif f == 2:
            cur = (raw + above) & 255
        elif f == 3:
            cur = np.zeros(W * C, dtype=np.int64)
            for x in range(W * C):
                a = cur[x - C] if x >= C else 0
                cur[x] = (raw[x] + ((a + above[x]) >> 1)) & 255
        elif f == 4:
            cur = np.zeros(W * C, dtype=np.int64)
            for x in range(W * C):
                a = cur[x - C] if x >= C else 0
                b = above[x]
                c = above[x - C] if x >= C else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                cur[x] = (raw[x] + (a if (pa <= pb and pa <= pc) else (b if pb <= pc else c))) & 255
        else:
            raise ValueError('filter byte %d in row %d' % (f, r))
        out[r] = cur
        above = cur
    return out.astype(np.uint8).reshape(H, W, C)


def plane(u8, rule):
    """Channel 0 after a plane rule of gx_png_unfilter: 0 the byte, 1 the reference's ShapeStacks arithmetic, 2 byte >> 5."""
    b = u8[..., 0]
    if rule == 1:
        return ((b.astype(np.float32) / np.float32(255.0)) / np.float32(32.0)).astype(np.uint8)
    return (b >> 5) if rule == 2 else b.copy()
