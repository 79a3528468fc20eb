"""A numpy restatement of the device cache's kernels (genesis_amd/csrc/gx_cache.hip), sharing no code with them: the quantise
step with both mismatch counts, the int16 narrowing with its misfit count, both gathers and the padded-stride layout.  All
arithmetic is float32, as the kernels'."""
import numpy as np

F32 = np.float32
ONE_OVER_255 = F32(1.0) / F32(255.0)


def row_stride(row_bytes):
    """Rows start 16-byte aligned: the stride is the row rounded up to a multiple of 16 bytes."""
    return (int(row_bytes) + 15) // 16 * 16


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def unit(q, mode):
    """byte -> float32: mode 0 a true division by 255, mode 1 a product with the float32 1 / 255."""
    q = np.asarray(q).astype(F32)
    return q / F32(255.0) if mode == 0 else q * ONE_OVER_255


def quantise(v):
    """float32 values -> (bytes q = clamp(rint(v * 255), 0, 255) with NaN -> 0, div_miss, mul_miss): the counts of the values
    whose bits differ from q / 255 and from q * (1 / 255)."""
    v = np.ascontiguousarray(v, dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.rint(v * F32(255.0))                         # half to even, as rintf
        q = np.where(r >= 0, np.where(r <= 255, r, F32(255.0)), F32(0.0))     # NaN fails r >= 0
    q = q.astype(np.uint8)
    div_miss = int(np.count_nonzero(bits(v) != bits(unit(q, 0))))
    mul_miss = int(np.count_nonzero(bits(v) != bits(unit(q, 1))))
    return q, div_miss, mul_miss


def narrow_labels(labels):
    """int64 -> (int16 by truncation to the low 16 bits, the count of values outside -32768 .. 32767)."""
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    misfit = int(np.count_nonzero((labels < -32768) | (labels > 32767)))
    return (labels & 0xffff).astype(np.uint16).view(np.int16), misfit


def new_store(rows, row_bytes, fill=0):
    return np.full((rows, row_stride(row_bytes)), fill, dtype=np.uint8)


def store_frames(store, first_row, batch):
    """batch float32 [B,C,H,W] -> rows first_row.. of the uint8 store [rows, stride]; pad bytes stay.  -> (div_miss, mul_miss)"""
    B = batch.shape[0]
    q, div_miss, mul_miss = quantise(batch)
    q = q.reshape(B, -1)
    store[first_row:first_row + B, :q.shape[1]] = q
    return div_miss, mul_miss


def store_labels(store, first_row, labels):
    """labels int64 [B,1,H,W] -> rows first_row.. as little-endian int16; -> label_misfit"""
    B = labels.shape[0]
    s, misfit = narrow_labels(labels)
    raw = s.reshape(B, -1).view(np.uint8)
    store[first_row:first_row + B, :raw.shape[1]] = raw
    return misfit


def gather_frames(store, shape, rows, mode):
    C, H, W = shape
    return unit(store[np.asarray(rows), :C * H * W], mode).reshape(len(rows), C, H, W)


def gather_labels(store, shape, rows):
    H, W = shape
    raw = np.ascontiguousarray(store[np.asarray(rows), :2 * H * W])
    return raw.view(np.int16).astype(np.int64).reshape(len(rows), 1, H, W)
