"""A numpy restatement of what genesis_amd.tbwriter writes, from the published rules and not from its code: the byte rule of a
picture, PNG's five scanline filters with the minimum-sum-of-absolute-differences choice, CRC-32C bit by bit, TFRecord framing, and
a protobuf wire decoder for Event, Summary, Summary.Value, Summary.Image and HistogramProto.  Test infrastructure, like
tests/png_restatement.py.  numpy and the standard library only."""
import struct
import zlib

import numpy as np


# ---- pictures ------------------------------------------------------------------------------------------------------------------
def quantise(array, dataformats):
    """An array in 'CHW', 'HWC' or 'HW' -> uint8 [H, W, C].  Floats: trunc(clamp(x, 0, 1) * 255) with the product in float32 and
    NaN -> 0; uint8: the bytes; other integers: the value clamped to 0..255."""
    a = np.asarray(array)
    if dataformats == 'CHW':
        a = np.moveaxis(a, 0, 2)
    elif dataformats == 'HW':
        a = a.reshape(a.shape + (1,))
    else:
        assert dataformats == 'HWC'
    if a.dtype.kind == 'f':
        x = np.array(a, dtype=np.float32)
        nan = x != x
        x[nan] = 0
        x[x < 0] = 0
        x[x > 1] = 1
        prod = x * np.float32(255.0)
        assert prod.dtype == np.float32
        return np.floor(prod).astype(np.int64).astype(np.uint8)      # (the product is in [0, 255]: floor is truncation)
    v = a.astype(np.int64)
    v[v < 0] = 0
    v[v > 255] = 255
    return v.astype(np.uint8)


# ---- test pictures -------------------------------------------------------------------------------------------------------------
def picture(kind, C, H, W, seed):
    """[H, W, C] with ramps, noise, constant rows, out-of-range values and NaN."""
    rng = np.random.RandomState(seed)
    yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing='ij')
    ramp = (xx * 3 + yy * 5 + cc * 11) / 255.0
    a = np.where(yy % 3 == 0, ramp, rng.rand(H, W, C) * 1.4 - 0.2)
    if H > 1:
        a[H // 2] = 0.5                      # a constant row
    if kind == 'fp32':
        a = a.astype(np.float32)
        a.reshape(-1)[::7] = np.nan
        a.reshape(-1)[3::11] = -3.0
        a.reshape(-1)[5::13] = 1.0 + 1e-3
        return a
    if kind == 'uint8':
        return (np.clip(a, 0, 1) * 255).astype(np.uint8)
    v = (a * 300 - 20).astype(np.int64)      # below 0 and above 255
    return v


def as_format(hwc, dataformats):
    if dataformats == 'CHW':
        return np.ascontiguousarray(hwc.transpose(2, 0, 1))
    return hwc[:, :, 0].copy() if dataformats == 'HW' else hwc


def _signed_cost(row):
    """Sum over the row of |byte read as a signed byte|."""
    return int(np.abs(row.astype(np.uint8).view(np.int8).astype(np.int64)).sum())


def filter_rows(u8_hwc):
    """uint8 [H, W, C] -> int array [H, 5, W C]: every row under each of the five filters (None, Sub, Up, Average, Paeth), mod 256;
    the left neighbour is C bytes back, everything outside the picture is 0."""
    H, W, C = u8_hwc.shape
    n = W * C
    img = u8_hwc.reshape(H, n).astype(np.int64)
    out = np.zeros((H, 5, n), np.int64)
    for r in range(H):
        x = img[r]
        b = img[r - 1] if r > 0 else np.zeros(n, np.int64)
        a = np.concatenate([np.zeros(C, np.int64), x[:n - C]]) if n > C else np.zeros(n, np.int64)
        c = np.concatenate([np.zeros(C, np.int64), b[:n - C]]) if n > C else np.zeros(n, np.int64)
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[r] = np.stack([x, x - a, x - b, x - (a + b) // 2, x - pred]) % 256
    return out


def pack_rows(u8_hwc):
    """uint8 [H, W, C] -> the scanline stream (bytes): per row the filter-type byte, then that filter's bytes; the filter with the
    smallest sum of |signed byte| over the row, ties to the lowest filter number."""
    cand = filter_rows(u8_hwc)
    out = bytearray()
    for r in range(cand.shape[0]):
        costs = [_signed_cost(cand[r, k]) for k in range(5)]
        k = costs.index(min(costs))
        out.append(k)
        out += cand[r, k].astype(np.uint8).tobytes()
    return bytes(out)


def filter_costs(u8_hwc):
    """[H][5] sums of |signed byte|: lets a test show that its input really makes two filters tie."""
    cand = filter_rows(u8_hwc)
    return [[_signed_cost(cand[r, k]) for k in range(5)] for r in range(cand.shape[0])]


def png_parts(png):
    """A PNG as this project writes it -> (W, H, colour type, the inflated IDAT stream); checks the signature, the chunk order
    IHDR, IDAT, IEND and every chunk's CRC-32."""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(png):
        size, kind = struct.unpack('>I4s', png[pos:pos + 8])
        body = png[pos + 8:pos + 8 + size]
        assert struct.unpack('>I', png[pos + 8 + size:pos + 12 + size])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        pos += 12 + size
    assert [k for k, _ in chunks] == [b'IHDR', b'IDAT', b'IEND']
    W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and chunks[2][1] == b''
    return W, H, colour, zlib.decompress(chunks[1][1])


# ---- CRC-32C and TFRecord framing ----------------------------------------------------------------------------------------------
def _crc_table():
    table = []
    for byte in range(256):
        c = byte
        for _ in range(8):      # bit by bit, reflected polynomial 0x82f63b78 (Castagnoli)
            c = (c >> 1) ^ 0x82f63b78 if c & 1 else c >> 1
        table.append(c)
    return table


_TABLE = _crc_table()


def crc32c(data):
    c = 0xffffffff
    for b in bytes(data):
        c = _TABLE[(c ^ b) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff


def masked_crc32c(data):
    c = crc32c(data)
    return ((((c >> 15) | (c << 17)) & 0xffffffff) + 0xa282ead8) & 0xffffffff


def split_records(data):
    """An event file's bytes -> the data of every record; both checksums of each are checked here."""
    pos, out = 0, []
    while pos < len(data):
        head = data[pos:pos + 8]
        assert len(head) == 8
        size = struct.unpack('<Q', head)[0]
        assert struct.unpack('<I', data[pos + 8:pos + 12])[0] == masked_crc32c(head), 'length checksum of record %d' % len(out)
        body = data[pos + 12:pos + 12 + size]
        assert len(body) == size
        assert struct.unpack('<I', data[pos + 12 + size:pos + 16 + size])[0] == masked_crc32c(body), 'data checksum of record %d' % len(out)
        out.append(body)
        pos += 16 + size
    return out


# ---- protobuf ----------------------------------------------------------------------------------------------------------------------
def wire(buf):
    """-> [(field number, wire type, int for varints / bytes otherwise)]"""
    pos, out = 0, []
    while pos < len(buf):
        key, pos = _varint(buf, pos)
        number, kind = key >> 3, key & 7
        if kind == 0:
            v, pos = _varint(buf, pos)
        elif kind == 1:
            v, pos = buf[pos:pos + 8], pos + 8
        elif kind == 5:
            v, pos = buf[pos:pos + 4], pos + 4
        else:
            assert kind == 2, kind
            size, pos = _varint(buf, pos)
            v, pos = buf[pos:pos + size], pos + size
        assert pos <= len(buf)
        out.append((number, kind, v))
    return out


def _varint(buf, pos):
    v = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7f) << shift
        shift += 7
        if b < 0x80:
            return v, pos


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def _double(b):
    return struct.unpack('<d', b)[0]


def decode_event(buf):
    """Event -> dict(wall_time, step, file_version or None, values = [dict(tag, and simple_value | image | histo)])."""
    e = dict(wall_time=0.0, step=0, file_version=None, values=[])
    for number, kind, v in wire(buf):
        if (number, kind) == (1, 1):
            e['wall_time'] = _double(v)
        elif (number, kind) == (2, 0):
            e['step'] = _signed(v)
        elif (number, kind) == (3, 2):
            e['file_version'] = v.decode()
        elif (number, kind) == (5, 2):
            for n1, k1, value in wire(v):
                assert (n1, k1) == (1, 2)
                e['values'].append(_decode_value(value))
        else:
            raise AssertionError('Event field %d of wire type %d' % (number, kind))
    return e


def _decode_value(buf):
    out = {}
    for number, kind, v in wire(buf):
        if (number, kind) == (1, 2):
            out['tag'] = v.decode()
        elif (number, kind) == (2, 5):
            out['simple_value'] = np.frombuffer(v, '<f4')[0]
        elif (number, kind) == (4, 2):
            image = {}
            for n1, k1, x in wire(v):
                if k1 == 0:
                    image[{1: 'height', 2: 'width', 3: 'colorspace'}[n1]] = _signed(x)
                else:
                    assert (n1, k1) == (4, 2)
                    image['encoded_image_string'] = x
            out['image'] = image
        elif (number, kind) == (5, 2):
            histo = dict(bucket_limit=[], bucket=[])
            for n1, k1, x in wire(v):
                if k1 == 1:
                    histo[{1: 'min', 2: 'max', 3: 'num', 4: 'sum', 5: 'sum_squares'}[n1]] = _double(x)
                else:
                    assert k1 == 2 and n1 in (6, 7) and len(x) % 8 == 0
                    histo['bucket_limit' if n1 == 6 else 'bucket'] += [_double(x[i:i + 8]) for i in range(0, len(x), 8)]
            out['histo'] = histo
        else:
            raise AssertionError('Summary.Value field %d of wire type %d' % (number, kind))
    return out


def read_file(path):
    with open(path, 'rb') as f:
        return [decode_event(r) for r in split_records(f.read())]
