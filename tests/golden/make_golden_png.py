"""Writes tests/golden/png_pil.npz, the fixture of the PNG decoder (genesis_amd/png.py, gx_png.cpp, gx_png.hip) and of the
ShapeStacks / Sketchy data configs.  The yardstick is Pillow, at zero tolerance:
    <case>_png    uint8 [n]          the stream
    <case>_u8     uint8 [H, W, C]    np.asarray(Image.open(stream))
for every case of HAND (streams assembled here with struct + zlib, so that the filter of every row is chosen) and of PIL
(streams Pillow encodes with its adaptive filter choice), then
    ss_rgb<S>          uint8 [S, S, 3]   Image.crop(centre 196) + resize((S, S), BILINEAR) of `pil_smooth224`, S = 64, 128
                                         (the ShapeStacks transform as make_golden_feeder.py states it; the tests divide by 255)
    ss_map_png         a 224 x 224 map whose channel 0 takes all of 0, 32, ..., 224
    ss_labels_ref<S>   int64 [1, S, S]   the REFERENCE's labels: its own load_segmap_as_matrix (imported live; it needs only
                                         matplotlib) followed by the crop / F.interpolate / long of shapestacks_config.py:155-163
    ss_labels_index<S> uint8 [1, S, S]   byte // 32 through the same crop and interpolate
and `broken_<name>_png` for every case of BROKEN, each with the substring its error must contain.

Importing this module needs neither Pillow nor matplotlib nor the fixture; only main() does.
Run from the repository root: python tests/golden/make_golden_png.py"""
import io
import os
import os.path as osp
import struct
import sys
import zlib

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
NPZ = osp.join(HERE, 'png_pil.npz')

BAND = {1: 1024, 3: 341, 4: 256}           # rows of one band of the kernel: 1024 // C
CYCLE = 'cycle'                            # row r has filter r % 5

# (case, W, H, C, filter of every row or CYCLE)
HAND = [('f%d_c%d_5x3' % (f, C), 5, 3, C, f) for C in (1, 3, 4) for f in range(5)]
HAND += [('cycle_c%d_%dx%d' % (C, W, H), W, H, C, CYCLE) for C in (1, 3, 4) for W, H in ((1, 1), (1, 7), (7, 1), (67, 9))]
HAND += [('band_c%d_3x%d' % (C, H), 3, H, C, CYCLE) for C in (1, 3, 4) for H in (BAND[C], BAND[C] + 1)]
HAND += [('chunks_c3_67x9', 67, 9, 3, CYCLE)]      # several IDAT chunks, one of them empty, and an ancillary chunk before them
HAND_NAMES = [c[0] for c in HAND]
# (case, size, content)
PIL = [('pil_smooth224', 224, 'smooth'), ('pil_mixed128', 128, 'mixed'), ('pil_noise64', 64, 'noise')]
PIL_NAMES = [c[0] for c in PIL]
GOOD_NAMES = HAND_NAMES + PIL_NAMES
# (case, the substring its error must contain)
BROKEN = [('crc', 'CRC mismatch in the IDAT chunk'), ('truncated', 'ends early'), ('filter5', 'filter byte 5'),
          ('interlaced', 'Adam7'), ('depth16', '16-bit'), ('palette', 'palette'), ('short', 'inflates to')]
SS_SIZES = (64, 128)
SS_FRAME = 'pil_smooth224'
CENTRE_CROP = 196

SIGNATURE = b'\x89PNG\r\n\x1a\n'
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def ihdr(W, H, colour_type, depth=8, interlace=0):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, depth, colour_type, 0, 0, interlace))


def row_filters(H, spec):
    return [r % 5 for r in range(H)] if spec == CYCLE else [int(spec)] * H


def filter_rows(img, filters):
    """img uint8 [H, W, C] -> the filtered frame (a filter byte and W * C bytes per row) with filters[r] on row r."""
    H, W, C = img.shape
    flat = img.reshape(H, W * C).astype(np.int64)
    out = np.zeros((H, 1 + W * C), dtype=np.uint8)
    zero = np.zeros(W * C, dtype=np.int64)
    for r in range(H):
        x = flat[r]
        a = np.concatenate([zero[:C], x[:-C]]) if W > 1 else zero
        b = flat[r - 1] if r else zero
        c = (np.concatenate([zero[:C], b[:-C]]) if W > 1 else zero)
        f = filters[r]
        if f == 0:
            pred = zero
        elif f == 1:
            pred = a
        elif f == 2:
            pred = b
        elif f == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[r, 0] = f
        out[r, 1:] = (x - pred) & 255
    return out.tobytes()


def assemble(img, filters, idat_cuts=None, extra=b''):
    """A PNG stream of img with the given row filters; idat_cuts: the zlib stream is cut into IDAT chunks at these offsets
    (an offset given twice makes an empty chunk); extra: chunks put between IHDR and the first IDAT."""
    H, W, C = img.shape
    z = zlib.compress(filter_rows(img, filters), 6)
    cuts = [0] + sorted(idat_cuts or []) + [len(z)]
    idat = b''.join(chunk(b'IDAT', z[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1))
    return SIGNATURE + ihdr(W, H, COLOUR_TYPE[C]) + extra + idat + chunk(b'IEND', b'')


def content_image(kind, H, W, C, seed):
    """A seeded uint8 [H, W, C] image: 'noise' (uniform bytes), 'smooth' (gradients and a slow wave) or 'mixed' (smooth with
    hard-edged rectangles and a noisy quarter)."""
    rng = np.random.RandomState(seed)
    if kind == 'noise':
        return rng.randint(0, 256, (H, W, C)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = [255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1),
              127.5 + 127.5 * np.sin(x / 23.0 + 1.0) * np.cos(y / 31.0 + 2.0), 255.0 - 255.0 * x / max(W - 1, 1)]
    img = np.stack(planes[:C], axis=2)
    if kind == 'mixed':
        for _ in range(4):
            y0, x0 = rng.randint(0, H), rng.randint(0, W)
            img[y0:y0 + rng.randint(1, H // 2 + 2), x0:x0 + rng.randint(1, W // 2 + 2)] = rng.choice([0, 255], C)
        img[:H // 4, :W // 4] += rng.randint(-60, 61, (H // 4, W // 4, C))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def hand_stream(name):
    i = HAND_NAMES.index(name)
    _, W, H, C, spec = HAND[i]
    img = content_image('noise', H, W, C, 7000 + i)
    if name.startswith('chunks'):
        z = len(zlib.compress(filter_rows(img, row_filters(H, spec)), 6))
        return img, assemble(img, row_filters(H, spec), idat_cuts=[z // 3, z // 3, 2 * z // 3],
                             extra=chunk(b'tEXt', b'Comment\x00an ancillary chunk the decoder skips'))
    return img, assemble(img, row_filters(H, spec))


def map_image():
    """A 224 x 224 RGB map: channel 0 = 32 * label, eight labels in blocks that do not line up with the crop or the resize."""
    y, x = np.mgrid[0:224, 0:224]
    label = ((y // 37) * 3 + x // 29) % 8
    return np.stack([32 * label, 255 - 32 * label, (x + y) % 256], axis=2).astype(np.uint8)


def pil_decode(stream):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(stream))))


def pil_encode(img):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='PNG')
    return buf.getvalue()


def stream_filters(stream):
    """The filter byte of every row of a good 8-bit stream (for the report main() prints)."""
    p, pos, z = bytes(stream), 8, b''
    while pos < len(p):
        n, kind = struct.unpack('>I', p[pos:pos + 4])[0], p[pos + 4:pos + 8]
        if kind == b'IHDR':
            W, H, _, ct = struct.unpack('>IIBB', p[pos + 8:pos + 18])
        if kind == b'IDAT':
            z += p[pos + 8:pos + 8 + n]
        pos += 12 + n
    C = {0: 1, 2: 3, 6: 4}[ct]
    return np.frombuffer(zlib.decompress(z), dtype=np.uint8).reshape(H, 1 + W * C)[:, 0]


def broken_streams(good):
    """name -> stream, made from `good` = the stream of f1_c3_5x3 and its image."""
    img, stream = good
    H, W, C = img.shape
    idat = stream.index(b'IDAT')
    flipped = bytearray(stream)
    flipped[idat + 6] ^= 0x40
    rows = bytearray(filter_rows(img, [1] * H))
    rows[1 + W * C] = 5                                  # the filter byte of row 1
    z5 = zlib.compress(bytes(rows), 6)
    short = zlib.compress(filter_rows(img, [1] * H)[:-1], 6)
    body = stream[stream.index(b'IDAT') - 4:]
    return {
        'crc': bytes(flipped),
        'truncated': stream[:idat + 8],
        'filter5': SIGNATURE + ihdr(W, H, 2) + chunk(b'IDAT', z5) + chunk(b'IEND', b''),
        'interlaced': SIGNATURE + ihdr(W, H, 2, interlace=1) + body,
        'depth16': SIGNATURE + ihdr(W, H, 2, depth=16) + body,
        'palette': SIGNATURE + ihdr(W, H, 3) + chunk(b'PLTE', bytes(range(48))) + body,
        'short': SIGNATURE + ihdr(W, H, 2) + chunk(b'IDAT', short) + chunk(b'IEND', b''),
    }


def reference_labels(map_png, size):
    """The reference's instance labels of a map file: load_segmap_as_matrix imported from the reference tree, then the crop,
    F.interpolate and cast of datasets/shapestacks_config.py:155-163."""
    import importlib.util
    import tempfile
    import torch
    import torch.nn.functional as F
    root = os.environ.get('GENESIS_REFERENCE_ROOT', '/root/reference')
    spec = importlib.util.spec_from_file_location('ref_segmentation_utils',
                                                  osp.join(root, 'third_party', 'shapestacks', 'segmentation_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as tmp:
        path = osp.join(tmp, 'iseg.map')
        with open(path, 'wb') as f:
            f.write(map_png)
        masks = mod.load_segmap_as_matrix(path)
    return crop_interpolate(masks, size), float(masks.max())


def crop_interpolate(masks, size):
    import torch
    import torch.nn.functional as F
    o = (masks.shape[0] - CENTRE_CROP) // 2
    m = torch.FloatTensor(np.ascontiguousarray(masks[None, o:o + CENTRE_CROP, o:o + CENTRE_CROP]))
    if size != CENTRE_CROP:
        m = F.interpolate(m.unsqueeze(0), size=size).squeeze(0)
    return m.type(torch.LongTensor).numpy()


def main():
    from PIL import Image
    out = {}
    for name in HAND_NAMES:
        img, stream = hand_stream(name)
        got = pil_decode(stream)
        if got.ndim == 2:
            got = got[:, :, None]
        assert np.array_equal(got, img), name
        out[name + '_png'] = np.frombuffer(stream, dtype=np.uint8)
        out[name + '_u8'] = got
    for i, (name, S, kind) in enumerate(PIL):
        img = content_image(kind, S, S, 3, 7100 + i)
        stream = pil_encode(img)
        assert np.array_equal(pil_decode(stream), img)
        out[name + '_png'] = np.frombuffer(stream, dtype=np.uint8)
        out[name + '_u8'] = img
        print('%s: %d bytes, rows per filter 0..4: %s' % (name, len(stream), np.bincount(stream_filters(stream), minlength=5).tolist()))
    frame = Image.open(io.BytesIO(bytes(out[SS_FRAME + '_png'])))
    o = (224 - CENTRE_CROP) // 2
    for S in SS_SIZES:
        out['ss_rgb%d' % S] = np.asarray(frame.crop((o, o, o + CENTRE_CROP, o + CENTRE_CROP)).resize((S, S), Image.BILINEAR))
    m = map_image()
    map_png = pil_encode(m)
    assert sorted(set(m[:, :, 0].ravel().tolist())) == list(range(0, 256, 32))
    out['ss_map_png'] = np.frombuffer(map_png, dtype=np.uint8)
    out['ss_map_u8'] = pil_decode(map_png)
    for S in SS_SIZES:
        ref, largest = reference_labels(map_png, S)
        print('reference labels at %d: largest value before the cast %.4f, after %d' % (S, largest, int(ref.max())))
        out['ss_labels_ref%d' % S] = ref
        out['ss_labels_index%d' % S] = crop_interpolate((m[:, :, 0] // 32).astype(np.float32), S).astype(np.uint8)
    for name, stream in broken_streams(hand_stream('f1_c3_5x3')).items():
        out['broken_%s_png' % name] = np.frombuffer(stream, dtype=np.uint8)
    assert sorted(n for n, _ in BROKEN) == sorted(k[7:-4] for k in out if k.startswith('broken_'))
    np.savez_compressed(NPZ, **out)
    print('%s: %d good streams, %d bytes' % (NPZ, len(GOOD_NAMES), osp.getsize(NPZ)))


if __name__ == '__main__':
    sys.path.insert(0, osp.dirname(osp.dirname(HERE)))
    main()
