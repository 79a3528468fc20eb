"""Writes tests/golden/imagefile_pil.npz, the fixture of the loose-image-file path (genesis_amd/imagefile.py, gx_jpeg.cpp's
_any entry points, gx_imagefile.hip), with Pillow only.  For every case of JPEG_CASES and PNG_CASES:
    <case>_stream   uint8 [n]            the stream of a seeded image: JPEGs encoded by Pillow, PNGs assembled with all five
                                         filter types in every file (encode_png says why)
    <case>_u8       uint8 [H, W(, C)]    the pixels Pillow decodes from it, in the file's own mode (L, RGB or RGBA)
    <case>_s<S>     uint8 [S, S, 3]      for S in SIZES: torchvision's Resize(S) + CenterCrop(S) on the PIL image, restated:
                                         Image.open(f).convert('RGB').resize((w', h'), Image.BILINEAR).crop(window)
plus four streams the decoder must refuse: refuse_progressive, refuse_cmyk, refuse_palette, refuse_png16.  The yardstick is at
zero tolerance.  The archive is written with fixed time stamps, so that running this again gives back the committed file
byte for byte.  `--dump DIR` also writes every stream as a file (DIR/<case>.jpg|.png: the input of
tools/probe/imagefile_host_check.cpp).  Importing this module needs neither Pillow nor the fixture; only main() needs Pillow.

The frames are the smallest at which tiling, halos and index arithmetic can fail (sizes are width x height): one pixel; one
MCU; 7 x 9 (no whole block); 136 x 24 and 24 x 136 (more than GX_JPEGR_BLOCKS_PER_WG = 128 blocks, three pixel tiles of 64
columns / nine of 16 rows); 145 x 131 4:2:0, 264 x 40 4:2:2 and 131 x 145 4:4:4 (odd sizes, three and more tiles on both axes,
chroma edges inside an MCU); a 200 x 200 grey frame; 520 x 16, 16 x 520 and 2056 x 8 (long rows and columns, byte offsets past
2^15); and beside the PNG sizes 7 x 9, 145 x 131 and 520 x 16 a 9 x 700 RGBA frame: three bands of the unfilter kernel's
1024 / 4 rows, each handing its last row to the next.

Run from the repository root: python tests/golden/make_golden_imagefile.py [--dump DIR]"""
import io
import os
import os.path as osp
import sys
import zipfile
import zlib

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
NPZ = osp.join(HERE, 'imagefile_pil.npz')
SIZES = (8, 20, 64)

# (case, W, H, sampling class (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0; None: grey), quality, content, restart_marker_blocks)
JPEG_CASES = [
    ('j1x1_420_q75', 1, 1, 2, 75, 'mixed', 0),
    ('j16x16_420_q100', 16, 16, 2, 100, 'noise', 0),
    ('j7x9_422_q30', 7, 9, 1, 30, 'mixed', 0),
    ('j136x24_444_q75', 136, 24, 0, 75, 'mixed', 0),
    ('j24x136_420_q75_rst', 24, 136, 2, 75, 'mixed', 3),
    ('j145x131_420_q75', 145, 131, 2, 75, 'mixed', 0),
    ('j264x40_422_q100', 264, 40, 1, 100, 'smooth', 0),
    ('j131x145_444_q30', 131, 145, 0, 30, 'mixed', 0),
    ('j200x200_grey_q75', 200, 200, None, 75, 'mixed', 0),
    ('j520x16_420_q75', 520, 16, 2, 75, 'smooth', 0),
    ('j16x520_422_q75', 16, 520, 1, 75, 'smooth', 0),
    ('j2056x8_420_q30', 2056, 8, 2, 30, 'smooth', 0),
]
# (case, W, H, C, content)
PNG_CASES = [(('p%dx%d_' % (w, h)) + {1: 'grey', 3: 'rgb', 4: 'rgba'}[c], w, h, c, kind)
             for (w, h, kind) in ((7, 9, 'noise'), (145, 131, 'mixed'), (520, 16, 'mixed')) for c in (1, 3, 4)]
PNG_CASES.append(('p9x700_rgba', 9, 700, 4, 'smooth'))      # three bands of the unfilter kernel's 1024 / 4 rows
JPEG_NAMES = [c[0] for c in JPEG_CASES]
PNG_NAMES = [c[0] for c in PNG_CASES]
CASE_NAMES = JPEG_NAMES + PNG_NAMES
REFUSED = ('refuse_progressive', 'refuse_cmyk', 'refuse_palette', 'refuse_png16')


def case_size(name):
    """(H, W) of a case."""
    for c in JPEG_CASES + PNG_CASES:
        if c[0] == name:
            return c[2], c[1]
    raise KeyError(name)


def content_image(kind, H, W, C, seed):
    """A seeded uint8 [H, W, C] image: 'smooth' (gradients and a slow wave), 'noise' (uniform bytes) or 'mixed' (smooth with
    hard-edged rectangles of saturated colour and a noisy corner)."""
    rng = np.random.RandomState(seed)
    if kind == 'noise':
        return rng.randint(0, 256, (H, W, C)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    planes = [255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1),
              127.5 + 127.5 * np.sin(x / 5.0 + rng.rand() * 6.0) * np.cos(y / 7.0 + rng.rand() * 6.0),
              255.0 - 200.0 * x * y / max((W - 1) * (H - 1), 1)]
    img = np.stack(planes[:C] if C != 1 else [planes[2]], axis=2)
    if kind == 'mixed':
        for _ in range(4):
            y0, x0 = rng.randint(0, H), rng.randint(0, W)
            img[y0:y0 + rng.randint(1, H // 2 + 2), x0:x0 + rng.randint(1, W // 2 + 2)] = rng.choice([0, 255], C)
        h4, w4 = (H + 3) // 4, (W + 3) // 4
        img[:h4, :w4] += rng.randint(-60, 61, (h4, w4, C))
    elif kind != 'smooth':
        raise ValueError(kind)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def pil_image(img):
    from PIL import Image
    return Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img)


def encode_jpeg(img, sampling, quality, restart_blocks=0, **extra):
    buf = io.BytesIO()
    if restart_blocks:
        extra['restart_marker_blocks'] = restart_blocks
    if sampling is not None:
        extra['subsampling'] = sampling
    pil_image(img).save(buf, format='JPEG', quality=quality, **extra)
    return buf.getvalue()


def encode_png(img):
    """A PNG stream of img whose row r has filter r % 5.  Pillow's own encoder never chooses the Average filter, whatever the
    content, so the rows are filtered and the chunks assembled by make_golden_png (struct + zlib); Pillow DECODES the stream,
    which is what the yardstick is."""
    import make_golden_png as MP
    return MP.assemble(img, MP.row_filters(img.shape[0], MP.CYCLE))


def resize_crop_geometry(H, W, S):
    """torchvision's Resize(S) + CenterCrop(S): (h', w', top', left')."""
    if W <= H:
        w2, h2 = S, int(S * H / W)
    else:
        w2, h2 = int(S * W / H), S
    return h2, w2, int(round((h2 - S) / 2.0)), int(round((w2 - S) / 2.0))


def pil_transform(stream, S):
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(stream))).convert('RGB')
    h2, w2, top, left = resize_crop_geometry(im.height, im.width, S)
    out = im.resize((w2, h2), Image.BILINEAR).crop((left, top, left + S, top + S))
    return np.asarray(out)


def png_row_filters(stream):
    """The filter byte of every row of an 8-bit, non-interlaced PNG stream."""
    s = bytes(stream)
    at, idat, ihdr = 8, b'', None
    while at < len(s):
        n = int.from_bytes(s[at:at + 4], 'big')
        kind = s[at + 4:at + 8]
        if kind == b'IHDR':
            ihdr = s[at + 8:at + 8 + n]
        if kind == b'IDAT':
            idat += s[at + 8:at + 8 + n]
        at += 12 + n
    W, H = int.from_bytes(ihdr[:4], 'big'), int.from_bytes(ihdr[4:8], 'big')
    C = {0: 1, 2: 3, 6: 4}[ihdr[9]]
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + W * C)
    return rows[:, 0]


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same file."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def build():
    from PIL import Image
    out = {}
    for i, (name, W, H, sampling, quality, kind, rst) in enumerate(JPEG_CASES):
        img = content_image(kind, H, W, 1 if sampling is None else 3, 7000 + i)
        stream = encode_jpeg(img, sampling, quality, rst)
        assert (b'\xff\xdd' in stream) == bool(rst), name
        out[name + '_stream'] = np.frombuffer(stream, dtype=np.uint8)
    filters = np.zeros(5, dtype=np.int64)
    for i, (name, W, H, C, kind) in enumerate(PNG_CASES):
        stream = encode_png(content_image(kind, H, W, C, 7100 + i))
        counts = np.bincount(png_row_filters(stream), minlength=5)
        assert (counts > 0).all(), (name, counts)                # all five filter types are present in every file
        filters += counts
        out[name + '_stream'] = np.frombuffer(stream, dtype=np.uint8)
    print('PNG rows per filter 0..4: %s' % filters.tolist())
    for name in CASE_NAMES:
        stream = out[name + '_stream']
        im = Image.open(io.BytesIO(bytes(stream)))
        H, W = case_size(name)
        assert (im.height, im.width) == (H, W) and im.mode in ('L', 'RGB', 'RGBA'), (name, im.size, im.mode)
        out[name + '_u8'] = np.asarray(im)
        for S in SIZES:
            t = pil_transform(stream, S)
            assert t.shape == (S, S, 3) and t.dtype == np.uint8
            out['%s_s%d' % (name, S)] = t
    base = content_image('mixed', 32, 32, 3, 6999)
    out['refuse_progressive'] = np.frombuffer(encode_jpeg(base, 2, 75, progressive=True), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(base).convert('CMYK').save(buf, format='JPEG', quality=75)
    out['refuse_cmyk'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(base).convert('P', palette=Image.ADAPTIVE, colors=16).save(buf, format='PNG')
    out['refuse_palette'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray((base[:, :, 0].astype(np.uint16) * 257)).save(buf, format='PNG')
    out['refuse_png16'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    return out


def dump(out, folder):
    os.makedirs(folder, exist_ok=True)
    for name in CASE_NAMES + list(REFUSED):
        stream = bytes(out[name + '_stream'] if name in CASE_NAMES else out[name])
        ext = '.png' if stream[:4] == b'\x89PNG' else '.jpg'
        with open(osp.join(folder, name + ext), 'wb') as f:
            f.write(stream)


def main(argv):
    out = build()
    write_npz(NPZ, out)
    print('%s: %d cases, %d bytes' % (NPZ, len(CASE_NAMES), osp.getsize(NPZ)))
    if '--dump' in argv:
        dump(out, argv[argv.index('--dump') + 1])


if __name__ == '__main__':
    sys.path.insert(0, HERE)
    main(sys.argv[1:])
