"""Writes tests/golden/jpeg_pil.npz, the fixture of the JPEG decoder (genesis_amd/jpeg.py, gx_jpeg.cpp, gx_jpeg.hip):
for every case of CASES the JPEG byte string Pillow (libjpeg-turbo) encodes from a seeded image and the RGB pixels
Pillow decodes from that string (Image.open(...).convert('RGB')) -- the yardstick, at zero tolerance:
    <case>_jpeg   uint8 [n]         the stream
    <case>_rgb    uint8 [H, W, 3]   Pillow's decoded pixels
plus two streams the decoder must reject, `progressive_jpeg` and `grey_jpeg`.  The other rejected cases are made in
the tests by patching header bytes.

Also the tiny GQN TFRecord writer the tests use in tmp_path (write_gqn_tfrecord): tf.Example protos with `frames` (a
bytes_list of JPEG strings) and `cameras` (a float_list), framed with genesis_amd.tfrecord.masked_crc32c.  Importing this
module needs neither Pillow nor the fixture; only main() needs Pillow.

Run from the repository root: python tests/golden/make_golden_jpeg.py"""
import io
import os.path as osp
import struct
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
NPZ = osp.join(HERE, 'jpeg_pil.npz')

# (case, H, W, sampling class (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), quality, content, optimize, restart_marker_blocks)
CASES = [
    ('s64_420_q75_mixed', 64, 64, 2, 75, 'mixed', False, 0),
    ('s64_420_q30_smooth', 64, 64, 2, 30, 'smooth', False, 0),
    ('s64_420_q95_noise', 64, 64, 2, 95, 'noise', False, 0),
    ('s64_420_q100_mixed', 64, 64, 2, 100, 'mixed', False, 0),
    ('s64_420_q50_mixed_opt', 64, 64, 2, 50, 'mixed', True, 0),
    ('s64_420_q85_smooth_rst', 64, 64, 2, 85, 'smooth', False, 2),
    ('s64_444_q75_mixed', 64, 64, 0, 75, 'mixed', False, 0),
    ('s64_422_q75_mixed', 64, 64, 1, 75, 'mixed', False, 0),
    ('s64_444_q90_noise_opt_rst', 64, 64, 0, 90, 'noise', True, 3),
    ('s64_422_q30_smooth_rst', 64, 64, 1, 30, 'smooth', False, 1),
    ('s16_420_q75_mixed', 16, 16, 2, 75, 'mixed', False, 0),
    ('s16_444_q95_noise', 16, 16, 0, 95, 'noise', False, 0),
    ('s16_422_q50_mixed', 16, 16, 1, 50, 'mixed', False, 0),
    ('s8_420_q75_mixed', 8, 8, 2, 75, 'mixed', False, 0),
    ('s8_444_q100_noise', 8, 8, 0, 100, 'noise', False, 0),
    ('s8_422_q30_smooth', 8, 8, 1, 30, 'smooth', False, 0),
    ('s40x56_420_q75_mixed', 40, 56, 2, 75, 'mixed', False, 0),
    ('s40x56_422_q95_noise_opt', 40, 56, 1, 95, 'noise', True, 0),
    ('s40x56_444_q30_smooth', 40, 56, 0, 30, 'smooth', False, 0),
    ('s38x50_420_q85_mixed', 38, 50, 2, 85, 'mixed', False, 0),
    ('s38x50_422_q75_mixed', 38, 50, 1, 75, 'mixed', False, 0),
    ('s38x50_444_q60_mixed', 38, 50, 0, 60, 'mixed', False, 0),
    ('s17x33_420_q75_mixed', 17, 33, 2, 75, 'mixed', False, 0),
    ('s17x33_422_q90_smooth', 17, 33, 1, 90, 'smooth', False, 0),
    ('s17x33_444_q95_noise', 17, 33, 0, 95, 'noise', False, 0),
    ('s128_420_q90_mixed', 128, 128, 2, 90, 'mixed', False, 0),
]
CASE_NAMES = [c[0] for c in CASES]
GQN_CASES = [c[0] for c in CASES if (c[1], c[2], c[3]) == (64, 64, 2)]      # one geometry, as a GQN file holds


def case(name):
    return CASES[CASE_NAMES.index(name)]


def content_image(kind, H, W, seed):
    """A seeded uint8 [H, W, 3] image: 'smooth' (gradients and a slow wave), 'noise' (uniform bytes) or 'mixed' (smooth with
    hard-edged rectangles of saturated colour and a noisy quarter)."""
    rng = np.random.RandomState(seed)
    if kind == 'noise':
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([255.0 * x / max(W - 1, 1), 255.0 * y / max(H - 1, 1),
                    127.5 + 127.5 * np.sin(x / 5.0 + rng.rand() * 6.0) * np.cos(y / 7.0 + rng.rand() * 6.0)], axis=2)
    if kind == 'mixed':
        for _ in range(4):
            y0, x0 = rng.randint(0, H), rng.randint(0, W)
            img[y0:y0 + rng.randint(1, H // 2 + 2), x0:x0 + rng.randint(1, W // 2 + 2)] = rng.choice([0, 255], 3)
        img[:(H + 1) // 2, :(W + 1) // 2] += rng.randint(-60, 61, ((H + 1) // 2, (W + 1) // 2, 3))
    elif kind != 'smooth':
        raise ValueError(kind)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def encode(img, sampling, quality, optimize=False, restart_blocks=0, **extra):
    from PIL import Image
    buf = io.BytesIO()
    if restart_blocks:
        extra['restart_marker_blocks'] = restart_blocks
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling=sampling, optimize=optimize, **extra)
    return buf.getvalue()


def pil_decode(stream):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(stream))).convert('RGB'))


# ---- the GQN TFRecord writer (protobuf wire format written out by hand)
def _varint(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def _field(number, payload):
    return _varint((number << 3) | 2) + _varint(len(payload)) + payload


def gqn_example(frames, cameras):
    """One tf.Example: features { 'frames': bytes_list of the JPEG strings, 'cameras': float_list (packed) }."""
    bytes_list = b''.join(_field(1, bytes(f)) for f in frames)
    float_list = _field(1, struct.pack('<%df' % len(cameras), *cameras))
    entries = (_field(1, _field(1, b'frames') + _field(2, _field(1, bytes_list))) +
               _field(1, _field(1, b'cameras') + _field(2, _field(2, float_list))))
    return _field(1, entries)


def write_gqn_tfrecord(path, records):
    """records: a list of (frames, cameras) -> an uncompressed TFRecord file of tf.Example protos."""
    from genesis_amd.tfrecord import masked_crc32c
    with open(path, 'wb') as f:
        for frames, cameras in records:
            data = gqn_example(frames, cameras)
            head = struct.pack('<Q', len(data))
            f.write(head + struct.pack('<I', masked_crc32c(head)) + data + struct.pack('<I', masked_crc32c(data)))


def main():
    out = {}
    for i, (name, H, W, sampling, quality, kind, optimize, rst) in enumerate(CASES):
        img = content_image(kind, H, W, 9000 + i)
        stream = encode(img, sampling, quality, optimize, rst)
        rgb = pil_decode(stream)
        assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8
        out[name + '_jpeg'] = np.frombuffer(stream, dtype=np.uint8)
        out[name + '_rgb'] = rgb
        has_dri = b'\xff\xdd' in stream
        assert has_dri == bool(rst), (name, has_dri)
    img = content_image('mixed', 32, 32, 8999)
    out['progressive_jpeg'] = np.frombuffer(encode(img, 2, 75, progressive=True), dtype=np.uint8)
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img[:, :, 0]).save(buf, format='JPEG', quality=75)
    out['grey_jpeg'] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
    np.savez_compressed(NPZ, **out)
    print('%s: %d cases, %d bytes' % (NPZ, len(CASES), osp.getsize(NPZ)))


if __name__ == '__main__':
    sys.path.insert(0, osp.dirname(osp.dirname(HERE)))
    main()
