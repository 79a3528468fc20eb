"""Writes tests/golden/feeder_pil.npz: Pillow's crop + BILINEAR resize of seeded uint8 frames, the expected outputs of the
feeder's bilinear transform (genesis_amd/feeder.py transform_frames, resize='bilinear').  What torchvision's
CenterCrop + Resize do to a PIL image (datasets/shapestacks_config.py:126-130) is Image.crop then Image.resize(BILINEAR).

The inputs are not stored: tests/test_feeder_transform_*.py regenerate them with feeder_case_frames() and check them
against the stored checksum.  Run from the repository root: python tests/golden/make_golden_feeder.py"""
import os.path as osp
import zlib

import numpy as np

# (name, frames [B, Hs, Ws, C], crop window (top, left, h, w), output (H, W))
CASES = [
    ('shapestacks64', (2, 224, 224, 3), (14, 14, 196, 196), (64, 64)),
    ('shapestacks128', (1, 224, 224, 3), (14, 14, 196, 196), (128, 128)),
    ('clevr64', (2, 240, 320, 3), (24, 64, 192, 192), (64, 64)),
    ('up48_96', (1, 48, 48, 3), (0, 0, 48, 48), (96, 96)),
    ('odd_gray', (2, 100, 77, 1), (3, 2, 95, 71), (33, 50)),
    ('tiny', (2, 7, 9, 3), (0, 0, 7, 9), (5, 13)),
    ('ratio16_gray', (2, 512, 520, 1), (0, 4, 512, 512), (32, 32)),
    ('ratio15_rgb', (1, 480, 480, 3), (0, 15, 480, 450), (32, 30)),
    # 301 x 3 bytes a row: two column tiles of 151 and 150 (a ragged last tile), and bands of 3 rows (a ragged last band)
    ('ragged_tile', (1, 64, 320, 3), (0, 5, 64, 310), (8, 301)),
]


def feeder_case_frames(name):
    """uint8 [B, Hs, Ws, C] inputs of case `name`, from a seeded RandomState (same in the script and the tests)."""
    i = [c[0] for c in CASES].index(name)
    return np.random.RandomState(1000 + i).randint(0, 256, CASES[i][1]).astype(np.uint8)


def checksum(a):
    return np.int64(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def pil_crop_resize(frame, box, size):
    from PIL import Image
    top, left, h, w = box
    im = Image.fromarray(frame if frame.shape[2] == 3 else frame[:, :, 0])
    r = np.asarray(im.crop((left, top, left + w, top + h)).resize((size[1], size[0]), Image.BILINEAR))
    return r if r.ndim == 3 else r[:, :, None]


def main():
    out = {}
    for name, _, box, size in CASES:
        frames = feeder_case_frames(name)
        out[name + '_in_crc'] = checksum(frames)
        out[name + '_out'] = np.stack([pil_crop_resize(f, box, size) for f in frames])
    path = osp.join(osp.dirname(osp.abspath(__file__)), 'feeder_pil.npz')
    np.savez_compressed(path, **out)
    print(path, osp.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
