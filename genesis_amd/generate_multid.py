"""Multi-dSprites generator -- drop-in for the reference's `scripts/generate_multid.py` without Pillow.

`generate(sprites, dataset_size, num_objects=None, unique=False)` returns what the reference's function returns: float32
frames [N,64,64,3] (byte / 255) and float64 instance masks [N,64,64,1].  It draws from Python's global `random` with the
reference's calls in the reference's order (:32-34, :48, :57, :61-67) -- per image `choice` x 3 for the background,
`randint(1, 4)` unless num_objects is given, and per object `randint(0, 737279)` then `choice` x 3, drawn again while
`unique` and the colour is already used in the image -- so a caller who seeds as the reference does gets its stream and its
bytes.  The draws are a few numbers per image and stay on the host; the pasting (:47-73, a Python loop over PIL images in the
reference) is gx_sprites_compose, in chunks of CHUNK images: the chunk's drawn sprites are fetched with `sprites[i]` (an
ndarray is fancy-indexed) into pinned memory, copied, composed in one launch, and the frames and masks copied back.

`main()` seeds `random` with 0 and writes the reference's twelve files in its order (rand4 training / validation / test, then
the unique-colour three) to the reference's paths; --sprites / --out / --sizes override the sprites file, the output folder
and the three split sizes.  The dSprites archive (dsprites_ndarray_co1sh3sc6or40x32y32_64x64.npz, key 'imgs') is not
downloaded: a missing file raises, naming it."""
import argparse
import os
import random

import numpy as np
import torch

from genesis_amd import feeder
from genesis_amd._lib import GenesisHipError

COLOUR_VALUES = [0, 63, 127, 191, 255]
MAX_SPRITE_INDEX = 737279               # randint's upper bound (:61): the last image of the dSprites archive
MAX_OBJECTS = feeder.MAX_SPRITES_PER_IMAGE
SIZE = feeder.SPRITE_SIZE
CHUNK = 2048                            # images composed per launch: at most 32 MB of sprites in pinned memory
SPRITES_FILE = 'data/multi_dsprites/dsprites-dataset/dsprites_ndarray_co1sh3sc6or40x32y32_64x64.npz'
OUT_FOLDER = 'data/multi_dsprites/processed'
SPLITS = (('training', 50000), ('validation', 10000), ('test', 10000))


def rand_rgb_tuple():
    return random.choice(COLOUR_VALUES), random.choice(COLOUR_VALUES), random.choice(COLOUR_VALUES)


def draw(num_images, num_objects=None, unique=False):
    """The host half of `num_images` images, consuming the global `random` stream exactly as the reference's loop does:
    (count int32 [n], sprite indices (a flat list, image after image, in paste order), colours uint8 [n, 5, 3])."""
    count = np.zeros(num_images, dtype=np.int32)
    colours = np.zeros((num_images, MAX_OBJECTS + 1, 3), dtype=np.uint8)
    indices = []
    for i in range(num_images):
        used = [rand_rgb_tuple()]
        num_sprites = random.randint(1, 4) if num_objects is None else num_objects
        for _ in range(num_sprites):
            indices.append(random.randint(0, MAX_SPRITE_INDEX))
            colour = rand_rgb_tuple()
            while unique and colour in used:
                colour = rand_rgb_tuple()
            used.append(colour)
        count[i] = num_sprites
        colours[i, :len(used)] = used
    return count, indices, colours


def fetch_sprites(sprites, indices, out):
    """out[j] = sprites[indices[j]] as uint8 with non-zero = set (np.array(sprites[i], dtype=bool), :62)."""
    k = len(indices)
    if isinstance(sprites, np.ndarray):
        if sprites.dtype == np.uint8:
            np.take(sprites, indices, axis=0, out=out[:k])
        else:
            out[:k] = sprites[indices] != 0
    else:
        for j, i in enumerate(indices):
            out[j] = np.asarray(sprites[i]) != 0
    return out[:k]


def generate(sprites, dataset_size, num_objects=None, unique=False, device='cuda'):
    if num_objects is not None and not 0 <= int(num_objects) <= MAX_OBJECTS:
        raise GenesisHipError('generate_multid: num_objects must be in 0..%d, not %r' % (MAX_OBJECTS, num_objects))
    shape = tuple(np.shape(sprites[0]))
    if shape != (SIZE, SIZE):
        raise GenesisHipError('generate_multid: sprites must be %d x %d, not %s' % (SIZE, SIZE, list(shape)))
    device = torch.device(device)
    if device.type != 'cuda':
        raise GenesisHipError('generate_multid: the images are composed on the HIP device; there is no CPU path')
    all_images = np.empty((dataset_size, SIZE, SIZE, 3), dtype=np.float32)
    all_instance_masks = np.empty((dataset_size, SIZE, SIZE, 1), dtype=np.float64)
    chunk = max(1, min(CHUNK, dataset_size))
    pin_sprites = torch.empty(chunk * MAX_OBJECTS, SIZE, SIZE, dtype=torch.uint8, pin_memory=True)
    dev_sprites = torch.empty(chunk * MAX_OBJECTS, SIZE, SIZE, dtype=torch.uint8, device=device)
    dev_img = torch.empty(chunk, SIZE, SIZE, 3, dtype=torch.float32, device=device)
    dev_mask = torch.empty(chunk, SIZE, SIZE, dtype=torch.uint8, device=device)
    pin_mask = torch.empty(chunk, SIZE, SIZE, dtype=torch.uint8, pin_memory=True)
    with torch.cuda.device(device):
        for a in range(0, dataset_size, chunk):
            n = min(chunk, dataset_size - a)
            count, indices, colours = draw(n, num_objects, unique)
            first = (np.cumsum(count) - count).astype(np.int32)
            k = len(indices)
            if k:
                fetch_sprites(sprites, indices, pin_sprites.numpy())
                dev_sprites[:k].copy_(pin_sprites[:k], non_blocking=True)
            stack = dev_sprites[:max(k, 1)]
            if int((first + count).max()) > max(k, 1):        # first + count against the stack, before the launch
                raise GenesisHipError('generate_multid: a sprite range reaches past the %d sprites of the chunk' % k)
            feeder.sprites_compose(stack, torch.from_numpy(first).to(device), torch.from_numpy(count).to(device),
                                   torch.from_numpy(colours).to(device), dev_img[:n], dev_mask[:n])
            torch.from_numpy(all_images[a:a + n]).copy_(dev_img[:n])          # waits for the launch
            pin_mask[:n].copy_(dev_mask[:n])
            all_instance_masks[a:a + n, :, :, 0] = pin_mask[:n].numpy()
            if (a + n) // 10000 > a // 10000:
                print(f"Processing [{(a + n) // 10000 * 10000} | {dataset_size}]")
    return all_images, all_instance_masks


def load_sprites(path):
    if not os.path.exists(path):
        raise FileNotFoundError('generate_multid: sprites file %s does not exist (the dSprites archive, key \'imgs\'; it is not '
                                'downloaded)' % path)
    return np.load(path, encoding='latin1')['imgs']


def main(argv=None):
    ap = argparse.ArgumentParser(description='Writes the Multi-dSprites .npy files multid_config.py reads.')
    ap.add_argument('--sprites', default=SPRITES_FILE, help='the dSprites .npz archive (key imgs)')
    ap.add_argument('--out', default=OUT_FOLDER, help='folder the twelve .npy files are written to')
    ap.add_argument('--sizes', type=int, nargs=3, default=[n for _, n in SPLITS], metavar=('TRAIN', 'VAL', 'TEST'),
                    help='frames of the three splits')
    ap.add_argument('--device', default='cuda')
    args = ap.parse_args(argv)
    sprites = load_sprites(args.sprites)
    os.makedirs(args.out, exist_ok=True)
    random.seed(0)
    for unique in (False, True):
        for (mode, _), size in zip(SPLITS, args.sizes):
            print('Generate %s images%s...' % (mode, ' (unique colours)' if unique else ''))
            images, masks = generate(sprites, size, unique=unique, device=args.device)
            print('Saving...')
            suffix = '_rand4_unique.npy' if unique else '_rand4.npy'
            np.save(os.path.join(args.out, mode + '_images' + suffix), images)
            np.save(os.path.join(args.out, mode + '_masks' + suffix), masks)
        print('Done!')


if __name__ == '__main__':
    main()
