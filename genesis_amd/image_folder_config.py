"""A folder of image files -- the data config for a user's own images, which the reference's users get by pointing a
torchvision dataset at a directory; without Pillow or torchvision.

The same Forge-style contract as the other data configs: importing this file registers the data flags,
`load(cfg) -> (train, val, test)` builds three loaders at cfg.batch_size, all shuffled, the short last batch kept, and each
loader has `__len__`, `batch_size`, `__iter__`, and `StopIteration` at the end of the epoch, after which it can be iterated
again.  A loader yields {'input': fp32 [B, 3, img_size, img_size] in [0, 1]} ON THE DEVICE: every file -- PNG or JPEG, of any
size, grey, RGB or RGBA -- under Resize(img_size, BILINEAR) + CenterCrop(img_size) + ToTensor, the transform the reference
applies to loose frames (datasets/apc_config.py:144-147), bit for bit what Pillow computes (genesis_amd/imagefile.py).

Splits.  When <data_folder>/train, /val and /test all exist, each folder is a split: its .png / .jpg / .jpeg files (any letter
case), found recursively, sorted by path.  Otherwise every such file under <data_folder> is listed, sorted, shuffled with
random.Random(0) and split a tenth to val, a tenth to test and the rest to train, the way the reference splits APC's scenes
(datasets/apc_config.py:58-64).  Either way the list of a split is written to <data_folder>/<mode>_images.txt, one path
relative to <data_folder> per line, and read from there when it exists.  The order of an epoch is a numpy permutation seeded
with cfg.seed, not torch's sampler.  `load(cfg, shard=(rank, world))` keeps every world-th file of each split.  There are no
label maps: a folder of images has none."""
import os
import random

from genesis_amd import compat as _compat

_compat.install()

from forge import flags  # noqa: E402
from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import data_cache, imagefile, loading  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

flags.DEFINE_string('data_folder', 'data/images', 'Path to data folder.')
flags.DEFINE_integer('img_size', 64, 'Dimension of images. Images are square.')
flags.DEFINE_integer('num_workers', 4, 'Number of threads for loading data.')
flags.DEFINE_integer('K_steps', 7, 'Number of object slots.')

MODES = ('train', 'val', 'test')
EXTENSIONS = ('.png', '.jpg', '.jpeg')


def list_path(data_folder, mode):
    """Where the file list of a split lives: <data_folder>/<mode>_images.txt."""
    return os.path.join(data_folder, mode + '_images.txt')


def find_images(folder):
    """The image files under folder (recursively), as paths relative to it, sorted."""
    found = []
    for root, _, names in os.walk(folder):
        for name in names:
            if os.path.splitext(name)[1].lower() in EXTENSIONS:
                found.append(os.path.relpath(os.path.join(root, name), folder))
    return sorted(found)


def has_split_folders(data_folder):
    return all(os.path.isdir(os.path.join(data_folder, mode)) for mode in MODES)


def seeded_split(files):
    """{mode: files}: the sorted list shuffled with random.Random(0), a tenth each to val and test, the rest to train; each
    split's list sorted again, as the reference writes it."""
    files = sorted(files)
    random.Random(0).shuffle(files)
    tenth = len(files) // 10
    return {'val': sorted(files[:tenth]), 'test': sorted(files[tenth:2 * tenth]), 'train': sorted(files[2 * tenth:])}


def split_files(data_folder, mode):
    """The paths of a split, relative to data_folder.  The list file decides when it exists; otherwise the files are found
    on disk and the list files are written, so that later runs skip the search and keep the split."""
    if mode not in MODES:
        raise ValueError('image_folder: no split %r (one of %s)' % (mode, ', '.join(MODES)))
    listed = list_path(data_folder, mode)
    if not os.path.exists(listed):
        if has_split_folders(data_folder):
            splits = {m: [os.path.join(m, f) for f in find_images(os.path.join(data_folder, m))] for m in MODES}
        else:
            splits = seeded_split(find_images(data_folder))
        for m in MODES:
            if not os.path.exists(list_path(data_folder, m)):
                with open(list_path(data_folder, m), 'w') as f:
                    f.write(''.join(name + '\n' for name in splits[m]))
        fprint('image_folder: %s split: %d files found on disk, list written to %s' % (mode, len(splits[mode]), listed))
        return splits[mode]
    with open(listed) as f:
        files = [line.strip() for line in f if line.strip()]
    fprint('image_folder: %s split: %d files listed in %s' % (mode, len(files), listed))
    return files


def load(cfg, shard=None, device='cuda', **unused_kwargs):
    del unused_kwargs
    if not os.path.isdir(cfg.data_folder):
        raise GenesisHipError('image_folder: data folder %s does not exist' % cfg.data_folder)
    fprint('image_folder: %d reader threads' % min(cfg.num_workers, loading.MAX_WORKERS))
    loaders = []
    for mode in MODES:
        files = [os.path.join(cfg.data_folder, f) for f in split_files(cfg.data_folder, mode)]
        loaders.append(imagefile.ImageFileLoader(files, cfg.batch_size, cfg.img_size, shuffle=True, seed=getattr(cfg, 'seed', 0),
                                                 num_workers=cfg.num_workers, device=device, shard=shard,
                                                 max_side=getattr(cfg, 'max_side', 1024), name='image_folder'))
    return data_cache.wrap_loaders(cfg, tuple(loaders), name='image_folder')
