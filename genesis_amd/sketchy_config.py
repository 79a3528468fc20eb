"""Sketchy -- drop-in for the reference's `datasets/sketchy_config.py` without Pillow or torchvision.

Same Forge-style contract: importing this file registers the data flags with the reference's defaults (:28-32),
`load(cfg) -> (train, val, test)` builds the reference's three loaders (:43-61: train and valid at cfg.batch_size, test at
batch size 1, all shuffled, the short last batch kept), and each loader has `__len__`, `batch_size`, `__iter__`, and
`StopIteration` at the end of the epoch, after which it can be iterated again.  A loader yields {'input': fp32 [B,C,128,128]
in [0,1]} ON THE DEVICE: the stored 128 x 128 frames scaled by / 255, no crop and no resize (:89-92: to_tensor).

The file list of a split (:71-84) is <data_folder>/processed/<mode>_images.txt, one path per line, when that file exists;
otherwise the files <data_folder>/processed/<mode>/ep*/ep*.png are globbed and the list is written there, as the reference
does.  Reading, decoding and the order of an epoch: genesis_amd/png.py (PngFileLoader) and shapestacks_config.py; the order
is a numpy permutation seeded with cfg.seed, not torch's sampler.  `load(cfg, shard=(rank, world))` keeps every world-th
file of each split.  No throughput printout at load time."""
import os
import glob

from genesis_amd import compat as _compat

_compat.install()

from forge import flags  # noqa: E402
from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import data_cache, loading, png  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

flags.DEFINE_string('data_folder', 'data/sketchy', 'Path to data folder.')
flags.DEFINE_integer('num_workers', 4, 'Number of threads for loading data.')
flags.DEFINE_integer('img_size', 128, 'Dimension of images. Images are square.')
flags.DEFINE_integer('K_steps', 10, 'Number of object slots.')

MODES = ('train', 'valid', 'test')
IMG_SIZE = 128


def list_path(data_folder, mode):
    """Where the file list of a split lives: <data_folder>/processed/<mode>_images.txt."""
    return os.path.join(data_folder, 'processed', mode + '_images.txt')


def read_list(path):
    """The paths a list file holds, one per line, surrounding white space removed."""
    with open(path) as f:
        return [line.strip() for line in f]


def write_list(path, files):
    with open(path, 'w') as f:
        f.write(''.join(name + '\n' for name in files))


def split_files(data_folder, mode):
    """The paths of a split.  The list file decides when it exists; otherwise the frames are found on disk
    (processed/<mode>/ep*/ep*.png, in glob's order) and the list file is written, so that later runs skip the search."""
    if mode not in MODES:
        raise ValueError('sketchy: no split %r (one of %s)' % (mode, ', '.join(MODES)))
    listed = list_path(data_folder, mode)
    if os.path.exists(listed):
        files = read_list(listed)
        fprint('sketchy: %s split: %d frames listed in %s' % (mode, len(files), listed))
    else:
        files = glob.glob(os.path.join(data_folder, 'processed', mode, 'ep*', 'ep*.png'))
        write_list(listed, files)
        fprint('sketchy: %s split: %d frames found on disk, list written to %s' % (mode, len(files), listed))
    return files


def load(cfg, shard=None, device='cuda', **unused_kwargs):
    del unused_kwargs
    if not os.path.exists(cfg.data_folder):
        raise GenesisHipError('sketchy: data folder %s does not exist' % cfg.data_folder)
    if cfg.img_size != IMG_SIZE:                        # the frames are stored at 128 x 128 and are not resized
        raise AssertionError('sketchy: img_size must be %d, not %r' % (IMG_SIZE, cfg.img_size))
    fprint('sketchy: %d reader threads' % min(cfg.num_workers, loading.MAX_WORKERS))
    rank, world = loading.parse_shard(shard, 'sketchy')
    loaders = []
    for mode, batch_size, workers in (('train', cfg.batch_size, cfg.num_workers), ('valid', cfg.batch_size, cfg.num_workers),
                                      ('test', 1, 1)):
        files = split_files(cfg.data_folder, mode)[rank::world]
        loaders.append(png.PngFileLoader(files, batch_size, shuffle=True, seed=getattr(cfg, 'seed', 0), num_workers=workers,
                                         device=device, name='sketchy'))
    return data_cache.wrap_loaders(cfg, tuple(loaders), name='sketchy')
