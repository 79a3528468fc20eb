"""ShapeStacks -- drop-in for the reference's `datasets/shapestacks_config.py` without Pillow, torchvision or matplotlib.

Same Forge-style contract: importing this file registers the data flags with the reference's defaults (:34-43),
`load(cfg) -> (train, val, test)` builds the reference's three loaders (:66-95: all at cfg.batch_size, all shuffled, the short
last batch kept), and each loader has `__len__`, `batch_size`, `__iter__`, and `StopIteration` at the end of the epoch, after
which it can be iterated again.  A loader yields {'input': fp32 [B,3,S,S] in [0,1], 'instances': int64 [B,1,S,S]} ON THE
DEVICE ('instances' only with cfg.load_instances).

The dataset (third_party/shapestacks/shapestacks_provider.py:34-67): <data_folder>/splits/<split_name>/{train,eval,test}.txt
lists scenarios, one per line; the frames of a scenario are the files of <data_folder>/recordings/<scenario> named
rgb-*-mono-0.png, in os.listdir order: 224 x 224 RGB PNGs.  The instance map of a frame (:151-154) is
<data_folder>/iseg/<scenario>/iseg-w=0-f=0-l=0-c=original-cam_<cam>-mono-0.map with cam = name.split('-')[5][4:]; a .map
file is a PNG.  Frames are centre-cropped to 196 (feeder.centre_box), resized to img_size with Pillow's bilinear filter
unless img_size is 196 (:126-129), and scaled by / 255; maps take the same crop and F.interpolate's nearest (:155-163).

What runs where.  cfg.num_workers threads (at most 16) read the files, check their chunks and inflate them in C
(gx_png_inflate; ctypes drops the GIL) straight into a pinned ring; per batch and kind one copy and ONE HIP launch
(gx_png_unfilter) undo the scanline filters, and the feeder's kernels crop, resample and scale (genesis_amd/png.py:
PngFileLoader).  No pixel is touched on the host.

Differences from the reference, on purpose:
  * Instance labels.  The reference's labels are ALL ZERO: load_segmap_as_matrix reads the map with matplotlib's imread,
    which returns float32 in [0, 1], divides by 32 (largest value 0.03), and the config casts to long.  `load(cfg)`
    reproduces that (rule 'shapestacks_reference').  `load(cfg, iseg_labels='index')` yields byte // 32 instead -- the
    encoding the map files are documented to have (eight labels in a uint8) -- so that ARI on ShapeStacks means something.
  * Order.  Every epoch is a fresh permutation from ONE generator per loader seeded with cfg.seed (numpy's, not torch's
    sampler): the order is not the reference's.  cfg.shuffle_test permutes the test file list once, from the same seed.
  * `load(cfg, shard=(rank, world))` keeps every world-th file of each split, from file `rank`, for one process per GPU.
  * No throughput printout at load time (the reference's loader_throughput consumes batches first)."""
import os
import shutil

import numpy as np

from genesis_amd import compat as _compat

_compat.install()

from forge import flags  # noqa: E402
from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import data_cache, loading, png  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

flags.DEFINE_string('data_folder', 'data/shapestacks', 'Path to data folder.')
flags.DEFINE_string('split_name', 'default', '{default, blocks_all, css_all}')
flags.DEFINE_integer('img_size', 64, 'Dimension of images. Images are square.')
flags.DEFINE_boolean('shuffle_test', False, 'Shuffle test set.')
flags.DEFINE_integer('num_workers', 4, 'Number of threads for loading data.')
flags.DEFINE_boolean('load_instances', True, 'Load instances.')
flags.DEFINE_boolean('copy_to_tmp', False, 'Copy files to /tmp.')
flags.DEFINE_integer('K_steps', 9, 'Number of recurrent steps.')

MAX_SHAPES = 6
CENTRE_CROP = 196
MODES = ('train', 'eval', 'test')
DATASET_PARTS = ('recordings', 'splits', 'iseg')     # what cfg.copy_to_tmp copies
TMP_FOLDER = '/tmp'
ISEG_LABELS = {'reference': 'shapestacks_reference', 'index': 'index'}


def frame_files(data_folder, split_name, mode):
    """The frames of a split, in the reference's order: the scenarios of splits/<split_name>/<mode>.txt (what follows the
    last newline is dropped), and of each the rgb-*-mono-0.png files of recordings/<scenario> as os.listdir lists them."""
    if mode not in MODES:
        raise ValueError('shapestacks: no split %r (one of %s)' % (mode, ', '.join(MODES)))
    with open(os.path.join(data_folder, 'splits', split_name, mode + '.txt')) as f:
        scenarios = f.read().split('\n')[:-1]
    files = []
    for scenario in scenarios:
        folder = os.path.join(data_folder, 'recordings', scenario)
        files += [os.path.join(folder, name) for name in os.listdir(folder)
                  if name.startswith('rgb-') and name.endswith('-mono-0.png')]
    return files


def map_file(data_folder, frame_file):
    """The instance map of a frame: iseg/<scenario>/iseg-w=0-f=0-l=0-c=original-cam_<cam>-mono-0.map."""
    parts = frame_file.split('/')
    cam = parts[-1].split('-')[5][4:]
    return os.path.join(data_folder, 'iseg', parts[-2], 'iseg-w=0-f=0-l=0-c=original-cam_' + cam + '-mono-0.map')


def copy_dataset(data_folder, target):
    """cfg.copy_to_tmp: copies the three directories a run reads into `target` (the reference copies them to /tmp, where an
    existing copy is an error, as it is here) and returns the folder to load from."""
    for part in DATASET_PARTS:
        source, copy = os.path.join(data_folder, part), os.path.join(target, part)
        fprint('shapestacks: copying %s -> %s' % (source, copy))
        shutil.copytree(source, copy)
    return target


def split_files(cfg, mode, shard=None):
    """(frame files, map files or None) of one split after cfg.shuffle_test and the shard."""
    files = frame_files(cfg.data_folder, cfg.split_name, mode)
    if mode == 'test' and cfg.shuffle_test:
        fprint('shapestacks: test split: %d files permuted once (shuffle_test)' % len(files))
        order = np.random.RandomState(int(getattr(cfg, 'seed', 0)) % (1 << 32)).permutation(len(files))
        files = [files[i] for i in order]
    rank, world = loading.parse_shard(shard, 'shapestacks')
    files = files[rank::world]
    maps = [map_file(cfg.data_folder, f) for f in files] if cfg.load_instances else None
    return files, maps


def load(cfg, iseg_labels='reference', shard=None, device='cuda', **unused_kwargs):
    del unused_kwargs
    if iseg_labels not in ISEG_LABELS:
        raise GenesisHipError('shapestacks: iseg_labels must be one of %s, not %r' % (sorted(ISEG_LABELS), iseg_labels))
    if not os.path.exists(cfg.data_folder):
        raise GenesisHipError('shapestacks: data folder %s does not exist' % cfg.data_folder)
    fprint('shapestacks: %d reader threads' % min(cfg.num_workers, loading.MAX_WORKERS))

    if cfg.copy_to_tmp:
        cfg.data_folder = copy_dataset(cfg.data_folder, TMP_FOLDER)

    size = None if cfg.img_size == CENTRE_CROP else int(cfg.img_size)
    loaders = []
    for mode, workers in (('train', cfg.num_workers), ('eval', cfg.num_workers), ('test', 1)):
        files, maps = split_files(cfg, mode, shard)
        loaders.append(png.PngFileLoader(files, cfg.batch_size, size=size, crop=CENTRE_CROP,
                                         resize='bilinear' if size else 'nearest', map_files=maps,
                                         label_rule=ISEG_LABELS[iseg_labels], shuffle=True, seed=getattr(cfg, 'seed', 0),
                                         num_workers=workers, device=device, name='shapestacks'))
    return data_cache.wrap_loaders(cfg, tuple(loaders), name='shapestacks')
