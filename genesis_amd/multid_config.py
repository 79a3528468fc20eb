"""Multi-dSprites -- drop-in for the reference's `datasets/multid_config.py` without DataLoader workers or torchvision.

Same Forge-style contract: importing this file registers the data flags with the reference's defaults (:28-39),
`load(cfg) -> (train, val, test)` builds the reference's three loaders (:68-94: all at cfg.batch_size, all shuffled, the short
last batch kept), and each loader has `__len__` = ceil(N / B), `batch_size`, `__iter__`, and `StopIteration` at the end of the
epoch, after which it can be iterated again.  A loader yields {'input': fp32 [B,3,S,S], 'instances': int64 [B,1,S,S]} ON THE
DEVICE ('instances' only with cfg.load_instances).

The files (:59-66, :119-123): <data_folder>/{training,validation,test}_images_rand4[_unique].npy, and for each the masks file
named by replacing 'images' with 'masks'.  scripts/generate_multid.py (here: genesis_amd/generate_multid.py) writes float32
frames [N,64,64,3] already divided by 255 and float64 masks [N,64,64,1].  ToTensor (:133, :139) moves HWC to CHW and divides
uint8 by 255 but leaves a float array as it is, so image files may be float32 (passed through) or uint8 (/ 255); mask files
may be uint8, int32, int64, float32 or float64 ([N,H,W,1] or [N,H,W]) and come out as int64 by truncation
(.type(LongTensor), :143).  With img_size != the stored size both are resampled nearest (F.interpolate's default, :134-142).

What runs where.  mem_map=False (the default): the split is RESIDENT.  The file is uploaded once, in chunks through two pinned
buffers, in its stored dtype; masks are narrowed to uint8 on the way when every label survives the round trip (checked per
chunk; a split with a label that does not fit is uploaded in its stored dtype instead).  50 000 float32 frames are 2.4 GB.
An epoch uploads its permutation (int64) once; a batch is then one launch of gx_rows_gather_f32chw and one of
gx_rows_gather_labels on the current stream and nothing else: no host copy, no synchronisation.  mem_map=True: the arrays
stay on the host (np.load(mmap_mode='r')); a batch's rows are gathered into a ring of pinned staging buffers, copied on a side
stream one batch ahead, and converted by the same two kernels without an index vector.

Differences from the reference, on purpose:
  * Order.  Every epoch is a fresh permutation from ONE numpy generator per loader seeded with cfg.seed (not torch's
    sampler): the order is not the reference's.  After `__iter__` the loader's `order` holds the epoch's row numbers.
  * `load(cfg, shard=(rank, world))` keeps the rows with index % world == rank of each split, for one process per GPU.
  * `num_workers` is accepted and unused: there is no per-sample host work to spread.
  * No throughput printout at load time (the reference's loader_throughput consumes batches first)."""
import os
import time

import numpy as np
import torch

from genesis_amd import compat as _compat

_compat.install()

from forge import flags  # noqa: E402
from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import feeder  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.loading import SlotEvents, host_wait, parse_shard  # noqa: E402

flags.DEFINE_string('data_folder', 'data/multi_dsprites/processed', 'Path to data folder.')
flags.DEFINE_boolean('unique_colours', False, 'Dataset with unique colours.')
flags.DEFINE_boolean('load_instances', True, 'Load instances.')
flags.DEFINE_integer('img_size', 64, 'Dimension of images. Images are square.')
flags.DEFINE_integer('num_workers', 4, 'Number of threads for loading data.')
flags.DEFINE_boolean('mem_map', False, 'Use memory mapping.')
flags.DEFINE_integer('K_steps', 5, 'Number of recurrent steps.')

MODES = ('training', 'validation', 'test')
IMAGE_DTYPES = ('float32', 'uint8')
MASK_DTYPES = ('uint8', 'int32', 'int64', 'float32', 'float64')
UPLOAD_CHUNK_BYTES = 64 << 20          # of each of the two pinned buffers a resident split is uploaded through
RING_DEPTH = 8                         # staged batches of the host-memmap mode


def file_name(mode, unique_colours):
    """The image file of a split: {training,validation,test}_images_rand4[_unique].npy (:59-66)."""
    if mode not in MODES:
        raise ValueError('multid: no split %r (one of %s)' % (mode, ', '.join(MODES)))
    return '%s_images_rand4%s.npy' % (mode, '_unique' if unique_colours else '')


def mask_path(image_path):
    """The masks file of an image file (:120): every 'images' of the path replaced by 'masks', as the reference does."""
    return image_path.replace('images', 'masks')


def open_split(image_path, load_instances=True):
    """(frames, masks or None): the two arrays of a split, memory-mapped and checked.  frames [N,H,W,3] float32 or uint8;
    masks [N,H,W] (the stored last axis of 1 dropped) in one of MASK_DTYPES."""
    frames = np.load(image_path, mmap_mode='r')
    if frames.ndim != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise GenesisHipError('multid: %s holds %s %s; frames must be [N,H,W,3]' % (image_path, frames.dtype, list(frames.shape)))
    if frames.dtype.name not in IMAGE_DTYPES:
        raise GenesisHipError('multid: %s holds %s %s; frames must be float32 (in [0,1]) or uint8' %
                              (image_path, frames.dtype, list(frames.shape)))
    if not load_instances:
        return frames, None
    path = mask_path(image_path)
    masks = np.load(path, mmap_mode='r')
    stored = list(masks.shape)
    if masks.ndim == 4 and masks.shape[3] == 1:
        masks = masks[..., 0]
    if masks.ndim != 3:
        raise GenesisHipError('multid: %s holds %s %s; masks must be [N,H,W,1] or [N,H,W]' % (path, masks.dtype, stored))
    if masks.dtype.name not in MASK_DTYPES:
        raise GenesisHipError('multid: %s holds %s %s; masks must be one of %s' % (path, masks.dtype, stored, ', '.join(MASK_DTYPES)))
    if masks.shape[0] != frames.shape[0]:
        raise GenesisHipError('multid: %s holds %d frames but %s holds %d masks' % (image_path, frames.shape[0], path, masks.shape[0]))
    if masks.shape[1:] != frames.shape[1:3]:
        raise GenesisHipError('multid: %s holds %s %s, which do not match the %d x %d frames of %s' %
                              (path, masks.dtype, stored, frames.shape[1], frames.shape[2], image_path))
    return frames, masks


def narrow_uint8(chunk):
    """A chunk of label maps as uint8 when every value survives the round trip, else None."""
    lo, hi = chunk.min(), chunk.max()
    if not (lo >= 0 and hi <= 255):                 # also false for NaN
        return None
    u8 = chunk.astype(np.uint8)
    return u8 if np.array_equal(u8, chunk) else None


def upload(array, device, narrow=False):
    """A host array (a memmap, or a strided view of one) -> a device tensor, in chunks of whole rows through two pinned
    buffers on the current stream.  narrow: to uint8, each chunk checked with narrow_uint8; returns None at the first chunk
    that does not fit (the caller then uploads the stored dtype)."""
    n = array.shape[0]
    dtype = np.dtype(np.uint8) if narrow else array.dtype
    row_bytes = int(np.prod(array.shape[1:])) * array.dtype.itemsize      # of the stored dtype: what the host touches per row
    rows = max(1, min(n, UPLOAD_CHUNK_BYTES // row_bytes))
    tdtype = torch.from_numpy(np.empty(0, dtype=dtype)).dtype
    dev = torch.empty(array.shape, dtype=tdtype, device=device)
    pinned = [torch.empty((rows,) + tuple(array.shape[1:]), dtype=tdtype, pin_memory=True) for _ in range(min(2, -(-n // rows)))]
    copied = [None] * len(pinned)
    stream = torch.cuda.current_stream(device)
    for k, a in enumerate(range(0, n, rows)):
        b = min(a + rows, n)
        chunk = array[a:b]
        s = k % len(pinned)
        host_wait(copied[s])                      # the copy that last read this pinned buffer has run
        if narrow:
            chunk = narrow_uint8(np.ascontiguousarray(chunk))
            if chunk is None:
                stream.synchronize()               # the pinned buffers are freed on return
                return None
        np.copyto(pinned[s].numpy()[:b - a], chunk, casting='unsafe')
        dev[a:b].copy_(pinned[s][:b - a], non_blocking=True)
        copied[s] = torch.cuda.Event()
        copied[s].record(stream)
    stream.synchronize()                           # once per split, at load time: the pinned buffers are freed on return
    return dev


def check_order(order, n):
    """An epoch's index vector against [0, n), on the host, before it is uploaded: the gather kernels do not check."""
    if len(order) and (int(order.min()) < 0 or int(order.max()) >= n):
        raise GenesisHipError('multid: an index of the epoch (%d .. %d) is outside the %d rows of the split'
                              % (int(order.min()), int(order.max()), n))


class MultidLoader(object):
    """One split.  `order` holds the file's row numbers in the order of the current epoch; batch i is rows
    order[i * B : (i + 1) * B]."""

    def __init__(self, image_path, batch_size, img_size=64, load_instances=True, mem_map=False, seed=0, shard=None,
                 device='cuda'):
        rank, world = parse_shard(shard, 'multid')
        if int(batch_size) <= 0:
            raise GenesisHipError('multid: batch_size must be positive, not %r' % (batch_size,))
        self.path = image_path
        self.batch_size = int(batch_size)
        self.img_size = int(img_size)
        self.mem_map = bool(mem_map)
        self.device = torch.device(device)
        self.frames, self.masks = open_split(image_path, load_instances)
        self.rows = np.arange(rank, self.frames.shape[0], world, dtype=np.int64)     # the file's rows this loader serves
        self.num_frames = len(self.rows)
        self.length = -(-self.num_frames // self.batch_size)
        self.rng = np.random.RandomState(int(seed) % (1 << 32))
        self.order = None
        self.pos = 0
        self.dev_frames = self.dev_masks = self.dev_order = None
        self.ring = None
        if self.device.type != 'cuda':
            raise GenesisHipError('multid: the loader delivers device batches; there is no CPU path (device %s)' % self.device)
        if not self.mem_map and self.num_frames:
            self._make_resident(rank, world)

    def _make_resident(self, rank, world):
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            self.dev_frames = upload(self.frames[rank::world], self.device)
            if self.masks is not None:
                mine = self.masks[rank::world]
                if self.masks.dtype != np.uint8:
                    self.dev_masks = upload(mine, self.device, narrow=True)
                if self.dev_masks is None:
                    self.dev_masks = upload(mine, self.device)
        held = self.dev_frames.numel() * self.dev_frames.element_size()
        if self.dev_masks is not None:
            held += self.dev_masks.numel() * self.dev_masks.element_size()
        fprint('multid: %s: %d frames resident on %s (%.1f MB, frames %s, masks %s) in %.2f s'
               % (os.path.basename(self.path), self.num_frames, self.device, held / 1e6, self.frames.dtype,
                  'none' if self.dev_masks is None else '%s as %s' % (self.masks.dtype, str(self.dev_masks.dtype).split('.')[-1]),
                  time.perf_counter() - t0))

    def __len__(self):
        return self.length

    def __iter__(self):
        perm = self.rng.permutation(self.num_frames).astype(np.int64)
        check_order(perm, self.num_frames)
        self.order = self.rows[perm]
        self.pos = 0
        if self.mem_map:
            if self.ring is None:
                self.ring = _StagingRing(self)
            self.ring.start()
        elif self.num_frames:
            self.dev_order = torch.from_numpy(perm).to(self.device)      # the epoch's one upload: positions in the resident split
        return self

    def __next__(self):
        if self.order is None:
            iter(self)
        if self.pos >= self.num_frames:
            raise StopIteration
        first = self.pos
        B = min(self.batch_size, self.num_frames - first)
        self.pos = first + B
        size = None if self.img_size == self.frames.shape[1] == self.frames.shape[2] else self.img_size
        if self.mem_map:
            return self.ring.next(first, B, size)
        batch = {'input': feeder.rows_gather(self.dev_frames, self.dev_order, first, B, size)}
        if self.dev_masks is not None:
            batch['instances'] = feeder.rows_gather_labels(self.dev_masks, self.dev_order, first, B, size)
        return batch

    def close(self):
        self.ring = None
        self.dev_frames = self.dev_masks = self.dev_order = None


class _StagingRing(object):
    """The host-memmap mode: RING_DEPTH slots of pinned staging + device buffers in the stored dtypes.  The rows of batch
    i + 1 are gathered from the memmap into a pinned slot and copied on a side stream while batch i is consumed; a slot is
    refilled only after the host has seen its copy and the kernels that read its device buffers complete (loading.SlotEvents
    explains why the host polls instead of making the copy stream wait for the compute stream)."""

    def __init__(self, loader):
        self.loader = loader
        B = loader.batch_size
        arrays = [loader.frames] + ([loader.masks] if loader.masks is not None else [])
        self.pinned, self.dev = [], []
        for _ in range(RING_DEPTH):
            shapes = [((B,) + tuple(a.shape[1:]), torch.from_numpy(np.empty(0, dtype=a.dtype)).dtype) for a in arrays]
            self.pinned.append([torch.empty(s, dtype=d, pin_memory=True) for s, d in shapes])
            self.dev.append([torch.empty(s, dtype=d, device=loader.device) for s, d in shapes])
        self.arrays = arrays
        self.events = SlotEvents(RING_DEPTH, loader.device)
        self.staged = {}                 # first row of a staged batch -> its slot
        self.tail = 0

    def start(self):
        self.staged = {}
        self._stage(0)

    def _stage(self, first):
        n = self.loader.num_frames
        if first >= n or first in self.staged:
            return
        B = min(self.loader.batch_size, n - first)
        rows = self.loader.order[first:first + B]
        s = self.tail
        self.events.free(s)
        for a, pin in zip(self.arrays, self.pinned[s]):
            np.take(a, rows, axis=0, out=pin.numpy()[:B])
        with self.events.copying(s):
            for pin, dev in zip(self.pinned[s], self.dev[s]):
                dev[:B].copy_(pin[:B], non_blocking=True)
        self.staged[first] = s
        self.tail = (s + 1) % RING_DEPTH

    def next(self, first, B, size):
        self._stage(first)
        s = self.staged.pop(first)
        with self.events.reading(s):
            batch = {'input': feeder.rows_gather(self.dev[s][0], None, 0, B, size)}
            if len(self.dev[s]) > 1:
                batch['instances'] = feeder.rows_gather_labels(self.dev[s][1], None, 0, B, size)
        self._stage(first + B)           # the next batch's rows, while the caller trains on this one
        return batch


def load(cfg, shard=None, device='cuda', **unused_kwargs):
    del unused_kwargs
    if not os.path.exists(cfg.data_folder):
        raise GenesisHipError('multid: data folder %s does not exist' % cfg.data_folder)
    if not hasattr(cfg, 'unique_colours'):
        cfg.unique_colours = False
    mem_map = bool(getattr(cfg, 'mem_map', False))
    fprint('multid: %s; num_workers=%s is not used' % ('arrays stay on the host (mem_map)' if mem_map else 'splits resident on the device',
                                                       getattr(cfg, 'num_workers', None)))
    return tuple(MultidLoader(os.path.join(cfg.data_folder, file_name(mode, cfg.unique_colours)), cfg.batch_size,
                              img_size=cfg.img_size, load_instances=cfg.load_instances, mem_map=mem_map,
                              seed=getattr(cfg, 'seed', 0), shard=shard, device=device)
                 for mode in MODES)
