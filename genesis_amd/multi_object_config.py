"""Multi-object datasets (ObjectsRoom, CLEVR with masks, Tetrominoes, Multi-dSprites) -- drop-in for the reference's
`datasets/multi_object_config.py` without TensorFlow.

Same Forge-style contract: importing this file registers the data flags with the reference's defaults (:32-44),
`load(cfg) -> (train, val, test)` applies the same per-dataset `img_size` / `K_steps` / `background_entities` /
`max_frames` rules (:67-100) and the same split (:119-126: test = the first 10 000 records, val the next 10 000, train
the rest), and each loader has `__len__` (num_frames // batch_size), `batch_size`, `__iter__` and `StopIteration` at the
end of the epoch, a short last batch included (tf.data's `batch`).  A loader yields
{'input': fp32 [B,3,S,S] in [0,1], 'instances': int64 [B,1,S,S]} ON THE DEVICE.

What runs where.  One background reader thread per epoch inflates the GZIP stream, scans and checks the records and
unpacks `image` and `mask` (one byte per bytes_list value on the wire) in C (genesis_amd/tfrecord.py) straight into the
shuffle pool, or into the batch buffer when shuffling is off; batches reach the consumer through a bounded queue.  The
host does no per-pixel Python work.  DeviceFeeder stages a batch in pinned memory and copies the uint8 frames and the
uint8 entity-mask stack as stored; the GPU converts the frames and turns the stack into the instance map, fused with
the CLEVR centre crop (192) and the nearest resize (gx_entity_masks_to_labels), where the reference loops over entities
on the host (:188-203).

Differences from the reference, on purpose:
  * Shuffling uses a pool of buffer_size * batch_size records, filled and then sampled (a uniformly drawn slot is
    emitted and refilled with the next record, as tf.data's shuffle does), seeded from cfg.seed.  The ORDER IS NOT
    TensorFlow's: its random generator is not reproduced.  Every epoch of a loader starts from the same seed, as a new
    one-shot iterator over a seeded tf.data shuffle does, so epochs repeat their order.
  * The quirk at :185/:201 is kept: `img_size` is compared with the frame height BEFORE the crop, so CLEVR with
    img_size = 240 comes out 192 x 192 (cropped, not resized).
  * `shard=(rank, world)` keeps the records with index % world == rank after the split (index counted inside the split),
    for one process per GPU.  `num_workers` is accepted and printed; there is one reader thread whatever it says.
  * No throughput printout at load time (the reference's loader_throughput consumes 105 batches first).
The pool holds decoded records, as tf.data's does: CLEVR at the defaults is 4096 records of 1.07 MB."""
import os

import numpy as np
import torch

from genesis_amd import compat as _compat

_compat.install()

from forge import flags  # noqa: E402
from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import data_cache, tfrecord  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.loading import Batcher, ShufflePool, parse_shard, threaded  # noqa: E402

flags.DEFINE_string('data_folder', 'data/multi-object-datasets', 'Path to data folder.')
flags.DEFINE_string('dataset', 'objects_room', '{multi_dsprites, objects_room, clevr, tetrominoes}')
flags.DEFINE_integer('img_size', -1, 'Dimension of images. Images are square.')
flags.DEFINE_integer('dataset_size', -1, 'Number of images to use.')
flags.DEFINE_integer('num_workers', 4, 'Number of threads for loading data.')
flags.DEFINE_integer('buffer_size', 128, 'TF records dataset.')
flags.DEFINE_integer('K_steps', -1, 'Number of recurrent steps.')

MULTI_DSPRITES = '/multi_dsprites/multi_dsprites_colored_on_colored.tfrecords'
OBJECTS_ROOM = '/objects_room/objects_room_train.tfrecords'
CLEVR = '/clevr_with_masks/clevr_with_masks_train.tfrecords'
TETROMINOS = '/tetrominoes/tetrominoes_train.tfrecords'
CLEVR_CROP = 192  # Following pre-processing in the IODINE paper

# file, stored frame (H, W), entities in the mask stack, its stored layout, and the reference's per-dataset rules
DATASETS = {
    'multi_dsprites': dict(file=MULTI_DSPRITES, frame=(64, 64), entities=5, layout='hwe', img_size=64, K_steps=5,
                           background_entities=1, max_frames=60000),
    'objects_room': dict(file=OBJECTS_ROOM, frame=(64, 64), entities=7, layout='ehw', img_size=64, K_steps=7,
                         background_entities=4, max_frames=1000000),
    'clevr': dict(file=CLEVR, frame=(240, 320), entities=11, layout='ehw', img_size=128, K_steps=11,
                  background_entities=1, max_frames=70000),
    'tetrominoes': dict(file=TETROMINOS, frame=(35, 35), entities=4, layout='ehw', img_size=32, K_steps=4,
                        background_entities=1, max_frames=60000),
}

_QUEUE_BATCHES = 4     # batches the reader thread may run ahead of the consumer


def mask_shape(frame, entities, layout):
    """Shape of one record's mask stack as stored: [E,H,W,1] ('ehw') or [H,W,E,1] ('hwe')."""
    H, W = frame
    return (entities, H, W, 1) if layout == 'ehw' else (H, W, entities, 1)


def output_size(frame, img_size):
    """(crop window or None, feeder size or None, S) as the reference's loader decides them (:180-186): frames that are not
    square are centre-cropped to CLEVR_CROP; the resize to img_size happens only if img_size differs from the frame
    height before the crop."""
    from genesis_amd.feeder import centre_box
    H, W = frame
    crop = centre_box(H, W, CLEVR_CROP) if H != W else None
    size = None if img_size == H else int(img_size)
    S = size if size is not None else (CLEVR_CROP if crop is not None else H)
    return crop, size, S


class HostBatches(object):
    """The host half of a loader, usable without a GPU: iterating it runs one epoch over records [start, stop) of the
    file (stop = None: to the end of the file) and yields dicts of uint8 numpy arrays
    {'input': [n,H,W,3], 'masks': [n] + mask_shape, 'index': int64 [n]}: n = batch_size except for a short last batch,
    'index' the records' positions in the file.  shard = (rank, world) keeps the records with
    (index - start) % world == rank.  shuffle_records <= 1 keeps the file's order.

    The epoch's reader thread does the inflating, checking and unpacking and fills a queue of at most _QUEUE_BATCHES
    batches; an error in it is raised by the consumer.  Closing the iterator (or dropping it) stops the thread."""

    def __init__(self, path, frame, entities, layout, start, stop, batch_size, shuffle_records=0, seed=0, shard=None,
                 verify_crc=True):
        if batch_size <= 0:
            raise GenesisHipError('multi_object: batch_size must be positive, not %r' % (batch_size,))
        rank, world = parse_shard(shard, 'multi_object')
        self.path = path
        self.frame = (int(frame[0]), int(frame[1]))
        self.entities = int(entities)
        self.layout = layout
        self.start = int(start)
        self.stop = None if stop is None else int(stop)
        self.batch_size = int(batch_size)
        self.shuffle_records = int(shuffle_records)
        self.seed = int(seed)
        self.rank, self.world = rank, world
        self.verify_crc = verify_crc
        self.image_shape = self.frame + (3,)
        self.mask_shape = mask_shape(self.frame, self.entities, layout)
        self.image_bytes = int(np.prod(self.image_shape))
        self.mask_bytes = int(np.prod(self.mask_shape))

    def num_records(self, total):
        """Records of [start, min(stop, total)) this shard keeps."""
        stop = total if self.stop is None else min(self.stop, total)
        n = max(0, stop - self.start)
        return (n - self.rank + self.world - 1) // self.world

    # ---- reader thread ----
    def _produce(self, put):
        """Runs the epoch and hands every batch to put(item); put returns False once the consumer has gone."""
        B, nb_img = self.batch_size, self.image_bytes
        batch = Batcher(lambda: (np.empty((B,) + self.image_shape, dtype=np.uint8), np.empty((B,) + self.mask_shape, dtype=np.uint8),
                                 np.empty(B, dtype=np.int64)),
                        B, lambda img, msk, idx: {'input': img, 'masks': msk, 'index': idx}, put)

        def unpack(rec, index, img_dst, mask_dst):
            try:
                tfrecord.unpack_bytes_list(rec, 'image', img_dst)
                tfrecord.unpack_bytes_list(rec, 'mask', mask_dst)
            except GenesisHipError as e:
                raise tfrecord.TFRecordError('%s: record %d: %s' % (self.path, index, e)) from None

        def emit_row(j):
            (img, msk, idx), n = batch.row()
            img[n].reshape(-1)[:] = rows[j, :nb_img]
            msk[n].reshape(-1)[:] = rows[j, nb_img:]
            idx[n] = rows_idx[j]
            return batch.written()

        N = self.shuffle_records
        if N > 1 and self.stop is not None:             # never more rows than the split can fill
            N = max(2, min(N, (self.stop - self.start + self.world - 1) // self.world))
        pool = ShufflePool(N, self.seed) if N > 1 else None
        rows = rows_idx = None
        for index, rec in enumerate(tfrecord.TFRecordReader(self.path, verify_crc=self.verify_crc)):
            if self.stop is not None and index >= self.stop:
                break
            if index < self.start or (index - self.start) % self.world != self.rank:
                continue
            if pool is None:                            # file order: unpacked straight into the batch
                (img, msk, idx), n = batch.row()
                unpack(rec, index, img[n], msk[n])
                idx[n] = index
                if not batch.written():
                    return
                continue
            if rows is None:
                rows = np.empty((N, nb_img + self.mask_bytes), dtype=np.uint8)      # pages are touched only as rows fill
                rows_idx = np.empty(N, dtype=np.int64)
            j, evict = pool.place()
            if evict and not emit_row(j):
                return
            unpack(rec, index, rows[j, :nb_img], rows[j, nb_img:])
            rows_idx[j] = index
        for j in pool.drain() if pool is not None else ():      # the stream has ended: the pool in random order
            if not emit_row(j):
                return
        batch.flush()

    def __iter__(self):
        return threaded(self._produce, 'multi_object_reader', _QUEUE_BATCHES)


class MultiObjectLoader(object):
    """One split on the device: HostBatches -> DeviceFeeder.  Mirrors the reference's MultiOjectLoader (:145-212):
    `__len__` = num_frames // batch_size, `__iter__` starts a new epoch, `__next__` returns
    {'input': fp32 [B,3,S,S], 'instances': int64 [B,1,S,S]} and raises StopIteration at the end of the epoch."""

    def __init__(self, host_batches, background_entities, num_frames, img_size, device='cuda', depth=None):
        self.host = host_batches
        self.background_entities = int(background_entities)
        self.num_frames = int(num_frames)
        self.batch_size = host_batches.batch_size
        self.length = self.num_frames // self.batch_size
        self.img_size = int(img_size)
        self.crop, self.size, self.out_size = output_size(host_batches.frame, self.img_size)
        self.device = device
        if depth is None:       # the feeder's deep ring (loading.SlotEvents), capped at 1 GiB of pinned staging for large frames
            slot = self.batch_size * (host_batches.image_bytes + host_batches.mask_bytes)
            depth = max(4, min(32, (1 << 30) // slot))
        self.depth = depth
        self.count = 0
        self.feeder = None
        self.epoch = None

    def __len__(self):
        return self.length

    def _host_iter(self):
        for b in self.epoch:
            yield {'input': b['input'], 'masks': b['masks']}

    def __iter__(self):
        from genesis_amd.feeder import DeviceFeeder
        if self.epoch is not None:
            self.epoch.close()                          # stops the previous epoch's reader thread
        if self.feeder is not None and any(self.feeder.filled):
            self.feeder = None                          # an epoch abandoned half way: its staged batches are dropped
        self.epoch = iter(self.host)
        self.count = 0
        if self.feeder is None:
            self.feeder = DeviceFeeder(self._host_iter(), self.size, device=self.device, depth=self.depth, crop=self.crop,
                                       background_entities=self.background_entities, mask_layout=self.host.layout)
        else:
            self.feeder.reset(self._host_iter())
        return self

    def __next__(self):
        if self.feeder is None:
            iter(self)
        try:
            batch = next(self.feeder)
        except StopIteration:
            fprint("Reached end of epoch.")
            fprint(f"Counted {self.count} batches, expected {self.length}.")
            self.epoch.close()
            raise
        self.count += 1
        return batch

    def close(self):
        if self.epoch is not None:
            self.epoch.close()
            self.epoch = None
        self.feeder = None


def configure(cfg):
    """Applies the reference's per-dataset defaults to cfg in place (:67-100, :105-113) and returns the dataset's entry
    of DATASETS plus the number of frames the splits are cut from."""
    if cfg.dataset not in DATASETS:
        raise NotImplementedError(f"{cfg.dataset} not a valid dataset.")
    d = DATASETS[cfg.dataset]
    cfg.img_size = d['img_size'] if cfg.img_size < 0 else cfg.img_size
    cfg.K_steps = d['K_steps'] if cfg.K_steps < 0 else cfg.K_steps
    max_frames = d['max_frames']
    if cfg.dataset_size > max_frames:
        fprint(f"WARNING: {cfg.dataset_size} frames requested, but only {max_frames} available.")
        cfg.dataset_size = max_frames
    total_sz = cfg.dataset_size if cfg.dataset_size > 0 else max_frames
    return d, total_sz


def host_splits(cfg, val_size=10000, test_size=10000, shard=None, shuffle=True):
    """(train, val, test) HostBatches and their frame counts [(tng_sz, val_sz, tst_sz)]: the host record streams behind
    load(), which need no GPU."""
    d, total_sz = configure(cfg)
    tng_sz = total_sz - val_size - test_size
    assert tng_sz > 0
    fprint(f"Dataset has {total_sz} frames")
    fprint(f"Splitting into {tng_sz}/{val_size}/{test_size} for tng/val/tst")
    path = cfg.data_folder + d['file']
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    pool = cfg.buffer_size * cfg.batch_size if shuffle else 0
    seed = getattr(cfg, 'seed', 0)

    def split(start, stop):
        return HostBatches(path, d['frame'], d['entities'], d['layout'], start, stop, cfg.batch_size, pool, seed, shard)

    # the reference cuts the stream at total_sz only when dataset_size is given (:109-113); otherwise train runs to the end
    # of the file while its length is counted from max_frames
    hosts = (split(test_size + val_size, total_sz if cfg.dataset_size > 0 else None), split(test_size, test_size + val_size),
             split(0, test_size))
    return hosts, (tng_sz, val_size, test_size)


def load(cfg, val_size=10000, test_size=10000, shard=None, device='cuda', shuffle=True, **unused_kwargs):
    del unused_kwargs
    fprint(f"Using {cfg.num_workers} data workers (one reader thread per loader).")
    hosts, sizes = host_splits(cfg, val_size, test_size, shard, shuffle)
    bg = DATASETS[cfg.dataset]['background_entities']
    world = 1 if shard is None else int(shard[1])
    rank = 0 if shard is None else int(shard[0])
    loaders = tuple(MultiObjectLoader(h, bg, (n - rank + world - 1) // world, cfg.img_size, device=device)
                    for h, n in zip(hosts, sizes))
    return data_cache.wrap_loaders(cfg, loaders, shuffle=bool(shuffle), name='multi_object')
