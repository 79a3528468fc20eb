"""GQN `rooms_ring_camera` -- drop-in for the reference's `datasets/gqn_config.py` without TensorFlow.

Same Forge-style contract: importing this file registers the data flags with the reference's defaults (:31-41),
`load(cfg) -> (train, val, test)` builds the reference's three loaders (:62-73: devel_train and devel_val at
cfg.batch_size, test at batch size 1), and each loader has `__len__`, `batch_size`, `__iter__`, and `StopIteration` at the
end of the epoch, after which it can be iterated again.  A loader yields {'input': fp32 [B,3,S,S] in [0,1]} ON THE DEVICE.

The dataset (third_party/tf_gqn/gqn_tfr_provider.py:64-69, :109-137): 2160 train and 240 test files of uncompressed
TFRecords under <data_folder>/rooms_ring_camera/{train,test}, named <i>-of-<n>.tfrecord with i from 1 and both numbers
zero-padded to the digits of n (0001-of-2160, 001-of-240); a record is a tf.Example whose `frames` holds ten 64 x 64 JPEG
strings and whose `cameras` (fifty floats) the reference discards, as this does.  devel_train takes the first
(n // val_frac) * (val_frac - 1) train files and devel_val the rest; len(loader) comes from the reference's 10.8 M / 1.2 M
records (:118-130), here files x records_per_file (5000).

What runs where.  `num_workers` threads (at most 16) each read their files with the CRC-checking TFRecord reader
(genesis_amd/tfrecord.py), pick ONE frame of every record and entropy-decode it in C (gx_jpeg_entropy_decode; ctypes
drops the GIL) into chunks of quantised coefficients.  One merger thread takes the chunks round-robin, shuffles the train
split through a pool and cuts batches; the consumer copies a batch into a pinned slot of a ring, sends it to the device in
one copy on a side stream, and ONE HIP launch (gx_jpeg_decode_f32chw) turns it into the fp32 batch: inverse DCT, chroma
upsampling, colour conversion, x (1/255) and the nearest resize to img_size.  No pixel is touched on the host.

Differences from the reference, on purpose:
  * Record order.  Worker w of W reads files w, w + W, ... of the split; the merger takes chunks of 32 consecutive records
    from the workers in turn (tf.data interleaves num_parallel_reads files one record at a time).  With one worker, or with
    files of at most 32 records, that is the order of the files.  The train split is then shuffled through a pool of
    buffer_size * batch_size records, filled and sampled as in multi_object_config.py, seeded from cfg.seed: the ORDER IS
    NOT TensorFlow's.  Every epoch of a loader starts from the same seed.
  * Frame choice.  The reference takes the first of a TF-shuffled index vector per parse batch, which cannot be reproduced.
    Here a generator seeded from (cfg.seed, file number) draws one frame index per record; `load(cfg, frame=k)` fixes it.
  * Scaling is u8 * (1/255) in fp32, TensorFlow's convert_image_dtype, not the feeder's true division.
  * `load(cfg, shard=(rank, world))` keeps every world-th file of each split, from file `rank`, for one process per GPU.
  * No throughput printout at load time (the reference's loader_throughput consumes 105 batches first)."""
import ctypes
import functools
import os
import queue
import threading

import numpy as np
import torch

from genesis_amd import compat as _compat

_compat.install()

from forge import flags  # noqa: E402
from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import _lib, data_cache, jpeg, tfrecord  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.loading import (END, MAX_WORKERS, Batcher, Outlet, ShufflePool, SlotEvents, parse_shard,  # noqa: E402
                                 threaded)
from genesis_amd.tfrecord import TFRecordError  # noqa: E402

flags.DEFINE_string('data_folder', 'data/gqn_datasets', 'Path to data folder.')
flags.DEFINE_integer('img_size', 64, 'Dimension of images. Images are square.')
flags.DEFINE_integer('val_frac', 60, 'Fraction of training images to use for validation.')
flags.DEFINE_integer('num_workers', 4, 'TF records dataset.')
flags.DEFINE_integer('buffer_size', 128, 'TF records dataset.')
flags.DEFINE_integer('K_steps', 7, 'Number of recurrent steps.')

DATASET = 'rooms_ring_camera'
TRAIN_FILES = 2160
TEST_FILES = 240
RECORDS_PER_FILE = 5000            # 2160 x 5000 = 10.8 M, 240 x 5000 = 1.2 M: the reference's hard-coded sizes
FRAMES_PER_RECORD = 10
CHUNK_RECORDS = 32                 # consecutive records of one file the merger takes at a time
MODES = ('train', 'test', 'devel_train', 'devel_val')

_QUEUE_BATCHES = 4                 # batches the merger may run ahead of the consumer
_QUEUE_CHUNKS = 2                  # chunks a worker may run ahead of the merger


def split_range(mode, val_frac, train_files=TRAIN_FILES, test_files=TEST_FILES):
    """(folder, first, end, n): the split is files first + 1 .. end of the n files of `folder`."""
    if mode not in MODES:
        raise ValueError("Mode not known.")
    n = test_files if mode == 'test' else train_files
    cut = (n // val_frac) * (val_frac - 1) if mode.startswith('devel') else 0
    first, end = (0, cut) if mode == 'devel_train' else ((cut, n) if mode == 'devel_val' else (0, n))
    return ('train' if mode.startswith('devel') else mode), first, end, n


def file_list(data_folder, mode, val_frac, train_files=TRAIN_FILES, test_files=TEST_FILES, shard=None):
    """Paths of the split's files, in order; shard = (rank, world) keeps every world-th one from `rank`."""
    folder, first, end, n = split_range(mode, val_frac, train_files, test_files)
    digits = len(str(n))
    base = os.path.join(data_folder, DATASET, folder)
    files = [os.path.join(base, '%0*d-of-%0*d.tfrecord' % (digits, i + 1, digits, n)) for i in range(first, end)]
    rank, world = parse_shard(shard, 'gqn')
    return files[rank::world]


def num_frames(mode, val_frac, train_files=TRAIN_FILES, test_files=TEST_FILES, records_per_file=RECORDS_PER_FILE):
    """Records the reference counts for a split (gqn_config.py:118-130), from which len(loader) follows."""
    train_sz, test_sz = train_files * records_per_file, test_files * records_per_file
    if mode == 'train':
        return train_sz
    if mode == 'test':
        return test_sz
    if mode == 'devel_train':
        return (train_sz // val_frac) * (val_frac - 1)
    if mode == 'devel_val':
        return train_sz // val_frac
    raise ValueError("Mode not known.")


def frame_rng(seed, file_number):
    """The generator that draws the frame index of every record of file `file_number` (1-based, as in its name)."""
    return np.random.RandomState((int(seed) * 1000003 + int(file_number)) % (1 << 32))


def _file_number(path):
    try:
        return int(os.path.basename(path).split('-')[0])
    except ValueError:
        return 0


class HostBatches(object):
    """The host half of a loader, usable without a GPU: iterating it runs one epoch over `files` and yields dicts
    {'coef': int16 [n, V], 'qtab': uint16 [n, 192], 'index': int64 [n, 3], 'geometry': (H, W, sampling class)}: the
    entropy-decoded frames of n records (batch_size, or fewer in the last batch) as jpeg.JpegStaging lays them out, and per
    record (position of its file in `files`, record in the file, frame in the record).  frame = None draws the frame
    from frame_rng(seed, file number).  shuffle_records <= 1 keeps the stream's order.

    Threads: min(num_workers, 16, len(files)) readers and one merger per epoch; an error in any of them is raised by the
    consumer.  Closing the iterator (or dropping it) stops them."""

    def __init__(self, files, batch_size, frame=None, shuffle_records=0, seed=0, num_workers=4,
                 frames_per_record=FRAMES_PER_RECORD, verify_crc=True):
        if batch_size <= 0:
            raise GenesisHipError('gqn: batch_size must be positive, not %r' % (batch_size,))
        if frame is not None and not 0 <= int(frame) < frames_per_record:
            raise GenesisHipError('gqn: frame must be in [0, %d), not %r' % (frames_per_record, frame))
        self.files = list(files)
        self.batch_size = int(batch_size)
        self.frame = None if frame is None else int(frame)
        self.shuffle_records = int(shuffle_records)
        self.seed = int(seed)
        self.workers = max(1, min(int(num_workers), MAX_WORKERS, max(1, len(self.files))))
        self.frames_per_record = int(frames_per_record)
        self.verify_crc = verify_crc

    # ---- reader threads ----
    def _read_files(self, w, put):
        """Worker w: files w, w + workers, ... as chunks (coef, qtab, index, geometry) of at most CHUNK_RECORDS records."""
        slots = max(64, self.frames_per_record)
        offsets, lengths = np.zeros(slots, dtype=np.int64), np.zeros(slots, dtype=np.int64)
        count = ctypes.c_int()
        geometry = None
        coef = qtab = index = None
        fill = 0
        for fi in range(w, len(self.files), self.workers):
            path = self.files[fi]
            rng = frame_rng(self.seed, _file_number(path)) if self.frame is None else None
            try:
                for r, rec in enumerate(tfrecord.TFRecordReader(path, compression='auto', verify_crc=self.verify_crc)):
                    k = self.frame if rng is None else int(rng.randint(self.frames_per_record))
                    try:
                        off, length = tfrecord.find_bytes_list(rec, 'frames')
                        _lib.call('gx_bytes_list_index', ctypes.c_void_p(rec.ctypes.data + off), length, slots,
                                  ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(lengths.ctypes.data), ctypes.byref(count))
                        if count.value != self.frames_per_record:
                            raise GenesisHipError("'frames' holds %d values, expected %d" % (count.value, self.frames_per_record))
                        stream = rec[off + int(offsets[k]):off + int(offsets[k]) + int(lengths[k])]
                        if geometry is None:
                            geometry = jpeg.jpeg_info(stream).geometry
                            values = sum(jpeg.plane_blocks(*geometry)) * 64
                        if coef is None:
                            coef = np.empty((CHUNK_RECORDS, values), dtype=np.int16)
                            qtab = np.empty((CHUNK_RECORDS, 192), dtype=np.uint16)
                            index = np.empty((CHUNK_RECORDS, 3), dtype=np.int64)
                        info = jpeg.entropy_decode(stream, coef[fill], qtab[fill])
                        if info.geometry != geometry:
                            raise GenesisHipError('a %d x %d %s frame among %d x %d %s ones'
                                                  % (info.width, info.height, jpeg.SAMPLING_NAMES[info.sampling], geometry[1],
                                                     geometry[0], jpeg.SAMPLING_NAMES[geometry[2]]))
                    except GenesisHipError as e:
                        raise TFRecordError('%s: record %d: frame %d: %s' % (path, r, k, e)) from None
                    index[fill] = (fi, r, k)
                    fill += 1
                    if fill == CHUNK_RECORDS:
                        if not put((coef, qtab, index, geometry)):
                            return
                        coef, fill = None, 0
            except TFRecordError as e:
                if str(e).startswith(path):
                    raise
                raise TFRecordError('%s: %s' % (path, e)) from None
            if fill:                                    # a chunk never spans two files
                if not put((coef[:fill], qtab[:fill], index[:fill], geometry)):
                    return
                coef, fill = None, 0

    def _records(self, stop):
        """The merged stream: (coef row, qtab row, index row, geometry) per record, chunks taken round-robin."""
        halt = threading.Event()                        # set when the merged stream ends, for whatever reason
        outlets = [Outlet(_QUEUE_CHUNKS, halt) for _ in range(self.workers)]
        threads = [o.start(functools.partial(self._read_files, w), 'gqn_reader_%d' % w) for w, o in enumerate(outlets)]
        try:
            live = list(range(self.workers))
            geometry = None
            while live:
                for w in list(live):
                    item = None
                    while item is None:
                        if stop.is_set():
                            return
                        try:
                            item = outlets[w].q.get(timeout=0.1)
                        except queue.Empty:
                            pass
                    if item is END:
                        live.remove(w)
                        continue
                    if isinstance(item, BaseException):
                        raise item
                    coef, qtab, index, g = item
                    if geometry is None:
                        geometry = g
                    elif g != geometry:
                        raise TFRecordError('%s: its frames are %s, those of earlier files %s'
                                            % (self.files[int(index[0, 0])], g, geometry))
                    for i in range(len(coef)):
                        yield coef[i], qtab[i], index[i], geometry
        finally:
            halt.set()
            for t in threads:
                t.join()

    def _produce(self, put):
        """Runs the epoch and hands every batch to put(item); put returns False once the consumer has gone."""
        B, N = self.batch_size, self.shuffle_records
        coef = geometry = None                          # of the current record; every record has the same ones

        def arrays(n):
            return (np.empty((n, coef.size), dtype=np.int16), np.empty((n, 192), dtype=np.uint16), np.empty((n, 3), dtype=np.int64))

        def emit(*record):
            dst, n = batch.row()
            for d, r in zip(dst, record):
                d[n] = r
            return batch.written()

        batch = Batcher(lambda: arrays(B), B, lambda c, q, ix: {'coef': c, 'qtab': q, 'index': ix, 'geometry': geometry}, put)
        pool = ShufflePool(N, self.seed) if N > 1 else None
        rows = None
        for coef, qtab, index, geometry in self._records(put.halt):
            if pool is None:
                if not emit(coef, qtab, index):
                    return
                continue
            if rows is None:
                rows = arrays(N)                        # pages are touched only as rows fill
            j, evict = pool.place()
            if evict and not emit(*(a[j] for a in rows)):
                return
            rows[0][j], rows[1][j], rows[2][j] = coef, qtab, index
        for j in pool.drain() if pool is not None else ():      # the stream has ended: the pool in random order
            if not emit(*(a[j] for a in rows)):
                return
        batch.flush()

    def __iter__(self):
        return threaded(self._produce, 'gqn_merger', _QUEUE_BATCHES)


class GQNLoader(object):
    """One split on the device: HostBatches -> a ring of pinned staging slots -> gx_jpeg_decode_f32chw.  Mirrors the
    reference's GQNLoader (:87-152): `__len__` = num_frames // batch_size, `__next__` returns {'input': fp32 [B,3,S,S]} and
    raises StopIteration at the end of the epoch; the next `__next__` or `__iter__` starts a new one.

    The copy of batch i + 1 runs on a side stream while batch i is consumed, and a slot is refilled only after the host has
    seen both its copy and the kernel that read it complete: loading.SlotEvents, which says why."""

    def __init__(self, host_batches, num_frames, img_size, device='cuda', depth=32):
        self.host = host_batches
        self.batch_size = host_batches.batch_size
        self.num_frames = int(num_frames)
        self.length = self.num_frames // self.batch_size
        self.img_size = int(img_size)
        self.device = torch.device(device)
        self.depth = max(2, int(depth))
        self.count = 0
        self.epoch = None
        self.geometry = None
        self.staging = [None] * self.depth
        self.dev = [None] * self.depth
        self.events = SlotEvents(self.depth, self.device)
        self.pending = None                 # (slot, n) of the batch whose copy is in flight
        self.slot = 0

    def __len__(self):
        return self.length

    def _prefetch(self):
        self.pending = None
        try:
            b = next(self.epoch)
        except StopIteration:
            return
        if b['geometry'] != self.geometry:              # the whole ring at once, the first time (feeder.py)
            for q in range(self.depth):
                self.events.free(q)
                self.staging[q] = jpeg.JpegStaging(self.batch_size, *b['geometry'])
                self.dev[q] = torch.empty(self.staging[q].nbytes, dtype=torch.uint8, device=self.device)
            self.geometry = b['geometry']
        s = self.slot
        self.events.free(s)
        n = len(b['coef'])
        self.staging[s].coef[:n] = b['coef']
        self.staging[s].qtab[:n] = b['qtab']
        with self.events.copying(s):
            self.dev[s].copy_(self.staging[s].buffer, non_blocking=True)
        self.pending = (s, n)
        self.slot = (s + 1) % self.depth

    def __iter__(self):
        if self.epoch is not None:
            self.epoch.close()                          # stops the previous epoch's threads
        self.epoch = iter(self.host)
        self.count = 0
        self._prefetch()
        return self

    def __next__(self):
        if self.epoch is None:
            iter(self)
        if self.pending is None:
            fprint("Reached end of epoch.")
            fprint(f"Counted {self.count} batches, expected {self.length}.")
            self.epoch.close()
            self.epoch = None
            raise StopIteration
        s, n = self.pending
        with self.events.reading(s):
            x = jpeg.decode_staged(self.dev[s], self.batch_size, n, self.geometry, self.img_size)
        self.count += 1
        self._prefetch()                                # fills the next slot while the caller trains on x
        return {'input': x}

    def close(self):
        if self.epoch is not None:
            self.epoch.close()
            self.epoch = None
        self.pending = None


def host_splits(cfg, frame=None, shard=None, shuffle=True, train_files=TRAIN_FILES, test_files=TEST_FILES,
                records_per_file=RECORDS_PER_FILE, frames_per_record=FRAMES_PER_RECORD):
    """((train, val, test) HostBatches, their record counts): the host streams behind load(), which need no GPU and
    read nothing until they are iterated."""
    rank, world = parse_shard(shard, 'gqn')
    seed = getattr(cfg, 'seed', 0)
    hosts, sizes = [], []
    for mode, batch_size, workers in (('devel_train', cfg.batch_size, cfg.num_workers), ('devel_val', cfg.batch_size, cfg.num_workers),
                                      ('test', 1, 1)):
        files = file_list(cfg.data_folder, mode, cfg.val_frac, train_files, test_files)
        mine = files[rank::world]
        pool = cfg.buffer_size * batch_size if (shuffle and 'train' in mode) else 0
        hosts.append(HostBatches(mine, batch_size, frame, pool, seed, workers, frames_per_record))
        total = num_frames(mode, cfg.val_frac, train_files, test_files, records_per_file)
        sizes.append(total * len(mine) // max(1, len(files)))
    return tuple(hosts), tuple(sizes)


def load(cfg, frame=None, shard=None, device='cuda', shuffle=True, train_files=TRAIN_FILES, test_files=TEST_FILES,
         records_per_file=RECORDS_PER_FILE, frames_per_record=FRAMES_PER_RECORD, **unused_kwargs):
    del unused_kwargs
    if cfg.num_workers == 0:
        fprint("Need to use at least one worker for loading tfrecords.")
        cfg.num_workers = 1
    if not os.path.exists(cfg.data_folder):
        raise Exception("Data folder does not exist.")
    fprint(f"Using {min(cfg.num_workers, MAX_WORKERS)} data workers.")
    hosts, sizes = host_splits(cfg, frame, shard, shuffle, train_files, test_files, records_per_file, frames_per_record)
    loaders = tuple(GQNLoader(h, n, cfg.img_size, device=device) for h, n in zip(hosts, sizes))
    # only the train split goes through the shuffle pool (host_splits)
    return data_cache.wrap_loaders(cfg, loaders, shuffle=(bool(shuffle), False, False), name='gqn')
