"""What the data loaders share on the host: the event poll, the shard argument, reading a file, and FileBatchLoader, the
epoch driver of the loaders that decode one file per frame (png.PngFileLoader, imagefile.ImageFileLoader).  Imports no
format module and not the feeder."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import GenesisHipError

MAX_WORKERS = 16


def read_file(path):
    with open(path, 'rb') as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


def host_wait(event):
    """Waits on the host until a HIP event (None: nothing to wait for) has happened, without a blocking runtime call."""
    if event is not None:
        while not event.query():
            time.sleep(2e-4)


def parse_shard(shard, name):
    """shard = (rank, world) or None -> (rank, world); `name` prefixes the refusal."""
    rank, world = (0, 1) if shard is None else (int(shard[0]), int(shard[1]))
    if not 0 <= rank < world:
        raise GenesisHipError('%s: shard must be (rank, world) with 0 <= rank < world, not %r' % (name, shard))
    return rank, world


class FileBatchLoader(object):
    """Batches decoded from one file per frame, on the device.  `__len__` = ceil(files / batch_size) (the reference's
    DataLoaders keep the short last batch), `batch_size`, `__iter__` / `__next__` with StopIteration at the end of the epoch,
    after which the loader can be iterated again.  Every epoch draws a fresh permutation of the files from one generator
    seeded with `seed` (shuffle=False: file order); `order` holds the file indices of the epoch in progress.

    `num_workers` reader threads (at most MAX_WORKERS) read the files and run the serial half of the decoder (C calls that
    drop the GIL) straight into a pinned slot of a ring of `depth`, up to depth - 1 batches ahead; per batch there is one
    copy on a side stream.  A slot is refilled only after the host has seen both its copy and the launches that read it
    complete.  A file that cannot be read or decoded raises GenesisHipError naming its path, from the `__next__` that would
    have returned its batch: the batches before it are delivered, the epoch ends there (the readers' outstanding work is
    cancelled or awaited, whatever they raise) and the next `__iter__` starts a new one.

    A subclass supplies the format:
        _open_ring()            -> the ring of `depth` slots, kept as self.ring until close(); called when the first batch
                                   is needed
        _jobs(s, idx)           -> (path, decode) of every file of a batch, idx its file indices: a reader calls decode
                                   with the file's bytes, which writes into slot s
        _stage(s, n, results)   starts the copies of slot s on the current stream, once its n frames' readers have returned
                                   `results` (in _jobs' order) -> what _batch needs besides the slot
        _batch(s, staged)       -> the batch, launched on the current stream from slot s"""

    def __init__(self, files, batch_size, shuffle, seed, num_workers, device, depth, name):
        if batch_size <= 0:
            raise GenesisHipError('%s: batch_size must be positive, not %r' % (name, batch_size))
        self.files = list(files)
        self.batch_size = int(batch_size)
        self.shuffle = bool(shuffle)
        self.rng = np.random.RandomState(int(seed) % (1 << 32))
        self.workers = max(1, min(int(num_workers), MAX_WORKERS))
        self.device = torch.device(device)
        self.depth = max(2, int(depth))
        self.name = name
        self.length = -(-len(self.files) // self.batch_size)
        self.pool = None
        self.ring = None
        self.copy_stream = None
        self.ready = [None] * self.depth
        self.consumed = [None] * self.depth
        self.jobs = {}                          # batch number -> futures
        self.order = None
        self.pending = None                     # (batch number, what _stage returned) of the batch whose copy is in flight
        self.count = 0
        self.failed = None                      # a reader's error of the batch after the one just returned

    def __len__(self):
        return self.length

    def _read(self, path, decode):
        try:
            return decode(read_file(path))
        except (GenesisHipError, OSError) as e:
            raise GenesisHipError('%s: %s: %s' % (self.name, path, e)) from None

    def _submit(self, k):
        """Hands the files of batch k to the reader threads; they write into slot k % depth."""
        if k >= self.length:
            return
        s = k % self.depth
        host_wait(self.ready[s])                        # the slot's last copy has left the pinned buffer
        host_wait(self.consumed[s])
        idx = self.order[k * self.batch_size:(k + 1) * self.batch_size]
        self.jobs[k] = [self.pool.submit(self._read, path, decode) for path, decode in self._jobs(s, idx)]

    def _copy(self, k):
        """Waits for the readers of batch k and starts its copy on the side stream."""
        self.pending = None
        if k >= self.length:
            return
        error, results = None, []
        for j in self.jobs.pop(k):
            try:
                results.append(j.result())
            except Exception as e:                      # noqa: BLE001  (whatever a reader raised: the epoch ends either way)
                error = error or e
        if error is not None:
            self._drop()
            raise error
        s = k % self.depth
        n = min(self.batch_size, len(self.files) - k * self.batch_size)
        with torch.cuda.stream(self.copy_stream):
            staged = self._stage(s, n, results)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.ready[s] = ev
        self.pending = (k, staged)

    def _drop(self):
        for jobs in self.jobs.values():
            for j in jobs:
                j.cancel()
        for jobs in self.jobs.values():
            for j in jobs:
                if not j.cancelled():
                    try:
                        j.result()
                    except Exception:                   # noqa: BLE001  (the epoch is being dropped)
                        pass
        self.jobs = {}
        self.order = None
        self.pending = None

    def __iter__(self):
        if not self.files:
            raise GenesisHipError('%s: no files' % self.name)
        self._drop()                                    # an epoch that was left half way
        self.failed = None
        if self.pool is None:
            self.ring = self._open_ring()
            self.copy_stream = torch.cuda.Stream(device=self.device)
            self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix=self.name + '_reader')
        n = len(self.files)
        self.order = self.rng.permutation(n) if self.shuffle else np.arange(n)
        self.count = 0
        for k in range(self.depth - 1):
            self._submit(k)
        self._copy(0)
        return self

    def __next__(self):
        if self.failed is not None:
            e, self.failed = self.failed, None
            raise e
        if self.order is None:
            iter(self)
        if self.pending is None:
            self.order = None
            raise StopIteration
        k, staged = self.pending
        s = k % self.depth
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.ready[s])
        batch = self._batch(s, staged)
        done = torch.cuda.Event()
        done.record(cur)
        self.consumed[s] = done
        self.count += 1
        self._submit(k + self.depth - 1)                # keeps the readers depth - 1 batches ahead ...
        try:
            self._copy(k + 1)                           # ... and the next batch's copy under the caller's step
        except Exception as e:                          # noqa: BLE001
            self.failed = e                             # batch k is good and is returned; the next call raises
        return batch

    def close(self):
        self._drop()
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None
            self.ring = None
