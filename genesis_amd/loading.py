"""What the data loaders share on the host: the event poll, the shard argument, reading a file; the pieces of the record
readers (multi_object_config, gqn_config): Outlet and threaded(), the producer thread behind a bounded queue, ShufflePool,
the seeded draw sequence of the shuffle, and Batcher, which cuts the stream into batches; SlotEvents, the hand-shake of
every ring of pinned staging slots (feeder.DeviceFeeder, gqn_config.GQNLoader, multid_config's memmap ring and
FileBatchLoader); and FileBatchLoader, the epoch driver of the loaders that decode one file per frame (png.PngFileLoader,
imagefile.ImageFileLoader).  Imports no format module and not the feeder."""
import contextlib
import queue
import threading
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


END = object()      # what a producer thread puts last when it ran to the end


class Outlet(object):
    """A producer thread's end of a bounded queue `q`.  put = Outlet(maxsize, halt): put(item) blocks while the queue is
    full and returns False once `halt` is set, which is how the consumer says that it has gone."""

    def __init__(self, maxsize, halt):
        self.q = queue.Queue(maxsize=maxsize)
        self.halt = halt

    def __call__(self, item):
        while not self.halt.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def start(self, produce, name):
        """Runs produce(put) in a daemon thread -> the thread.  After the items the queue gets END, or instead of it
        whatever produce raised."""
        def run():
            try:
                produce(self)
                self(END)
            except BaseException as e:                  # handed to the consumer
                self(e)

        t = threading.Thread(target=run, name=name, daemon=True)
        t.start()
        return t


def threaded(produce, name, maxsize):
    """Yields the items that produce(put) puts, from a thread `name` that runs at most `maxsize` items ahead, and raises
    what produce raised.  Closing the generator, dropping it or an exception in the consumer sets put.halt, after which
    put returns False, and joins the thread."""
    put = Outlet(maxsize, threading.Event())
    t = put.start(produce, name)
    try:
        while True:
            item = put.q.get()
            if item is END:
                return
            if isinstance(item, BaseException):
                raise item
            yield item
    finally:
        put.halt.set()
        t.join()


class ShufflePool(object):
    """The decisions of a shuffle pool of N rows, as tf.data's shuffle makes them; the caller owns the rows.  The draws are
    the order of the training data for a seed: none while the pool fills, one randint(N) per record after that, and one
    permutation of the filled rows at the end of the stream (none if there was no record)."""

    def __init__(self, N, seed):
        self.N = N
        self.fill = 0
        self.rng = np.random.RandomState(seed)

    def place(self):
        """-> (row the next record goes into, whether that row holds a record that has to be emitted first)."""
        if self.fill < self.N:
            self.fill += 1
            return self.fill - 1, False
        return int(self.rng.randint(self.N)), True

    def drain(self):
        """The rows in the order in which they are emitted once the stream has ended."""
        return self.rng.permutation(self.fill) if self.fill else ()


class Batcher(object):
    """The batch under construction.  new() -> its arrays, batch_size rows each, made when the first row is asked for;
    row() -> (arrays, n), the caller writes row n of each; written() counts it and hands a full batch, item(*arrays), to
    put; flush() does so with the short last one.  Both return False once the consumer has gone.  A batch that was put is
    not written again: the next row() makes new arrays."""

    def __init__(self, new, batch_size, item, put):
        self.new, self.batch_size, self.item, self.put = new, batch_size, item, put
        self.arrays = None
        self.n = 0

    def row(self):
        if self.arrays is None:
            self.arrays = self.new()
        return self.arrays, self.n

    def written(self):
        self.n += 1
        return self.flush() if self.n == self.batch_size else True

    def flush(self):
        if not self.n:
            return True
        arrays, n = self.arrays, self.n
        self.arrays, self.n = None, 0
        return self.put(self.item(*(a[:n] for a in arrays)))


class SlotEvents(object):
    """The hand-shake of a ring of `depth` staging slots (pinned host buffer + device buffer) whose host->device copies run
    on a side stream, `copy_stream` (made at the first copy), while the consumer's stream, the current one of `device`,
    reads earlier slots.  The ring's owner keeps the buffers and decides which slot is next; per slot s it does
        free(s)             waits ON THE HOST until the slot may be refilled: its last copy has left the pinned buffer
                            (`ready[s]`) and the launches that read its device buffer have run (`consumed[s]`)
        with copying(s):    the copies of slot s, which run on copy_stream; records ready[s] after them
        with reading(s):    the launches that read slot s, on the current stream, which first waits for ready[s] (copy ->
                            compute, one event); records consumed[s] after them

    Why the host polls.  TrainStep.step never host-syncs, so the host runs far ahead of the device: the kernel that reads
    a slot may still be queued behind many training steps when the ring comes round to that slot again.  A slot is
    therefore refilled only after the HOST has seen both of its events complete, by polling; nothing on the device waits
    compute -> copy.  Measured on MI355X / ROCm 7 under HIP-graph replay (tools/feeder_probe.py): a device-side compute ->
    copy event wait per batch costs 22 % img/s, and a host that blocks on an event fewer than ~30 batches old starves the
    graph-launch queue (depth 2: 1450 img/s, depth 8: 3700, against 6535 resident) -- hence DeviceFeeder's deep ring: at
    depth 32 the poll passes immediately in steady state (64x64: 26 MB)."""

    def __init__(self, depth, device):
        self.device = torch.device(device)
        self.copy_stream = None
        self.ready = [None] * depth
        self.consumed = [None] * depth

    def free(self, s):
        host_wait(self.ready[s])
        host_wait(self.consumed[s])

    @contextlib.contextmanager
    def copying(self, s):
        if self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(device=self.device)
        with torch.cuda.stream(self.copy_stream):
            yield
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.ready[s] = ev

    @contextlib.contextmanager
    def reading(self, s):
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.ready[s])
        yield
        done = torch.cuda.Event()
        done.record(cur)
        self.consumed[s] = done


class FileBatchLoader(object):
    """Batches decoded from one file per frame, on the device.  `__len__` = ceil(files / batch_size) (the reference's
    DataLoaders keep the short last batch), `batch_size`, `__iter__` / `__next__` with StopIteration at the end of the epoch,
    after which the loader can be iterated again.  Every epoch draws a fresh permutation of the files from one generator
    seeded with `seed` (shuffle=False: file order); `order` holds the file indices of the epoch in progress.

    `num_workers` reader threads (at most MAX_WORKERS) read the files and run the serial half of the decoder (C calls that
    drop the GIL) straight into a pinned slot of a ring of `depth`, up to depth - 1 batches ahead; per batch there is one
    copy on a side stream.  A slot is refilled only after the host has seen both its copy and the launches that read it
    complete (SlotEvents).  A file that cannot be read or decoded raises GenesisHipError naming its path, from the `__next__` that would
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
        self.events = SlotEvents(self.depth, self.device)
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
        self.events.free(s)
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
        with self.events.copying(s):
            staged = self._stage(s, n, results)
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
        with self.events.reading(s):
            batch = self._batch(s, staged)
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
