"""A loader's decoded split kept on the device after its first epoch.

Most loaders here decode on the device but are bound by per-file host work, and deliver fewer frames a second than the
training step consumes.  A decoded 64 x 64 frame is 12 KB as bytes, so the whole split usually
fits the device many times over: `CachedLoader(loader)` passes the first epoch through unchanged while it narrows every batch
back to bytes (labels to int16) into a resident store, and serves every later epoch from that store the way
multid_config.MultidLoader serves its resident split: an epoch uploads one permutation, a batch is one gather launch per field.

The cache is exact or it is off.  The store kernel counts, on the device, the frame values that are not bit for bit
byte / 255 (mode 0) or byte * (1 / 255) (mode 1, what the JPEG path of GQN delivers) and the labels that do not fit int16; one
host read at the end of the first complete epoch picks the mode or switches the cache off.  Off means: the wrapper passes the
wrapped loader's batches through for good, with one printed line that says why.  It never breaks the run it was switched on for.

What the option changes, on purpose:
  * Cached epochs reshuffle every epoch from the wrapper's own numpy generator (seeded with `seed`), not the loader's; the
    record readers (multi_object_config, gqn_config) repeat one order without it.
  * A loader that is only ever consumed partly (an evaluation over `num_batches` batches) never becomes resident: an epoch left
    before StopIteration discards what was filled.
  * With one process per GPU each rank caches its own shard.
  * A split that does not fit the budget (GQN's full train split: 10.8 M frames x 12 KB) switches itself off.

Switching it on: `cfg.cache_on_device = True` (an attribute, not a registered flag) or the environment variable
GENESIS_DATA_CACHE (`1`: the default budget, half of the free device memory; another number: GB per loader) make the data
configs wrap their three loaders: wrap_loaders().

Resident epochs can be augmented on the device (genesis_amd/augment.py): `CachedLoader(loader, augment=Augment(...))` serves
them through ONE launch of gx_cache_gather_aug per batch instead of the two plain gathers; cfg.augment or GENESIS_AUGMENT
make wrap_loaders() do that for the train loader."""
import ctypes
import os
import time

import numpy as np
import torch

from genesis_amd import compat as _compat

_compat.install()

from forge.experiment_tools import fprint  # noqa: E402

from genesis_amd import _lib  # noqa: E402
from genesis_amd import augment as _augment  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

ENV = 'GENESIS_DATA_CACHE'
KEYS = ('input', 'instances')
MODES = ('byte / 255', 'byte * (1 / 255)')
MAX_LAUNCH_ROWS = 65535                     # of one launch of the kernels (gridDim.y)
DIV_MISS, MUL_MISS, LABEL_MISFIT = 0, 1, 2  # the counters' words


def row_stride(row_bytes):
    """The byte stride of a store's rows: the row rounded up to a multiple of 16, so that every row starts 16-byte aligned."""
    return -(-int(row_bytes) // 16) * 16


def new_store(rows, row_bytes, device):
    """An uninitialised store of `rows` rows of row_bytes bytes: uint8 [rows, row_stride(row_bytes)]."""
    return torch.empty(int(rows), row_stride(row_bytes), dtype=torch.uint8, device=device)


def new_counters(device):
    """The three int64 device words (div_miss, mul_miss, label_misfit) the store kernels add to, zeroed."""
    return torch.zeros(3, dtype=torch.int64, device=device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check_store(store, row_bytes):
    if not (isinstance(store, torch.Tensor) and store.is_cuda and store.dtype == torch.uint8 and store.dim() == 2
            and store.is_contiguous() and store.shape[1] == row_stride(row_bytes)):
        raise GenesisHipError('data_cache: the store must be a contiguous uint8 device tensor [rows, %d] (new_store)'
                              % row_stride(row_bytes))


def _check_batch(t, dtype, what, channels=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise GenesisHipError('data_cache: %s must be on the HIP device; there is no CPU path' % what)
    if t.dtype != dtype or t.dim() != 4 or not t.is_contiguous() or 0 in t.shape or (channels and t.shape[1] != channels):
        raise GenesisHipError('data_cache: %s must be a contiguous %s [B,%s,H,W] tensor, not %s %s'
                              % (what, dtype, channels or 'C', t.dtype, list(t.shape)))


def _check_counters(counters):
    if not (isinstance(counters, torch.Tensor) and counters.is_cuda and counters.dtype == torch.int64
            and counters.is_contiguous() and counters.numel() == 3):
        raise GenesisHipError('data_cache: the counters must be three int64 device words (new_counters)')


def store_frames(batch, store, first_row, counters):
    """batch fp32 [B,C,H,W] -> rows first_row .. first_row + B of `store` as bytes, one launch of gx_cache_store_u8 on the
    current stream; counters[0] / [1] grow by the values that are not byte / 255 / not byte * (1 / 255), bit for bit."""
    _check_batch(batch, torch.float32, 'frames')
    B, C, H, W = batch.shape
    _check_store(store, C * H * W)
    _check_counters(counters)
    _lib.call('gx_cache_store_u8', _ptr(batch), _ptr(store), int(store.shape[1]), int(first_row), int(store.shape[0]),
              _ptr(counters), B, C, H, W, _stream(batch))


def store_labels(labels, store, first_row, counters):
    """labels int64 [B,1,H,W] -> rows first_row .. first_row + B of `store` as int16, one launch of
    gx_cache_store_labels_i16; counters[2] grows by the values outside -32768 .. 32767."""
    _check_batch(labels, torch.int64, 'label maps', channels=1)
    B, _, H, W = labels.shape
    _check_store(store, 2 * H * W)
    _check_counters(counters)
    _lib.call('gx_cache_store_labels_i16', _ptr(labels), _ptr(store), int(store.shape[1]), int(first_row), int(store.shape[0]),
              _ptr(counters), B, H, W, _stream(labels))


def _gather_args(store, idx, first, B):
    if idx is not None and not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1
                                and idx.is_contiguous()):
        raise GenesisHipError('data_cache: idx must be a contiguous int64 vector on the HIP device')
    n = int(store.shape[0] if idx is None else idx.shape[0])
    first = int(first)
    B = n - first if B is None else int(B)
    if first < 0 or B <= 0 or first + B > n:
        raise GenesisHipError('data_cache: rows %d .. %d reach outside the %d %s'
                              % (first, first + B, n, 'rows stored' if idx is None else 'indices'))
    return first, B, (None if idx is None else _ptr(idx)), (0 if idx is None else n)


def gather_frames(store, shape, idx=None, first=0, B=None, mode=0):
    """-> fp32 [B, C, H, W] ((C, H, W) = shape): the rows idx[first : first + B] of a frame store (idx: int64 device vector;
    None: the rows first : first + B themselves), each byte / 255 (mode 0) or * (1 / 255) (mode 1).  One launch of
    gx_cache_gather_f32 on the current stream and nothing else.  The values of idx are NOT checked: the caller checks them on
    the host before uploading."""
    C, H, W = (int(v) for v in shape)
    _check_store(store, C * H * W)
    first, B, pidx, nidx = _gather_args(store, idx, first, B)
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=store.device)
    _lib.call('gx_cache_gather_f32', _ptr(store), int(store.shape[1]), int(store.shape[0]), pidx, nidx, first, int(mode), _ptr(out),
              B, C, H, W, _stream(store))
    return out


def gather_labels(store, shape, idx=None, first=0, B=None):
    """-> int64 [B, 1, H, W] ((H, W) = shape): the same rows of a label store, one launch of gx_cache_gather_labels."""
    H, W = (int(v) for v in shape)
    _check_store(store, 2 * H * W)
    first, B, pidx, nidx = _gather_args(store, idx, first, B)
    out = torch.empty(B, 1, H, W, dtype=torch.int64, device=store.device)
    _lib.call('gx_cache_gather_labels', _ptr(store), int(store.shape[1]), int(store.shape[0]), pidx, nidx, first, _ptr(out), B, H, W,
              _stream(store))
    return out


def check_order(order, n):
    """An epoch's cache rows against [0, n), on the host, before they are uploaded: the gather kernels do not check
    (multid_config.check_order)."""
    if len(order) and (int(order.min()) < 0 or int(order.max()) >= n):
        raise GenesisHipError('data_cache: a row of the epoch (%d .. %d) is outside the %d rows cached'
                              % (int(order.min()), int(order.max()), n))


class CachedLoader(object):
    """Wraps a loader of device batches {'input': fp32 [B,C,H,W]} (+ 'instances': int64 [B,1,H,W]).  `cache_state` is
    'filling' until the first complete epoch has been stored, then 'resident' or 'off: <reason>'; `order` holds the cache
    rows of a resident epoch (batch k is rows order[k * B : (k + 1) * B]); `loader` is the wrapped one.  With `augment` (an
    augment.Augment) the resident epochs are augmented: `epoch` is the counter the random draws are keyed with, 0 in the first
    resident epoch and one more at every later resident __iter__; set_epoch() sets the next one's when a run is resumed.  The
    filling epoch and a cache that is off deliver the wrapped loader's batches as they are."""

    def __init__(self, loader, budget_bytes=None, shuffle=None, seed=0, name=None, augment=None):
        if not (hasattr(loader, '__len__') and hasattr(loader, 'batch_size')):
            raise GenesisHipError('data_cache: the loader (%s) needs __len__ and batch_size: the store is sized from them'
                                  % type(loader).__name__)
        if int(loader.batch_size) <= 0:
            raise GenesisHipError('data_cache: batch_size must be positive, not %r' % (loader.batch_size,))
        if budget_bytes is not None and not budget_bytes > 0:
            raise GenesisHipError('data_cache: budget_bytes must be positive, not %r' % (budget_bytes,))
        if augment is not None and not isinstance(augment, _augment.Augment):
            raise GenesisHipError('data_cache: augment must be an augment.Augment or None, not %r' % (augment,))
        self.loader = loader
        self.augment = augment
        self.epoch = 0                     # the resident epoch in progress, from 0: what the augmentation's draws are keyed with
        self.next_epoch = 0                # ... and the one the next resident __iter__ starts (set_epoch)
        self.batch_size = int(loader.batch_size)
        self.budget_bytes = None if budget_bytes is None else int(budget_bytes)
        self.shuffle = shuffle
        self.rng = np.random.RandomState(int(seed) % (1 << 32))
        self.name = name or type(loader).__name__
        self.cache_state = 'filling'
        self.order = None
        self.mode = None
        self.rows = 0                      # rows cached (resident) / stored so far this epoch (filling)
        self.source = None                 # the wrapped loader's epoch in progress
        self.started = None
        self.shapes = None                 # {key: (shape[1:], dtype)} of the first batch
        self.frames = self.labels = self.counters = self.dev_order = None
        self.pos = 0
        self.told = False                  # the filling epoch's line about augmentation has been printed

    def __len__(self):
        if self.cache_state == 'resident':
            return -(-self.rows // self.batch_size)
        return len(self.loader)

    # ---- epochs ----
    def __iter__(self):
        if self.cache_state == 'resident':
            shuffle = getattr(self.loader, 'shuffle', True) if self.shuffle is None else self.shuffle
            order = (self.rng.permutation(self.rows) if shuffle else np.arange(self.rows)).astype(np.int64)
            check_order(order, self.rows)
            self.order = order
            self.dev_order = torch.from_numpy(order).to(self.frames.device)       # the epoch's one upload
            self.pos = 0
            self.epoch = self.next_epoch
            self.next_epoch += 1
            return self
        if self.cache_state == 'filling':
            if self.budget_bytes is None and torch.cuda.is_available():
                self.budget_bytes = max(1, torch.cuda.mem_get_info()[0] // 2)
            self.rows = 0                                                         # an epoch left half way is discarded
            if self.counters is not None:
                self.counters.zero_()
            self.started = time.perf_counter()
            if self.augment is not None and not self.told:
                self.told = True
                fprint('data_cache: %s: the epoch that fills the cache is not augmented; resident epochs are (%r)'
                       % (self.name, self.augment))
        self.source = iter(self.loader)
        return self

    def __next__(self):
        if self.cache_state == 'resident':
            return self._gather()
        if self.source is None:
            iter(self)
            if self.cache_state == 'resident':
                return self._gather()
        try:
            batch = next(self.source)
        except StopIteration:
            self.source = None
            if self.cache_state == 'filling' and self.rows:
                self._decide()
            raise
        if self.cache_state == 'filling':
            try:
                reason = self._store(batch)
            except GenesisHipError as e:
                reason = str(e)
            if reason:
                self._off(reason)
        return batch

    def _gather(self):
        if self.dev_order is None:
            iter(self)
        if self.pos >= self.rows:
            self.dev_order = None                       # `order` keeps the finished epoch's rows until the next one starts
            raise StopIteration
        first = self.pos
        B = min(self.batch_size, self.rows - first)
        self.pos = first + B
        (shape, _) = self.shapes['input']
        if self.augment is not None:
            x, y = _augment.gather(self.frames, self.labels, shape, self.augment, self.epoch, self.dev_order, first, B, self.mode)
            return {'input': x} if y is None else {'input': x, 'instances': y}
        batch = {'input': gather_frames(self.frames, shape, self.dev_order, first, B, self.mode)}
        if self.labels is not None:
            batch['instances'] = gather_labels(self.labels, self.shapes['instances'][0][1:], self.dev_order, first, B)
        return batch

    # ---- filling ----
    def _store(self, batch):
        """Stores one batch of the filling epoch; -> None, or why the cache cannot go on."""
        if not isinstance(batch, dict) or 'input' not in batch or any(k not in KEYS for k in batch):
            keys = sorted(batch) if isinstance(batch, dict) else type(batch).__name__
            return 'a batch has keys other than input / instances (%s)' % (keys,)
        for k in batch:
            if not (isinstance(batch[k], torch.Tensor) and batch[k].is_cuda):
                return "a batch's %r is a host tensor" % k
        shapes = {k: (tuple(batch[k].shape[1:]), batch[k].dtype) for k in batch}
        B = int(batch['input'].shape[0])
        if self.shapes is None:
            reason = self._allocate(batch, shapes)
            if reason:
                return reason
        if shapes != self.shapes or any(int(batch[k].shape[0]) != B or not batch[k].is_contiguous() for k in batch):
            return 'a batch (%s) differs in shape or dtype from the first one (%s)' % (
                ', '.join('%s %s %s' % (k, batch[k].dtype, list(batch[k].shape)) for k in sorted(batch)),
                ', '.join('%s %s [B, %s]' % (k, d, ', '.join(map(str, s))) for k, (s, d) in sorted(self.shapes.items())))
        if B == 0:
            return None
        if B > MAX_LAUNCH_ROWS:
            return 'a batch of %d rows is more than one launch stores (%d)' % (B, MAX_LAUNCH_ROWS)
        capacity = int(self.frames.shape[0])
        if self.rows + B > capacity:
            return 'the loader delivered more than the len(loader) * batch_size = %d rows the store was sized for' % capacity
        store_frames(batch['input'], self.frames, self.rows, self.counters)
        if self.labels is not None:
            store_labels(batch['instances'], self.labels, self.rows, self.counters)
        self.rows += B
        return None

    def _allocate(self, batch, shapes):
        x = batch['input']
        if x.dtype != torch.float32 or x.dim() != 4:
            return 'frames are %s %s, not float32 [B,C,H,W]' % (x.dtype, list(x.shape))
        y = batch.get('instances')
        if y is not None and (y.dtype != torch.int64 or y.dim() != 4 or y.shape[1] != 1 or y.shape[2:] != x.shape[2:]):
            return 'label maps are %s %s, not int64 [B,1,H,W] of the frames\' size' % (y.dtype, list(y.shape))
        if self.augment is not None and x.shape[1] > _augment.MAX_CHANNELS:
            return 'frames of %d channels cannot be augmented (at most %d)' % (x.shape[1], _augment.MAX_CHANNELS)
        capacity = len(self.loader) * self.batch_size
        if capacity <= 0:
            return 'the loader has no batches'
        C, H, W = shapes['input'][0]
        need = capacity * (row_stride(C * H * W) + (row_stride(2 * H * W) if y is not None else 0))
        if self.budget_bytes is not None and need > self.budget_bytes:
            return 'the store of %d rows would take %d bytes, over the budget of %d bytes' % (capacity, need, self.budget_bytes)
        try:
            self.frames = new_store(capacity, C * H * W, x.device)
            self.labels = new_store(capacity, 2 * H * W, x.device) if y is not None else None
            self.counters = new_counters(x.device)
        except RuntimeError as e:                       # out of memory: the budget was a guess
            self.frames = self.labels = self.counters = None
            return 'the store of %d bytes could not be allocated (%s)' % (need, str(e).splitlines()[0])
        self.shapes = shapes
        return None

    def _decide(self):
        """The end of the first complete epoch: ONE host read of the three counters."""
        div_miss, mul_miss, label_misfit = (int(v) for v in self.counters.tolist())
        if label_misfit:
            return self._off('%d label values do not fit int16' % label_misfit)
        if div_miss and mul_miss:
            return self._off('the frames are not bytes / 255: %d values differ from byte / 255 and %d from byte * (1 / 255)'
                             % (div_miss, mul_miss))
        self.mode = 0 if div_miss == 0 else 1
        self.cache_state = 'resident'
        self.order = None
        self.counters = None
        if hasattr(self.loader, 'close'):
            self.loader.close()
        held = self.rows * (self.frames.shape[1] + (self.labels.shape[1] if self.labels is not None else 0))
        fprint('data_cache: %s: %d rows resident on %s (%.1f MB, frames as %s, labels %s) after an epoch of %.2f s'
               % (self.name, self.rows, self.frames.device, held / 1e6, MODES[self.mode],
                  'none' if self.labels is None else 'int16', time.perf_counter() - self.started))

    def _off(self, reason):
        self.cache_state = 'off: ' + reason
        self.frames = self.labels = self.counters = self.dev_order = None
        self.shapes = None
        self.rows = 0
        fprint('data_cache: %s: not cached, batches pass through%s: %s'
               % (self.name, '' if self.augment is None else ', augmentation is off too', reason))

    def set_epoch(self, n):
        """The counter of the next resident epoch to start (resuming a run: the number of resident epochs already trained on)."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 0:
            raise GenesisHipError('data_cache: set_epoch takes a non-negative integer, not %r' % (n,))
        self.epoch = self.next_epoch = n

    def close(self):
        """Frees the store and closes the wrapped loader (which becoming resident has done already); iterating again passes
        the wrapped loader's batches through."""
        resident = self.cache_state == 'resident'
        self.source = None
        self.order = None
        self.frames = self.labels = self.counters = self.dev_order = None
        self.shapes = None
        self.rows = 0
        if resident or self.cache_state == 'filling':
            self.cache_state = 'off: closed'
        if not resident and hasattr(self.loader, 'close'):
            self.loader.close()


def requested(cfg):
    """(on, budget_bytes): whether cfg.cache_on_device or GENESIS_DATA_CACHE ask for the cache, and the budget per loader
    (None: the default, half of the free device memory).  The variable: unset, empty or 0 = off, 1 = on with the default
    budget, any other positive number = on with that many GB (1e9 bytes) per loader."""
    text = os.environ.get(ENV, '').strip()
    if text and text != '0':
        if text == '1':
            return True, None
        try:
            gb = float(text)
        except ValueError:
            gb = -1.0
        if not gb > 0:
            raise GenesisHipError('data_cache: %s=%r is neither 0, 1 nor a positive number of GB' % (ENV, text))
        return True, max(1, int(gb * 1e9))
    return bool(getattr(cfg, 'cache_on_device', False)), None


def wrap_loaders(cfg, loaders, shuffle=None, name=None):
    """The data configs' switch: `loaders` itself unless the cache is requested() or augmentation is (augment.requested: cfg.augment
    / GENESIS_AUGMENT), else a tuple with CachedLoaders around them.  shuffle: one value, or one per loader; None follows the
    loader's own `shuffle` attribute (True without one).  Augmentation wraps loader 0 (train), under the same budget rule,
    whether or not the cache was asked for; the other loaders follow the cache switch alone and are never augmented."""
    on, budget = requested(cfg)
    aug = _augment.requested(cfg)
    if not on and aug is None:
        return loaders
    shuffles = list(shuffle) if isinstance(shuffle, (tuple, list)) else [shuffle] * len(loaders)
    return tuple(CachedLoader(l, budget, shuffle=s, seed=getattr(cfg, 'seed', 0), name='%s[%d]' % (name, i) if name else None,
                              augment=aug if i == 0 else None) if on or i == 0 else l
                 for i, (l, s) in enumerate(zip(loaders, shuffles)))
