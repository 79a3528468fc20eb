"""Averaged weights for an unchanged training loop (the reference's train.py with torch's own optimiser and schedulers): an
exponential moving average of every parameter in ONE launch per update (gx_ema_multi, include/genesis_hip.h) instead of a `lerp_` per
parameter and a second model object.

`ModelEMA(model, decay, warmup=False)`: `update()` after `optimiser.step()`; `with ema.applied():` runs evaluation, FID or picture
logging on the averaged weights with the same `model` object.  The average is kept in each parameter's own dtype (as
torch.optim.swa_utils.AveragedModel and timm keep it); buffers (BatchNorm running statistics) are not averaged.  TrainStep has the
same average inside its optimiser launch (`TrainStep(ema_decay=)`)."""
import collections
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GenesisHipError
from .schedule import check_ema_decay

# descriptor words and sizes of gx_ema_multi (tests/test_lr_ema_cpu.py holds them against include/genesis_hip.h)
FP32, FP64 = 0, 1
D_SRC, D_DST, D_N, D_DTYPE, D_WORK = range(5)
DESC_WORDS = 5
CHUNK = 8192            # elements per unit of work
MAX_GRID = 1024         # workgroups of the launch, whatever the element count


def _p(addr):
    return ctypes.c_void_p(addr)


def make_table(segments):
    """segments: (parameter address, average address, elements, FP32 | FP64) each -> (int64 table [S, DESC_WORDS], total chunks)."""
    table = np.zeros((len(segments), DESC_WORDS), np.int64)
    work = 0
    for i, (src, dst, n, dtype) in enumerate(segments):
        table[i] = (src, dst, n, dtype, work)
        work += -(-int(n) // CHUNK)
    return table, work


def ema_multi(table, table_dev, step, decay, warmup=False, decay_used=None, stream=None):
    """One gx_ema_multi launch over a table from make_table (host copy and device copy); step: the device int64 counter holding t."""
    if stream is None:
        stream = _p(torch.cuda.current_stream(step.device).cuda_stream)
    _lib.call('gx_ema_multi', _p(table.ctypes.data), _p(table_dev.data_ptr()), table.size, table.shape[0], _p(step.data_ptr()),
              float(decay), int(bool(warmup)), _p(decay_used.data_ptr()) if decay_used is not None else None, stream)


class ModelEMA(object):
    """e <- e + (1 - decay_t)(p - e) for every parameter of `model` (those that exist at construction, whether or not they require a
    gradient), decay_t = decay, or min(decay, (1 + t) / (10 + t)) with warmup, t = the number of updates so far.  The average starts
    as a copy of the parameters.  Refused with GenesisHipError: parameters on the host, of a dtype other than float32 / float64 or
    not contiguous, and -- in update() / applied() -- a parameter set that is no longer the one seen at construction."""

    def __init__(self, model, decay, warmup=False):
        try:
            self.decay = check_ema_decay(decay, 'decay')
        except ValueError as e:
            raise GenesisHipError(str(e))
        if self.decay is None:
            raise GenesisHipError('decay must be a number in [0, 1), got None')
        self.warmup = bool(warmup)
        self.model = model
        named = [(n, p) for n, p in model.named_parameters() if p.numel()]
        if not named:
            raise GenesisHipError('ModelEMA: the model has no parameters')
        self.device = named[0][1].device
        for n, p in named:
            if not p.is_cuda:
                raise GenesisHipError('ModelEMA: parameter %s is on %s; the average is kept on the HIP device, there is no CPU path'
                                      % (n, p.device))
            if p.device != self.device:
                raise GenesisHipError('ModelEMA: parameter %s is on %s, the ones before it on %s' % (n, p.device, self.device))
            if p.dtype not in (torch.float32, torch.float64):
                raise GenesisHipError('ModelEMA: parameter %s is %s; float32 and float64 are supported' % (n, p.dtype))
            if not p.is_contiguous():
                raise GenesisHipError('ModelEMA: parameter %s of shape %s with strides %s is not contiguous'
                                      % (n, tuple(p.shape), p.stride()))
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        with torch.no_grad():
            self.shadow = [p.detach().clone() for p in self.params]
        self._key = self._signature()
        self.table, self.work = make_table([(p.data_ptr(), e.data_ptr(), p.numel(), FP32 if p.dtype == torch.float32 else FP64)
                                            for p, e in zip(self.params, self.shadow)])
        with torch.cuda.device(self.device):
            self.table_dev = torch.from_numpy(self.table).to(self.device)
            self.updates = torch.zeros((), dtype=torch.int64, device=self.device)
            self.decay_used = torch.zeros((), dtype=torch.float64, device=self.device)
        self._applied = False

    def _signature(self):
        return tuple((id(p), p.data_ptr(), p.numel(), p.dtype) for _, p in self.model.named_parameters() if p.numel())

    def _check_unchanged(self, what):
        if self._signature() != self._key:
            raise GenesisHipError('ModelEMA.%s: the model\'s parameters are not the ones seen at construction (added, removed, moved '
                                  'or re-allocated); build a new ModelEMA' % what)

    def update(self):
        """After optimiser.step(): bump the update counter and average, two launches, no host read."""
        self._check_unchanged('update')
        if self._applied:
            raise GenesisHipError('ModelEMA.update inside applied(): the parameters hold the averaged weights')
        stream = _p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.call('gx_step_increment', _p(self.updates.data_ptr()), stream)
        ema_multi(self.table, self.table_dev, self.updates, self.decay, self.warmup, self.decay_used, stream)

    @contextlib.contextmanager
    def applied(self):
        """Inside, the model's parameters hold the averaged weights (contents swapped on the device); swapped back on exit, also on
        an exception."""
        self._check_unchanged('applied')
        if self._applied:
            raise GenesisHipError('ModelEMA.applied is not re-entrant')
        self._swap()
        self._applied = True
        try:
            yield self.model
        finally:
            self._applied = False
            self._swap()

    def _swap(self):
        with torch.no_grad():
            for p, e in zip(self.params, self.shadow):
                tmp = p.detach().clone()
                p.copy_(e)
                e.copy_(tmp)

    def state_dict(self):
        return {'decay': self.decay, 'warmup': self.warmup, 'updates': int(self.updates),
                'ema_state_dict': collections.OrderedDict((n, e.detach().clone()) for n, e in zip(self.names, self.shadow))}

    def load_state_dict(self, sd):
        esd = sd['ema_state_dict']
        missing = [n for n in self.names if n not in esd]
        if missing:
            raise GenesisHipError('ModelEMA.load_state_dict: no average for %s' % ', '.join(missing[:5]))
        with torch.no_grad():
            for n, e in zip(self.names, self.shadow):
                e.copy_(esd[n])
            self.updates.fill_(int(sd.get('updates', 0)))
