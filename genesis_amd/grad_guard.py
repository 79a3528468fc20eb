"""Gradient-norm clipping and the skip-on-non-finite rule without a host read (gx_grad_guard, include/genesis_hip.h).

`torch.nn.utils.clip_grad_norm_` is a norm launch per parameter, a stack, a norm, a clamp and a multiply per parameter;
`torch.isfinite(...).item()` stalls the host every iteration.  Here the gradients are the segments of ONE streaming reduction that
leaves a small device record -- S = sum g^2 in fp64, the norm, torch's clip coefficient, the scale the optimiser launch multiplies
the gradient by, an "everything is finite" flag and a cumulative count of skipped steps -- which the guarded tail launches of the
training step (`TrainStep(max_grad_norm=, skip_nonfinite=)`) and `gx_scale_multi_guarded` read on the device.

`GradGuard(tensors)`: the descriptor table (host and device copy), the workspace and the record for a fixed set of segments,
allocated once; `run()` is the guard call, `scale()` the in-place multiply by the coefficient.
`clip_grad_norm_`: the import replacement for torch's function in an unchanged loop."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import GenesisHipError

# descriptor words, sizes and record offsets of gx_grad_guard (tests/test_grad_guard_cpu.py holds them against include/genesis_hip.h)
FP32, FP64 = 0, 1
D_SRC, D_N, D_DTYPE, D_WORK = range(4)
DESC_WORDS = 4
CHUNK = 8192            # elements per unit of work
MAX_GRID = 1024         # workgroups of the reduction, whatever the element count
MAX_CHECK = 8
R_S, R_NORM, R_COEF, R_SCALE, R_OK, R_SKIPPED = 0, 8, 12, 16, 20, 24
RECORD_BYTES = 32


def _p(addr):
    return ctypes.c_void_p(addr)


def make_table(segments):
    """segments: (device address, elements, FP32 | FP64) each -> (int64 table [S, DESC_WORDS], total chunks)."""
    table = np.zeros((len(segments), DESC_WORDS), np.int64)
    work = 0
    for i, (addr, n, dtype) in enumerate(segments):
        table[i] = (addr, n, dtype, work)
        work += -(-int(n) // CHUNK)
    return table, work


class GradGuard(object):
    """The guard over a fixed set of contiguous fp32 / fp64 device tensors (read in place).  `record` is the device record;
    `S` (fp64), `norm`, `coef`, `scale` (fp32), `ok` (int32) and `skipped` (int64) are 0-dim views of it: reading one is the
    caller's synchronisation, never the guard's."""

    def __init__(self, tensors):
        tensors = list(tensors)
        if not tensors:
            raise GenesisHipError('GradGuard: no segment')
        self.device = tensors[0].device
        segs = []
        for t in tensors:
            if not t.is_cuda or t.device != self.device:
                raise GenesisHipError('GradGuard: every segment must be on the same HIP device (got %s and %s)' % (self.device, t.device))
            if t.dtype not in (torch.float32, torch.float64) or not t.is_contiguous() or t.numel() == 0:
                raise GenesisHipError('GradGuard: a segment must be a contiguous, non-empty float32 or float64 tensor (got %s %s)'
                                      % (t.dtype, tuple(t.shape)))
            segs.append((t.data_ptr(), t.numel(), FP32 if t.dtype == torch.float32 else FP64))
        self.tensors = tensors                      # (keeps the memory the table points at alive)
        self.table, self.work = make_table(segs)
        with torch.cuda.device(self.device):
            self.table_dev = torch.from_numpy(self.table).to(self.device)
            self.ws_bytes = _lib.query('gx_grad_guard_ws_bytes', self.work)
            self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=self.device)
            self.record = torch.zeros(RECORD_BYTES // 8, dtype=torch.int64, device=self.device)
        raw = self.record.view(torch.uint8)
        self.S = raw[R_S:R_S + 8].view(torch.float64)[0]
        self.norm = raw[R_NORM:R_NORM + 4].view(torch.float32)[0]
        self.coef = raw[R_COEF:R_COEF + 4].view(torch.float32)[0]
        self.scale_factor = raw[R_SCALE:R_SCALE + 4].view(torch.float32)[0]
        self.ok = raw[R_OK:R_OK + 4].view(torch.int32)[0]
        self.skipped = raw[R_SKIPPED:R_SKIPPED + 8].view(torch.int64)[0]

    def _stream(self):
        return _p(torch.cuda.current_stream(self.device).cuda_stream)

    def run(self, gscale=1.0, max_norm=None, check=None, force_ok=False):
        """The guard call (two launches).  gscale: the factor the optimiser launch would receive (1 / world); max_norm: None for
        no clipping; check: a contiguous fp32 device tensor of at most MAX_CHECK scalars that must be finite too."""
        n_check = 0 if check is None else check.numel()
        _lib.call('gx_grad_guard', _p(self.table.ctypes.data), _p(self.table_dev.data_ptr()), self.table.size, self.table.shape[0],
                  _p(check.data_ptr()) if n_check else None, n_check, float(gscale), float(max_norm) if max_norm else 0.0,
                  int(bool(force_ok)), _p(self.record.data_ptr()), _p(self.ws.data_ptr()), self.ws_bytes, self._stream())

    def scale(self):
        """Every element of every segment times `coef`, in its own type, in place (one launch; nothing is touched for coef == 1)."""
        _lib.call('gx_scale_multi_guarded', _p(self.table.ctypes.data), _p(self.table_dev.data_ptr()), self.table.size,
                  self.table.shape[0], _p(self.record.data_ptr()), self._stream())


def check_max_grad_norm(value, name='max_grad_norm'):
    """None, or a positive finite number -> float; anything else: ValueError naming the argument."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or \
            not math.isfinite(float(value)) or float(value) <= 0.0:
        raise ValueError('%s must be a positive finite number (or None: no clipping), got %r' % (name, value))
    return float(value)


# ---- the drop-in ------------------------------------------------------------------------------------------------------------
_CACHE = collections.OrderedDict()      # (device, (address, elements, dtype) per gradient) -> GradGuard
_CACHE_ENTRIES = 4


def _guard_for(grads):
    key = (grads[0].device,) + tuple((g.data_ptr(), g.numel(), g.dtype) for g in grads)
    guard = _CACHE.get(key)
    if guard is None:
        from . import autostep
        # every gradient a view of the unchanged loop's flat buffers (their padding is zero): one segment per buffer
        flat = autostep.flat_grad_buffers(grads)
        guard = GradGuard(flat if flat is not None else grads)
        _CACHE[key] = guard
        while len(_CACHE) > _CACHE_ENTRIES:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return guard


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Import replacement for torch.nn.utils.clip_grad_norm_, called where a loop calls that function (between loss.backward() and
    optimiser.step()): one guard call over all gradients and one in-place scale launch by
    clamp(max_norm / (total_norm + 1e-6), max=1), which returns without touching memory when the coefficient is 1.  Returns the
    total norm as a device fp32 scalar -- no host read here; a non-finite norm gives torch's result for error_if_nonfinite=False
    (the coefficient above, NaN propagated).  Parameters without a gradient are skipped.  The squares are summed in fp64 over all
    elements (torch: the fp32 norm of per-tensor fp32 norms).  Refused with GenesisHipError: norm_type other than 2,
    error_if_nonfinite=True (it needs a host read), max_norm that is not a positive number, gradients on the host, of a dtype other
    than float32 / float64, or not contiguous.  `foreach` is accepted and ignored."""
    if float(norm_type) != 2.0:
        raise GenesisHipError('norm_type=%r is not supported: only the 2-norm is reduced on the device' % (norm_type,))
    if error_if_nonfinite:
        raise GenesisHipError('error_if_nonfinite=True needs a host read of the norm in every call and is not supported; '
                              'test the returned norm where the loop already synchronises')
    try:
        mx = float(max_norm)
    except (TypeError, ValueError):
        mx = float('nan')
    if not mx > 0.0:
        raise GenesisHipError('max_norm=%r: expected a positive number' % (max_norm,))
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    for i, g in enumerate(grads):
        if not g.is_cuda:
            raise GenesisHipError('parameters: gradient %d is on %s; the norm is reduced on the HIP device, there is no CPU path'
                                  % (i, g.device))
        if g.dtype not in (torch.float32, torch.float64):
            raise GenesisHipError('parameters: gradient %d is %s; float32 and float64 are supported' % (i, g.dtype))
        if not g.is_contiguous():
            raise GenesisHipError('parameters: gradient %d of shape %s with strides %s is not contiguous' % (i, tuple(g.shape), g.stride()))
        if g.device != grads[0].device:
            raise GenesisHipError('parameters: gradient %d is on %s, the ones before it on %s' % (i, g.device, grads[0].device))
    grads = [g for g in grads if g.numel()]
    if not grads:
        return torch.tensor(0.0)
    guard = _guard_for(grads)
    guard.run(1.0, mx, force_ok=True)
    guard.scale()
    return guard.norm.clone()            # (the record is overwritten by the next call)
