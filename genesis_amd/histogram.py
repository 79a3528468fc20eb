"""The reference's histogram logging with its tags and order, computed on the device: `log_grads_and_weights` (train.py:340-345),
`log_distributions` (train.py:313-325) and `add_histogram` for one tensor.  tensorboardX's add_histogram copies the tensor to the
host, widens it to float64 and runs numpy.histogram over its 'tensorflow' table of 1549 edges, plus min, max, sum and dot -- per
tensor, several hundred copies and synchronisations per logging event.

Here every tensor queued on a `Histograms` object is one segment of ONE gx_hist_multi call (include/genesis_hip.h): one upload of
the descriptor table, the call's launches, and ONE device-to-host copy of all counts, statistics and tallies.  What reaches the
writer is what tensorboardX's make_histogram would put into its HistogramProto, through `writer.add_histogram_raw` (tensorboardX
>= 1.7 and torch.utils.tensorboard both have it; it writes the event add_histogram would).

Not here: `max_bins`, numpy's string bin rules and integer bin counts, host tensors, non-contiguous tensors, other dtypes than
fp32 / fp64 (all refused by name).  The event-file writer: genesis_amd/tbwriter.py."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GenesisHipError

# element types, descriptor words and sizes of gx_hist_multi (tests/test_histogram_cpu.py holds them against include/genesis_hip.h)
FP32, FP64 = 0, 1
D_SRC, D_N, D_DTYPE, D_WORK = range(4)
DESC_WORDS = 4
CHUNK = 8192            # elements one workgroup histograms
MAX_EDGES = 4096

Histogram = collections.namedtuple('Histogram', 'tag min max num sum sum_squares bucket_limits bucket_counts nan below above')
Histogram.__doc__ = """One queued tensor as tensorboardX's HistogramProto holds it (min, max, num, sum, sum_squares, bucket_limits,
bucket_counts), and how many of its values were NaN, below the first edge and above the last one (they are in no bucket)."""


# ---- the edge table --------------------------------------------------------------------------------------------------------
_DEFAULT = None
_DEVICE_EDGES = {}      # (bytes, device) -> device tensor [n_edges] float64


def default_bins():
    """tensorboardX's 'tensorflow' table as a read-only float64 array: 774 positive edges 1e-12 * 1.1^n below 1e20 made by repeated
    multiplication in Python floats (the bits matter), mirrored around 0: 1549 edges, 1548 bins."""
    global _DEFAULT
    if _DEFAULT is None:
        pos, v = [], 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        _DEFAULT = np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)
        _DEFAULT.setflags(write=False)
    return _DEFAULT


def _edges(bins):
    """`bins` of add_histogram -> the float64 edge table, or GenesisHipError naming the argument."""
    if isinstance(bins, str):
        if bins == 'tensorflow':
            return default_bins()
        raise GenesisHipError("bins=%r: numpy's string bin rules are not supported; 'tensorflow' or a sequence of edges is" % bins)
    if isinstance(bins, (bool, int, np.integer)) or np.ndim(bins) == 0:
        raise GenesisHipError("bins=%s: a bin count is not supported; 'tensorflow' or a sequence of edges is" % (bins,))
    try:
        e = np.ascontiguousarray(bins, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise GenesisHipError('bins: not a sequence of numbers (%s)' % err)
    if e.ndim != 1 or not 2 <= e.size <= MAX_EDGES:
        raise GenesisHipError('bins: expected a 1-D sequence of 2 to %d edges, got shape %s' % (MAX_EDGES, e.shape))
    if not np.all(np.isfinite(e)) or not np.all(e[1:] > e[:-1]):
        raise GenesisHipError('bins: the edges must be finite and strictly increasing')
    return e


def _device_edges(edges, device):
    key = (edges.tobytes(), str(device))
    if key not in _DEVICE_EDGES:
        _DEVICE_EDGES[key] = torch.from_numpy(np.array(edges)).to(device)
    return _DEVICE_EDGES[key]


def trim(counts, edges):
    """tensorboardX's trimming of a full count vector: with `first` and `last` the first and last non-empty bins,
    (edges[first : last + 2], counts[first - 1 : last + 1]) -- the extra leading empty bucket carries the left limit; for
    first == 0 a zero is put in front instead.  Both lists are empty when every bin is."""
    counts = np.asarray(counts)
    filled = np.flatnonzero(counts)
    if filled.size == 0:
        return [], []
    first, last = int(filled[0]), int(filled[-1])
    kept = counts[first - 1:last + 1].tolist() if first > 0 else [0] + counts[:last + 1].tolist()
    return np.asarray(edges)[first:last + 2].tolist(), kept


# ---- the queue: tensors collected on the host, histogrammed by one call -------------------------------------------------------
class Histograms(object):
    """add(tag, tensor) queues a contiguous fp32 or fp64 device tensor of any shape (it is read in place: do not change it before
    compute()); compute() histograms everything queued with one table upload, one gx_hist_multi call and one device-to-host copy,
    returns the `Histogram` records in queue order and empties the queue.  bins: 'tensorflow' or a 1-D strictly increasing sequence
    of 2 .. 4096 edges."""

    def __init__(self, bins='tensorflow', max_bins=None):
        if max_bins is not None:
            raise GenesisHipError('max_bins=%r is not supported: the buckets are not subsampled' % (max_bins,))
        self.edges = _edges(bins)
        self.items = []      # (tag, tensor)
        self.device = None

    def add(self, tag, tensor):
        if not torch.is_tensor(tensor):
            raise GenesisHipError('histogram %r: expected a tensor, got %s' % (tag, type(tensor).__name__))
        if tensor.dtype not in (torch.float32, torch.float64):
            raise GenesisHipError('histogram %r: expected float32 or float64, got %s' % (tag, tensor.dtype))
        if not tensor.is_contiguous():
            raise GenesisHipError('histogram %r: the tensor %s with strides %s is not contiguous' % (tag, tuple(tensor.shape), tensor.stride()))
        if tensor.numel() == 0:
            raise GenesisHipError('histogram %r: the tensor %s has no element' % (tag, tuple(tensor.shape)))
        if tensor.numel() >= 1 << 31:
            raise GenesisHipError('histogram %r: %d elements; fewer than 2^31 are supported' % (tag, tensor.numel()))
        if not tensor.is_cuda:
            raise GenesisHipError('histogram %r: histograms are computed on the HIP device; there is no CPU path (got a tensor on %s)'
                                  % (tag, tensor.device))
        if self.device is None:
            self.device = tensor.device
        elif tensor.device != self.device:
            raise GenesisHipError('histogram %r: on %s, the tensors queued before it on %s' % (tag, tensor.device, self.device))
        self.items.append((str(tag), tensor.detach()))

    def compute(self):
        S = len(self.items)
        if S == 0:
            return []
        n_edges = self.edges.size
        nb = n_edges - 1
        table = np.zeros((S, DESC_WORDS), np.int64)
        work = 0
        for i, (_, t) in enumerate(self.items):
            table[i] = (t.data_ptr(), t.numel(), FP32 if t.dtype == torch.float32 else FP64, work)
            work += -(-t.numel() // CHUNK)
        with torch.cuda.device(self.device):
            edges = _device_edges(self.edges, self.device)
            dev_table = torch.from_numpy(table).to(self.device)
            # one buffer for everything that goes to the host: stats fp64 [S, 4], tally uint64 [S, 3], counts uint32 [S, nb]
            out = torch.empty(7 * S + (S * nb + 1) // 2, dtype=torch.int64, device=self.device)
            ws_bytes = _lib.query('gx_hist_multi_ws_bytes', work)
            ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=self.device)
            base = out.data_ptr()
            _lib.call('gx_hist_multi', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(dev_table.data_ptr()), table.size, S,
                      ctypes.c_void_p(edges.data_ptr()), n_edges, ctypes.c_void_p(base + 56 * S), ctypes.c_void_p(base),
                      ctypes.c_void_p(base + 32 * S), ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                      ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
            host = out.cpu().numpy()
        stats = host[:4 * S].view(np.float64).reshape(S, 4)
        tally = host[4 * S:7 * S].view(np.uint64).reshape(S, 3)
        counts = host[7 * S:].view(np.uint32)[:S * nb].reshape(S, nb)
        records = []
        for i, (tag, t) in enumerate(self.items):
            nan, below, above = (int(v) for v in tally[i])
            # numpy's min, max, sum and dot are NaN as soon as one value is
            mn, mx, sm, sq = (float('nan'),) * 4 if nan else (float(v) for v in stats[i])
            limits, kept = trim(counts[i], self.edges)
            records.append(Histogram(tag, mn, mx, t.numel(), sm, sq, limits, kept, nan, below, above))
        self.items = []      # (the allocator hands the tensors' memory out again in stream order only)
        return records


def _write(writer, record, global_step):
    writer.add_histogram_raw(record.tag, record.min, record.max, record.num, record.sum, record.sum_squares, record.bucket_limits,
                             record.bucket_counts, global_step)


# ---- the reference's calls ---------------------------------------------------------------------------------------------------
def add_histogram(writer, tag, values, global_step=None, bins='tensorflow', max_bins=None):
    """writer.add_histogram(tag, values, global_step, bins) for one device tensor, handed on as writer.add_histogram_raw(tag, min,
    max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step)."""
    h = Histograms(bins, max_bins)
    h.add(tag, values)
    _write(writer, h.compute()[0], global_step)


def log_grads_and_weights(model, writer, iter_idx):
    """train.py:341-345: 'weights/<name>' and 'grads/<name>' of every model.named_parameters() entry, interleaved as the reference
    logs them, from one pass.  A parameter whose .grad is None gets no 'grads/' call (the reference raises inside tensorboardX)."""
    h = Histograms()
    for name, param in model.named_parameters():
        h.add('weights/%s' % name, param.data)
        if param.grad is not None:
            h.add('grads/%s' % name, param.grad)
    for record in h.compute():
        _write(writer, record, iter_idx)


_DISTRIBUTION_KEYS = ('mu_k', 'sigma_k', 'pmu_k', 'psigma_k')


def log_distributions(writer, att_stats, comp_stats, iter_idx):
    """train.py:313-325: 'att_<key>_<step>' for every entry of att_stats[key], then 'comp_<key>_<step>' for comp_stats, key in
    mu_k, sigma_k, pmu_k, psigma_k; a dict that is None and a key that is absent are skipped.  One pass for all of them."""
    h = Histograms()
    for prefix, stats in (('att', att_stats), ('comp', comp_stats)):
        if stats is None:
            continue
        for key in _DISTRIBUTION_KEYS:
            if key not in stats:
                continue
            for step, val in enumerate(stats[key]):
                h.add('%s_%s_%d' % (prefix, key, step), val)
    for record in h.compute():
        _write(writer, record, iter_idx)
