"""genesis_amd.histogram without a GPU: the edge table, the descriptor constants against the header, every refusal of gx_hist_multi
(raised from the host copy of the table, before any launch) and of the Python layer (raised before the library is called), and
the trimming rule against its restatement."""
import ctypes
import os.path as osp
import re

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd import histogram as hist
from genesis_amd._lib import GenesisHipError
from tests import hist_restatement as R

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def test_default_table():
    e = hist.default_bins()
    assert e.dtype == np.float64 and e.shape == (1549,)
    assert np.all(e[1:] > e[:-1])
    assert e[774] == 0.0 and e[775] == 1e-12
    assert np.array_equal(e, -e[::-1])
    assert e[-1] < 1e20 <= e[-1] * 1.1
    assert e[776] == 1e-12 * 1.1 and e[777] == 1e-12 * 1.1 * 1.1            # repeated multiplication, not 1.1 ** n
    assert np.array_equal(e, R.default_bins())
    assert hist.default_bins() is e                                           # made once


def test_constants_match_the_header():
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define GX_HIST_(\w+) (\d+)', header)}
    assert sorted(defs) == sorted(['FP32', 'FP64', 'D_SRC', 'D_N', 'D_DTYPE', 'D_WORK', 'DESC_WORDS', 'CHUNK', 'MAX_EDGES'])
    for name, v in defs.items():
        assert getattr(hist, name) == v, name
    words = sorted(v for k, v in defs.items() if k.startswith('D_') and k != 'DESC_WORDS')
    assert words == list(range(len(words))) and len(words) <= defs['DESC_WORDS']


# ---- gx_hist_multi: refusals with fake device addresses (validation reads no device memory) -------------------------------------
FAKE = 4096


def _segment(**over):
    row = [0] * hist.DESC_WORDS
    fields = dict(SRC=FAKE, N=100, DTYPE=hist.FP32, WORK=0)
    fields.update(over)
    for k, v in fields.items():
        row[getattr(hist, 'D_' + k)] = v
    return row


def _call(rows, n_segments=None, n_edges=1549, table_words=None, edges=FAKE, counts=FAKE, stats=FAKE, tally=FAKE, ws=FAKE,
          ws_bytes=1 << 30, table_dev=FAKE):
    table = np.array([w for row in rows for w in row], np.int64)
    _lib.call('gx_hist_multi', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(table_dev),
              table.size if table_words is None else table_words, len(rows) if n_segments is None else n_segments,
              ctypes.c_void_p(edges), n_edges, ctypes.c_void_p(counts), ctypes.c_void_p(stats), ctypes.c_void_p(tally),
              ctypes.c_void_p(ws), ws_bytes, None)


@pytest.mark.parametrize('rows, kwargs, message', [
    ([_segment()], dict(edges=0), 'null pointer'),
    ([_segment()], dict(counts=0), 'null pointer'),
    ([_segment()], dict(stats=0), 'null pointer'),
    ([_segment()], dict(tally=0), 'null pointer'),
    ([_segment()], dict(ws=0), 'null pointer'),
    ([_segment()], dict(table_dev=0), 'null pointer'),
    ([_segment()], dict(n_segments=0), 'n_segments = 0 below 1'),
    ([_segment()], dict(n_edges=1), r'n_edges = 1 outside \[2, 4096\]'),
    ([_segment()], dict(n_edges=4097), r'n_edges = 4097 outside \[2, 4096\]'),
    ([_segment(N=0)], {}, r'segment 0: N = 0 outside \[1, 2\^31\)'),
    ([_segment(N=-5)], {}, 'segment 0: N = -5 outside'),
    ([_segment(N=1 << 31)], {}, 'segment 0: N = 2147483648 outside'),
    ([_segment(DTYPE=2)], {}, 'segment 0: unknown dtype 2'),
    ([_segment(DTYPE=-1)], {}, 'segment 0: unknown dtype -1'),
    ([_segment(SRC=0)], {}, 'segment 0: null source'),
    ([_segment(SRC=FAKE + 2)], {}, 'segment 0: source 0x1002 is not aligned to its 4-byte elements'),
    ([_segment(SRC=FAKE + 4, DTYPE=1)], {}, 'segment 0: source 0x1004 is not aligned to its 8-byte elements'),
    ([_segment(WORK=1)], {}, 'segment 0: WORK = 1, the prefix is 0'),
    ([_segment(N=8193), _segment(WORK=1)], {}, 'segment 1: WORK = 1, the prefix is 2'),      # 8193 elements are two chunks
    ([_segment(), _segment(WORK=1)], dict(table_words=7), '2 segments do not fit a table of 7 words'),
    ([_segment(N=8193)], dict(ws_bytes=64), 'workspace of 64 bytes, 128 needed'),
    ([_segment()], dict(edges=FAKE + 4), '8-byte aligned'),
])
def test_hist_multi_refuses_before_launching(rows, kwargs, message):
    with pytest.raises(GenesisHipError, match=message):
        _call(rows, **kwargs)


def test_aligned_slices_pass_the_address_check():
    """A 4-byte-aligned fp32 slice and an 8-byte-aligned fp64 slice are legal segments: the call gets past them to the next check."""
    with pytest.raises(GenesisHipError, match='workspace'):
        _call([_segment(SRC=FAKE + 4), _segment(SRC=FAKE + 8, DTYPE=1, WORK=1)], ws_bytes=0)
    assert _lib.query('gx_hist_multi_ws_bytes', 3) == 192 and _lib.query('gx_hist_multi_ws_bytes', 0) == 0


# ---- the Python layer: refused before the library is called ----------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def fail(*args, **kwargs):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'call', fail)
    monkeypatch.setattr(_lib, 'query', fail)


class _NoWriter(object):
    def add_histogram_raw(self, *args, **kwargs):
        raise AssertionError('the writer was called')


@pytest.mark.parametrize('values, message', [
    (torch.zeros(4, 4), 'no CPU path'),                                  # a host tensor
    (torch.zeros(4, dtype=torch.int64), 'expected float32 or float64, got torch.int64'),
    (torch.zeros(4, dtype=torch.float16), 'expected float32 or float64, got torch.float16'),
    (torch.zeros(4, 6)[:, ::2], 'not contiguous'),
    (torch.zeros(0, 3), "histogram 'the_tag': the tensor \\(0, 3\\) has no element"),
    ([1.0, 2.0], 'expected a tensor'),
])
def test_tensors_refused_before_the_library_is_called(no_library, values, message):
    with pytest.raises(GenesisHipError, match=message):
        hist.add_histogram(_NoWriter(), 'the_tag', values, 3)
    h = hist.Histograms()
    with pytest.raises(GenesisHipError, match="histogram 'the_tag'"):
        h.add('the_tag', values)
    assert h.items == [] and h.compute() == []


@pytest.mark.parametrize('kwargs, message', [
    (dict(max_bins=512), 'max_bins=512'),
    (dict(bins=10), 'bins=10: a bin count'),
    (dict(bins=np.int64(10)), 'bins=10: a bin count'),
    (dict(bins='auto'), "bins='auto'"),
    (dict(bins='fd'), "bins='fd'"),
    (dict(bins=[0.0, 1.0, 1.0]), 'bins: the edges must be finite and strictly increasing'),
    (dict(bins=[0.0, 2.0, 1.0]), 'bins: the edges must be finite and strictly increasing'),
    (dict(bins=[0.0, float('inf')]), 'bins: the edges must be finite and strictly increasing'),
    (dict(bins=[0.0, float('nan'), 1.0]), 'bins: the edges must be finite and strictly increasing'),
    (dict(bins=np.linspace(0.0, 1.0, 4097)), r'bins: expected a 1-D sequence of 2 to 4096 edges, got shape \(4097,\)'),
    (dict(bins=[0.5]), r'bins: expected a 1-D sequence of 2 to 4096 edges, got shape \(1,\)'),
    (dict(bins=np.zeros((2, 2))), 'bins: expected a 1-D sequence'),
])
def test_bins_refused_before_the_library_is_called(no_library, kwargs, message):
    with pytest.raises(GenesisHipError, match=message):
        hist.add_histogram(_NoWriter(), 'tag', torch.zeros(4), 0, **kwargs)
    with pytest.raises(GenesisHipError, match=message):
        hist.Histograms(**kwargs)


def test_accepted_bins():
    assert hist.Histograms().edges is hist.default_bins()
    assert hist.Histograms(np.linspace(-1.0, 1.0, 4096)).edges.shape == (4096,)
    assert hist.Histograms([0, 1]).edges.tolist() == [0.0, 1.0]
    assert hist.Histograms((-1.5, 0, 2)).edges.dtype == np.float64


def test_drop_ins_with_nothing_to_log_call_nothing(no_library):
    hist.log_distributions(_NoWriter(), None, None, 5)
    hist.log_distributions(_NoWriter(), {'colour': torch.zeros(3)}, {'z_k': [torch.zeros(3)]}, 5)
    hist.log_grads_and_weights(torch.nn.Sequential(), _NoWriter(), 5)


# ---- trimming -----------------------------------------------------------------------------------------------------------------------
EDGES = np.array([-2.0, -1.0, 0.0, 0.5, 1.0, 4.0, 9.0])      # six bins


@pytest.mark.parametrize('counts, limits, kept', [
    ([3, 0, 1, 0, 0, 0], [-2.0, -1.0, 0.0, 0.5], [0, 3, 0, 1]),              # the first bin non-empty: a zero goes in front
    ([0, 0, 5, 0, 7, 0], [0.0, 0.5, 1.0, 4.0], [0, 5, 0, 7]),                # an interior run: the empty bin before it is kept
    ([0, 0, 0, 2, 0, 0], [0.5, 1.0], [0, 2]),                                # a single bin
    ([0, 0, 0, 0, 0, 4], [4.0, 9.0], [0, 4]),                                # the last bin alone
    ([1, 2, 3, 4, 5, 6], EDGES.tolist(), [0, 1, 2, 3, 4, 5, 6]),              # every bin
    ([0, 0, 0, 0, 0, 0], [], []),                                            # all bins empty
])
def test_trimming_by_hand_and_against_the_restatement(counts, limits, kept):
    got = hist.trim(np.array(counts, np.uint32), EDGES)
    assert got == (limits, kept)
    assert got == R.trim(counts, EDGES)
    assert all(type(c) is int for c in got[1]) and all(type(e) is float for e in got[0])


def test_restatement_on_a_case_by_hand():
    """numpy's rule for explicit edges: left-closed bins, the last one closed on both ends, NaN and outside values in no bin."""
    v = np.array([-2.0, -1.0, -0.0, 0.49, 9.0, 9.5, -3.0, np.nan, 4.0], np.float32)
    r = R.make_histogram(v, EDGES)
    assert r['counts'].tolist() == [1, 1, 2, 0, 0, 2]
    assert (r['nan'], r['below'], r['above'], r['num']) == (1, 1, 1, 9)
    assert r['bucket_limits'] == EDGES.tolist() and r['bucket_counts'] == [0, 1, 1, 2, 0, 0, 2]
    assert all(x != x for x in (r['min'], r['max'], r['sum'], r['sum_squares']))
    r = R.make_histogram(v[[0, 1, 2, 3, 4, 5, 6, 8]], EDGES)
    assert (r['min'], r['max'], r['sum']) == (-3.0, 9.5, float(np.float32(0.49)) + 16.5)
    r = R.make_histogram(np.array([np.inf, -np.inf, 1.0]), EDGES)
    assert (r['min'], r['max'], r['below'], r['above']) == (-np.inf, np.inf, 1, 1) and r['sum'] != r['sum'] and r['sum_squares'] == np.inf
