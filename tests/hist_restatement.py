"""numpy restatement of what tensorboardX's add_histogram computes for one tensor, written from its published rules (tensorboardX is
not installed where this project is tested): the 'tensorflow' edge table, numpy.histogram of the values widened to float64 over
explicit edges, the trimming to the support with one empty bucket in front, min / max / num, and the two sums -- here by
math.fsum, so that an implementation's summation order can be held to a bound instead of to numpy's own order.  numpy only."""
import math

import numpy as np


def default_bins():
    """v = 1e-12; while v < 1e20: v *= 1.1 -- the positive edges; the table is their negatives reversed, 0, and the edges."""
    positive = []
    v = 1e-12
    while v < 1e20:
        positive.append(v)
        v *= 1.1
    return np.array([-p for p in positive[::-1]] + [0.0] + positive, dtype=np.float64)


def trim(counts, edges):
    """(bucket limits, bucket counts) as lists: from the first non-empty bin `first` to the last one `last`, the limits
    edges[first : last + 2] and the counts of the bins first - 1 .. last (a zero in front when first == 0); two empty lists when no
    bin holds anything."""
    counts = [int(c) for c in counts]
    filled = [i for i, c in enumerate(counts) if c > 0]
    if not filled:
        return [], []
    first, last = filled[0], filled[-1]
    limits = [float(e) for e in edges[first:last + 2]]
    if first > 0:
        return limits, counts[first - 1:last + 1]
    return limits, [0] + counts[:last + 1]


def _sum(terms):
    """The exactly rounded sum of finite terms; IEEE's answer (an infinity, or NaN for inf - inf or a NaN term) otherwise."""
    if np.all(np.isfinite(terms)):
        return math.fsum(terms.tolist())
    with np.errstate(invalid='ignore'):
        return float(np.sum(terms))


def make_histogram(values, edges=None):
    """values: any array of float32 or float64.  -> dict of min, max, num, sum, sum_squares, bucket_limits, bucket_counts (what
    goes into the HistogramProto), counts (all bins), nan / below / above (the values numpy.histogram puts in no bin), and
    sum_bound / sum_squares_bound = N 2^-52 sum|term|: the worst case of adding the N terms in fp64 in any order (each of the
    N - 1 additions rounds a partial sum no larger than sum|term| by 2^-53 relative, to first order; 2^-52 leaves room for a
    product v v that is rounded before it is added, or not)."""
    edges = default_bins() if edges is None else np.asarray(edges, dtype=np.float64)
    v = np.asarray(values).reshape(-1).astype(np.float64)
    assert v.size > 0
    counts, _ = np.histogram(v, bins=edges)
    limits, kept = trim(counts, edges)
    with np.errstate(invalid='ignore', over='ignore'):
        squares = v * v
        res = dict(min=float(v.min()), max=float(v.max()), num=int(v.size), sum=_sum(v), sum_squares=_sum(squares),
                   bucket_limits=limits, bucket_counts=kept, counts=counts,
                   nan=int(np.isnan(v).sum()), below=int((v < edges[0]).sum()), above=int((v > edges[-1]).sum()))
        res['sum_bound'] = v.size * 2.0 ** -52 * _sum(np.abs(v))
        res['sum_squares_bound'] = v.size * 2.0 ** -52 * _sum(squares)
    return res


class RecordingWriter(object):
    """Keeps what add_histogram_raw is called with, in order."""

    def __init__(self):
        self.calls = []

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None):
        self.calls.append(dict(tag=tag, min=min, max=max, num=num, sum=sum, sum_squares=sum_squares,
                               bucket_limits=bucket_limits, bucket_counts=bucket_counts, global_step=global_step))


def same_number(a, b):
    """a == b, with NaN equal to NaN."""
    return (a != a and b != b) or a == b


def assert_matches(got, values, edges=None, what=''):
    """A record (a Histogram of genesis_amd.histogram or a RecordingWriter call) against the restatement of `values`: limits,
    counts, num, min and max exactly; the sums within their bounds, or the same infinity / NaN."""
    get = got.get if isinstance(got, dict) else lambda k: getattr(got, k)
    want = make_histogram(values, edges)
    assert get('bucket_limits') == want['bucket_limits'], what
    assert get('bucket_counts') == want['bucket_counts'], what
    assert get('num') == want['num'], what
    for key in ('min', 'max'):
        assert same_number(get(key), want[key]), (what, key, get(key), want[key])
    for key in ('sum', 'sum_squares'):
        g, w = get(key), want[key]
        if math.isfinite(w):
            assert abs(g - w) <= want[key + '_bound'], (what, key, g, w, want[key + '_bound'])
        else:
            assert same_number(g, w), (what, key, g, w)
    if not isinstance(got, dict):
        assert (got.nan, got.below, got.above) == (want['nan'], want['below'], want['above']), what
        assert sum(got.bucket_counts) + got.nan + got.below + got.above == got.num, what
    return want
