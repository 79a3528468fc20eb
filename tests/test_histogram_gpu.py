"""genesis_amd.histogram on the device against the numpy restatement of tensorboardX's make_histogram (tests/hist_restatement.py).
Bucket limits and counts, min, max, num and the three tallies (NaN, below the first edge, above the last) must be EXACT.  The two
sums are held to |got - fsum| <= N 2^-52 sum|term|, the worst case of adding N fp64 terms in any order with a product that may be
fused into its addition -- a bound from the number format, not from a measurement."""
import numpy as np
import pytest
import torch

from genesis_amd import histogram as hist
from tests import hist_restatement as R
from tests.common import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = hist.CHUNK
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3)
SPECIALS = np.array([0.0, -0.0, 1e-13, -1e-13, np.float32(1e-45), np.float32(1e-12), 3e20, -3e20, np.inf, -np.inf], np.float32)
assert SPECIALS[4] > 0 and SPECIALS[4] == np.nextafter(np.float32(0), np.float32(1))      # the smallest denormal


def values(kind, n, seed):
    """kind: 'wide' sign x 10^U(-14, 21) (both out-of-range tallies and the [0, 1e-12) bin are hit), 'normal' N(0, 0.02),
    'specials' wide values with the special ones among them, 'nan' normal values with one NaN."""
    rng = np.random.RandomState(seed)
    if kind in ('wide', 'specials'):
        v = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-14, 21, n)).astype(np.float32)
        if kind == 'specials':
            k = min(n, len(SPECIALS))
            v[rng.permutation(n)[:k]] = SPECIALS[:k]
        return v
    v = (0.02 * rng.randn(n)).astype(np.float32)
    if kind == 'nan':
        v[rng.randint(n)] = np.nan
    return v


def place(v, offset, dtype):
    """The host values as a device slice that starts `offset` elements into a larger buffer (offset 0: a 16-byte-aligned base)."""
    buf = torch.zeros(offset + v.size + 5, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + v.size]
    t.copy_(torch.from_numpy(v).to(dtype))
    return t


def histograms(tensors, bins='tensorflow'):
    h = hist.Histograms(bins)
    for i, t in enumerate(tensors):
        h.add('t%d' % i, t)
    return h.compute()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('offset', [0, 1, 3])
@pytest.mark.parametrize('kind', ['wide', 'normal', 'specials', 'nan'])
def test_lengths_and_alignment(kind, offset, dtype):
    """One segment per length -- around the wave, the workgroup and the chunk -- in one call; from an aligned base and from slices
    whose first element is 4 and 12 (fp64: 8 and 24) bytes behind one."""
    host = [values(kind, n, 1000 * offset + n) for n in LENGTHS]
    tensors = [place(v, offset, dtype) for v in host]
    assert all(t.data_ptr() % 16 == (offset * t.element_size()) % 16 for t in tensors)
    records = histograms(tensors)
    assert [r.tag for r in records] == ['t%d' % i for i in range(len(LENGTHS))]
    for n, v, r in zip(LENGTHS, host, records):
        want = R.assert_matches(r, v, what='%s n=%d offset=%d' % (kind, n, offset))
        if kind == 'nan':
            assert r.nan == 1 and all(x != x for x in (r.min, r.max, r.sum, r.sum_squares))
            clean = v[~np.isnan(v)]
            if clean.size:      # counts as without the NaN; num counts it
                assert r.bucket_counts == R.make_histogram(clean)['bucket_counts'] and r.num == clean.size + 1
            else:
                assert r.bucket_counts == [] and r.bucket_limits == [] and r.num == 1
        if kind in ('wide', 'specials') and n >= C - 1:      # (about 1 value in 70 lands in each of the three)
            assert want['below'] > 0 and want['above'] > 0 and want['counts'][774] > 0      # the cases the values were made for


def test_specials_one_by_one():
    """Each special value as a segment of its own: where it lands is stated here, not only compared."""
    e = hist.default_bins()
    records = histograms([place(SPECIALS[i:i + 1], 1, torch.float32) for i in range(len(SPECIALS))])
    for v, r in zip(SPECIALS, records):
        R.assert_matches(r, np.array([v]), what=repr(v))
    zero, neg_zero, tiny, neg_tiny, denormal, first, big, neg_big, inf, neg_inf = records
    for r in (zero, neg_zero, tiny, denormal):                      # [0, 1e-12)
        assert r.bucket_limits == [0.0, 1e-12] and r.bucket_counts == [0, 1]
    assert neg_tiny.bucket_limits == [-1e-12, 0.0] and neg_tiny.bucket_counts == [0, 1]
    # float32(1e-12) lies just below the double 1e-12: the widened value decides, not the decimal one
    assert float(np.float32(1e-12)) < 1e-12 and first.bucket_limits == [0.0, 1e-12]
    for r, tally in ((big, (0, 0, 1)), (inf, (0, 0, 1)), (neg_big, (0, 1, 0)), (neg_inf, (0, 1, 0))):
        assert (r.nan, r.below, r.above) == tally and r.bucket_limits == [] and r.bucket_counts == []
    assert inf.max == np.inf and inf.sum == np.inf and neg_inf.min == -np.inf and e[-1] < 3e20


@pytest.mark.parametrize('shift', [0, 1, -1], ids=['edges', 'next_above', 'next_below'])
def test_boundary_rule_on_the_table_itself(shift):
    """An fp64 segment of the 1549 edges: bin i gets exactly one, the last bin two.  Their fp64 neighbours above: one per bin and
    the last one outside; below: the first one outside, then one per bin."""
    e = hist.default_bins()
    v = e.copy() if shift == 0 else np.nextafter(e, np.inf * shift)
    r, = histograms([place(v, 1, torch.float64)])
    R.assert_matches(r, v)
    nb = e.size - 1
    if shift == 0:
        assert r.bucket_counts == [0] + [1] * (nb - 1) + [2] and (r.below, r.above) == (0, 0)
    elif shift == 1:
        assert r.bucket_counts == [0] + [1] * nb and (r.below, r.above) == (0, 1)
    else:
        assert r.bucket_counts == [0] + [1] * nb and (r.below, r.above) == (1, 0)
    assert r.bucket_limits == e.tolist() and r.nan == 0


@pytest.mark.parametrize('value', [0.0, 0.3, -7.25e-5])
def test_contention_all_equal(value):
    """Every lane of every wave on one bin: a zero gradient, a constant bias."""
    n = 100000
    v32 = np.float32(value)
    t = torch.full((n,), float(v32), dtype=torch.float32, device=DEV)
    r, = histograms([t])
    R.assert_matches(r, np.full(n, v32))
    assert r.bucket_counts == [0, n] and r.num == n and r.min == r.max == float(v32)
    assert r.sum == n * float(v32)      # exact: a 24-bit value times a count below 2^17 fits fp64's 53 bits at every partial sum


def test_many_segments_and_identical_bits():
    """300 segments of 1 .. 300 elements, fp32 and fp64 in turn, cut back to back out of two flat buffers as parameters are: each
    record against its own segment; then the same call again (and a segment of several chunks, twice): the same bits."""
    S = 300
    flat = {torch.float32: torch.zeros(S * (S + 1) // 2 + 8, dtype=torch.float32, device=DEV),
            torch.float64: torch.zeros(S * (S + 1) // 2 + 8, dtype=torch.float64, device=DEV)}
    used = {torch.float32: 1, torch.float64: 1}
    host, tensors = [], []
    for i in range(S):
        n, dtype = i + 1, (torch.float32, torch.float64)[i % 2]
        v = values(('normal', 'wide')[(i // 2) % 2], n, 7000 + i)
        t = flat[dtype][used[dtype]:used[dtype] + n]
        t.copy_(torch.from_numpy(v).to(dtype))
        used[dtype] += n
        host.append(v)
        tensors.append(t)
    records = histograms(tensors)
    assert len(records) == S
    for i, (v, r) in enumerate(zip(host, records)):
        assert r.tag == 't%d' % i
        R.assert_matches(r, v, what='segment %d' % i)
    big = torch.from_numpy(values('wide', 5 * C + 17, 5)).to(DEV)
    R.assert_matches(histograms([big])[0], big.cpu().numpy(), what='six chunks')
    records, again = records + histograms([big]), histograms(tensors) + histograms([big])

    def bits(recs):
        return np.array([[r.min, r.max, r.sum, r.sum_squares] for r in recs], np.float64).view(np.int64)
    assert np.array_equal(bits(records), bits(again))
    assert [(r.bucket_limits, r.bucket_counts, r.nan, r.below, r.above) for r in records] == \
        [(r.bucket_limits, r.bucket_counts, r.nan, r.below, r.above) for r in again]


def test_two_edges_give_one_bin_closed_on_both_ends():
    v = np.array([-0.5, 0.5, 0.0, -0.0, 0.25, np.nextafter(-0.5, -1), np.nextafter(0.5, 1), 3.0, -np.inf, np.nan], np.float64)
    r, = histograms([place(v, 1, torch.float64)], bins=[-0.5, 0.5])
    assert r.bucket_limits == [-0.5, 0.5] and r.bucket_counts == [0, 5]
    assert (r.nan, r.below, r.above, r.num) == (1, 2, 2, 10)
    R.assert_matches(r, v, [-0.5, 0.5])
    f = np.float32
    v32 = np.array([-0.5, 0.5, 0.0, -0.0, 0.25, np.nextafter(f(-0.5), f(-1)), np.nextafter(f(0.5), f(1)), 3.0, -np.inf], f)
    r, = histograms([place(v32, 3, torch.float32)], bins=(-0.5, 0.5))
    R.assert_matches(r, v32, [-0.5, 0.5])
    assert r.bucket_counts == [0, 5] and r.min == -np.inf and r.max == 3.0


def test_4096_uniform_edges():
    e = np.linspace(-1.0, 1.0, 4096)
    rng = np.random.RandomState(11)
    v = (0.5 * rng.randn(20000)).astype(np.float32)
    v[:4] = (-1.0, 1.0, 0.0, np.float32(e[2047]))
    v64 = np.concatenate([e, rng.uniform(-1.1, 1.1, 3000)])      # the edges themselves, and values around them
    r32, r64 = histograms([place(v, 3, torch.float32), place(v64, 1, torch.float64)], bins=e)
    want = R.assert_matches(r32, v, e)
    assert want['below'] > 0 and want['above'] > 0 and want['counts'][-1] > 0
    want = R.assert_matches(r64, v64, e)
    assert want['counts'].min() >= 1 and want['counts'][-1] >= 2


# ---- the drop-ins on the smallest GENESIS-V2 model of the parity tests ----------------------------------------------------------------
@pytest.fixture(scope='module')
def trained():
    """The 'tiny' fixture's model after one forward / backward through the plain loss.backward() path."""
    import genesis_amd.genesisv2_config as G
    from genesis_amd.compat.attrdict import AttrDict
    gold = Golden('tiny')
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(dict(dynamic_K=False), **dict(gold.cfg, debug=False, multi_gpu=False))))
    model.load_state_dict(gold.weights(model.state_dict()))
    model = model.to(DEV).train()
    x, rand_pixel, eps_k = gold.inputs()
    recon, losses, stats, att_stats, comp_stats = model(x.to(DEV), rand_pixel.to(DEV), torch.stack(eps_k).to(DEV))
    (losses.err.mean(0) + torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()).backward()
    torch.cuda.synchronize()
    return model, att_stats, comp_stats


def reference_tags(model):
    tags = []
    for name, param in model.named_parameters():      # train.py:341-345
        tags.append('weights/%s' % name)
        if param.grad is not None:
            tags.append('grads/%s' % name)
    return tags


def test_log_grads_and_weights(trained):
    model = trained[0]
    params = dict(model.named_parameters())
    assert params['att_process.log_sigma'].dtype == torch.float64 and params['att_process.log_sigma'].grad is not None
    assert sum(p.grad is not None for p in params.values()) > len(params) // 2
    w = R.RecordingWriter()
    hist.log_grads_and_weights(model, w, 17)
    assert [c['tag'] for c in w.calls] == reference_tags(model)
    assert 'weights/att_process.log_sigma' in [c['tag'] for c in w.calls] and 'grads/att_process.log_sigma' in [c['tag'] for c in w.calls]
    for c in w.calls:
        kind, name = c['tag'].split('/', 1)
        source = params[name].detach() if kind == 'weights' else params[name].grad
        R.assert_matches(c, source.cpu().numpy(), what=c['tag'])
        assert c['global_step'] == 17 and type(c['num']) is int and type(c['min']) is float
    # a parameter without a gradient: its 'grads/' call is absent and nothing else moves
    name = 'att_process.log_sigma'
    kept, params[name].grad = params[name].grad, None
    try:
        w2 = R.RecordingWriter()
        hist.log_grads_and_weights(model, w2, 17)
    finally:
        params[name].grad = kept
    assert [c for c in w.calls if c['tag'] != 'grads/' + name] == w2.calls


def test_add_histogram_is_one_call_of_the_pass(trained):
    model = trained[0]
    name, param = next(iter(model.named_parameters()))
    w, w1 = R.RecordingWriter(), R.RecordingWriter()
    hist.log_grads_and_weights(model, w, 3)
    hist.add_histogram(w1, 'weights/' + name, param.data, 3)
    assert w1.calls == w.calls[:1]
    e = np.linspace(-0.5, 0.5, 11)
    hist.add_histogram(w1, 'custom', param.data, bins=e)
    assert w1.calls[1]['global_step'] is None
    R.assert_matches(w1.calls[1], param.detach().cpu().numpy(), e)


def test_log_distributions(trained):
    _, att_stats, comp_stats = trained
    K = len(comp_stats['mu_k'])
    assert att_stats is not None and K > 1 and 'pmu_k' not in comp_stats
    w = R.RecordingWriter()
    hist.log_distributions(w, att_stats, comp_stats, 9)
    # GENESIS-V2's attention statistics carry none of the four keys: only the component posteriors are logged
    assert [c['tag'] for c in w.calls] == ['comp_%s_%d' % (key, k) for key in ('mu_k', 'sigma_k') for k in range(K)]
    for c in w.calls:
        _, key, _, k = c['tag'].split('_')
        R.assert_matches(c, comp_stats[key + '_k'][int(k)].detach().cpu().numpy(), what=c['tag'])
        assert c['global_step'] == 9
    none = R.RecordingWriter()
    hist.log_distributions(none, att_stats, None, 9)
    assert none.calls == []
    # dicts with all four keys on the attention side and a missing one on the component side, in the reference's order
    att = {key: comp_stats['sigma_k' if 'sigma' in key else 'mu_k'][:2] for key in ('psigma_k', 'pmu_k', 'sigma_k', 'mu_k')}
    comp = {'psigma_k': comp_stats['sigma_k'][:1], 'z_k': comp_stats['mu_k']}
    both = R.RecordingWriter()
    hist.log_distributions(both, att, comp, 9)
    assert [c['tag'] for c in both.calls] == ['att_mu_k_0', 'att_mu_k_1', 'att_sigma_k_0', 'att_sigma_k_1', 'att_pmu_k_0', 'att_pmu_k_1',
                                              'att_psigma_k_0', 'att_psigma_k_1', 'comp_psigma_k_0']
    assert both.calls[0] == dict(w.calls[0], tag='att_mu_k_0') and both.calls[-1] == dict(w.calls[K], tag='comp_psigma_k_0')
