"""The device cache of decoded splits on the GPU (genesis_amd/data_cache.py, csrc/gx_cache.hip): the four kernels against the
numpy restatement (tests/data_cache_restatement.py) with bytes and counts exact, the round trip of both byte -> float rules bit
for bit, CachedLoader over small fake loaders of fixed device tensors, and one end-to-end run through image_folder_config.
Everything at zero tolerance: the kernels round a product to a byte, divide or multiply one byte, or copy a label."""
import os
import sys

import numpy as np
import pytest
import torch

from genesis_amd import data_cache
from genesis_amd.compat.attrdict import AttrDict
from genesis_amd.data_cache import CachedLoader
from tests import data_cache_restatement as R

pytestmark = pytest.mark.gpu

SHAPES = [(3, 8, 8), (3, 5, 7), (1, 1, 1), (3, 64, 64)]      # a row of 192 bytes; of 105 (tail, padded stride); of 1; 3 blocks a row
BATCHES = [1, 5, 32]
SENTINEL = 0xA7
F32 = np.float32


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    """A data config registers its flags when it is first imported, and the first definition of a name keeps its default:
    the configs imported here must not decide the defaults that other modules' tests see later, so the flag table is put
    back and a config this module was the first to import is forgotten again (its next import registers its flags anew)."""
    from genesis_amd import compat
    compat.install()
    from forge import flags
    saved = dict(flags.FLAGS)
    configs = ['genesis_amd.' + name for name in ('image_folder_config',)]
    fresh = [m for m in configs if m not in sys.modules]
    yield
    flags.FLAGS.clear()
    flags.FLAGS.update(saved)
    for m in fresh:
        sys.modules.pop(m, None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same_bits(got, want):
    """A device tensor against a numpy array: dtype, shape and every bit (floats compared as int32)."""
    got = host(got)
    want = np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.float32:
        got, want = got.view(np.int32), np.ascontiguousarray(want).view(np.int32)
    return np.array_equal(got, want)


def sentinel_store(rows, row_bytes):
    store = data_cache.new_store(rows, row_bytes, 'cuda')
    store.fill_(SENTINEL)
    return store, R.new_store(rows, row_bytes, fill=SENTINEL)


def make_frames(rng, B, shape, mode=0):
    return R.unit(rng.randint(0, 256, size=(B,) + tuple(shape)), mode)


def make_labels(rng, B, H, W):
    labels = rng.randint(-1, 300, size=(B, 1, H, W)).astype(np.int64)
    special = np.array([-1, 0, 255, 32767, -32768], dtype=np.int64)
    flat = labels.reshape(-1)
    flat[:min(len(special), flat.size)] = special[:flat.size]
    return labels


# ---- the kernels against the restatement ----
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_store_and_gather_equal_the_restatement(shape, B):
    C, H, W = shape
    rng = np.random.RandomState(1000 * B + C * H * W)
    rows, first_row = B + 5, 3                                   # a store at first_row > 0, rows on both sides left alone
    frames = make_frames(rng, B, shape, mode=rng.randint(2))
    frames.reshape(-1)[rng.randint(frames.size)] = F32(0.3)      # one value that is no byte either way
    labels = make_labels(rng, B, H, W)
    store, want_store = sentinel_store(rows, C * H * W)
    lstore, want_lstore = sentinel_store(rows, 2 * H * W)
    assert store.shape[1] == R.row_stride(C * H * W) and store.shape[1] % 16 == 0 and store.data_ptr() % 16 == 0
    counters = data_cache.new_counters('cuda')
    data_cache.store_frames(dev(frames), store, first_row, counters)
    data_cache.store_labels(dev(labels), lstore, first_row, counters)
    div_miss, mul_miss = R.store_frames(want_store, first_row, frames)
    misfit = R.store_labels(want_lstore, first_row, labels)
    assert host(counters).tolist() == [div_miss, mul_miss, misfit] and div_miss >= 1 and mul_miss >= 1 and misfit == 0
    # every byte of the store: the rows written, and the pad bytes and neighbouring rows still the sentinel
    assert same_bits(store, want_store) and same_bits(lstore, want_lstore)
    if C * H * W % 16:
        assert (want_store[first_row:first_row + B, C * H * W:] == SENTINEL).all()
    # gathers: a permuted index vector (with a repeat) over the written rows, and no index vector
    perm = first_row + rng.permutation(B)
    perm = np.concatenate([perm, perm[:1]]).astype(np.int64)
    idx = dev(perm)
    for mode in (0, 1):
        assert same_bits(data_cache.gather_frames(store, shape, idx, 0, len(perm), mode), R.gather_frames(want_store, shape, perm, mode))
        assert same_bits(data_cache.gather_frames(store, shape, idx, 1, B, mode), R.gather_frames(want_store, shape, perm[1:], mode))
        assert same_bits(data_cache.gather_frames(store, shape, None, first_row, B, mode),
                         R.gather_frames(want_store, shape, range(first_row, first_row + B), mode))
    assert same_bits(data_cache.gather_labels(lstore, (H, W), idx, 0, len(perm)), R.gather_labels(want_lstore, (H, W), perm))
    assert same_bits(data_cache.gather_labels(lstore, (H, W), None, first_row, B), labels)
    # the counters accumulate over launches
    data_cache.store_frames(dev(frames), store, 0, counters)
    assert host(counters).tolist() == [2 * div_miss, 2 * mul_miss, misfit]


def test_what_does_not_fit_is_counted_not_stored_silently():
    shape = (3, 5, 7)
    rng = np.random.RandomState(5)
    frames = make_frames(rng, 2, shape)
    frames[0, 1, 2, 3] = np.nan
    frames[1, 2, 4, 6] = F32(1.5)                                 # in the row's scalar tail
    frames[1, 0, 0, 0] = F32(-0.0)
    labels = make_labels(rng, 2, 5, 7)
    labels[1, 0, 4, 6] = 40000
    labels[0, 0, 2, 2] = -40000
    store, want_store = sentinel_store(2, 105)
    lstore, want_lstore = sentinel_store(2, 70)
    counters = data_cache.new_counters('cuda')
    data_cache.store_frames(dev(frames), store, 0, counters)
    data_cache.store_labels(dev(labels), lstore, 0, counters)
    div_miss, mul_miss = R.store_frames(want_store, 0, frames)
    clean = np.where(np.isfinite(frames) & (frames <= 1) & (R.bits(frames) != R.bits(F32(-0.0))), frames, F32(0.0))
    assert div_miss == 3 and mul_miss == 3 + R.quantise(clean)[2]        # NaN, 1.5 and -0.0 in both counters
    assert R.store_labels(want_lstore, 0, labels) == 2                   # both labels counted
    assert host(counters).tolist() == [div_miss, mul_miss, 2]
    assert same_bits(store, want_store) and same_bits(lstore, want_lstore)
    assert host(store)[0, 1 * 35 + 2 * 7 + 3] == 0 and host(store)[1, 2 * 35 + 4 * 7 + 6] == 255
    # the labels that fit come back, negative ones included
    back = host(data_cache.gather_labels(lstore, (5, 7)))
    fits = (labels >= -32768) & (labels <= 32767)
    assert np.array_equal(back[fits], labels[fits]) and (labels[fits] < 0).any() and 32767 in back


@pytest.mark.parametrize('mode', (0, 1))
def test_round_trip_of_all_256_bytes(mode):
    occurrences = 3
    values = np.tile(np.arange(256), occurrences).reshape(2, 3, 16, 8)
    frames = R.unit(values, mode)
    store = data_cache.new_store(2, 384, 'cuda')
    counters = data_cache.new_counters('cuda')
    data_cache.store_frames(dev(frames), store, 0, counters)
    assert host(counters).tolist() == ([0, 126 * occurrences, 0] if mode == 0 else [126 * occurrences, 0, 0])
    assert np.array_equal(host(store).reshape(-1), values.reshape(-1))
    assert same_bits(data_cache.gather_frames(store, (3, 16, 8), mode=mode), frames)      # compared as int32 views
    assert not same_bits(data_cache.gather_frames(store, (3, 16, 8), mode=1 - mode), frames)


def test_python_entry_points_refuse_before_any_launch():
    from genesis_amd._lib import GenesisHipError
    store = data_cache.new_store(4, 192, 'cuda')
    counters = data_cache.new_counters('cuda')
    x = torch.zeros(2, 3, 8, 8, device='cuda')
    with pytest.raises(GenesisHipError, match='no CPU path'):
        data_cache.store_frames(x.cpu(), store, 0, counters)
    with pytest.raises(GenesisHipError, match='contiguous'):
        data_cache.store_frames(x.double(), store, 0, counters)
    with pytest.raises(GenesisHipError, match='new_store'):
        data_cache.store_frames(x, data_cache.new_store(4, 100, 'cuda'), 0, counters)
    with pytest.raises(GenesisHipError, match='capacity'):
        data_cache.store_frames(x, store, 3, counters)
    with pytest.raises(GenesisHipError, match='reach outside'):
        data_cache.gather_frames(store, (3, 8, 8), None, 3, 2)
    with pytest.raises(GenesisHipError, match='int64 vector'):
        data_cache.gather_frames(store, (3, 8, 8), torch.zeros(2, dtype=torch.int32, device='cuda'), 0, 2)
    with pytest.raises(GenesisHipError, match='bad mode'):
        data_cache.gather_frames(store, (3, 8, 8), None, 0, 2, mode=2)


# ---- the wrapper over fake loaders ----
class FakeLoader(object):
    """Yields fixed device tensors: the same objects every epoch."""

    def __init__(self, batches, batch_size, shuffle=None):
        self.batches = batches
        self.batch_size = batch_size
        self.epochs = self.closed = 0
        if shuffle is not None:
            self.shuffle = shuffle

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        self.epochs += 1
        return iter(self.batches)

    def close(self):
        self.closed += 1


SHAPE = (3, 5, 7)


def fake_batches(sizes=(5, 5, 2), labels=True, seed=0, mode=0):
    rng = np.random.RandomState(seed)
    out = []
    for B in sizes:
        b = {'input': dev(make_frames(rng, B, SHAPE, mode))}
        if labels:
            b['instances'] = dev(make_labels(rng, B, SHAPE[1], SHAPE[2]))
        out.append(b)
    return out


def recorded(batches):
    return {k: np.concatenate([host(b[k]) for b in batches]) for k in batches[0]}


def epoch(loader):
    return list(loader)


@pytest.mark.parametrize('mode', (0, 1))
def test_resident_epochs_equal_the_first_bit_for_bit(mode, capsys):
    batches = fake_batches(mode=mode)
    fake = FakeLoader(batches, 5)
    w = CachedLoader(fake, shuffle=False, name='fake')
    assert w.cache_state == 'filling' and len(w) == 3 and w.batch_size == 5 and w.loader is fake
    first = epoch(w)
    assert len(first) == 3 and all(got[k] is b[k] for got, b in zip(first, batches) for k in b)    # the loader's own tensors
    assert w.cache_state == 'resident' and w.mode == mode and fake.closed == 1 and len(w) == 3
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('data_cache: fake')]
    assert len(line) == 1 and '12 rows resident' in line[0] and data_cache.MODES[mode] in line[0] and ' MB' in line[0] and ' s' in line[0]
    for _ in range(2):
        again = epoch(w)
        assert w.order.tolist() == list(range(12)) and len(again) == 3
        for got, b in zip(again, batches):
            assert sorted(got) == sorted(b) and all(got[k] is not b[k] for k in b)
            assert all(same_bits(got[k], host(b[k])) for k in b)
    assert fake.epochs == 1 and fake.closed == 1 and w.cache_state == 'resident'
    w.close()
    assert fake.closed == 1


def test_shuffled_epochs_follow_order_and_the_seed():
    batches = fake_batches()
    rec = recorded(batches)
    orders = []
    for attempt in range(2):
        w = CachedLoader(FakeLoader(batches, 5), shuffle=True, seed=7)
        epoch(w)
        for _ in range(2):
            got = epoch(w)
            order = w.order
            assert sorted(order.tolist()) == list(range(12)) and [len(b['input']) for b in got] == [5, 5, 2]
            for k, b in enumerate(got):
                rows = order[k * 5:(k + 1) * 5]
                assert same_bits(b['input'], rec['input'][rows]) and same_bits(b['instances'], rec['instances'][rows])
            orders.append(order.tolist())
    assert orders[0] != orders[1] and orders[:2] == orders[2:]            # a new order every epoch; the same seed, the same orders
    # shuffle=None follows the wrapped loader's attribute, read when the epoch starts
    w = CachedLoader(FakeLoader(batches, 5, shuffle=False))
    epoch(w), epoch(w)
    assert w.order.tolist() == list(range(12))
    w.loader.shuffle = True
    epoch(w)
    assert w.order.tolist() != list(range(12)) and sorted(w.order.tolist()) == list(range(12))


def test_an_abandoned_epoch_is_discarded():
    batches = fake_batches(labels=False)
    fake = FakeLoader(batches, 5)
    w = CachedLoader(fake, shuffle=False)
    it = iter(w)
    assert next(it)['input'] is batches[0]['input']
    assert w.cache_state == 'filling' and fake.closed == 0
    assert len(epoch(w)) == 3 and w.cache_state == 'resident' and w.rows == 12 and fake.epochs == 2
    got = epoch(w)
    assert [len(b['input']) for b in got] == [5, 5, 2] and all('instances' not in b for b in got)
    assert all(same_bits(g['input'], host(b['input'])) for g, b in zip(got, batches))


def off_after_an_epoch(w, batches, reason, capsys):
    for _ in range(3):
        got = epoch(w)
        assert len(got) == len(batches) and all(g[k] is b[k] for g, b in zip(got, batches) for k in b)       # passed through
    assert w.cache_state.startswith('off: ') and reason in w.cache_state, w.cache_state
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('data_cache:')]
    assert len(lines) == 1 and reason in lines[0]                                                            # printed once
    assert w.loader.epochs == 3 and len(w) == len(batches)


def test_off_over_the_budget(capsys):
    batches = fake_batches()
    w = CachedLoader(FakeLoader(batches, 5), budget_bytes=1024)
    off_after_an_epoch(w, batches, 'over the budget', capsys)
    need = 15 * (R.row_stride(105) + R.row_stride(70))
    assert '%d bytes' % need in w.cache_state and '1024 bytes' in w.cache_state


def test_off_frames_that_are_no_bytes(capsys):
    batches = fake_batches()
    batches[1]['input'][2, 1, 3, 3] = 0.3
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'not bytes / 255', capsys)


def test_off_a_label_that_does_not_fit(capsys):
    batches = fake_batches()
    batches[2]['instances'][1, 0, 4, 6] = 40000
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'do not fit int16', capsys)


def test_off_an_extra_key(capsys):
    batches = fake_batches()
    batches[1]['depth'] = batches[1]['input']
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'keys other than', capsys)


def test_off_a_changing_shape_or_dtype(capsys):
    batches = fake_batches()
    batches[2]['input'] = torch.zeros(2, 3, 5, 8, device='cuda')
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'differs in shape or dtype', capsys)
    batches = fake_batches()
    batches[1]['instances'] = batches[1]['instances'].int()
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'differs in shape or dtype', capsys)
    batches = fake_batches()
    del batches[1]['instances']
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'differs in shape or dtype', capsys)


def test_off_more_rows_than_the_loader_announced(capsys):
    batches = fake_batches(sizes=(5, 6, 5), labels=False)
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'delivered more than', capsys)


def test_off_a_host_tensor(capsys):
    batches = fake_batches()
    batches[0]['input'] = batches[0]['input'].cpu()
    off_after_an_epoch(CachedLoader(FakeLoader(batches, 5)), batches, 'host tensor', capsys)


def test_a_resident_epoch_makes_no_host_read():
    """The batches of a resident epoch under torch's sync debug mode 'error', which turns every synchronising call into an
    exception, as tests/test_image_quality_gpu.py does (a build without that mode captures the batches in a graph instead: a
    capture admits no host read either).  The epoch's one upload of its permutation happens in __iter__, outside."""
    batches = fake_batches()
    w = CachedLoader(FakeLoader(batches, 5), shuffle=True)
    epoch(w), epoch(w)                                                   # resident, and the allocator has seen the sizes
    assert w.cache_state == 'resident'
    it = iter(w)
    torch.cuda.synchronize()
    supported = True
    got = []
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()
            supported = False                                            # the mode did not catch a plain host read
        except RuntimeError:
            pass
        if supported:
            got = [next(it) for _ in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not supported:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = [next(it) for _ in range(3)]
        graph.replay()
    with pytest.raises(StopIteration):
        next(it)
    rec = recorded(batches)
    assert same_bits(torch.cat([b['input'] for b in got]), rec['input'][w.order])


# ---- end to end: a folder of PNGs through image_folder_config ----
def test_image_folder_epoch_two_comes_from_the_cache(tmp_path):
    import genesis_amd.image_folder_config as IF
    from genesis_amd.visualise import save_png
    rng = np.random.RandomState(3)
    for i in range(10):
        save_png(os.path.join(str(tmp_path), 'f%02d.png' % i), rng.randint(0, 256, size=(11 + i % 3, 9 + i % 4, 3)).astype(np.uint8))
    cfg = AttrDict(data_folder=str(tmp_path), img_size=8, num_workers=2, batch_size=3, seed=0, cache_on_device=True)
    train, val, test = IF.load(cfg)
    try:
        assert type(train) is CachedLoader and len(train.loader.files) == 8 and len(train) == 3
        train.loader.shuffle = False                                     # the wrapper follows it: both epochs in file order
        first = [b['input'].clone() for b in train]
        assert train.cache_state == 'resident' and train.mode == 0 and train.rows == 8 and train.loader.pool is None    # closed
        assert [tuple(b.shape) for b in first] == [(3, 3, 8, 8), (3, 3, 8, 8), (2, 3, 8, 8)]
        second = [b['input'] for b in train]
        assert len(second) == 3 and all(same_bits(g, host(f)) for g, f in zip(second, first))
        assert len({host(f).tobytes() for f in first}) == 3              # (three different batches, not one repeated)
    finally:
        for l in (train, val, test):
            l.close()
