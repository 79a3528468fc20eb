"""Augmentation of cached batches on the GPU (genesis_amd/augment.py, gx_cache_gather_aug in csrc/gx_cache.hip): the kernel
against the numpy restatement of "augment v1" (tests/augment_restatement.py) with parameters, frames and labels bit for bit,
the identities the definition gives against the plain gathers, determinism per cache row, CachedLoader's augmented resident
epochs over a small fake loader, and one end-to-end run through image_folder_config.  Everything is at zero tolerance: the
definition fixes every rounding."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from genesis_amd import _lib, augment, data_cache
from genesis_amd._lib import GenesisHipError
from genesis_amd.augment import Augment
from genesis_amd.compat.attrdict import AttrDict
from genesis_amd.data_cache import CachedLoader
from tests import augment_restatement as A
from tests import data_cache_restatement as R

pytestmark = pytest.mark.gpu

# an aligned row; tails, a padded stride and scalar stores; a degenerate window; one channel, wider than high; 4 blocks a plane
SHAPES = [(3, 8, 8), (3, 5, 7), (1, 1, 1), (1, 3, 17), (3, 64, 64)]
BATCHES = [1, 5, 32]
SENTINEL = 0xA7
MARGIN = 64
F32 = np.float32
ONE_BITS = int(np.array(1.0, dtype=F32).view(np.int32))
# (flip, min_side, brightness, colour): each operation alone, all together, and a window that may shrink to one column
CASES = {'flip': (0.5, 1.0, 0.0, 0.0), 'crop': (0.0, 0.4, 0.0, 0.0), 'brightness': (0.0, 1.0, 0.3, 0.0),
         'colour': (0.0, 1.0, 0.0, 0.2), 'all': (0.5, 0.4, 0.3, 0.2), 'wmin 1': (0.5, 1e-6, 0.3, 0.2)}


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    """A data config registers its flags when it is first imported, and the first definition of a name keeps its default:
    the config imported here must not decide the defaults that other modules' tests see later, so the flag table is put
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
    """A device tensor or numpy array against a numpy array: dtype, shape and every bit (floats compared as int32)."""
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.float32:
        got, want = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32)
    return np.array_equal(got, want)


def make_labels(rng, rows, H, W):
    labels = rng.randint(-5, 300, size=(rows, 1, H, W)).astype(np.int64)
    labels[:, 0, 0, 0] = np.resize(np.array([32767, -32767, -1, 0], dtype=np.int64), rows)
    return labels


def make_stores(rng, rows, shape, labels=True):
    """-> (device frame store, device label store or None, numpy frame store, numpy label store or None), rows random bytes"""
    C, H, W = shape
    want = R.new_store(rows, C * H * W, fill=SENTINEL)
    R.store_frames(want, 0, R.unit(rng.randint(0, 256, size=(rows, C, H, W)), 0))
    want_l = None
    if labels:
        want_l = R.new_store(rows, 2 * H * W, fill=SENTINEL)
        assert R.store_labels(want_l, 0, make_labels(rng, rows, H, W)) == 0
    return dev(want), (dev(want_l) if labels else None), want, want_l


class Margined(object):
    """A device buffer of `nbytes` payload bytes between two margins of sentinel bytes; `skew` bytes move the payload off
    the 16-byte grid."""

    def __init__(self, nbytes, skew=0):
        self.lo, self.n = MARGIN + skew, nbytes
        self.buf = torch.full((self.lo + nbytes + MARGIN,), SENTINEL, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.lo)

    def payload(self, dtype, shape):
        raw = host(self.buf)
        assert (raw[:self.lo] == SENTINEL).all() and (raw[self.lo + self.n:] == SENTINEL).all(), 'a margin was written'
        return raw[self.lo:self.lo + self.n].copy().view(dtype).reshape(shape)


def raw_gather(store, lstore, shape, a, epoch, idx, first, B, mode, skew=0):
    """One call of the C entry point into margined buffers -> (frames, labels or None, params) as numpy arrays."""
    C, H, W = shape
    out = Margined(B * C * H * W * 4, skew)
    out_l = Margined(B * H * W * 8, skew) if lstore is not None else None
    table = Margined(B * 8 * 4)
    _lib.call('gx_cache_gather_aug', ctypes.c_void_p(store.data_ptr()), int(store.shape[1]),
              None if lstore is None else ctypes.c_void_p(lstore.data_ptr()), 0 if lstore is None else int(lstore.shape[1]),
              int(store.shape[0]), None if idx is None else ctypes.c_void_p(idx.data_ptr()), 0 if idx is None else int(idx.shape[0]),
              first, mode, a.seed, epoch, a.flip_t, a.wmin(W), a.brightness, a.colour, out.ptr,
              None if out_l is None else out_l.ptr, table.ptr, B, C, H, W,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return (out.payload(np.float32, (B, C, H, W)), None if out_l is None else out_l.payload(np.int64, (B, 1, H, W)),
            table.payload(np.int32, (B, 8)))


def restated(want, want_l, shape, rows, a, epoch, mode):
    return A.gather(want, want_l, shape, rows, a.seed, epoch, a.flip_t, a.wmin(shape[2]), a.brightness, a.colour, mode)


def all_same(got, want):
    return all((g is None and w is None) or same_bits(g, w) for g, w in zip(got, want)) and len(got) == len(want)


# ---- the kernel against the restatement ----
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_frames_labels_and_parameters_equal_the_restatement(shape, B):
    C, H, W = shape
    rng = np.random.RandomState(1000 * B + C * H * W)
    rows = B + 5
    store, lstore, want, want_l = make_stores(rng, rows, shape)
    perm = rng.permutation(rows)[:B].astype(np.int64)
    repeated = np.concatenate([perm[:1], perm, perm[-1:]])          # B + 2 entries: `first` = 1 is the permutation itself
    repeats = np.resize(perm[:2], B + 1).astype(np.int64)           # the same one or two rows over and over
    geometry = set()
    for k, (name, (flip, min_side, brightness, colour)) in enumerate(sorted(CASES.items())):
        a = Augment(flip, min_side, brightness, colour, seed=17 + k)
        if name == 'wmin 1':
            assert a.wmin(W) == 1
        epoch = k
        # a permutation behind an offset, with labels
        got = raw_gather(store, lstore, shape, a, epoch, dev(repeated), 1, B, k % 2)
        assert all_same(got, restated(want, want_l, shape, perm, a, epoch, k % 2)), name
        geometry.update(map(tuple, got[2][:, :5].tolist()))
        # no index vector, no labels, the other mode, outputs off the 16-byte grid
        got = raw_gather(store, None, shape, a, epoch, None, 2, B, 1 - k % 2, skew=8)
        assert all_same(got, restated(want, None, shape, range(2, 2 + B), a, epoch, 1 - k % 2)), name
        # repeated rows, through the Python entry point
        got = augment.gather(store, lstore, shape, a, epoch, dev(repeats), 1, B, mode=k % 2, return_params=True)
        assert all_same(got, restated(want, want_l, shape, repeats[1:], a, epoch, k % 2)), name
        assert len(augment.gather(store, None, shape, a, epoch, B=B)) == 2
    if B == 32 and W >= 8:
        assert len(geometry) > 32                                    # (the cases did draw different flips and windows)


def test_the_parameter_table_over_300_rows_epochs_and_seeds():
    """Rows above 255, so that more than a byte of the row enters the counter; epochs beyond 2^31; a seed with a high half."""
    shape = (3, 8, 8)
    store, _, want, _ = make_stores(np.random.RandomState(3), 300, shape, labels=False)
    tables = []
    for seed in (0, (7 << 32) | 5):
        a = Augment(0.5, 0.3, 0.3, 0.2, seed=seed)
        for epoch in (0, 1, (1 << 31) + 5):
            got = raw_gather(store, None, shape, a, epoch, None, 0, 300, 0)[2]
            table = np.stack([A.params_row(A.params(seed, epoch, r, a.flip_t, a.wmin(8), a.brightness, a.colour, 3, 8, 8))
                              for r in range(300)])
            assert same_bits(got, table), (seed, epoch)
            tables.append(got)
    assert len({t.tobytes() for t in tables}) == 6
    assert len({t[r].tobytes() for t in tables[:1] for r in range(300)}) > 290          # row 256 + k is not row k again
    # one channel: the gains the frame does not have are 1
    shape = (1, 3, 17)
    store, _, want, _ = make_stores(np.random.RandomState(4), 8, shape, labels=False)
    got = raw_gather(store, None, shape, Augment(0.5, 0.5, 0.3, 0.2), 0, None, 0, 8, 0)[2]
    assert (got[:, 6:] == ONE_BITS).all() and (got[:, 5] != ONE_BITS).any()


# ---- identities ----
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_everything_off_is_the_plain_gathers_and_flip_one_their_mirror(shape):
    C, H, W = shape
    rng = np.random.RandomState(C * H * W)
    store, lstore, _, _ = make_stores(rng, 12, shape)
    idx = dev(rng.permutation(12).astype(np.int64))
    for mode in (0, 1):
        plain = data_cache.gather_frames(store, shape, idx, 2, 9, mode)
        plain_l = data_cache.gather_labels(lstore, (H, W), idx, 2, 9)
        x, y, table = augment.gather(store, lstore, shape, Augment(flip=0.0), 5, idx, 2, 9, mode, return_params=True)
        assert same_bits(x, host(plain)) and same_bits(y, host(plain_l))
        assert same_bits(table, np.tile(np.array([0, 0, 0, W, H, ONE_BITS, ONE_BITS, ONE_BITS], dtype=np.int32), (9, 1)))
        x, y = augment.gather(store, lstore, shape, Augment(flip=1.0), 5, idx, 2, 9, mode)
        assert same_bits(x, host(torch.flip(plain, dims=[3]))) and same_bits(y, host(torch.flip(plain_l, dims=[3])))


@pytest.mark.parametrize('mode', (0, 1))
def test_a_white_frame_never_exceeds_one(mode):
    shape = (3, 8, 8)
    store = data_cache.new_store(64, 192, 'cuda')
    store.fill_(255)
    x, _, table = augment.gather(store, None, shape, Augment(0.5, 0.4, 0.9, 0.0, seed=2), 0, mode=mode, return_params=True)
    bits = host(x).view(np.int32)
    gains = host(table)[:, 5].copy().view(F32)
    assert bits.max() == ONE_BITS and bits.min() > 0
    assert (gains > 1.0).sum() > 10 and (gains < 1.0).sum() > 10
    assert (bits[gains >= 1.0] == ONE_BITS).all() and (bits[gains < 0.99] < ONE_BITS).all()


# ---- determinism ----
def test_a_row_is_the_same_wherever_it_is_delivered():
    shape = (3, 5, 7)
    rng = np.random.RandomState(11)
    store, lstore, _, _ = make_stores(rng, 40, shape)
    a = Augment(0.5, 0.4, 0.3, 0.2, seed=4)
    order = rng.permutation(40).astype(np.int64)
    x, y, table = (host(t) for t in augment.gather(store, lstore, shape, a, 3, dev(order), 0, 32, return_params=True))
    other = np.concatenate([order[32:35], order[[7, 0, 31, 7, 12]], order[35:]])      # entries 3 .. 7: rows of the first batch
    x2, y2, table2 = (host(t) for t in augment.gather(store, lstore, shape, a, 3, dev(other), 3, 5, return_params=True))
    for k, b in enumerate((7, 0, 31, 7, 12)):
        assert same_bits(x2[k], x[b]) and same_bits(y2[k], y[b]) and same_bits(table2[k], table[b])
    assert not same_bits(x[7], x[0])
    for b in (0, 31):                                                # alone in its batch, without an index vector
        row = int(order[b])
        x1, y1, table1 = augment.gather(store, lstore, shape, a, 3, None, row, 1, return_params=True)
        assert same_bits(x1[0], x[b]) and same_bits(y1[0], y[b]) and same_bits(table1[0], table[b])


def test_the_next_epoch_draws_anew():
    shape = (3, 8, 8)
    store, _, want, _ = make_stores(np.random.RandomState(12), 32, shape, labels=False)
    a = Augment(0.5, 0.4, 0.3, 0.2, seed=6)
    e = 4
    tables = [np.stack([A.params_row(A.params(a.seed, epoch, r, a.flip_t, a.wmin(8), a.brightness, a.colour, 3, 8, 8))
                        for r in range(32)]) for epoch in (e, e + 1)]
    assert (tables[0] != tables[1]).any(axis=1).sum() >= 1           # the restatement first, for this seed
    got = [raw_gather(store, None, shape, a, epoch, None, 0, 32, 0) for epoch in (e, e + 1)]
    assert same_bits(got[0][2], tables[0]) and same_bits(got[1][2], tables[1])
    assert (got[0][2] != got[1][2]).any(axis=1).sum() >= 1 and not same_bits(got[0][0], got[1][0])
    again = raw_gather(store, None, shape, a, e, None, 0, 32, 0)
    assert same_bits(again[0], got[0][0]) and same_bits(again[2], got[0][2])          # and the same epoch draws the same


def test_the_python_entry_point_refuses_before_any_launch():
    store = data_cache.new_store(4, 192, 'cuda')
    with pytest.raises(GenesisHipError, match='must be an Augment'):
        augment.gather(store, None, (3, 8, 8), 'flip', 0)
    with pytest.raises(GenesisHipError, match='4 channels'):
        augment.gather(data_cache.new_store(4, 256, 'cuda'), None, (4, 8, 8), Augment(), 0)
    with pytest.raises(GenesisHipError, match='new_store'):
        augment.gather(store, data_cache.new_store(4, 100, 'cuda'), (3, 8, 8), Augment(), 0)
    with pytest.raises(GenesisHipError, match='does not go with'):
        augment.gather(store, data_cache.new_store(5, 128, 'cuda'), (3, 8, 8), Augment(), 0)
    with pytest.raises(GenesisHipError, match='reach outside'):
        augment.gather(store, None, (3, 8, 8), Augment(), 0, None, 3, 2)
    with pytest.raises(GenesisHipError, match='negative epoch'):
        augment.gather(store, None, (3, 8, 8), Augment(), -1)


# ---- the wrapper over a fake loader ----
class FakeLoader(object):
    """Yields fixed device tensors: the same objects every epoch."""

    def __init__(self, batches, batch_size):
        self.batches = batches
        self.batch_size = batch_size
        self.epochs = self.closed = 0

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
        b = {'input': dev(R.unit(rng.randint(0, 256, size=(B,) + SHAPE), mode))}
        if labels:
            b['instances'] = dev(make_labels(rng, B, SHAPE[1], SHAPE[2]))
        out.append(b)
    return out


def numpy_stores(batches):
    """What the filling epoch leaves in the stores, by the restatement."""
    x = np.concatenate([host(b['input']) for b in batches])
    want = R.new_store(len(x), x[0].size)
    R.store_frames(want, 0, x)
    want_l = None
    if 'instances' in batches[0]:
        want_l = R.new_store(len(x), 2 * SHAPE[1] * SHAPE[2])
        R.store_labels(want_l, 0, np.concatenate([host(b['instances']) for b in batches]))
    return want, want_l


def epoch_equals(batches, want, want_l, order, a, epoch, mode, sizes=(5, 5, 2)):
    assert [len(b['input']) for b in batches] == list(sizes)
    first = 0
    for b in batches:
        n = len(b['input'])
        x, y, _ = restated(want, want_l, SHAPE, order[first:first + n], a, epoch, mode)
        assert same_bits(b['input'], x) and (('instances' not in b) if y is None else same_bits(b['instances'], y))
        first += n
    return True


@pytest.mark.parametrize('labels,mode', ((True, 0), (False, 1)))
def test_cached_loader_augments_its_resident_epochs(labels, mode, capsys):
    batches = fake_batches(labels=labels, mode=mode)
    want, want_l = numpy_stores(batches)
    a = Augment(0.5, 0.4, 0.3, 0.2, seed=21)
    fake = FakeLoader(batches, 5)
    w = CachedLoader(fake, shuffle=True, seed=3, name='fake', augment=a)
    first = list(w)
    assert len(first) == 3 and all(got[k] is b[k] for got, b in zip(first, batches) for k in b)     # the loader's own tensors
    assert w.cache_state == 'resident' and w.mode == mode and fake.closed == 1
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('data_cache: fake')]
    assert len(lines) == 2 and 'not augmented' in lines[0] and 'rows resident' in lines[1]
    orders = []
    for counter in (0, 1):
        got = list(w)
        assert w.epoch == counter and sorted(w.order.tolist()) == list(range(12))
        assert epoch_equals(got, want, want_l, w.order, a, counter, mode)
        orders.append(w.order.tolist())
    assert orders[0] != orders[1]
    w.set_epoch((1 << 31) + 5)                                       # a resumed run
    got = list(w)
    assert w.epoch == (1 << 31) + 5 and epoch_equals(got, want, want_l, w.order, a, (1 << 31) + 5, mode)
    got = list(w)
    assert w.epoch == (1 << 31) + 6 and epoch_equals(got, want, want_l, w.order, a, (1 << 31) + 6, mode)
    assert fake.epochs == 1 and [l for l in capsys.readouterr().out.splitlines() if l.startswith('data_cache:')] == []
    w.close()


def test_when_the_cache_is_off_so_is_augmentation(capsys):
    batches = fake_batches()
    w = CachedLoader(FakeLoader(batches, 5), budget_bytes=1024, name='fake', augment=Augment(0.5, 0.4, 0.3, 0.2))
    for _ in range(3):
        got = list(w)
        assert len(got) == 3 and all(g[k] is b[k] for g, b in zip(got, batches) for k in b)         # passed through
    assert w.cache_state.startswith('off: ') and 'over the budget' in w.cache_state
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('data_cache: fake')]
    assert len(lines) == 2 and 'not augmented' in lines[0]
    assert 'not cached' in lines[1] and 'augmentation is off too' in lines[1] and 'over the budget' in lines[1]
    # frames of four channels: refused by the wrapper, which goes off instead of breaking the run
    four = [{'input': torch.zeros(2, 4, 5, 7, device='cuda')}]
    w = CachedLoader(FakeLoader(four, 2), name='four', augment=Augment())
    assert [b['input'] is four[0]['input'] for b in list(w) + list(w)] == [True, True]
    assert 'cannot be augmented' in w.cache_state


# ---- end to end: a folder of PNGs through image_folder_config with cfg.augment ----
def test_image_folder_epochs_two_and_three_are_augmented(tmp_path, monkeypatch):
    import genesis_amd.image_folder_config as IF
    from genesis_amd.visualise import save_png
    monkeypatch.delenv(data_cache.ENV, raising=False)
    monkeypatch.delenv(augment.ENV, raising=False)
    rng = np.random.RandomState(3)
    for i in range(10):
        save_png(os.path.join(str(tmp_path), 'f%02d.png' % i), rng.randint(0, 256, size=(11 + i % 3, 9 + i % 4, 3)).astype(np.uint8))
    cfg = AttrDict(data_folder=str(tmp_path), img_size=8, num_workers=2, batch_size=3, seed=5,
                   augment='flip,min_side=0.5,brightness=0.2,colour=0.1')
    train, val, test = IF.load(cfg)
    try:
        assert type(train) is CachedLoader and type(val) is not CachedLoader and type(test) is not CachedLoader
        a = train.augment
        assert (a.flip, a.min_side, a.brightness, a.colour, a.seed) == (0.5, 0.5, 0.2, 0.1, 5)
        train.loader.shuffle = False                                     # the wrapper follows it: every epoch in file order
        first = [b['input'].clone() for b in train]
        assert train.cache_state == 'resident' and train.mode == 0 and train.rows == 8
        want = R.new_store(8, 192)
        R.store_frames(want, 0, np.concatenate([host(f) for f in first]))
        for counter in (0, 1):
            got = [b['input'] for b in train]
            assert train.epoch == counter and [len(g) for g in got] == [3, 3, 2]
            x, _, table = restated(want, None, (3, 8, 8), range(8), a, counter, 0)
            assert same_bits(torch.cat(got), x)
            assert not same_bits(torch.cat(got), np.concatenate([host(f) for f in first]))
            assert len({tuple(r) for r in table[:, :5].tolist()}) > 1
    finally:
        for l in (train, val, test):
            l.close()
