"""Augmentation of cached batches (genesis_amd/augment.py, gx_cache_gather_aug in csrc/gx_cache.hip) without a GPU: the
generator's known answer, Augment and its parser, the argument checks of the C entry point, the switch in wrap_loaders
(cfg.augment / GENESIS_AUGMENT) and the identities of the numpy restatement the GPU tests compare the kernel with."""
import ctypes
import math

import numpy as np
import pytest

from genesis_amd import _lib
from genesis_amd._lib import GenesisHipError
from genesis_amd.compat.attrdict import AttrDict
from tests import augment_restatement as A
from tests import data_cache_restatement as R

F32 = np.float32
ONE_BITS = int(np.array(1.0, dtype=F32).view(np.int32))


# ---- the generator ----
def test_philox_known_answers():
    assert A.philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # the second and third vectors of Random123's kat_vectors for philox4x32-10
    assert A.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert A.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_the_words_of_a_frame():
    """Call A / call B, the key from the seed's halves, the row's halves and the epoch's low word in the counter."""
    seed, epoch, row = (7 << 32) | 5, (1 << 31) + 5, (3 << 32) | 300
    r = A.words(seed, epoch, row)
    assert r[:4] == A.philox4x32_10((300, 3, (1 << 31) + 5, 0xA06), (5, 7))
    assert r[4:] == A.philox4x32_10((300, 3, (1 << 31) + 5, 0xA07), (5, 7))
    assert A.words(seed, epoch + (1 << 32), row) == r and A.words(seed, epoch + 1, row) != r
    assert len({tuple(A.words(seed, 0, k)) for k in (0, 1, 256, 1 << 32)}) == 4


# ---- Augment ----
def test_augment_accepts_and_exposes():
    from genesis_amd.augment import Augment
    a = Augment()
    assert (a.flip, a.min_side, a.brightness, a.colour, a.seed) == (0.5, 1.0, 0.0, 0.0, 0)
    assert a.flip_t == 1 << 23 and a.wmin(64) == 64 and a.wmin(1) == 1
    assert Augment(flip=0).flip_t == 0 and Augment(flip=1).flip_t == 1 << 24 and Augment(flip=0.25).flip_t == 1 << 22
    assert Augment(flip=0.3).flip_t == int(round(0.3 * 2 ** 24))
    for min_side, W in ((0.4, 64), (0.4, 7), (0.5, 8), (0.01, 8), (1e-9, 64), (0.999, 64), (0.75, 17)):
        assert Augment(min_side=min_side).wmin(W) == max(1, int(math.ceil(min_side * W)))
    assert Augment(min_side=0.4).wmin(64) == 26 and Augment(min_side=0.01).wmin(8) == 1 and Augment(min_side=0.5).wmin(8) == 4
    assert Augment(seed=-1).seed == (1 << 64) - 1 and Augment(seed=(1 << 64) + 3).seed == 3
    assert 'min_side=0.4' in repr(Augment(min_side=0.4))


def test_augment_refusals_name_the_argument():
    from genesis_amd.augment import Augment
    for kwargs, name in ((dict(flip=-0.1), 'flip'), (dict(flip=1.5), 'flip'), (dict(flip=float('nan')), 'flip'),
                         (dict(flip='0.5'), 'flip'), (dict(flip=True), 'flip'),
                         (dict(min_side=0), 'min_side'), (dict(min_side=1.01), 'min_side'), (dict(min_side=-1), 'min_side'),
                         (dict(min_side=None), 'min_side'),
                         (dict(brightness=1.0), 'brightness'), (dict(brightness=-0.1), 'brightness'),
                         (dict(brightness=float('nan')), 'brightness'), (dict(brightness=1.0 - 1e-12), 'brightness'),
                         (dict(colour=1.0), 'colour'), (dict(colour=-1e-3), 'colour'), (dict(colour=float('inf')), 'colour'),
                         (dict(seed=1.5), 'seed'), (dict(seed='3'), 'seed')):
        with pytest.raises(GenesisHipError, match='augment: ' + name):
            Augment(**kwargs)


def test_augment_parse():
    from genesis_amd.augment import Augment
    a = Augment.parse('flip=0.5,min_side=0.6,brightness=0.2,colour=0.1')
    assert (a.flip, a.min_side, a.brightness, a.colour, a.seed) == (0.5, 0.6, 0.2, 0.1, 0)
    a = Augment.parse(' flip , colour = 0.25 ', seed=9)
    assert (a.flip, a.min_side, a.brightness, a.colour, a.seed) == (0.5, 1.0, 0.0, 0.25, 9)
    a = Augment.parse('min_side=0.5')
    assert (a.flip, a.min_side, a.brightness, a.colour) == (0.0, 0.5, 0.0, 0.0)          # what is not named is off
    assert Augment.parse('flip=1').flip_t == 1 << 24
    for text, what in (('flop=0.5', 'unknown key'), ('flip,zoom=2', 'unknown key'), ('', 'unknown key'), ('flip,,colour=0.1', 'unknown key'),
                       ('min_side', 'needs a value'), ('brightness=', 'no number'), ('colour=much', 'no number'),
                       ('flip,flip=0.2', 'twice'), ('flip=2', 'flip must be'), ('brightness=1', 'brightness must be')):
        with pytest.raises(GenesisHipError, match=what):
            Augment.parse(text)
    with pytest.raises(GenesisHipError, match='expected a text'):
        Augment.parse(0.5)


# ---- the C ABI: every argument is checked before any launch, so none of this needs a device ----
P = ctypes.c_void_p(4096)            # a non-null, 16-byte aligned address that is never dereferenced
NAME = 'gx_cache_gather_aug'


def _aug(frames=P, stride=112, labels=P, label_stride=80, rows=8, idx=None, idx_len=0, first=0, mode=0, seed=0, epoch=0,
         flip_t=1 << 23, wmin=3, brightness=0.25, colour=0.5, out=P, out_labels=P, params=None, B=2, C=3, H=5, W=7):
    _lib.call(NAME, frames, stride, labels, label_stride, rows, idx, idx_len, first, mode, seed, epoch, flip_t, wmin, brightness,
              colour, out, out_labels, params, B, C, H, W, None)


def test_the_entry_point_is_declared_and_exported():
    decls = _lib.declarations()
    assert NAME in decls and hasattr(_lib.load(), NAME)
    ret, args = decls[NAME]
    assert ret == 'int' and args[-1] == ('gx_stream_t', 'stream')
    assert [n for _, n in args] == ['frames', 'frame_stride', 'labels', 'label_stride', 'rows', 'idx', 'idx_len', 'first', 'mode',
                                    'seed', 'epoch', 'flip_t', 'wmin', 'brightness', 'colour', 'out', 'out_labels', 'params_out',
                                    'B', 'C', 'H', 'W', 'stream']
    assert dict((n, t) for t, n in args)['seed'] == 'unsigned long long'


def test_argument_validation_needs_no_gpu():
    # what gx_cache_gather_f32 refuses, with its messages
    for null in ('frames', 'out'):
        with pytest.raises(GenesisHipError, match='null pointer'):
            _aug(**{null: None})
    with pytest.raises(GenesisHipError, match='B at most 65535'):
        _aug(B=65536, rows=1 << 20)
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(rows=0)):
        with pytest.raises(GenesisHipError, match='bad dims'):
            _aug(**bad)
    for stride in (120, 0):
        with pytest.raises(GenesisHipError, match='multiple of 16'):
            _aug(stride=stride)
    with pytest.raises(GenesisHipError, match='shorter than a row'):
        _aug(stride=64)
    with pytest.raises(GenesisHipError, match='16-byte aligned'):
        _aug(frames=ctypes.c_void_p(4096 + 8))
    with pytest.raises(GenesisHipError, match='negative first'):
        _aug(first=-1)
    with pytest.raises(GenesisHipError, match='reach past'):
        _aug(first=7)                                                # no index vector: rows 7, 8 of 8
    with pytest.raises(GenesisHipError, match='reach past'):
        _aug(idx=P, idx_len=5, first=4)                              # first + B past idx_len, although the store has the rows
    for mode in (-1, 2):
        with pytest.raises(GenesisHipError, match='bad mode'):
            _aug(mode=mode)
    # the label store is checked like the frame store
    for label_stride in (72, 0):
        with pytest.raises(GenesisHipError, match='labels: .*multiple of 16'):
            _aug(label_stride=label_stride)
    with pytest.raises(GenesisHipError, match='labels: .*shorter than a row'):
        _aug(label_stride=64)                                        # 5 * 7 int16 are 70 bytes
    with pytest.raises(GenesisHipError, match='labels: .*16-byte aligned'):
        _aug(labels=ctypes.c_void_p(4096 + 2))
    # what only this entry point refuses
    for kwargs in (dict(labels=None), dict(out_labels=None)):
        with pytest.raises(GenesisHipError, match='both or neither'):
            _aug(**kwargs)
    with pytest.raises(GenesisHipError, match='at most 3 channels'):
        _aug(C=4, stride=144)
    with pytest.raises(GenesisHipError, match='frame too large'):
        _aug(B=1, C=1, H=1, W=32768, stride=32768, label_stride=65536, wmin=1)
    with pytest.raises(GenesisHipError, match='frame too large'):
        _aug(B=1, C=1, H=32768, W=1, stride=32768, label_stride=65536, wmin=1)
    with pytest.raises(GenesisHipError, match='negative epoch'):
        _aug(epoch=-1)
    for flip_t in (-1, (1 << 24) + 1):
        with pytest.raises(GenesisHipError, match='flip_t'):
            _aug(flip_t=flip_t)
    for wmin in (0, -3, 8):
        with pytest.raises(GenesisHipError, match='wmin'):
            _aug(wmin=wmin)
    for name in ('brightness', 'colour'):
        for v in (1.0, -0.25, 1.5, float('nan'), float('inf')):
            with pytest.raises(GenesisHipError, match=name):
                _aug(**{name: v})


# ---- wrap_loaders ----
class Plain(object):
    batch_size = 4

    def __len__(self):
        return 3

    def __iter__(self):
        return iter(())


@pytest.mark.parametrize('cache', (False, True), ids=('cache not asked for', 'cache asked for'))
def test_wrap_loaders_augments_the_train_loader_only(cache, monkeypatch):
    from genesis_amd import augment, data_cache
    from genesis_amd.data_cache import CachedLoader
    monkeypatch.delenv(data_cache.ENV, raising=False)
    monkeypatch.delenv(augment.ENV, raising=False)
    loaders = (Plain(), Plain(), Plain())
    base = dict(seed=11, cache_on_device=cache)

    def checked(got, want_aug):
        assert isinstance(got, tuple) and len(got) == 3
        assert type(got[0]) is CachedLoader and got[0].loader is loaders[0] and got[0].name == 'plain[0]'
        a = got[0].augment
        assert type(a) is augment.Augment and (a.flip, a.min_side, a.brightness, a.colour, a.seed) == want_aug
        assert got[0].epoch == 0 and got[0].cache_state == 'filling' and got[0].shuffle is True
        for i in (1, 2):
            if cache:
                assert type(got[i]) is CachedLoader and got[i].loader is loaders[i] and got[i].augment is None
                assert got[i].shuffle is False
            else:
                assert got[i] is loaders[i]

    # neither setting: exactly what the cache switch alone does
    got = data_cache.wrap_loaders(AttrDict(base), loaders, shuffle=(True, False, False), name='plain')
    if cache:
        assert [type(w) for w in got] == [CachedLoader] * 3 and all(w.augment is None for w in got)
    else:
        assert got is loaders
    for off in (None, '', False):
        again = data_cache.wrap_loaders(AttrDict(base, augment=off), loaders, name='plain')
        assert (again is loaders) if not cache else all(w.augment is None for w in again)
    # cfg.augment as a text, seeded with cfg.seed
    checked(data_cache.wrap_loaders(AttrDict(base, augment='flip,min_side=0.5'), loaders, shuffle=(True, False, False), name='plain'),
            (0.5, 0.5, 0.0, 0.0, 11))
    # ... as an Augment, taken as it is
    mine = augment.Augment(flip=0.25, colour=0.5, seed=3)
    got = data_cache.wrap_loaders(AttrDict(base, augment=mine), loaders, shuffle=(True, False, False), name='plain')
    checked(got, (0.25, 1.0, 0.0, 0.5, 3))
    assert got[0].augment is mine
    # the environment variable, alone and ahead of cfg.augment
    monkeypatch.setenv(augment.ENV, 'brightness=0.25')
    checked(data_cache.wrap_loaders(AttrDict(base), loaders, shuffle=(True, False, False), name='plain'), (0.0, 1.0, 0.25, 0.0, 11))
    checked(data_cache.wrap_loaders(AttrDict(base, augment='flip'), loaders, shuffle=(True, False, False), name='plain'),
            (0.0, 1.0, 0.25, 0.0, 11))
    monkeypatch.setenv(augment.ENV, 'zoom=2')
    with pytest.raises(GenesisHipError, match='unknown key'):
        data_cache.wrap_loaders(AttrDict(base), loaders)
    # the budget rule is the cache's
    monkeypatch.setenv(augment.ENV, 'flip')
    monkeypatch.setenv(data_cache.ENV, '2')
    got = data_cache.wrap_loaders(AttrDict(seed=11), loaders)
    assert [type(w) for w in got] == [CachedLoader] * 3 and {w.budget_bytes for w in got} == {2 * 10 ** 9}
    assert [w.augment is not None for w in got] == [True, False, False]


def test_cached_loader_takes_an_augment_or_none():
    from genesis_amd.augment import Augment
    from genesis_amd.data_cache import CachedLoader
    with pytest.raises(GenesisHipError, match='augment must be'):
        CachedLoader(Plain(), augment='flip')
    w = CachedLoader(Plain(), augment=Augment())
    assert w.epoch == 0
    w.set_epoch(7)
    assert w.epoch == 7
    for bad in (-1, 1.5, None, True):
        with pytest.raises(GenesisHipError, match='set_epoch'):
            w.set_epoch(bad)
    assert CachedLoader(Plain()).augment is None


# ---- the restatement's identities ----
SHAPES = [(3, 5, 7), (3, 8, 8), (1, 3, 17), (3, 16, 16), (1, 1, 1)]


def _stores(rng, rows, shape):
    C, H, W = shape
    store = R.new_store(rows, C * H * W, fill=0xA7)
    lstore = R.new_store(rows, 2 * H * W, fill=0xA7)
    R.store_frames(store, 0, R.unit(rng.randint(0, 256, size=(rows, C, H, W)), 0))
    labels = rng.randint(-3, 300, size=(rows, 1, H, W)).astype(np.int64)
    labels.reshape(-1)[:2] = (32767, -32767)[:labels.size]
    R.store_labels(lstore, 0, labels)
    return store, lstore


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_everything_off_is_the_plain_gather(shape):
    C, H, W = shape
    rng = np.random.RandomState(C * H * W)
    store, lstore = _stores(rng, 6, shape)
    rows = [4, 0, 5, 4]
    for mode in (0, 1):
        x, y, table = A.gather(store, lstore, shape, rows, seed=3, epoch=2, flip_t=0, wmin=W, brightness=0.0, colour=0.0, mode=mode)
        assert np.array_equal(R.bits(x), R.bits(R.gather_frames(store, shape, rows, mode)))
        assert np.array_equal(y, R.gather_labels(lstore, (H, W), rows))
        assert np.array_equal(table, np.tile(np.array([0, 0, 0, W, H, ONE_BITS, ONE_BITS, ONE_BITS], dtype=np.int32), (4, 1)))
    assert A.gather(store, None, shape, rows, 3, 2, 0, W, 0.0, 0.0, 0)[1] is None


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_flip_only_is_the_mirror_image(shape):
    C, H, W = shape
    rng = np.random.RandomState(C * H * W + 1)
    store, lstore = _stores(rng, 6, shape)
    rows = list(range(6))
    x, y, table = A.gather(store, lstore, shape, rows, seed=0, epoch=0, flip_t=1 << 24, wmin=W, brightness=0.0, colour=0.0, mode=0)
    assert (table[:, 0] == 1).all()
    assert np.array_equal(R.bits(x), R.bits(R.gather_frames(store, shape, rows, 0)[..., ::-1]))
    assert np.array_equal(y, R.gather_labels(lstore, (H, W), rows)[..., ::-1])
    # a probability of a half flips some rows and not others, each either the frame or its mirror image
    x, y, table = A.gather(store, lstore, shape, range(6), seed=1, epoch=0, flip_t=1 << 23, wmin=W, brightness=0.0, colour=0.0, mode=0)
    plain = R.gather_frames(store, shape, rows, 0)
    for b in range(6):
        assert np.array_equal(R.bits(x[b]), R.bits(plain[b, ..., ::-1] if table[b, 0] else plain[b]))
    flips = np.array([A.params(1, 0, r, 1 << 23, 8, 0.0, 0.0, 3, 8, 8)[0] for r in range(200)])
    assert 70 < flips.sum() < 130


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_a_constant_frame_stays_constant_and_windows_stay_inside(shape):
    C, H, W = shape
    store = R.new_store(300, C * H * W)
    values = np.arange(300) % 256
    store[:, :C * H * W] = values[:, None].astype(np.uint8)
    lstore = R.new_store(300, 2 * H * W)
    R.store_labels(lstore, 0, np.broadcast_to((np.arange(300) - 5).reshape(300, 1, 1, 1), (300, 1, H, W)).astype(np.int64))
    rows = list(range(300))
    for wmin in sorted({1, max(1, W // 2), W}):
        x, y, table = A.gather(store, lstore, shape, rows, seed=5, epoch=1, flip_t=1 << 23, wmin=wmin, brightness=0.0, colour=0.0, mode=0)
        assert np.array_equal(R.bits(x), R.bits(np.broadcast_to(R.unit(values, 0)[:, None, None, None], x.shape)))
        assert np.array_equal(y, np.broadcast_to((np.arange(300) - 5)[:, None, None, None], y.shape))
        flip, x0, y0, w, h = (table[:, k].astype(np.int64) for k in range(5))
        assert (w >= wmin).all() and (w <= W).all() and (h >= 1).all() and (h <= H).all()
        assert (x0 >= 0).all() and (x0 + w <= W).all() and (y0 >= 0).all() and (y0 + h <= H).all()
        assert np.array_equal(h, np.clip((w * H + W // 2) // W, 1, H))
        if W >= 8 and wmin == 1:
            assert len(set(w.tolist())) > 2 and len(set(x0.tolist())) > 2           # (the draws do vary)
    # with gains the values stay in [0, 1] and a frame stays constant per channel
    x, _, table = A.gather(store, None, shape, rows, seed=5, epoch=1, flip_t=0, wmin=1, brightness=0.9, colour=0.9, mode=1)
    assert x.min() >= 0 and x.max() <= 1 and (x == x[:, :, :1, :1]).all()
    gains = table[:, 5:5 + C].copy().view(F32)
    assert (gains > 0.0).all() and (gains < 4.0).all() and len(np.unique(gains)) > 100
    assert (table[:, 5 + C:] == ONE_BITS).all()
