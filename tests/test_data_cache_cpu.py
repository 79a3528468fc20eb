"""The device cache of decoded splits (genesis_amd/data_cache.py, csrc/gx_cache.hip) without a GPU: the byte / 255 arithmetic
the two gather modes rest on, the argument checks of the four C entry points, CachedLoader's refusals, and the switch in
the data configs (cfg.cache_on_device / GENESIS_DATA_CACHE)."""
import ctypes
import os
import os.path as osp
import shutil
import sys

import numpy as np
import pytest

from genesis_amd import _lib
from genesis_amd._lib import GenesisHipError
from genesis_amd.compat.attrdict import AttrDict
from tests import data_cache_restatement as R

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
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
    configs = ['genesis_amd.' + name for name in ('image_folder_config', 'shapestacks_config', 'sketchy_config',
                                                  'multi_object_config', 'gqn_config')]
    fresh = [m for m in configs if m not in sys.modules]
    yield
    flags.FLAGS.clear()
    flags.FLAGS.update(saved)
    for m in fresh:
        sys.modules.pop(m, None)


# ---- arithmetic ----
def test_bytes_survive_the_round_trip_in_their_own_mode():
    b = np.arange(256)
    for mode in (0, 1):
        v = R.unit(b, mode)
        assert v.dtype == F32
        q, div_miss, mul_miss = R.quantise(v)
        assert np.array_equal(q, b)                                  # rint((b / 255f) * 255) == b, and the same for b * (1 / 255f)
        assert np.array_equal(R.bits(R.unit(q, mode)), R.bits(v))    # ... and the mode's way back reproduces the bits
        assert (div_miss, mul_miss)[mode] == 0


def test_division_reproduces_130_of_the_256_products():
    """Why mode 1 exists: b * (1 / 255f) has other bits than b / 255f for 126 of the 256 bytes."""
    b = np.arange(256)
    same = R.bits(R.unit(b, 0)) == R.bits(R.unit(b, 1))
    assert int(same.sum()) == 130
    _, div_miss, mul_miss = R.quantise(R.unit(b, 1))
    assert (div_miss, mul_miss) == (126, 0)
    _, div_miss, mul_miss = R.quantise(R.unit(b, 0))
    assert (div_miss, mul_miss) == (0, 126)


def test_restatement_counts_what_is_not_a_byte_and_keeps_the_pad():
    v = np.array([0.0, 1.0, 0.3, 1.5, -0.2, np.nan, -0.0, 0.5], dtype=F32)
    q, div_miss, mul_miss = R.quantise(v)
    assert q.tolist() == [0, 255, 76, 255, 0, 0, 0, 128]
    assert (div_miss, mul_miss) == (6, 6)                            # all but 0.0 and 1.0
    s, misfit = R.narrow_labels(np.array([-1, 0, 255, 32767, -32768, 40000, -40000], dtype=np.int64))
    assert s.tolist() == [-1, 0, 255, 32767, -32768, 40000 - 65536, 65536 - 40000] and misfit == 2
    assert [R.row_stride(n) for n in (1, 15, 16, 17, 105, 192)] == [16, 16, 16, 32, 112, 192]
    store = R.new_store(4, 105, fill=0xAB)
    values = np.arange(2 * 105) % 256
    batch = R.unit(values, 0).reshape(2, 3, 5, 7)
    assert R.store_frames(store, 1, batch) == (0, int(np.count_nonzero(R.bits(R.unit(values, 0)) != R.bits(R.unit(values, 1)))))
    assert (store[0] == 0xAB).all() and (store[3] == 0xAB).all() and (store[1:3, 105:] == 0xAB).all()
    assert np.array_equal(R.bits(R.gather_frames(store, (3, 5, 7), [2, 1], 0)), R.bits(batch[[1, 0]]))
    labels = np.array([-1, 0, 255, 32767, 7, 8], dtype=np.int64).reshape(1, 1, 2, 3)
    lstore = R.new_store(2, 12, fill=0xCD)
    assert R.store_labels(lstore, 1, labels) == 0
    assert np.array_equal(R.gather_labels(lstore, (2, 3), [1]), labels) and (lstore[1, 12:] == 0xCD).all() and (lstore[0] == 0xCD).all()


# ---- the C ABI: every argument is checked before any launch, so none of this needs a device ----
P = ctypes.c_void_p(4096)            # a non-null, 16-byte aligned address that is never dereferenced


def _store_u8(batch=P, store=P, stride=112, first_row=0, capacity=8, counters=P, B=2, C=3, H=5, W=7):
    _lib.call('gx_cache_store_u8', batch, store, stride, first_row, capacity, counters, B, C, H, W, None)


def _store_labels(labels=P, store=P, stride=80, first_row=0, capacity=8, counters=P, B=2, H=5, W=7):
    _lib.call('gx_cache_store_labels_i16', labels, store, stride, first_row, capacity, counters, B, H, W, None)


def _gather(store=P, stride=112, rows=8, idx=None, idx_len=0, first=0, mode=0, out=P, B=2, C=3, H=5, W=7):
    _lib.call('gx_cache_gather_f32', store, stride, rows, idx, idx_len, first, mode, out, B, C, H, W, None)


def _gather_labels(store=P, stride=80, rows=8, idx=None, idx_len=0, first=0, out=P, B=2, H=5, W=7):
    _lib.call('gx_cache_gather_labels', store, stride, rows, idx, idx_len, first, out, B, H, W, None)


def test_the_entry_points_are_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name in ('gx_cache_store_u8', 'gx_cache_store_labels_i16', 'gx_cache_gather_f32', 'gx_cache_gather_labels'):
        assert name in decls and hasattr(lib, name)
        assert decls[name][1][-1] == ('gx_stream_t', 'stream')


@pytest.mark.parametrize('call', [_store_u8, _store_labels, _gather, _gather_labels], ids=lambda f: f.__name__)
def test_argument_validation_needs_no_gpu(call):
    storing = call in (_store_u8, _store_labels)
    for null in (('batch' if call is _store_u8 else 'labels', 'store', 'counters') if storing else ('store', 'out')):
        with pytest.raises(GenesisHipError, match='null pointer'):
            call(**{null: None})
    with pytest.raises(GenesisHipError, match='B at most 65535'):
        call(B=65536, **(dict(capacity=1 << 20) if storing else dict(rows=1 << 20)))
    for bad in (dict(B=0), dict(H=0), dict(W=-1)):
        with pytest.raises(GenesisHipError, match='bad dims'):
            call(**bad)
    with pytest.raises(GenesisHipError, match='multiple of 16'):
        call(stride=120)
    with pytest.raises(GenesisHipError, match='multiple of 16'):
        call(stride=0)
    with pytest.raises(GenesisHipError, match='shorter than a row'):
        call(stride=64)
    with pytest.raises(GenesisHipError, match='16-byte aligned'):
        call(store=ctypes.c_void_p(4096 + 8))
    if storing:
        with pytest.raises(GenesisHipError, match='negative first_row'):
            call(first_row=-1)
        with pytest.raises(GenesisHipError, match="past the store's capacity"):
            call(first_row=7)                                         # rows 7, 8 of 8
        with pytest.raises(GenesisHipError, match='8-byte aligned'):
            call(counters=ctypes.c_void_p(4096 + 4))
    else:
        with pytest.raises(GenesisHipError, match='negative first'):
            call(first=-1)
        with pytest.raises(GenesisHipError, match='reach past'):
            call(first=7)                                             # no index vector: rows 7, 8 of 8
        with pytest.raises(GenesisHipError, match='reach past'):
            call(idx=P, idx_len=5, first=4)                           # first + B past idx_len, although the store has the rows
    if call is _gather:
        for mode in (-1, 2):
            with pytest.raises(GenesisHipError, match='bad mode'):
                call(mode=mode)
        with pytest.raises(GenesisHipError, match='bad dims'):
            call(C=0)


# ---- CachedLoader's refusals ----
class Plain(object):
    batch_size = 4

    def __len__(self):
        return 3

    def __iter__(self):
        return iter(())


def test_cached_loader_construction_refusals():
    from genesis_amd.data_cache import CachedLoader

    class NoLen(object):
        batch_size = 4

    class NoBatchSize(object):
        def __len__(self):
            return 3

    for bad in (NoLen(), NoBatchSize(), [1, 2, 3]):
        with pytest.raises(GenesisHipError, match='__len__ and batch_size'):
            CachedLoader(bad)
    for budget in (0, -1, -0.5):
        with pytest.raises(GenesisHipError, match='budget_bytes must be positive'):
            CachedLoader(Plain(), budget_bytes=budget)
    w = CachedLoader(Plain(), budget_bytes=1 << 20, shuffle=False, seed=3, name='plain')
    assert len(w) == 3 and w.batch_size == 4 and isinstance(w.loader, Plain) and w.cache_state == 'filling' and w.order is None
    w.close()


def test_the_environment_variable(monkeypatch):
    from genesis_amd import data_cache
    cfg = AttrDict(batch_size=4)
    monkeypatch.delenv(data_cache.ENV, raising=False)
    assert data_cache.requested(cfg) == (False, None)
    assert data_cache.requested(AttrDict(cache_on_device=True)) == (True, None)
    loaders = (Plain(), Plain(), Plain())
    assert data_cache.wrap_loaders(cfg, loaders) is loaders
    for text, want in (('', (False, None)), ('0', (False, None)), ('1', (True, None)), ('2', (True, 2 * 10 ** 9)),
                       ('0.5', (True, 5 * 10 ** 8))):
        monkeypatch.setenv(data_cache.ENV, text)
        assert data_cache.requested(cfg) == want
    for text in ('yes', '-3'):
        monkeypatch.setenv(data_cache.ENV, text)
        with pytest.raises(GenesisHipError, match=data_cache.ENV):
            data_cache.requested(cfg)
    monkeypatch.setenv(data_cache.ENV, '2')
    wrapped = data_cache.wrap_loaders(AttrDict(seed=5), loaders, shuffle=(True, False, None), name='plain')
    assert [type(w) for w in wrapped] == [data_cache.CachedLoader] * 3 and [w.loader for w in wrapped] == list(loaders)
    assert [w.shuffle for w in wrapped] == [True, False, None] and {w.budget_bytes for w in wrapped} == {2 * 10 ** 9}
    assert wrapped[1].name == 'plain[1]'


# ---- the data configs: wrapped when asked, today's objects otherwise ----
def _both_ways(load, cfg, plain_type, monkeypatch):
    """load(cfg) three ways: neither switch (plain loaders), cfg.cache_on_device, GENESIS_DATA_CACHE.  -> the wrapped tuple"""
    from genesis_amd import data_cache
    monkeypatch.delenv(data_cache.ENV, raising=False)
    plain = load(AttrDict(cfg))
    assert len(plain) == 3 and all(type(l) is plain_type for l in plain)
    wrapped = load(AttrDict(cfg, cache_on_device=True))
    monkeypatch.setenv(data_cache.ENV, '3')
    by_env = load(AttrDict(cfg))
    monkeypatch.delenv(data_cache.ENV)
    for got, budget in ((wrapped, None), (by_env, 3 * 10 ** 9)):
        assert len(got) == 3
        for w, p in zip(got, plain):
            assert type(w) is data_cache.CachedLoader and type(w.loader) is plain_type and w.cache_state == 'filling'
            assert len(w) == len(p) and w.batch_size == p.batch_size and w.budget_bytes == budget
    assert all(type(l) is plain_type for l in load(AttrDict(cfg, cache_on_device=False)))
    return wrapped


def test_image_folder_config(tmp_path, monkeypatch):
    import genesis_amd.image_folder_config as F
    from genesis_amd.imagefile import ImageFileLoader
    for mode, n in (('train', 9), ('val', 2), ('test', 1)):
        os.makedirs(str(tmp_path / mode))
        for i in range(n):
            (tmp_path / mode / ('f%d.png' % i)).write_bytes(b'never read')
    cfg = dict(data_folder=str(tmp_path), img_size=8, num_workers=2, batch_size=4, seed=3)
    wrapped = _both_ways(F.load, cfg, ImageFileLoader, monkeypatch)
    assert [len(w) for w in wrapped] == [3, 1, 1] and wrapped[0].batch_size == 4
    assert all(w.shuffle is None and w.loader.shuffle for w in wrapped)       # follows the loader's own attribute
    assert wrapped[0].name == 'image_folder[0]'


def test_sketchy_and_shapestacks_configs(tmp_path, monkeypatch):
    import genesis_amd.shapestacks_config as S
    import genesis_amd.sketchy_config as K
    from genesis_amd.png import PngFileLoader
    root = str(tmp_path / 'sketchy')
    for mode, n in (('train', 5), ('valid', 2), ('test', 2)):
        os.makedirs(osp.join(root, 'processed', mode, 'ep0'))
        for i in range(n):
            with open(osp.join(root, 'processed', mode, 'ep0', 'ep0_%d.png' % i), 'wb') as f:
                f.write(b'never read')
    wrapped = _both_ways(K.load, dict(data_folder=root, img_size=128, num_workers=1, batch_size=2, seed=0), PngFileLoader, monkeypatch)
    assert [len(w) for w in wrapped] == [3, 1, 2] and [w.batch_size for w in wrapped] == [2, 2, 1]
    root = str(tmp_path / 'shapestacks')
    scenario = 'env_ccs-hard-h=2-vcom=0-vpsf=0-v=60'
    for sub in ('recordings', 'iseg'):
        os.makedirs(osp.join(root, sub, scenario))
    os.makedirs(osp.join(root, 'splits', 'default'))
    for cam in (1, 7, 12):
        for path in (osp.join(root, 'recordings', scenario, 'rgb-w=5-f=2-l=1-c=unique-cam_%d-mono-0.png' % cam),
                     osp.join(root, 'iseg', scenario, 'iseg-w=0-f=0-l=0-c=original-cam_%d-mono-0.map' % cam)):
            with open(path, 'wb') as f:
                f.write(b'never read')
    for mode in S.MODES:
        with open(osp.join(root, 'splits', 'default', mode + '.txt'), 'w') as f:
            f.write(scenario + '\n')
    cfg = dict(data_folder=root, split_name='default', img_size=64, shuffle_test=False, num_workers=2, load_instances=True,
               copy_to_tmp=False, batch_size=2, seed=1)
    wrapped = _both_ways(S.load, cfg, PngFileLoader, monkeypatch)
    assert [len(w) for w in wrapped] == [2, 2, 2] and all(w.shuffle is None for w in wrapped)


def test_multi_object_config(tmp_path, monkeypatch):
    import genesis_amd.multi_object_config as M
    dst = str(tmp_path) + M.DATASETS['objects_room']['file']
    os.makedirs(osp.dirname(dst))
    shutil.copy(osp.join(GOLDEN, 'multi_object_objects_room.tfrecords'), dst)
    cfg = dict(data_folder=str(tmp_path), dataset='objects_room', img_size=-1, dataset_size=25, num_workers=4, buffer_size=2,
               K_steps=-1, batch_size=4, seed=0, debug=True)
    for shuffle in (True, False):
        load = lambda c, s=shuffle: M.load(c, val_size=6, test_size=5, shuffle=s)    # noqa: E731
        wrapped = _both_ways(load, cfg, M.MultiObjectLoader, monkeypatch)
        assert [len(w) for w in wrapped] == [3, 1, 1] and [w.shuffle for w in wrapped] == [shuffle] * 3


def test_gqn_config(tmp_path, monkeypatch):
    import genesis_amd.gqn_config as Q
    cfg = dict(data_folder=str(tmp_path), img_size=64, val_frac=4, num_workers=2, buffer_size=4, K_steps=7, batch_size=2, seed=0,
               debug=True)
    load = lambda c: Q.load(c, train_files=4, test_files=1, records_per_file=5)      # noqa: E731
    wrapped = _both_ways(load, cfg, Q.GQNLoader, monkeypatch)
    assert [len(w) for w in wrapped] == [7, 2, 5] and [w.batch_size for w in wrapped] == [2, 2, 1]
    assert [w.shuffle for w in wrapped] == [True, False, False]                      # only the train split is shuffled today
