"""The host half of the Multi-dSprites data config and generator (genesis_amd/multid_config.py, generate_multid.py), without
a GPU: the flags and their defaults against the reference's, the file-name rules, every rejection with the names it should
carry, the loader's length, and the generator's draw sequence against the number of random.choice calls the reference made
(tests/golden/multid_generate.npz, written by tests/golden/make_golden_multid.py)."""
import ast
import os
import os.path as osp
import random
import re
import sys

import numpy as np
import pytest

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, HERE)
import make_golden_multid as MG  # noqa: E402

from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

REFERENCE_DEFAULTS = dict(data_folder='data/multi_dsprites/processed', unique_colours=False, load_instances=True, img_size=64,
                          num_workers=4, mem_map=False, K_steps=5)


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    """A data config registers its flags when it is first imported, and the first definition of a name keeps its default:
    importing this config here must not decide the defaults the other data configs' tests see later in the same process."""
    from genesis_amd import compat
    compat.install()
    from forge import flags
    saved = dict(flags.FLAGS)
    yield
    flags.FLAGS.clear()
    flags.FLAGS.update(saved)


def _fresh_flags(module_name):
    """The flags a config registers when it is imported into an empty table."""
    import importlib
    from forge import flags
    flags.FLAGS.clear()
    sys.modules.pop(module_name, None)
    importlib.import_module(module_name)
    return dict(flags.FLAGS)


def reference_flag_definitions():
    """The flags.DEFINE_* calls of the reference's datasets/multid_config.py, read from its source (importing it needs
    torchvision), or None when the reference tree is not there."""
    path = osp.join(MG.REFERENCE_ROOT, 'datasets', 'multid_config.py')
    if not osp.exists(path):
        return None
    found = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith('DEFINE_'):
            found[ast.literal_eval(node.args[0])] = ast.literal_eval(node.args[1])
    return found


def test_live_against_reference_import():
    """The registered flags and defaults against the reference's own definitions when the reference tree is present, else
    against the same values as literals."""
    want = reference_flag_definitions()
    if want is None:
        want = REFERENCE_DEFAULTS
    assert want == REFERENCE_DEFAULTS
    got = _fresh_flags('genesis_amd.multid_config')
    assert got == want
    assert [type(got[k]) for k in sorted(got)] == [type(want[k]) for k in sorted(want)]


def test_file_names():
    import genesis_amd.multid_config as M
    assert [M.file_name(m, False) for m in M.MODES] == ['training_images_rand4.npy', 'validation_images_rand4.npy',
                                                        'test_images_rand4.npy']
    assert [M.file_name(m, True) for m in M.MODES] == ['training_images_rand4_unique.npy', 'validation_images_rand4_unique.npy',
                                                       'test_images_rand4_unique.npy']
    assert M.mask_path('d/training_images_rand4_unique.npy') == 'd/training_masks_rand4_unique.npy'
    assert M.mask_path('d/test_images_rand4.npy') == 'd/test_masks_rand4.npy'
    with pytest.raises(ValueError):
        M.file_name('valid', False)
    path = osp.join(MG.REFERENCE_ROOT, 'datasets', 'multid_config.py')
    if osp.exists(path):                                 # every name is spelled out in the reference's source
        text = open(path).read()
        for unique in (False, True):
            for m in M.MODES:
                assert "'%s'" % M.file_name(m, unique) in text


def write_split(folder, n, image_dtype='float32', mask_dtype='float64', mode='training', unique=False, masks_n=None,
                image_shape=None, mask_shape=None):
    import genesis_amd.multid_config as M
    path = osp.join(str(folder), M.file_name(mode, unique))
    np.save(path, np.zeros(image_shape or (n, 8, 8, 3), dtype=image_dtype))
    if mask_dtype is not None:
        np.save(M.mask_path(path), np.zeros(mask_shape or (masks_n or n, 8, 8, 1), dtype=mask_dtype))
    return path


def cfg_for(folder, **over):
    return AttrDict(dict(dict(data_folder=str(folder), unique_colours=False, load_instances=True, img_size=8, num_workers=4,
                              mem_map=True, K_steps=5, batch_size=8, seed=3, debug=True), **over))


def test_every_rejection_names_the_file_the_dtype_and_the_shape(tmp_path):
    import genesis_amd.multid_config as M
    for i, (kw, words) in enumerate((
            (dict(image_dtype='float64'), ('training_images_rand4.npy', 'float64', r'\[5, 8, 8, 3\]', 'float32')),
            (dict(image_dtype='int32'), ('training_images_rand4.npy', 'int32', r'\[5, 8, 8, 3\]')),
            (dict(image_shape=(5, 8, 8, 4)), ('training_images_rand4.npy', 'float32', r'\[5, 8, 8, 4\]', r'\[N,H,W,3\]')),
            (dict(image_shape=(5, 8, 8)), ('training_images_rand4.npy', 'float32', r'\[5, 8, 8\]', r'\[N,H,W,3\]')),
            (dict(mask_dtype='float16'), ('training_masks_rand4.npy', 'float16', r'\[5, 8, 8, 1\]', 'float64')),
            (dict(mask_dtype='bool'), ('training_masks_rand4.npy', 'bool', r'\[5, 8, 8, 1\]')),
            (dict(mask_shape=(5, 8, 8, 2)), ('training_masks_rand4.npy', 'float64', r'\[5, 8, 8, 2\]')),
            (dict(mask_shape=(5, 8, 4, 1)), ('training_masks_rand4.npy', 'float64', r'\[5, 8, 4, 1\]', '8 x 8')),
            (dict(masks_n=4), ('training_images_rand4.npy', '5 frames', 'training_masks_rand4.npy', '4 masks')))):
        folder = tmp_path / ('case%d' % i)
        folder.mkdir()
        path = write_split(folder, 5, **kw)
        with pytest.raises(GenesisHipError) as e:
            M.open_split(path)
        for w in words:
            assert re.search(w, str(e.value)), (w, str(e.value))
        for mode in M.MODES[1:]:
            write_split(folder, 5, mode=mode)
        with pytest.raises(GenesisHipError):             # the same through load(), whatever the mode
            M.load(cfg_for(folder))
    with pytest.raises(GenesisHipError, match='does not exist'):
        M.load(cfg_for(tmp_path / 'nowhere'))
    good = tmp_path / 'good'
    good.mkdir()
    path = write_split(good, 5)
    with pytest.raises(GenesisHipError, match='shard'):
        M.MultidLoader(path, 8, mem_map=True, shard=(2, 2))
    with pytest.raises(GenesisHipError, match='no CPU path'):
        M.MultidLoader(path, 8, mem_map=True, device='cpu')
    with pytest.raises(GenesisHipError, match='outside the 5 rows'):
        M.check_order(np.array([0, 5, 1]), 5)
    with pytest.raises(GenesisHipError, match='outside the 5 rows'):
        M.check_order(np.array([0, -1]), 5)
    M.check_order(np.array([4, 0]), 5)


@pytest.mark.parametrize('image_dtype', ['float32', 'uint8'])
@pytest.mark.parametrize('mask_dtype', ['uint8', 'int32', 'int64', 'float32', 'float64'])
def test_accepted_dtypes_open(tmp_path, image_dtype, mask_dtype):
    import genesis_amd.multid_config as M
    path = write_split(tmp_path, 5, image_dtype=image_dtype, mask_dtype=mask_dtype, mask_shape=(5, 8, 8) if mask_dtype == 'int32' else None)
    frames, masks = M.open_split(path)
    assert frames.shape == (5, 8, 8, 3) and masks.shape == (5, 8, 8) and masks.dtype == mask_dtype
    assert M.open_split(path, load_instances=False)[1] is None


def test_loader_lengths_and_unique_file_choice(tmp_path):
    import genesis_amd.multid_config as M
    for mode, n in zip(M.MODES, (37, 16, 1)):
        write_split(tmp_path, n, mode=mode)
        write_split(tmp_path, n + 1, mode=mode, unique=True)
    train, val, test = M.load(cfg_for(tmp_path))
    assert (len(train), len(val), len(test)) == (5, 2, 1) and train.batch_size == val.batch_size == test.batch_size == 8
    assert (train.num_frames, val.num_frames, test.num_frames) == (37, 16, 1)
    train, val, test = M.load(cfg_for(tmp_path, unique_colours=True, batch_size=19))
    assert (train.num_frames, val.num_frames, test.num_frames) == (38, 17, 2) and (len(train), len(val), len(test)) == (2, 1, 1)
    assert train.path.endswith('training_images_rand4_unique.npy')
    cfg = cfg_for(tmp_path)
    del cfg['unique_colours']                            # the reference tolerates a cfg without it (:55-56)
    assert M.load(cfg)[0].num_frames == 37
    mine = M.load(cfg_for(tmp_path), shard=(1, 3))[0]
    assert mine.rows.tolist() == list(range(1, 37, 3)) and len(mine) == 2
    assert M.load(cfg_for(tmp_path, load_instances=False))[0].masks is None


def test_narrowing_is_checked():
    import genesis_amd.multid_config as M
    labels = np.arange(5, dtype=np.float64).reshape(1, 5, 1)
    assert M.narrow_uint8(labels).dtype == np.uint8 and M.narrow_uint8(labels).ravel().tolist() == [0, 1, 2, 3, 4]
    for bad in (2.5, -1.0, 256.0, float('nan')):
        spoiled = labels.copy()
        spoiled[0, 2, 0] = bad
        assert M.narrow_uint8(spoiled) is None
    assert M.narrow_uint8(np.array([[[300]]], dtype=np.int64)) is None
    assert M.narrow_uint8(np.array([[[255]]], dtype=np.int32)).tolist() == [[[255]]]


def test_draws_consume_the_reference_stream(monkeypatch):
    """One stream for the three runs, as the fixture was made: every run makes the recorded number of random.choice calls,
    and what it draws is what the reference's images show."""
    import genesis_amd.generate_multid as G
    golden = np.load(MG.NPZ)
    calls = [0]
    real = random.choice

    def counting(seq):
        calls[0] += 1
        return real(seq)

    monkeypatch.setattr(random, 'choice', counting)
    random.seed(MG.SEED)
    for name, n, num_objects, unique, want in MG.RUNS:
        calls[0] = 0
        count, indices, colours = G.draw(n, num_objects, unique)
        assert calls[0] == want == int(golden[name + '_choices']), name
        images, masks = golden[name + '_images'], golden[name + '_masks']
        assert count.tolist() == [int(m.max()) for m in masks]          # the last sprite pasted is never hidden
        assert len(indices) == int(count.sum()) and all(0 <= i <= G.MAX_SPRITE_INDEX for i in indices)
        assert set(np.unique(colours).tolist()) <= set(G.COLOUR_VALUES)
        for i in range(n):                               # every visible label shows its drawn colour, 0 the background's
            for label in range(count[i] + 1):
                seen = images[i][masks[i] == label]
                assert (seen == colours[i, label]).all()
            if unique:
                used = [tuple(c) for c in colours[i, :count[i] + 1].tolist()]
                assert len(set(used)) == len(used)
        if name == 'unique48':
            assert want // 3 - n - len(indices) == MG.UNIQUE_REDRAWS and set(count.tolist()) == {1, 2, 3, 4}


def test_generator_rejections(tmp_path):
    import genesis_amd.generate_multid as G
    with pytest.raises(FileNotFoundError, match='no_such_sprites.npz'):
        G.main(['--sprites', str(tmp_path / 'no_such_sprites.npz'), '--out', str(tmp_path)])
    sprites = np.zeros((3, 64, 64), dtype=np.uint8)
    with pytest.raises(GenesisHipError, match='num_objects'):
        G.generate(sprites, 2, num_objects=5)
    with pytest.raises(GenesisHipError, match='64 x 64'):
        G.generate(np.zeros((3, 32, 32), dtype=np.uint8), 2)
    with pytest.raises(GenesisHipError, match='no CPU path'):
        G.generate(sprites, 2, device='cpu')
    assert (G.MAX_SPRITE_INDEX, G.COLOUR_VALUES, [n for _, n in G.SPLITS]) == (737279, [0, 63, 127, 191, 255], [50000, 10000, 10000])
