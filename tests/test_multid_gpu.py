"""Multi-dSprites on the device (genesis_amd/multid_config.py, generate_multid.py; gx_multid.hip).  The gather kernels against
the torch ops the reference's dataset applies on the host (datasets/multid_config.py:131-143: HWC -> CHW, uint8 / 255 or float
unchanged, F.interpolate(size), .type(LongTensor)), the loaders of both modes against the rows their `order` names, and the
generator against the reference's own output on the procedural sprite bank (tests/golden/multid_generate.npz).  Everything at
zero tolerance: the kernels copy, divide one byte by 255 in fp32, or convert an exactly held label."""
import os.path as osp
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.join(HERE, 'golden'))
sys.path.insert(0, HERE)
import make_golden_multid as MG  # noqa: E402
import multid_bank  # noqa: E402

from genesis_amd import feeder  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

pytestmark = pytest.mark.gpu

N, STORED, BATCH = 37, 64, 8
SIZES = (64, 32, 96, 50)
LABEL_DTYPES = ('uint8', 'int32', 'int64', 'float32', 'float64')


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    from genesis_amd import compat
    compat.install()
    from forge import flags
    saved = dict(flags.FLAGS)
    yield
    flags.FLAGS.clear()
    flags.FLAGS.update(saved)


@pytest.fixture(scope='module')
def split():
    """One stored split: uint8 frames, the float32 frames the generator would store for them, label maps 0..4."""
    rng = np.random.RandomState(11)
    u8 = rng.randint(0, 256, size=(N, STORED, STORED, 3)).astype(np.uint8)
    labels = rng.randint(0, 5, size=(N, STORED, STORED)).astype(np.uint8)
    return {'uint8': u8, 'float32': u8.astype(np.float32) / 255.0, 'labels': labels}


def expected_frames(stored_rows, size):
    """What dSpritesDataset.__getitem__ makes of stored rows [B,H,W,3] (uint8 or float32), batched."""
    x = torch.from_numpy(np.ascontiguousarray(stored_rows)).permute(0, 3, 1, 2).contiguous()
    if x.dtype == torch.uint8:
        x = x.to(torch.float32).div(255)
    if size != x.shape[2]:
        x = F.interpolate(x, size=size)
    return x


def expected_labels(stored_rows, size):
    x = torch.from_numpy(np.ascontiguousarray(stored_rows))[:, None].double()
    if size != x.shape[2]:
        x = F.interpolate(x, size=size)
    return x.type(torch.LongTensor)


def same(got, want):
    torch.cuda.synchronize()
    got = got.cpu()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)


REPEATS = [5, 5, 36, 0, 5, 36, 17, 0]                 # an index vector need not be a permutation


@pytest.mark.parametrize('size', SIZES)
@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_rows_gather_equals_torch(split, dtype, size):
    src = torch.from_numpy(split[dtype]).cuda()
    perm = np.random.RandomState(3).permutation(N)
    idx = torch.from_numpy(perm).cuda()
    for first, B in ((0, BATCH), (32, 5)):                                   # a full batch, and the short tail of an epoch
        assert same(feeder.rows_gather(src, idx, first, B, size), expected_frames(split[dtype][perm[first:first + B]], size))
        assert same(feeder.rows_gather(src, None, first, B, size), expected_frames(split[dtype][first:first + B], size))
    rows = REPEATS
    rep = torch.tensor([0] * 3 + rows, dtype=torch.int64).cuda()
    assert same(feeder.rows_gather(src, rep, 3, len(rows), size), expected_frames(split[dtype][rows], size))
    assert same(feeder.rows_gather(src, None, 0, None, size), expected_frames(split[dtype], size))    # all 37 rows: B defaults
    out = torch.full((5, 3, size, size), -1.0, device='cuda')
    assert feeder.rows_gather(src, idx, 32, 5, size, out=out) is out and same(out, expected_frames(split[dtype][perm[32:]], size))


@pytest.mark.parametrize('dtype', LABEL_DTYPES)
def test_rows_gather_labels_equals_torch(split, dtype):
    stored = split['labels'].astype(dtype)
    src = torch.from_numpy(stored).cuda()
    perm = np.random.RandomState(4).permutation(N)
    idx = torch.from_numpy(perm).cuda()
    for size in SIZES:
        for first, B in ((0, BATCH), (32, 5)):
            assert same(feeder.rows_gather_labels(src, idx, first, B, size), expected_labels(stored[perm[first:first + B]], size))
            assert same(feeder.rows_gather_labels(src, None, first, B, size), expected_labels(stored[first:first + B], size))
        rows = REPEATS
        rep = torch.tensor(rows, dtype=torch.int64).cuda()
        assert same(feeder.rows_gather_labels(src, rep, 0, len(rows), size), expected_labels(stored[rows], size))
    with_axis = torch.from_numpy(stored[..., None]).cuda()                  # [N,H,W,1], as the files store them
    assert same(feeder.rows_gather_labels(with_axis, idx, 0, BATCH, 50), expected_labels(stored[perm[:BATCH]], 50))


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'int32', 'int64'])
def test_labels_convert_by_truncation(dtype):
    values = [-2.75, -1.0, -0.5, 0.0, 0.5, 1.999, 2.0, 254.5, 255.0, 256.0, 70000.25, 1e6]
    if dtype.startswith('int'):
        values = [-3, -1, 0, 1, 255, 256, 70000, 2 ** 24]
    stored = np.resize(np.array(values, dtype=dtype), (3, 5, 7))
    got = feeder.rows_gather_labels(torch.from_numpy(stored).cuda(), None, 0, 3, (10, 4))
    want = F.interpolate(torch.from_numpy(stored)[:, None].double(), size=(10, 4)).type(torch.LongTensor)
    assert same(got, want)


def test_other_channel_counts_and_rejections(split):
    rng = np.random.RandomState(5)
    for C in (1, 4):
        u8 = rng.randint(0, 256, size=(3, 9, 13, C)).astype(np.uint8)
        want = F.interpolate(torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255), size=(7, 20))
        assert same(feeder.rows_gather(torch.from_numpy(u8).cuda(), None, 0, 3, (7, 20)), want)
    src = torch.from_numpy(split['uint8']).cuda()
    idx = torch.arange(N, device='cuda')
    with pytest.raises(GenesisHipError, match='reach outside the 37 indices'):
        feeder.rows_gather(src, idx, 32, 8)
    with pytest.raises(GenesisHipError, match='reach outside the 37 rows'):
        feeder.rows_gather(src, None, 32, 8)
    with pytest.raises(GenesisHipError, match='int64'):
        feeder.rows_gather(src, idx.int(), 0, 8)
    with pytest.raises(GenesisHipError, match='no CPU path'):
        feeder.rows_gather(src.cpu(), None, 0, 8)
    with pytest.raises(GenesisHipError, match='uint8 or float32'):
        feeder.rows_gather(src.double(), None, 0, 8)
    with pytest.raises(GenesisHipError, match='label maps'):
        feeder.rows_gather_labels(src.half()[..., 0], None, 0, 8)


# ---- the loaders
def loader_cfg(folder, **over):
    return AttrDict(dict(dict(data_folder=str(folder), unique_colours=False, load_instances=True, img_size=64, num_workers=4,
                              mem_map=False, K_steps=5, batch_size=BATCH, seed=7, debug=True), **over))


@pytest.fixture(scope='module')
def folder(tmp_path_factory, split):
    """training: float32 frames and float64 masks [N,64,64,1] as the generator stores them; validation: uint8 frames and int64
    masks with one label that no uint8 holds; test: 5 uint8 frames with float32 masks [N,64,64]."""
    import genesis_amd.multid_config as M
    d = tmp_path_factory.mktemp('multid')
    files = {}
    wide = split['labels'][:16].astype(np.int64)
    wide[3, 10, 10] = 300
    for mode, frames, masks in (('training', split['float32'], split['labels'].astype(np.float64)[..., None]),
                                ('validation', split['uint8'][:16], wide[..., None]),
                                ('test', split['uint8'][:5], split['labels'][:5].astype(np.float32))):
        path = osp.join(str(d), M.file_name(mode, False))
        np.save(path, frames)
        np.save(M.mask_path(path), masks)
        files[mode] = (frames, masks.reshape(masks.shape[:3]))
    return str(d), files


def check_epoch(loader, frames, masks, size, rows):
    batches = list(loader)
    order = loader.order
    assert sorted(order.tolist()) == sorted(rows) and len(batches) == len(loader) == -(-len(rows) // loader.batch_size)
    for i, b in enumerate(batches):
        take = order[i * loader.batch_size:(i + 1) * loader.batch_size]
        assert b['input'].is_cuda and same(b['input'], expected_frames(frames[take], size))
        if masks is None:
            assert set(b) == {'input'}
        else:
            assert set(b) == {'input', 'instances'} and same(b['instances'], expected_labels(masks[take], size))
    with pytest.raises(StopIteration):
        next(loader)
    return order.copy()


@pytest.mark.parametrize('mem_map', [False, True], ids=['resident', 'mem_map'])
def test_loaders_deliver_the_rows_of_their_order(folder, mem_map):
    import genesis_amd.multid_config as M
    d, files = folder
    train, val, test = M.load(loader_cfg(d, mem_map=mem_map))
    assert (len(train), len(val), len(test)) == (5, 2, 1) and train.batch_size == BATCH
    first = check_epoch(train, *files['training'], 64, range(N))
    second = check_epoch(train, *files['training'], 64, range(N))           # iterated again: a fresh permutation
    assert first.tolist() != second.tolist()
    check_epoch(val, *files['validation'], 64, range(16))
    check_epoch(test, *files['test'], 64, range(5))
    if not mem_map:                                                          # narrowed where every label fits, and only there
        assert train.dev_frames.dtype == torch.float32 and train.dev_masks.dtype == torch.uint8
        assert val.dev_frames.dtype == torch.uint8 and val.dev_masks.dtype == torch.int64
        assert test.dev_masks.dtype == torch.uint8
    again = M.load(loader_cfg(d, mem_map=mem_map))[0]                        # the order is a function of cfg.seed
    assert list(iter(again).order) == first.tolist()
    other = M.load(loader_cfg(d, mem_map=mem_map, seed=8))[0]
    assert list(iter(other).order) != first.tolist()
    half = iter(train)                                                       # an epoch abandoned half way, then a whole one
    next(half)
    check_epoch(train, *files['training'], 64, range(N))


@pytest.mark.parametrize('mem_map', [False, True], ids=['resident', 'mem_map'])
def test_shard_resize_and_no_instances(folder, mem_map):
    import genesis_amd.multid_config as M
    d, files = folder
    train, val, _ = M.load(loader_cfg(d, mem_map=mem_map, img_size=50, batch_size=5), shard=(1, 3))
    assert train.num_frames == 12 and len(train) == 3
    check_epoch(train, *files['training'], 50, range(1, N, 3))
    check_epoch(val, *files['validation'], 50, range(1, 16, 3))
    train = M.load(loader_cfg(d, mem_map=mem_map, img_size=32, load_instances=False))[0]
    assert train.masks is None
    check_epoch(train, files['training'][0], None, 32, range(N))


def test_mem_map_ring_comes_round_and_survives_an_abandoned_epoch(folder):
    """13 batches through the RING_DEPTH slots of the host-memmap mode: every slot is refilled; then an epoch left after one
    batch (with the next one staged), then a whole one."""
    import genesis_amd.multid_config as M
    d, files = folder
    train = M.load(loader_cfg(d, mem_map=True, batch_size=3))[0]
    assert len(train) == 13 > M.RING_DEPTH
    check_epoch(train, *files['training'], 64, range(N))
    half = iter(train)
    abandoned = half.order.copy()
    next(half)
    full = check_epoch(train, *files['training'], 64, range(N))
    assert full.tolist() != abandoned.tolist()


def test_a_loader_batch_through_the_model(folder):
    import genesis_amd.genesisv2_config as G
    import genesis_amd.multid_config as M
    from oracle import v2_oracle as O
    batch = next(iter(M.load(loader_cfg(folder[0], batch_size=4))[0]))
    assert tuple(batch['input'].shape) == (4, 3, 64, 64) and tuple(batch['instances'].shape) == (4, 1, 64, 64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(O.make_cfg(K_steps=3, img_size=64, feat_dim=16), debug=False, multi_gpu=False))).to('cuda:0').train()
    recon, losses, stats, _, _ = model(batch['input'])
    torch.cuda.synchronize()
    assert torch.isfinite(recon).all() and torch.isfinite(losses.err).all()
    assert all(torch.isfinite(k).all() for k in losses.kl_l_k)


# ---- the generator
def test_generate_reproduces_the_reference_bit_for_bit():
    import genesis_amd.generate_multid as G
    golden = np.load(MG.NPZ)
    bank = multid_bank.SpriteBank()
    random.seed(MG.SEED)
    for name, n, num_objects, unique, _ in MG.RUNS:                          # one stream, as the fixture was made
        images, masks = G.generate(bank, n, num_objects=num_objects, unique=unique)
        assert images.dtype == np.float32 and images.shape == (n, 64, 64, 3)
        assert masks.dtype == np.float64 and masks.shape == (n, 64, 64, 1)
        assert np.array_equal(images, golden[name + '_images'].astype('float32') / 255.0), name
        assert np.array_equal(masks[..., 0], golden[name + '_masks'].astype(np.float64)), name


def test_compose_in_chunks_and_from_an_array(monkeypatch):
    """A chunk size that does not divide the run and an ndarray of sprites (fancy-indexed) give the same images."""
    import genesis_amd.generate_multid as G
    sprites = multid_bank.first_sprites(48)
    monkeypatch.setattr(G, 'MAX_SPRITE_INDEX', 47)
    random.seed(5)
    whole = G.generate(sprites, 23, unique=True)
    monkeypatch.setattr(G, 'CHUNK', 7)
    random.seed(5)
    pieces = G.generate(sprites.astype(bool), 23, unique=True)
    assert np.array_equal(whole[0], pieces[0]) and np.array_equal(whole[1], pieces[1])
    random.seed(5)
    count, indices, colours = G.draw(23, None, True)
    k = 0
    for i in range(23):                                                      # the reference's loop, restated in numpy
        img = np.broadcast_to(colours[i, 0], (64, 64, 3)).copy()
        lab = np.zeros((64, 64))
        for o in range(count[i]):
            where = sprites[indices[k]] != 0
            img[where], lab[where] = colours[i, o + 1], o + 1
            k += 1
        assert np.array_equal(whole[0][i], img.astype('float32') / 255.0) and np.array_equal(whole[1][i, :, :, 0], lab)
    empty = G.generate(sprites, 3, num_objects=0)
    assert not empty[1].any() and (empty[0][:, :1, :1] == empty[0]).all()


def test_main_writes_the_files_the_config_reads(tmp_path, monkeypatch):
    import genesis_amd.generate_multid as G
    import genesis_amd.multid_config as M
    sprites = multid_bank.first_sprites(64)
    np.savez(str(tmp_path / 'sprites.npz'), imgs=sprites)
    monkeypatch.setattr(G, 'MAX_SPRITE_INDEX', 63)
    out = tmp_path / 'processed'
    G.main(['--sprites', str(tmp_path / 'sprites.npz'), '--out', str(out), '--sizes', '21', '9', '6'])
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted('%s_%s_rand4%s.npy' % (m, kind, u) for m in M.MODES for kind in ('images', 'masks') for u in ('', '_unique'))
    random.seed(0)                                                           # main's stream: seed 0, rand4 splits first
    first = G.generate(sprites, 21)
    stored = np.load(str(out / 'training_images_rand4.npy')), np.load(str(out / 'training_masks_rand4.npy'))
    assert stored[0].dtype == np.float32 and stored[1].dtype == np.float64 and stored[1].shape == (21, 64, 64, 1)
    assert np.array_equal(stored[0], first[0]) and np.array_equal(stored[1], first[1])
    for unique in (False, True):
        loaders = M.load(loader_cfg(out, unique_colours=unique))
        assert [l.num_frames for l in loaders] == [21, 9, 6]
        for loader, mode in zip(loaders, M.MODES):
            suffix = '_rand4_unique.npy' if unique else '_rand4.npy'
            frames, masks = np.load(str(out / (mode + '_images' + suffix))), np.load(str(out / (mode + '_masks' + suffix)))
            assert loader.dev_masks.dtype == torch.uint8 and 1 <= masks.max() <= 4
            check_epoch(loader, frames, masks[..., 0], 64, range(len(frames)))
