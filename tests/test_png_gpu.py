"""The device half of the PNG decoder (gx_png_unfilter through genesis_amd/png.py) against Pillow's bytes
(tests/golden/png_pil.npz) at zero tolerance, and the ShapeStacks and Sketchy data configs on small trees written in
tmp_path from the same streams: shapes, the short last batch, epochs, shards, labels under both rules, a corrupt file.
Everything here is integer arithmetic or one exact division, so the bar is equality."""
import os
import os.path as osp
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_png as MG  # noqa: E402

from genesis_amd import feeder, png  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    """A data config registers its flags when it is first imported, and the first definition of a name keeps its default:
    importing the PNG configs here must not decide the defaults the other data configs' tests see later in the same process."""
    from genesis_amd import compat
    compat.install()
    from forge import flags
    saved = dict(flags.FLAGS)
    yield
    flags.FLAGS.clear()
    flags.FLAGS.update(saved)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(MG.NPZ))


def exact_f32(u8):
    """uint8 [.., H, W, C] -> fp32 [.., C, H, W] = u8 / 255 (true division, ToTensor)."""
    t = torch.from_numpy(np.ascontiguousarray(u8)).float() / 255.0
    return t.movedim(-1, -3).contiguous()


@pytest.mark.parametrize('name', MG.GOOD_NAMES)
def test_kernel_equals_pillow_bit_for_bit(golden, name):
    """Every good fixture, one at a time: all five filters on every row (the first included) for C = 1, 3, 4, one column, one
    row, a width past the wave size, heights of exactly one band and one row past it, several IDAT chunks, Pillow's own
    adaptive filter choice."""
    want = golden[name + '_u8']
    x, u8 = png.decode_png_batch([golden[name + '_png']], return_u8=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1,) + want.shape
    assert int((u8[0].cpu().numpy() != want).sum()) == 0
    assert x.dtype == torch.float32 and tuple(x.shape) == (1, want.shape[2]) + want.shape[:2]
    assert torch.equal(x[0].cpu(), exact_f32(want))


@pytest.mark.parametrize('C', [1, 3, 4])
def test_batches_of_one_geometry_with_different_filters(golden, C):
    names = ['f%d_c%d_5x3' % (f, C) for f in range(5)]
    x, u8 = png.decode_png_batch([bytes(golden[n + '_png']) for n in names], return_u8=True)
    want = np.stack([golden[n + '_u8'] for n in names])
    assert np.array_equal(u8.cpu().numpy(), want) and torch.equal(x.cpu(), exact_f32(want))
    many = [names[(3 * i) % 5] for i in range(33)]
    out = torch.full((33, C, 3, 5), -1.0, device='cuda')
    got = png.decode_png_batch([golden[n + '_png'] for n in many], out=out)
    assert got is out and torch.equal(out.cpu(), exact_f32(np.stack([golden[n + '_u8'] for n in many])))


def test_a_batch_of_large_frames(golden):
    names = ['pil_smooth224'] * 3
    x, u8 = png.decode_png_batch([golden[n + '_png'] for n in names], return_u8=True)
    want = np.stack([golden[n + '_u8'] for n in names])
    assert np.array_equal(u8.cpu().numpy(), want) and torch.equal(x.cpu(), exact_f32(want))


@pytest.mark.parametrize('C,W', [(3, 3), (3, 67), (4, 67), (1, 9)])
def test_batches_of_different_frames_that_cross_a_band(C, W):
    """Three DIFFERENT frames of one geometry, one row taller than a band and (W = 67, 9) wider than the kernel's prefetch
    chunk, each with its own filter pattern: per-frame offsets and the hand-over row between bands.  The streams are
    assembled here (MG.assemble, whose output the fixture checks against Pillow), so the expected bytes are the images."""
    H = MG.BAND[C] + 1
    imgs = [MG.content_image('noise', H, W, C, 7300 + 10 * C + k) for k in range(3)]
    streams = [MG.assemble(img, [(r + 2 * k) % 5 for r in range(H)]) for k, img in enumerate(imgs)]
    x, u8 = png.decode_png_batch(streams, return_u8=True)
    want = np.stack(imgs)
    assert np.array_equal(u8.cpu().numpy(), want) and torch.equal(x.cpu(), exact_f32(want))
    labels = png.decode_png_labels(streams, 'byte')                  # the plane alone: no byte output to read back
    assert np.array_equal(labels.cpu().numpy()[:, 0], want[..., 0].astype(np.int64))


def test_plane_rules_without_the_byte_output(golden):
    """dst_plane0 alone (dst_u8 NULL), on a frame of two bands: the hand-over between bands does not go through dst_u8."""
    for name in ('band_c4_3x257', 'cycle_c3_67x9', 'cycle_c1_67x9'):
        want = golden[name + '_u8'][:, :, 0]
        for rule, expected in (('byte', want), ('index', want >> 5), ('shapestacks_reference', np.zeros_like(want))):
            got = png.decode_png_labels([golden[name + '_png']] * 2, rule)
            assert got.dtype == torch.int64 and tuple(got.shape) == (2, 1) + want.shape
            assert np.array_equal(got.cpu().numpy(), np.stack([expected[None]] * 2).astype(np.int64))


def test_arguments_are_checked(golden):
    a, b = golden['f1_c3_5x3_png'], golden['cycle_c3_67x9_png']
    with pytest.raises(GenesisHipError, match='mixed geometries'):
        png.decode_png_batch([a, b])
    with pytest.raises(GenesisHipError, match='mixed geometries'):
        png.decode_png_batch([a, golden['f1_c4_5x3_png']])
    with pytest.raises(GenesisHipError, match='out must be'):
        png.decode_png_batch([a], out=torch.empty(1, 3, 5, 3, device='cuda'))
    with pytest.raises(GenesisHipError, match='HIP device'):
        png.decode_png_batch([a], out=torch.empty(1, 3, 3, 5))
    with pytest.raises(GenesisHipError, match='Adam7'):
        png.decode_png_batch([golden['broken_interlaced_png']])
    with pytest.raises(GenesisHipError, match='CRC mismatch'):
        png.decode_png_batch([a, golden['broken_crc_png']])
    with pytest.raises(GenesisHipError, match='empty batch'):
        png.decode_png_batch([])


# ---- the ShapeStacks transform and labels
BOX = (14, 14, 196, 196)


@pytest.mark.parametrize('S', MG.SS_SIZES)
def test_shapestacks_frames_equal_pillow_crop_and_resize(golden, S):
    got = png.decode_png_batch([golden[MG.SS_FRAME + '_png']] * 2, size=S, crop=feeder.centre_box(224, 224, 196), resize='bilinear')
    assert feeder.centre_box(224, 224, 196) == BOX
    want = exact_f32(golden['ss_rgb%d' % S])
    assert tuple(got.shape) == (2, 3, S, S) and torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want)


@pytest.mark.parametrize('S', MG.SS_SIZES)
def test_shapestacks_labels_under_both_rules(golden, S):
    maps = [golden['ss_map_png']] * 2
    ref = png.decode_png_labels(maps, 'shapestacks_reference', size=S, crop=BOX)
    want = torch.from_numpy(golden['ss_labels_ref%d' % S])
    assert ref.dtype == torch.int64 and tuple(ref.shape) == (2, 1, S, S)
    assert int(ref.abs().max()) == 0 and torch.equal(ref[0].cpu(), want) and torch.equal(ref[1].cpu(), want)
    index = png.decode_png_labels(maps, 'index', size=S, crop=BOX)
    want = torch.from_numpy(golden['ss_labels_index%d' % S].astype(np.int64))
    assert torch.equal(index[0].cpu(), want) and torch.equal(index[1].cpu(), want)
    assert sorted(set(index.cpu().numpy().ravel().tolist())) == list(range(8))


# ---- the ShapeStacks data config on a small tree: 2 scenarios x 3 cameras
SCENARIOS = ['env_ccs-hard-h=2-vcom=0-vpsf=0-v=60', 'env_blocks-easy-h=3-vcom=1-vpsf=0-v=7']
CAMS = (1, 7, 12)


def tinted(frame, k):
    """Frame k of the tree: the fixture frame with a short stroke inside the crop window, a different one per frame."""
    img = frame.copy()
    img[100 + k, 100:108] = 40 * k
    return img


def write_tree(root, golden, frames=None):
    base = golden[MG.SS_FRAME + '_u8']
    rows = MG.row_filters(224, MG.CYCLE)
    k = 0
    for sc in SCENARIOS:
        os.makedirs(osp.join(root, 'recordings', sc))
        os.makedirs(osp.join(root, 'iseg', sc))
        for cam in CAMS:
            with open(osp.join(root, 'recordings', sc, 'rgb-w=5-f=2-l=1-c=unique-cam_%d-mono-0.png' % cam), 'wb') as f:
                f.write(MG.assemble(tinted(base, k), [(r + k) % 5 for r in rows]))
            with open(osp.join(root, 'iseg', sc, 'iseg-w=0-f=0-l=0-c=original-cam_%d-mono-0.map' % cam), 'wb') as f:
                f.write(golden['ss_map_png'].tobytes())
            k += 1
    os.makedirs(osp.join(root, 'splits', 'default'))
    for mode, scs in (('train', SCENARIOS), ('eval', SCENARIOS[:1]), ('test', SCENARIOS[1:])):
        with open(osp.join(root, 'splits', 'default', mode + '.txt'), 'w') as f:
            f.write('\n'.join(scs) + '\n')


@pytest.fixture(scope='module')
def tree(tmp_path_factory, golden):
    root = str(tmp_path_factory.mktemp('shapestacks'))
    write_tree(root, golden)
    return root


def ss_cfg(root, **kw):
    cfg = AttrDict(data_folder=root, split_name='default', img_size=64, shuffle_test=False, num_workers=2, load_instances=True,
                   copy_to_tmp=False, K_steps=9, batch_size=4, seed=0, debug=True)
    cfg.update(kw)
    return cfg


def frame_key(x):
    """The bytes of a decoded frame, to look it up among the expected ones."""
    return x.cpu().numpy().tobytes()


def test_shapestacks_loader(tree, golden):
    import genesis_amd.shapestacks_config as S
    train, val, test = S.load(ss_cfg(tree, img_size=196))
    assert [len(l) for l in (train, val, test)] == [2, 1, 1] and [l.batch_size for l in (train, val, test)] == [4, 4, 4]
    base = golden[MG.SS_FRAME + '_u8']
    want = {frame_key(exact_f32(tinted(base, k)[14:210, 14:210])): k for k in range(6)}
    assert len(want) == 6
    epochs = []
    for _ in range(2):
        seen = []
        it = iter(train)
        for expected in (4, 2):                                      # the short last batch ...
            batch = next(it)
            assert sorted(batch) == ['input', 'instances']
            x, m = batch['input'], batch['instances']
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (expected, 3, 196, 196)
            assert m.is_cuda and m.dtype == torch.int64 and tuple(m.shape) == (expected, 1, 196, 196) and int(m.abs().max()) == 0
            seen += [want[frame_key(f)] for f in x]                # KeyError: a frame that is none of the six, bit for bit
        with pytest.raises(StopIteration):                           # ... then the end of the epoch
            next(it)
        epochs.append(seen)
    assert sorted(epochs[0]) == sorted(epochs[1]) == list(range(6)) and epochs[0] != epochs[1]
    assert len(next(train)['input']) == 4                            # the next call starts another epoch
    for l in (train, val, test):
        l.close()
    # in file order, against the one-call path on the same files (each of which is one of the six, bit for bit)
    files = S.frame_files(tree, 'default', 'train')
    maps = [S.map_file(tree, f) for f in files]
    direct = png.decode_png_batch([png.read_file(f) for f in files], crop=BOX)
    direct_maps = png.decode_png_labels([png.read_file(f) for f in maps], 'index', crop=BOX)
    assert sorted(want[frame_key(f)] for f in direct) == list(range(6))
    for depth in (4, 8):                                             # 8: a ring deeper than the epoch's three batches
        loader = png.PngFileLoader(files, 2, crop=196, map_files=maps, label_rule='index', shuffle=False, num_workers=2,
                                   depth=depth)
        assert len(loader) == 3
        assert torch.equal(next(iter(loader))['input'], direct[:2])  # an epoch left half way after one batch ...
        it = iter(loader)                                            # ... and the next one: every file once, in order
        got = [next(it) for _ in range(3)]
        with pytest.raises(StopIteration):
            next(it)
        assert torch.equal(torch.cat([b['input'] for b in got]), direct)
        assert torch.equal(torch.cat([b['instances'] for b in got]), direct_maps)
        loader.close()


def test_shapestacks_loader_resized_sharded_and_without_instances(tree, golden):
    import genesis_amd.shapestacks_config as S
    files = S.frame_files(tree, 'default', 'train')
    train = S.load(ss_cfg(tree), iseg_labels='index', shard=(1, 2))[0]
    assert train.files == files[1::2] and len(train) == 1
    it = iter(train)
    order = [train.files[i] for i in train.order]
    batches = [next(it)]                                             # (list(it) would call iter() again: a new permutation)
    with pytest.raises(StopIteration):
        next(it)
    assert tuple(batches[0]['input'].shape) == (3, 3, 64, 64)
    want = torch.from_numpy(golden['ss_labels_index64'].astype(np.int64))
    for m in batches[0]['instances']:
        assert torch.equal(m.cpu(), want)
    # the frames of this shard, through Pillow-exact crop + bilinear: equal to the one-call path on the same files
    direct = png.decode_png_batch([png.read_file(f) for f in order], size=64, crop=BOX, resize='bilinear')
    assert torch.equal(batches[0]['input'], direct)
    train.close()
    plain = S.load(ss_cfg(tree, load_instances=False, img_size=128))[1]
    got = list(plain)
    assert [sorted(b) for b in got] == [['input']] and tuple(got[0]['input'].shape) == (3, 3, 128, 128)
    plain.close()


def test_a_corrupt_file_and_a_missing_map_name_their_paths(tmp_path, golden):
    import genesis_amd.shapestacks_config as S
    root = str(tmp_path)
    write_tree(root, golden)
    bad = S.frame_files(root, 'default', 'eval')[1]
    data = bytearray(open(bad, 'rb').read())
    data[len(data) // 2] ^= 0x10
    with open(bad, 'wb') as f:
        f.write(bytes(data))
    val = S.load(ss_cfg(root))[1]
    with pytest.raises(GenesisHipError, match=r'(?s)%s.*CRC mismatch' % re.escape(osp.basename(bad))):
        list(val)
    val.close()
    # a bad file in a later batch: the batches before it are delivered, then the error; the loader can be iterated again
    good = [f for f in S.frame_files(root, 'default', 'train') if f != bad]
    loader = png.PngFileLoader(good[:2] + [bad] + good[2:4], 1, shuffle=False, num_workers=2, name='shapestacks')
    it = iter(loader)
    for _ in range(2):
        assert tuple(next(it)['input'].shape) == (1, 3, 224, 224)
    with pytest.raises(GenesisHipError, match=r'(?s)%s.*CRC mismatch' % re.escape(osp.basename(bad))):
        next(it)
    assert tuple(next(loader)['input'].shape) == (1, 3, 224, 224)
    loader.close()
    gone = S.map_file(root, S.frame_files(root, 'default', 'test')[0])
    os.remove(gone)
    test = S.load(ss_cfg(root))[2]
    with pytest.raises(GenesisHipError, match='cam_.*-mono-0.map'):
        list(test)
    test.close()
    assert len(list(S.load(ss_cfg(root, load_instances=False))[2])) == 1


# ---- the Sketchy data config
def test_sketchy_loader(tmp_path, golden):
    import genesis_amd.sketchy_config as K
    root = str(tmp_path)
    base = golden['pil_mixed128_u8']
    for mode, n in (('train', 5), ('valid', 2), ('test', 2)):
        os.makedirs(osp.join(root, 'processed', mode, 'ep0'))
        for i in range(n):
            with open(osp.join(root, 'processed', mode, 'ep0', 'ep0_%d.png' % i), 'wb') as f:
                f.write(golden['pil_mixed128_png'].tobytes() if i == 0 else MG.assemble(np.roll(base, 3 * i, axis=0), [4] * 128))
    cfg = AttrDict(data_folder=root, img_size=128, num_workers=2, K_steps=10, batch_size=4, seed=1, debug=True)
    train, val, test = K.load(cfg)
    assert [len(l) for l in (train, val, test)] == [2, 1, 2] and [l.batch_size for l in (train, val, test)] == [4, 4, 1]
    want = {exact_f32(np.roll(base, 3 * i, axis=0)).numpy().tobytes() for i in range(5)}
    got = list(train)
    assert [tuple(b['input'].shape) for b in got] == [(4, 3, 128, 128), (1, 3, 128, 128)] and sorted(got[0]) == ['input']
    assert {f.cpu().numpy().tobytes() for b in got for f in b['input']} == want
    assert [tuple(b['input'].shape) for b in test] == [(1, 3, 128, 128)] * 2
    assert osp.exists(osp.join(root, 'processed', 'train_images.txt'))
    for l in (train, val, test):
        l.close()


def test_a_loader_batch_through_the_model(tree):
    import genesis_amd.genesisv2_config as G
    import genesis_amd.shapestacks_config as S
    from oracle import v2_oracle as O
    train = S.load(ss_cfg(tree))[0]
    batch = next(iter(train))
    train.close()
    assert tuple(batch['input'].shape) == (4, 3, 64, 64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(O.make_cfg(K_steps=3, img_size=64, feat_dim=16), debug=False, multi_gpu=False))).to('cuda:0').train()
    recon, losses, stats, _, _ = model(batch['input'])
    torch.cuda.synchronize()
    assert torch.isfinite(recon).all() and torch.isfinite(losses.err).all()
    assert all(torch.isfinite(k).all() for k in losses.kl_l_k)
