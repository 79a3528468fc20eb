"""Loose image files on the device (genesis_amd/imagefile.py, image_folder_config.py, gx_imagefile.hip) against Pillow
(tests/golden/imagefile_pil.npz, written by tests/golden/make_golden_imagefile.py) at zero tolerance: every stage is integer
arithmetic, and the final byte / 255 is one correctly rounded fp32 division on both sides.

The kernels' band and tile constants, which the fixture's frames are chosen against:
    gx_jpeg_decode_ragged, blocks -> planes   GX_JPEGR_BLOCKS_PER_WG = 128 blocks of a frame (Y, Cb, Cr in one list) a workgroup:
                                              145 x 131 4:2:0 has 270 + 2 * 90 blocks (four workgroups, the second and third
                                              straddling two planes), 7 x 9 has 6, 1 x 1 has 6 of which one pixel is real
    gx_jpeg_decode_ragged, planes -> pixels   tiles of GX_JPEGR_TILE_H = 16 rows x GX_JPEGR_TILE_W = 64 columns: 145 x 131 spans
                                              3 x 9 tiles, 131 x 145 spans 3 x 10, 2056 x 8 spans 33 x 1, 16 x 520 spans 1 x 33
    gx_png_unfilter_ragged                    bands of 1024 / C rows (1024, 341, 256), one workgroup per frame: 9 x 700 RGBA runs
                                              three bands; a row of 520 RGBA pixels is 2080 bytes of carry
    gx_u8_resample_ragged_f32chw              bands of at most 8 output rows, fewer when the source rows of a band would not fit
                                              32768 bytes of intermediate: S = 20 and S = 64 run three and eight bands, the last
                                              one of four rows at S = 20
Sizes are width x height."""
import os
import os.path as osp
import sys

import numpy as np
import pytest
import torch

HERE = osp.dirname(osp.abspath(__file__))
sys.path.insert(0, osp.join(HERE, 'golden'))
import make_golden_imagefile as MG  # noqa: E402

from genesis_amd import imagefile, jpeg, png  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

pytestmark = pytest.mark.gpu


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
def golden():
    return dict(np.load(MG.NPZ))


def interleaved():
    """All cases, JPEG and PNG alternating while both last."""
    j, p = list(MG.JPEG_NAMES), list(MG.PNG_NAMES)
    out = []
    while j or p:
        if j:
            out.append(j.pop(0))
        if p:
            out.append(p.pop(0))
    return out


def want_f32(golden, name, S):
    return torch.from_numpy(golden['%s_s%d' % (name, S)].astype(np.float32).transpose(2, 0, 1) / np.float32(255.0))


@pytest.fixture(scope='module')
def per_case(golden):
    """Every case decoded on its own, once: {name: (fp32 [3, 64, 64] on the host, uint8 [H, W, C] on the host)}."""
    out = {}
    for name in MG.CASE_NAMES:
        x, u8 = imagefile.decode_image_batch([golden[name + '_stream']], 64, return_u8=True)
        assert x.shape == (1, 3, 64, 64) and x.dtype == torch.float32 and x.is_cuda and len(u8) == 1
        out[name] = (x[0].cpu(), u8[0].cpu())
    return out


@pytest.mark.parametrize('name', MG.CASE_NAMES)
def test_decoded_bytes_equal_pillow(golden, per_case, name):
    want = golden[name + '_u8']
    got = per_case[name][1].numpy()
    assert got.shape == (want.shape + (1,) if want.ndim == 2 else want.shape)
    assert int((got.reshape(want.shape) != want).sum()) == 0


def test_one_ragged_batch_equals_the_per_case_results(golden, per_case):
    names = interleaved()
    assert len(names) == len(MG.CASE_NAMES) and {n[0] for n in names[:4]} == {'j', 'p'}
    x, u8 = imagefile.decode_image_batch([golden[n + '_stream'] for n in names], 64, return_u8=True)
    assert x.shape == (len(names), 3, 64, 64)
    for i, n in enumerate(names):
        assert torch.equal(u8[i].cpu(), per_case[n][1]), n
        assert torch.equal(x[i].cpu(), per_case[n][0]), n
    # 33 frames with repeats, into a caller's tensor
    names33 = [names[(5 * i) % len(names)] for i in range(33)]
    out = torch.full((33, 3, 64, 64), -1.0, device='cuda')
    got = imagefile.decode_image_batch([golden[n + '_stream'] for n in names33], 64, out=out)
    assert got is out
    for i, n in enumerate(names33):
        assert torch.equal(out[i].cpu(), per_case[n][0]), (i, n)


@pytest.mark.parametrize('S', MG.SIZES)
def test_transform_equals_pillow(golden, S):
    names = interleaved()
    x = imagefile.decode_image_batch([golden[n + '_stream'] for n in names], S).cpu()
    for i, n in enumerate(names):
        assert torch.equal(x[i], want_f32(golden, n, S)), (n, S)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_refusals_by_message(golden):
    good = golden['p7x9_rgb_stream']
    for key, what in (('refuse_progressive', 'progressive'), ('refuse_cmyk', 'four components'), ('refuse_palette', 'palette'),
                      ('refuse_png16', '16-bit samples')):
        with pytest.raises(GenesisHipError, match=what):
            imagefile.decode_image_batch([good, golden[key]], 8)
    with pytest.raises(GenesisHipError, match='145 x 131 frame exceeds max_side = 128'):
        imagefile.decode_image_batch([good, golden['j145x131_420_q75_stream']], 8, max_side=128)
    with pytest.raises(GenesisHipError, match='an empty batch'):
        imagefile.decode_image_batch([], 8)
    with pytest.raises(GenesisHipError, match='out must be on the HIP device'):
        imagefile.decode_image_batch([good], 8, out=torch.empty(1, 3, 8, 8))
    with pytest.raises(GenesisHipError, match=r'out must be a contiguous float32 tensor of shape \[1, 3, 8, 8\]'):
        imagefile.decode_image_batch([good], 8, out=torch.empty(1, 3, 8, 9, device='cuda'))
    with pytest.raises(GenesisHipError, match='out must be a contiguous float32'):
        imagefile.decode_image_batch([good], 8, out=torch.empty(1, 3, 8, 8, device='cuda', dtype=torch.float16))


def test_the_single_geometry_paths_keep_their_refusals(golden):
    with pytest.raises(GenesisHipError, match='mixed sizes'):
        jpeg.decode_jpeg_batch([golden['j16x16_420_q100_stream'], golden['j1x1_420_q75_stream']])
    with pytest.raises(GenesisHipError, match='mixed geometries'):
        png.decode_png_batch([golden['p7x9_rgb_stream'], golden['p145x131_rgb_stream']])
    with pytest.raises(GenesisHipError, match='larger than'):
        jpeg.decode_jpeg_batch([golden['j145x131_420_q75_stream']])
    x, u8 = jpeg.decode_jpeg_batch([golden['j16x16_420_q100_stream']], return_u8=True)
    assert np.array_equal(u8[0].cpu().numpy(), golden['j16x16_420_q100_u8'])


# ---- the loader and the folder config ---------------------------------------------------------------------------------------------
FOLDER_NAMES = [n for n in MG.CASE_NAMES if max(MG.case_size(n)) <= 264]      # max_side = 264 below


def write_folder(root, golden, names, sub=None):
    """names[i] -> <root>/[sub(i)/]f<i>.<ext>; returns the paths relative to root, in order."""
    rel = []
    for i, n in enumerate(names):
        r = 'f%02d%s' % (i, '.png' if n[0] == 'p' else ('.jpg', '.JPEG')[i % 2])
        if sub is not None:
            r = osp.join(sub(i), r)
        os.makedirs(osp.dirname(osp.join(root, r)), exist_ok=True)
        with open(osp.join(root, r), 'wb') as f:
            f.write(bytes(golden[n + '_stream']))
        rel.append(r)
    return rel


def epoch(loader):
    """(the epoch's file order, its batches concatenated on the host).  `for` would call __iter__ a second time and draw a new
    permutation, so the batches are taken with next()."""
    it = iter(loader)
    order = loader.order.copy()
    got = []
    while True:
        try:
            got.append(next(it)['input'])
        except StopIteration:
            return order, torch.cat(got).cpu()


def test_loader_order_short_batch_epochs_and_shard(tmp_path, golden):
    S = 20
    names = [FOLDER_NAMES[i % len(FOLDER_NAMES)] for i in range(11)]
    rel = write_folder(str(tmp_path), golden, names)
    files = [str(tmp_path / r) for r in rel]
    want = torch.stack([want_f32(golden, n, S) for n in names])
    loader = imagefile.ImageFileLoader(files, 4, S, shuffle=False, num_workers=3, max_side=264)
    assert len(loader) == 3 and loader.batch_size == 4
    batches = [b['input'] for b in loader]
    assert [tuple(b.shape) for b in batches] == [(4, 3, S, S), (4, 3, S, S), (3, 3, S, S)] and all(b.is_cuda for b in batches)
    assert torch.equal(torch.cat(batches).cpu(), want)
    assert torch.equal(torch.cat([b['input'] for b in loader]).cpu(), want)          # iterated again
    loader.close()
    # shuffled: a permutation per epoch, the same ones from the same seed
    orders = []
    for seed in (7, 7, 8):
        loader = imagefile.ImageFileLoader(files, 4, S, shuffle=True, seed=seed, num_workers=2, max_side=264)
        epochs = []
        for _ in range(2):
            order, got = epoch(loader)
            assert sorted(order.tolist()) == list(range(11)) and torch.equal(got, want[torch.from_numpy(order)])
            epochs.append(order.tolist())
        loader.close()
        orders.append(epochs)
    assert orders[0] == orders[1] and orders[0][0] != orders[0][1] and orders[0] != orders[2]
    # shard: every second file from the second on
    loader = imagefile.ImageFileLoader(files, 4, S, shuffle=False, num_workers=2, max_side=264, shard=(1, 2))
    assert loader.files == files[1::2] and len(loader) == 2
    assert torch.equal(torch.cat([b['input'] for b in loader]).cpu(), want[1::2])
    loader.close()
    # an epoch left half way after one batch: the next one delivers every file once
    loader = imagefile.ImageFileLoader(files, 4, S, shuffle=False, num_workers=2, max_side=264)
    assert torch.equal(next(iter(loader))['input'].cpu(), want[:4])
    order, got = epoch(loader)
    assert order.tolist() == list(range(11)) and torch.equal(got, want)
    loader.close()
    loader = imagefile.ImageFileLoader(files, 4, S, shuffle=True, seed=7, num_workers=2, max_side=264)
    assert tuple(next(iter(loader))['input'].shape) == (4, 3, S, S)
    order, got = epoch(loader)
    assert sorted(order.tolist()) == list(range(11)) and torch.equal(got, want[torch.from_numpy(order)])
    loader.close()
    # a ring deeper than the epoch's three batches: all of them, in order, then the end
    loader = imagefile.ImageFileLoader(files, 4, S, shuffle=False, num_workers=2, max_side=264, depth=8)
    it = iter(loader)
    batches = [next(it)['input'] for _ in range(3)]
    with pytest.raises(StopIteration):
        next(it)
    assert [len(b) for b in batches] == [4, 4, 3] and torch.equal(torch.cat(batches).cpu(), want)
    loader.close()


def test_loader_names_the_bad_file_after_the_good_batches(tmp_path, golden):
    S = 8
    names = [FOLDER_NAMES[i % len(FOLDER_NAMES)] for i in range(10)]
    rel = write_folder(str(tmp_path), golden, names)
    files = [str(tmp_path / r) for r in rel]
    with open(files[6], 'wb') as f:                     # a stream cut short, in the second batch
        f.write(bytes(golden[names[6] + '_stream'])[:40])
    loader = imagefile.ImageFileLoader(files, 4, S, shuffle=False, num_workers=2, max_side=264)
    it = iter(loader)
    first = next(it)['input']
    assert torch.equal(first.cpu(), torch.stack([want_f32(golden, n, S) for n in names[:4]]))
    with pytest.raises(GenesisHipError, match=r'imagefile: .*f06\.\w+: .*(ends early|expected)'):
        next(it)
    # the next epoch starts afresh and fails at the same place
    assert torch.equal(next(iter(loader))['input'].cpu(), first.cpu())
    loader.close()
    # a frame above max_side: named, with the argument
    loader = imagefile.ImageFileLoader(files[:4], 4, S, shuffle=False, num_workers=2, max_side=100)
    with pytest.raises(GenesisHipError, match=r'imagefile: .*f\d\d\.\w+: .*exceeds max_side = 100'):
        next(iter(loader))
    loader.close()
    # a file that is not there
    loader = imagefile.ImageFileLoader(files[:2] + [str(tmp_path / 'gone.png')], 4, S, shuffle=False, max_side=264)
    with pytest.raises(GenesisHipError, match=r'gone\.png'):
        next(iter(loader))
    loader.close()


def test_folder_config_and_one_training_step(tmp_path, golden):
    import genesis_amd.image_folder_config as F
    S = 64
    names = [FOLDER_NAMES[i % len(FOLDER_NAMES)] for i in range(12)]
    tree = str(tmp_path / 'tree')
    rel = write_folder(tree, golden, names, sub=lambda i: osp.join(('train', 'train', 'val', 'test')[i % 4], 'd%d' % (i % 2)))
    cfg = AttrDict(data_folder=tree, img_size=S, num_workers=2, batch_size=4, seed=1, max_side=264, K_steps=3)
    train, val, test = F.load(cfg)
    assert [len(l.files) for l in (train, val, test)] == [6, 3, 3] and [len(l) for l in (train, val, test)] == [2, 1, 1]
    by_path = {osp.join(tree, r): n for r, n in zip(rel, names)}
    for loader, mode in ((train, 'train'), (val, 'val'), (test, 'test')):
        assert loader.files == [osp.join(tree, r) for r in sorted(r for r in rel if r.startswith(mode))]
        order, got = epoch(loader)
        want = torch.stack([want_f32(golden, by_path[loader.files[i]], S) for i in order])
        assert torch.equal(got, want)
    # a flat folder: the seeded split and its list files decide
    flat = str(tmp_path / 'flat')
    write_folder(flat, golden, [FOLDER_NAMES[i % len(FOLDER_NAMES)] for i in range(20)])
    loaders = F.load(AttrDict(data_folder=flat, img_size=8, num_workers=2, batch_size=4, max_side=264))
    assert [len(l.files) for l in loaders] == [16, 2, 2]
    assert sorted(f for l in loaders for f in l.files) == sorted(osp.join(flat, r) for r in F.find_images(flat))
    assert all(osp.exists(F.list_path(flat, m)) for m in F.MODES)
    assert sum(b['input'].shape[0] for b in loaders[0]) == 16
    for l in loaders + (train, val, test):
        l.close()
    # one training step on a batch from the loader
    import genesis_amd.genesisv2_config as G
    from genesis_amd.trainer import TrainStep
    from oracle import v2_oracle as O
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(O.make_cfg(K_steps=4, img_size=32, feat_dim=16), debug=False, multi_gpu=False))).to('cuda').train()
    loader = F.load(AttrDict(cfg, img_size=32))[0]
    batch = next(iter(loader))['input']
    assert batch.shape == (4, 3, 32, 32)
    ts = TrainStep(model, 32)
    out = ts.step(batch).cpu()
    torch.cuda.synchronize()
    loader.close()
    assert int(ts.step_t) == 1 and bool(torch.isfinite(out[:3]).all()) and float(out[1]) > 0.0
