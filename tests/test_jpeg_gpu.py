"""The device half of the JPEG decoder (gx_jpeg_decode_f32chw through genesis_amd/jpeg.py) against Pillow's decoded pixels
(tests/golden/jpeg_pil.npz) at zero tolerance, and the GQN data config on tiny TFRecord files written in tmp_path from
the same streams: order, the short last batch, epochs, shuffling, the frame choice, one training step, a corrupt frame."""
import os.path as osp
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_jpeg as MG  # noqa: E402

from genesis_amd import jpeg  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402
from genesis_amd.tfrecord import TFRecordError  # noqa: E402

SCALE = np.float32(1.0) / np.float32(255.0)


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    """A data config registers its flags when it is first imported, and the first definition of a name keeps its default:
    importing gqn_config here must not decide the defaults the other data configs' tests see later in the same process."""
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


def exact_f32(rgb_u8):
    """uint8 [.., H, W, 3] -> fp32 [.., 3, H, W] = u8 * float32(1/255)."""
    t = torch.from_numpy(np.ascontiguousarray(rgb_u8)).float() * torch.tensor(SCALE)
    return t.movedim(-1, -3).contiguous()


@pytest.mark.parametrize('name', MG.CASE_NAMES)
def test_kernel_equals_pillow_bit_for_bit(golden, name):
    want = golden[name + '_rgb']
    x, u8 = jpeg.decode_jpeg_batch([golden[name + '_jpeg']], return_u8=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1,) + want.shape
    assert int((u8[0].cpu().numpy() != want).sum()) == 0
    assert x.dtype == torch.float32 and tuple(x.shape) == (1, 3) + want.shape[:2]
    assert torch.equal(x[0].cpu(), exact_f32(want))


def test_batches_with_a_table_per_frame(golden):
    names = ['s64_420_q75_mixed', 's64_420_q30_smooth', 's64_420_q95_noise', 's64_420_q100_mixed']
    assert {jpeg.jpeg_info(golden[n + '_jpeg']).geometry for n in names} == {(64, 64, 2)}         # one geometry ...
    x, u8 = jpeg.decode_jpeg_batch([bytes(golden[n + '_jpeg']) for n in names], return_u8=True)
    want = np.stack([golden[n + '_rgb'] for n in names])
    assert np.array_equal(u8.cpu().numpy(), want) and torch.equal(x.cpu(), exact_f32(want))      # ... four qualities
    one = jpeg.decode_jpeg_batch([golden[names[2] + '_jpeg']])
    assert torch.equal(one.cpu(), exact_f32(want[2:3]))
    many = [names[(5 * i) % 4] for i in range(33)]
    out = torch.full((33, 3, 64, 64), -1.0, device='cuda')
    got = jpeg.decode_jpeg_batch([golden[n + '_jpeg'] for n in many], out=out)
    assert got is out and torch.equal(out.cpu(), exact_f32(np.stack([golden[n + '_rgb'] for n in many])))


@pytest.mark.parametrize('name,size', [('s64_420_q75_mixed', 32), ('s64_422_q75_mixed', 128), ('s40x56_420_q75_mixed', (20, 20)),
                                       ('s40x56_444_q30_smooth', (20, 33))])
def test_resize_is_f_interpolate_of_the_exact_frame(golden, name, size):
    frame = exact_f32(golden[name + '_rgb'][None])
    got = jpeg.decode_jpeg_batch([golden[name + '_jpeg']], img_size=size)
    assert torch.equal(got.cpu(), F.interpolate(frame, size=size))


def test_arguments_are_checked(golden):
    a, b = golden['s64_420_q75_mixed_jpeg'], golden['s16_420_q75_mixed_jpeg']
    with pytest.raises(GenesisHipError, match='mixed sizes'):
        jpeg.decode_jpeg_batch([a, b])
    with pytest.raises(GenesisHipError, match='mixed sampling classes'):
        jpeg.decode_jpeg_batch([a, golden['s64_444_q75_mixed_jpeg']])
    with pytest.raises(GenesisHipError, match='out must be'):
        jpeg.decode_jpeg_batch([a], out=torch.empty(1, 3, 32, 32, device='cuda'))
    with pytest.raises(GenesisHipError, match='HIP device'):
        jpeg.decode_jpeg_batch([a], out=torch.empty(1, 3, 64, 64))
    with pytest.raises(GenesisHipError, match='progressive'):
        jpeg.decode_jpeg_batch([golden['progressive_jpeg']])
    with pytest.raises(GenesisHipError, match='empty batch'):
        jpeg.decode_jpeg_batch([])


# ---- the GQN data config on tiny files
TRAIN_FILES, TEST_FILES, RECORDS = 4, 1, 5             # val_frac = 4: three devel_train files, one devel_val file


def stream_name(split, fi, r, f):
    names = MG.GQN_CASES
    return names[(11 * (split == 'test') + 7 * fi + 3 * r + f) % len(names)]


@pytest.fixture(scope='module')
def gqn_folder(tmp_path_factory, golden):
    import genesis_amd.gqn_config as Q
    root = tmp_path_factory.mktemp('gqn')
    for split, n in (('train', TRAIN_FILES), ('test', TEST_FILES)):
        (root / 'rooms_ring_camera' / split).mkdir(parents=True)
        for fi, path in enumerate(Q.file_list(str(root), split, 4, TRAIN_FILES, TEST_FILES)):
            MG.write_gqn_tfrecord(path, [([bytes(golden[stream_name(split, fi, r, f) + '_jpeg']) for f in range(10)],
                                          [0.25 * i for i in range(50)]) for r in range(RECORDS)])
    return str(root)


def make_cfg(folder, **kw):
    cfg = AttrDict(data_folder=folder, img_size=64, val_frac=4, num_workers=2, buffer_size=2, K_steps=7, batch_size=4, seed=0,
                   debug=True)
    cfg.update(kw)
    return cfg


def load(cfg, **kw):
    import genesis_amd.gqn_config as Q
    return Q.load(cfg, train_files=TRAIN_FILES, test_files=TEST_FILES, records_per_file=RECORDS, **kw)


def want_frames(golden, split, records, frame):
    return exact_f32(np.stack([golden[stream_name(split, fi, r, frame) + '_rgb'] for fi, r in records]))


def test_load_yields_the_pillow_pixels_of_the_right_records_in_order(gqn_folder, golden):
    loaders = load(make_cfg(gqn_folder), frame=3, shuffle=False)
    assert [len(l) for l in loaders] == [15 // 4, 5 // 4, 5] and [l.batch_size for l in loaders] == [4, 4, 1]
    expected = [('train', [(fi, r) for fi in range(3) for r in range(RECORDS)]), ('train', [(3, r) for r in range(RECORDS)]),
                ('test', [(0, r) for r in range(RECORDS)])]
    for loader, (split, records) in zip(loaders, expected):
        want = want_frames(golden, split, records, 3)
        B = loader.batch_size
        for _ in range(2):                                   # two epochs through the same ring
            xs = []
            for batch in loader:
                assert sorted(batch) == ['input'] and batch['input'].is_cuda and batch['input'].dtype == torch.float32
                xs.append(batch['input'].cpu())
            assert [len(x) for x in xs] == [B] * (len(records) // B) + ([len(records) % B] if len(records) % B else [])
            assert torch.equal(torch.cat(xs), want)
            # the for loop has seen StopIteration; the next call starts another epoch, as the reference's loader does
            assert torch.equal(next(loader)['input'].cpu(), want[:B])
        loader.close()
    # img_size other than the stored 64: the kernel's own nearest resize
    small = load(make_cfg(gqn_folder, img_size=32), frame=3, shuffle=False)[1]
    got = torch.cat([b['input'].cpu() for b in small])
    assert torch.equal(got, F.interpolate(want_frames(golden, 'train', [(3, r) for r in range(RECORDS)], 3), size=32))
    small.close()


def test_shuffle_seed_and_frame_choice(gqn_folder, golden):
    def epoch(seed):
        train = load(make_cfg(gqn_folder, seed=seed))[0]
        index = np.concatenate([b['index'] for b in train.host])
        x = torch.cat([b['input'].cpu() for b in train])
        train.close()
        return index, x

    index, x = epoch(3)
    assert sorted(map(tuple, index[:, :2].tolist())) == [(fi, r) for fi in range(3) for r in range(RECORDS)]      # each once
    assert index[:, :2].tolist() != [[fi, r] for fi in range(3) for r in range(RECORDS)]
    assert len(set(index[:, 2].tolist())) > 1 and 0 <= index[:, 2].min() and index[:, 2].max() < 10
    want = exact_f32(np.stack([golden[stream_name('train', fi, r, f) + '_rgb'] for fi, r, f in index.tolist()]))
    assert torch.equal(x, want)
    again, x2 = epoch(3)
    assert again.tolist() == index.tolist() and torch.equal(x2, x)
    other, _ = epoch(4)
    assert other.tolist() != index.tolist()


def test_a_ring_of_two_slots_refilled_and_an_abandoned_epoch(gqn_folder):
    """8 shuffled batches through a ring of depth 2, so every slot is refilled three times: each batch is bit-equal to the
    host restatement's pixels of the records the host stream's 'index' names.  Then an epoch left after one batch, then a
    whole one, which equals a fresh loader's."""
    import genesis_amd.gqn_config as Q
    sys.path.insert(0, osp.dirname(GOLDEN))
    import jpeg_restatement as R
    cfg = make_cfg(gqn_folder, batch_size=2, seed=5)
    (host, _, _), (frames, _, _) = Q.host_splits(cfg, train_files=TRAIN_FILES, test_files=TEST_FILES, records_per_file=RECORDS)
    want = [exact_f32(np.stack([R.decode_pixels(c, q, *b['geometry']) for c, q in zip(b['coef'], b['qtab'])])) for b in host]
    assert [len(w) for w in want] == [2] * 7 + [1]
    assert np.concatenate([b['index'] for b in host])[:, :2].tolist() != [[fi, r] for fi in range(3) for r in range(RECORDS)]

    def epoch(loader):
        return [b['input'].cpu() for b in loader]

    loader = Q.GQNLoader(host, frames, cfg.img_size, depth=2)
    got = epoch(loader)
    assert len(got) == 8 and all(torch.equal(g, w) for g, w in zip(got, want))
    assert torch.equal(next(iter(loader))['input'].cpu(), want[0])           # abandoned here, with the second batch staged
    got = epoch(loader)
    fresh = epoch(Q.GQNLoader(host, frames, cfg.img_size, depth=2))
    assert len(got) == len(fresh) == 8 and all(torch.equal(g, f) and torch.equal(g, w) for g, f, w in zip(got, fresh, want))
    loader.close()


def test_train_step_on_a_yielded_batch_has_a_finite_elbo(gqn_folder):
    import genesis_amd.genesisv2_config as G
    from genesis_amd.trainer import TrainStep
    from oracle import v2_oracle as O
    cfg = make_cfg(gqn_folder)
    train = load(cfg)[0]
    batch = next(iter(train))
    train.close()
    assert batch['input'].shape == (4, 3, 64, 64)
    mcfg = O.make_cfg(K_steps=cfg.K_steps, img_size=cfg.img_size, feat_dim=16)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(mcfg, debug=False, multi_gpu=False))).to('cuda:0').train()
    ts = TrainStep(model, cfg.img_size)
    out = ts.step(batch['input']).cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), out
    assert int(ts.step_t) == 1


def test_a_truncated_frame_names_file_record_and_frame(tmp_path, golden):
    import genesis_amd.gqn_config as Q
    (tmp_path / 'rooms_ring_camera' / 'train').mkdir(parents=True)
    (tmp_path / 'rooms_ring_camera' / 'test').mkdir(parents=True)
    stream = bytes(golden[MG.GQN_CASES[0] + '_jpeg'])
    good = ([stream] * 10, [0.0] * 50)
    bad = ([stream] * 3 + [stream[:len(stream) // 2]] + [stream] * 6, [0.0] * 50)
    files = Q.file_list(str(tmp_path), 'train', 2, 2, 1) + Q.file_list(str(tmp_path), 'test', 2, 2, 1)
    for path in files:
        MG.write_gqn_tfrecord(path, [good, good, bad] if path.endswith('2-of-2.tfrecord') else [good, good])
    cfg = make_cfg(str(tmp_path), val_frac=2)
    train, val, _ = Q.load(cfg, frame=3, shuffle=False, train_files=2, test_files=1, records_per_file=2)
    assert len(list(train)) == 1
    with pytest.raises(TFRecordError, match=r'2-of-2\.tfrecord: record 2: frame 3: .*ends early'):
        list(val)
    val.close()
    val = Q.load(cfg, frame=4, shuffle=False, train_files=2, test_files=1, records_per_file=2)[1]
    assert sum(len(b['input']) for b in val) == 3
