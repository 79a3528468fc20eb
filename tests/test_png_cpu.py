"""The host half of the PNG decoder and of the ShapeStacks / Sketchy data configs, without a GPU: the C chunk walk and
inflate (gx_png_info, gx_png_inflate) followed by a numpy restatement of the five filters (tests/png_restatement.py) against
Pillow's bytes (tests/golden/png_pil.npz, written by tests/golden/make_golden_png.py) at zero tolerance; the broken
streams, each with its own message; staging from two threads; the file lists, map paths and flags of the two configs."""
import os
import os.path as osp
import sys
import threading

import numpy as np
import pytest

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, HERE)
import make_golden_png as MG  # noqa: E402
import png_restatement as R  # noqa: E402

from genesis_amd import png  # noqa: E402
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


def host_decode(stream):
    """(PngInfo, uint8 [H, W, C]): the C inflate, then the numpy restatement of the filters."""
    info = png.png_info(stream)
    dst = np.full(info.inflated_size + 3, 0x55, dtype=np.uint8)
    got = png.inflate(stream, dst)
    assert got.geometry == info.geometry and got.inflated_size == info.inflated_size
    assert (dst[info.inflated_size:] == 0x55).all()                  # nothing written past the frame
    return info, R.unfilter(dst[:info.inflated_size], info.height, info.width, info.channels)


def test_the_fixture_covers_what_it_should(golden):
    assert osp.getsize(MG.NPZ) < 512 * 1024
    hand = {c[0]: c for c in MG.HAND}
    assert {(c[3], c[4]) for c in MG.HAND if (c[1], c[2]) == (5, 3)} == {(C, f) for C in (1, 3, 4) for f in range(5)}
    assert {(c[1], c[2]) for c in MG.HAND} >= {(1, 1), (1, 7), (7, 1), (5, 3), (67, 9), (3, 341), (3, 342), (3, 256), (3, 257)}
    assert golden['chunks_c3_67x9_png'].tobytes().count(b'IDAT') == 4 and b'tEXt' in golden['chunks_c3_67x9_png'].tobytes()
    for name in ('cycle_c3_67x9', 'band_c4_3x257'):
        assert set(MG.stream_filters(golden[name + '_png']).tolist()) == {0, 1, 2, 3, 4}, hand[name]
    assert len(set(MG.stream_filters(golden['pil_noise64_png']).tolist())) >= 2        # Pillow's adaptive choice mixes filters
    assert sorted(set(golden['ss_map_u8'][:, :, 0].ravel().tolist())) == list(range(0, 256, 32))


@pytest.mark.parametrize('name', MG.GOOD_NAMES)
def test_info_reports_the_geometry(golden, name):
    want = golden[name + '_u8']
    info = png.png_info(golden[name + '_png'])
    H, W, C = want.shape
    assert info.geometry == (H, W, C) and info.bytes_per_pixel == C and info.bit_depth == 8 and info.interlace == 0
    assert info.colour_type == {1: 0, 3: 2, 4: 6}[C] and info.inflated_size == H * (1 + W * C) == png.frame_bytes(H, W, C)


@pytest.mark.parametrize('name', MG.GOOD_NAMES + ['ss_map'])
def test_inflate_and_restatement_equal_pillow(golden, name):
    _, got = host_decode(golden[name + '_png'])
    want = golden[name + '_u8']
    assert got.shape == want.shape and int((got != want).sum()) == 0


@pytest.mark.parametrize('name,message', MG.BROKEN)
def test_broken_streams_are_rejected_by_name(golden, name, message):
    stream = golden['broken_%s_png' % name]
    dst = np.zeros(1 << 12, dtype=np.uint8)
    with pytest.raises(GenesisHipError, match=message):
        png.inflate(stream, dst)


def test_other_rejections_and_bounds(golden):
    good = golden['f1_c3_5x3_png'].tobytes()
    dst = np.zeros(1 << 12, dtype=np.uint8)
    for patch, message in (((25, 4), r'grey\+alpha'), ((24, 4), 'under 8 bits'), ((0, 0x88), 'signature')):
        bad = bytearray(good)
        bad[patch[0]] = patch[1]
        if patch[0] >= 16:                               # inside IHDR: its checksum has to follow
            bad[29:33] = MG.chunk(b'IHDR', bytes(bad[16:29]))[-4:]
        with pytest.raises(GenesisHipError, match=message):
            png.inflate(bytes(bad), dst)
    big = MG.SIGNATURE + MG.ihdr(4097, 3, 2) + good[33:]
    with pytest.raises(GenesisHipError, match='larger than the 4096 x 4096'):
        png.png_info(big)
    iend = good.index(b'IEND') - 4
    with pytest.raises(GenesisHipError, match='missing IEND'):
        png.inflate(good[:iend], dst)
    with pytest.raises(GenesisHipError, match='missing IDAT'):
        png.inflate(good[:33] + good[iend:], dst)
    with pytest.raises(GenesisHipError, match='missing IHDR'):
        png.inflate(good[:8] + good[33:], dst)
    with pytest.raises(GenesisHipError, match='dst holds 10'):
        png.inflate(good, np.zeros(10, dtype=np.uint8))
    with pytest.raises(GenesisHipError, match='unknown critical chunk'):
        png.inflate(good[:33] + MG.chunk(b'ABCD', b'xy') + good[33:], dst)
    first = good.index(b'IDAT') - 4
    n = int.from_bytes(good[first:first + 4], 'big')
    z = good[first + 8:first + 8 + n]
    apart = good[:first] + MG.chunk(b'IDAT', z[:3]) + MG.chunk(b'tEXt', b'k\x00v') + MG.chunk(b'IDAT', z[3:]) + good[iend:]
    with pytest.raises(GenesisHipError, match='not consecutive'):
        png.inflate(apart, dst)
    together = good[:first] + MG.chunk(b'IDAT', z[:3]) + MG.chunk(b'IDAT', z[3:]) + MG.chunk(b'tEXt', b'k\x00v') + good[iend:]
    assert png.inflate(together, dst).geometry == (3, 5, 3)
    # every prefix and every single flipped byte is either decoded or rejected, never a crash
    for n in range(len(good)):
        with pytest.raises(GenesisHipError):
            png.inflate(good[:n], dst)
    rejected = 0
    for i in range(len(good)):
        bad = bytearray(good)
        bad[i] ^= 0x21
        try:
            png.inflate(bytes(bad), dst)
        except GenesisHipError:
            rejected += 1
    assert rejected == len(good)                         # signature, lengths, types and payloads are all under a check


def test_staging_from_two_threads_and_mixed_geometries(golden):
    names = ['f%d_c3_5x3' % f for f in range(5)]
    st = png.PngStaging(64, 3, 5, 3, pin=False)
    errors = []

    def fill(slots):
        try:
            for i in slots:
                st.decode(i, golden[names[i % 5] + '_png'])
        except Exception as e:                           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=fill, args=(range(w, 64, 2),)) for w in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(64):
        assert np.array_equal(R.unfilter(st.frames[i], 3, 5, 3), golden[names[i % 5] + '_u8'])
    with pytest.raises(GenesisHipError, match='mixed geometries.*5 x 3 frame with 4 channels among 5 x 3 ones with 3'):
        st.decode(0, golden['f0_c4_5x3_png'])
    with pytest.raises(GenesisHipError, match='mixed geometries.*67 x 9'):
        st.decode(0, golden['cycle_c3_67x9_png'])
    with pytest.raises(GenesisHipError, match='at most 4096'):
        png.PngStaging(1, 5000, 5, 3, pin=False)


def test_there_is_no_cpu_path(golden):
    import torch
    stream = golden['f1_c3_5x3_png']
    with pytest.raises(GenesisHipError, match='no CPU path'):
        png.decode_png_batch([stream], device='cpu')
    with pytest.raises(GenesisHipError, match='no CPU path'):
        png.decode_png_labels([stream], 'index', device='cpu')
    with pytest.raises(GenesisHipError, match='empty batch'):
        png.decode_png_batch([])
    with pytest.raises(GenesisHipError, match='no CPU path'):
        png.decode_staged(torch.zeros(48, dtype=torch.uint8), 1, 1, (3, 5, 3))
    with pytest.raises(GenesisHipError, match='plane rule'):
        png.decode_png_labels([stream], 'labels')


# ---- the ShapeStacks file list on a temporary tree
SCENARIOS = ['env_ccs-hard-h=2-vcom=0-vpsf=0-v=60', 'env_blocks-easy-h=3-vcom=1-vpsf=0-v=7', 'env_unlisted-h=2-vcom=0-vpsf=0-v=1']
CAMS = (1, 7, 12)


def write_shapestacks_tree(root, frame, mapfile):
    for sub in ('recordings', 'iseg'):
        for sc in SCENARIOS:
            os.makedirs(osp.join(root, sub, sc))
    os.makedirs(osp.join(root, 'splits', 'default'))
    for sc in SCENARIOS:
        for cam in CAMS:
            with open(osp.join(root, 'recordings', sc, 'rgb-w=5-f=2-l=1-c=unique-cam_%d-mono-0.png' % cam), 'wb') as f:
                f.write(frame)
            with open(osp.join(root, 'iseg', sc, 'iseg-w=0-f=0-l=0-c=original-cam_%d-mono-0.map' % cam), 'wb') as f:
                f.write(mapfile)
        for other in ('rgb-w=5-f=2-l=1-c=unique-cam_1-mono-1.png', 'vseg-w=5-cam_1-mono-0.png', 'log.txt'):
            with open(osp.join(root, 'recordings', sc, other), 'wb') as f:
                f.write(b'not a frame')
    for mode, scs, tail in (('train', SCENARIOS[:2], '\n'), ('eval', SCENARIOS[1:2], '\n'), ('test', SCENARIOS[:1], '\nnot-terminated')):
        with open(osp.join(root, 'splits', 'default', mode + '.txt'), 'w') as f:
            f.write('\n'.join(scs) + tail)


def test_shapestacks_file_list_and_map_paths(tmp_path, golden):
    import genesis_amd.shapestacks_config as S
    root = str(tmp_path)
    write_shapestacks_tree(root, golden['f1_c3_5x3_png'].tobytes(), golden['f1_c1_5x3_png'].tobytes())
    want = {'train': SCENARIOS[:2], 'eval': SCENARIOS[1:2], 'test': SCENARIOS[:1]}
    for mode, scs in want.items():
        files = S.frame_files(root, 'default', mode)
        expected = [osp.join(root, 'recordings', sc, n) for sc in scs for n in os.listdir(osp.join(root, 'recordings', sc))
                    if n.startswith('rgb-') and n.endswith('-mono-0.png')]
        assert files == expected and len(files) == 3 * len(scs)
        assert sorted(osp.basename(f) for f in files[:3]) == sorted('rgb-w=5-f=2-l=1-c=unique-cam_%d-mono-0.png' % c for c in CAMS)
        for f in files:
            m = S.map_file(root, f)
            cam = osp.basename(f).split('cam_')[1].split('-')[0]
            assert m == osp.join(root, 'iseg', osp.basename(osp.dirname(f)), 'iseg-w=0-f=0-l=0-c=original-cam_%s-mono-0.map' % cam)
            assert osp.exists(m)
    with pytest.raises(ValueError):
        S.frame_files(root, 'default', 'valid')
    cfg = AttrDict(data_folder=root, split_name='default', shuffle_test=True, load_instances=True, seed=5)
    files, maps = S.split_files(cfg, 'train', shard=(1, 2))
    assert files == S.frame_files(root, 'default', 'train')[1::2] and maps == [S.map_file(root, f) for f in files]
    shuffled, _ = S.split_files(cfg, 'test')
    assert sorted(shuffled) == sorted(S.frame_files(root, 'default', 'test')) and S.split_files(cfg, 'test')[0] == shuffled
    cfg.load_instances = False
    assert S.split_files(cfg, 'eval')[1] is None
    with pytest.raises(GenesisHipError, match='shard'):
        S.split_files(cfg, 'train', shard=(2, 2))


def test_shapestacks_file_list_equals_the_reference(tmp_path, golden):
    ref_root = os.environ.get('GENESIS_REFERENCE_ROOT', '/root/reference')
    provider = osp.join(ref_root, 'third_party', 'shapestacks', 'shapestacks_provider.py')
    if not osp.exists(provider):
        pytest.skip('reference tree not present')
    import importlib.util
    import genesis_amd.shapestacks_config as S
    spec = importlib.util.spec_from_file_location('ref_shapestacks_provider', provider)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    root = str(tmp_path)
    write_shapestacks_tree(root, b'x', b'y')
    for mode in S.MODES:
        names, labels = ref._get_filenames_with_labels(mode, root, osp.join(root, 'splits', 'default'))
        assert S.frame_files(root, 'default', mode) == names and len(labels) == len(names)


def test_sketchy_list_is_written_and_then_read(tmp_path, golden):
    import genesis_amd.sketchy_config as K
    root = str(tmp_path)
    for mode, eps in (('train', 2), ('valid', 1), ('test', 1)):
        for e in range(eps):
            os.makedirs(osp.join(root, 'processed', mode, 'ep%d' % e))
            for i in range(3):
                with open(osp.join(root, 'processed', mode, 'ep%d' % e, 'ep%d_%d.png' % (e, i)), 'wb') as f:
                    f.write(b'x')
            with open(osp.join(root, 'processed', mode, 'ep%d' % e, 'notes.txt'), 'wb') as f:
                f.write(b'x')
    found = K.split_files(root, 'train')
    assert len(found) == 6 and all(f.endswith('.png') for f in found)
    listed = osp.join(root, 'processed', 'train_images.txt')
    assert open(listed).read() == ''.join(f + '\n' for f in found)
    with open(listed, 'w') as f:                          # the list, once written, is what counts
        f.write(''.join(p + ' \n' for p in found[:4]))
    assert K.split_files(root, 'train') == found[:4]
    assert len(K.split_files(root, 'valid')) == 3 and osp.exists(osp.join(root, 'processed', 'valid_images.txt'))
    with pytest.raises(AssertionError):
        K.load(AttrDict(data_folder=root, img_size=64, num_workers=1, batch_size=2, seed=0, debug=True))


def _fresh_flags(module_name):
    """The flags a config registers when it is imported into an empty table."""
    import importlib
    from forge import flags
    flags.FLAGS.clear()
    sys.modules.pop(module_name, None)
    importlib.import_module(module_name)
    return dict(flags.FLAGS)


def test_both_configs_register_the_reference_flags():
    got = _fresh_flags('genesis_amd.shapestacks_config')
    assert got == dict(data_folder='data/shapestacks', split_name='default', img_size=64, shuffle_test=False, num_workers=4,
                       load_instances=True, copy_to_tmp=False, K_steps=9)
    import genesis_amd.shapestacks_config as S
    assert (S.MAX_SHAPES, S.CENTRE_CROP) == (6, 196)
    got = _fresh_flags('genesis_amd.sketchy_config')
    assert got == dict(data_folder='data/sketchy', num_workers=4, img_size=128, K_steps=10)
