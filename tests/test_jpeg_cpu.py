"""The host half of the JPEG decoder and of the GQN data config, without a GPU: the C entropy decoder
(gx_jpeg_info, gx_jpeg_entropy_decode) followed by a numpy restatement of the pixel arithmetic (tests/jpeg_restatement.py)
against Pillow's decoded pixels (tests/golden/jpeg_pil.npz, written by tests/golden/make_golden_jpeg.py) at zero
tolerance; the rejected stream kinds, each with its own message; truncated and corrupted streams (host runs only);
gx_bytes_list_index; and the GQN file lists, split boundaries and lengths, computed with no data read."""
import ctypes
import io
import os.path as osp
import sys

import numpy as np
import pytest

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, HERE)
import jpeg_restatement as R  # noqa: E402
import make_golden_jpeg as MG  # noqa: E402

from genesis_amd import _lib, jpeg, tfrecord  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402


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


def host_decode(stream):
    """(JpegInfo, uint8 [H, W, 3]): the C entropy decoder, then the numpy restatement."""
    info = jpeg.jpeg_info(stream)
    coef = np.full(sum(info.blocks) * 64, 0x5555, dtype=np.int16)
    qtab = np.zeros((3, 64), dtype=np.uint16)
    got = jpeg.entropy_decode(stream, coef, qtab)
    assert got.geometry == info.geometry and got.blocks == info.blocks
    return info, R.decode_pixels(coef, qtab, info.height, info.width, info.sampling)


def test_the_fixture_covers_what_it_should(golden):
    assert osp.getsize(MG.NPZ) < 300 * 1024
    cases = MG.CASES
    assert {(c[1], c[2]) for c in cases} == {(64, 64), (16, 16), (8, 8), (40, 56), (38, 50), (17, 33), (128, 128)}
    assert {c[3] for c in cases} == {0, 1, 2} and {c[5] for c in cases} == {'smooth', 'noise', 'mixed'}
    assert min(c[4] for c in cases) == 30 and max(c[4] for c in cases) == 100
    assert sum(c[6] and not c[7] for c in cases) >= 2 and sum(bool(c[7]) and not c[6] for c in cases) >= 2
    assert sum(bool(c[6] and c[7]) for c in cases) >= 1
    assert len(MG.GQN_CASES) >= 4


@pytest.mark.parametrize('name', MG.CASE_NAMES)
def test_entropy_decoder_and_restatement_equal_pillow(golden, name):
    info, rgb = host_decode(golden[name + '_jpeg'])
    want = golden[name + '_rgb']
    assert rgb.shape == want.shape
    assert int((rgb != want).sum()) == 0


@pytest.mark.parametrize('name', MG.CASE_NAMES)
def test_info_reports_the_geometry(golden, name):
    _, H, W, sampling, _, _, _, rst = MG.case(name)
    info = jpeg.jpeg_info(golden[name + '_jpeg'])
    assert (info.height, info.width, info.components, info.sampling) == (H, W, 3, sampling)
    assert info.blocks == jpeg.plane_blocks(H, W, sampling)
    assert sum(info.blocks) * 64 == sum(bh * bw for bh, bw in R.plane_blocks_hw(H, W, sampling)) * 64
    # Pillow's restart_marker_blocks counts MCUs
    assert info.restart_interval == rst


def test_freshly_encoded_images_equal_pillow():
    pytest.importorskip('PIL')
    rng = np.random.RandomState(11)
    for i, (H, W, sampling, quality, kind, optimize, rst) in enumerate([
            (64, 64, 2, 80, 'mixed', False, 0), (24, 40, 1, 55, 'noise', True, 0), (33, 17, 2, 92, 'mixed', False, 1),
            (9, 23, 0, 70, 'smooth', True, 2), (128, 96, 2, 40, 'mixed', False, 0)]):
        img = MG.content_image(kind, H, W, int(rng.randint(1 << 30)))
        stream = MG.encode(img, sampling, quality, optimize, rst)
        info, rgb = host_decode(stream)
        assert info.sampling == sampling
        assert int((rgb != MG.pil_decode(stream)).sum()) == 0, (H, W, sampling, quality)


def _sof_offset(stream):
    at = bytes(stream).find(b'\xff\xc0')
    assert at > 0
    return at


def test_rejected_streams_say_which_case_it_is(golden):
    base = golden['s16_444_q95_noise_jpeg']
    sof = _sof_offset(base)
    with pytest.raises(GenesisHipError, match='progressive'):
        jpeg.jpeg_info(golden['progressive_jpeg'])
    with pytest.raises(GenesisHipError, match='greyscale'):
        jpeg.jpeg_info(golden['grey_jpeg'])
    four = base.copy()
    four[sof + 9] = 4                                   # Nf
    with pytest.raises(GenesisHipError, match='four components'):
        jpeg.jpeg_info(four)
    deep = base.copy()
    deep[sof + 4] = 12                                  # P
    with pytest.raises(GenesisHipError, match='12-bit'):
        jpeg.jpeg_info(deep)
    wide = base.copy()
    wide[sof + 11] = 0x31                               # H x V of the first component
    with pytest.raises(GenesisHipError, match='sampling factors 3x1'):
        jpeg.jpeg_info(wide)
    dqt = bytes(base).find(b'\xff\xdb')
    q16 = base.copy()
    q16[dqt + 4] |= 0x10                                # Pq = 1
    with pytest.raises(GenesisHipError, match='16-bit quantisation'):
        jpeg.jpeg_info(q16)
    big = base.copy()
    big[sof + 5:sof + 7] = (0, 129)                     # height
    with pytest.raises(GenesisHipError, match='larger than'):
        jpeg.jpeg_info(big)
    ext = base.copy()
    ext[sof + 1] = 0xC1
    with pytest.raises(GenesisHipError, match='extended'):
        jpeg.jpeg_info(ext)
    arith = base.copy()
    arith[sof + 1] = 0xC9
    with pytest.raises(GenesisHipError, match='arithmetic'):
        jpeg.jpeg_info(arith)
    with pytest.raises(GenesisHipError, match='ends early'):
        jpeg.entropy_decode(base[:len(base) - 40], np.zeros(12 * 64, dtype=np.int16), np.zeros(192, dtype=np.uint16))
    with pytest.raises(GenesisHipError, match='the buffer holds'):
        jpeg.entropy_decode(base, np.zeros(11 * 64, dtype=np.int16), np.zeros(192, dtype=np.uint16))
    with pytest.raises(GenesisHipError, match='no SOI'):
        jpeg.jpeg_info(b'not a jpeg')


@pytest.mark.parametrize('name', ['s38x50_444_q60_mixed', 's64_422_q30_smooth_rst', 's40x56_420_q75_mixed'])
def test_truncated_and_corrupted_streams_return_or_raise(golden, name):
    """Host runs only: every call returns or raises GenesisHipError.  The output buffers sit between guard words that must
    stay intact, whatever the stream says."""
    stream = golden[name + '_jpeg']
    info = jpeg.jpeg_info(stream)
    n = sum(info.blocks) * 64
    lib = _lib.load()
    guard = 64
    coef = np.zeros(n + 2 * guard, dtype=np.int16)
    qtab = np.zeros(192 + 2 * guard, dtype=np.uint16)
    raw = np.zeros(8, dtype=np.int32)

    def run(data):
        coef[:guard] = coef[-guard:] = 0x1234
        qtab[:guard] = qtab[-guard:] = 0x4321
        rc = lib.gx_jpeg_entropy_decode(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.c_void_p(coef[guard:].ctypes.data), n,
                                        ctypes.c_void_p(qtab[guard:].ctypes.data), ctypes.c_void_p(raw.ctypes.data))
        assert rc in (0, -1, -3), rc
        assert (coef[:guard] == 0x1234).all() and (coef[-guard:] == 0x1234).all()
        assert (qtab[:guard] == 0x4321).all() and (qtab[-guard:] == 0x4321).all()
        return rc

    assert run(np.ascontiguousarray(stream)) == 0
    failures = 0
    for length in range(len(stream)):
        cut = np.ascontiguousarray(stream[:length]).copy()      # its own allocation: an over-read leaves the array
        failures += run(cut) != 0
    assert failures >= len(stream) - 4                  # all but the cuts inside the final EOI marker / padding
    start = bytes(stream).find(b'\xff\xda')
    start += 2 + ((int(stream[start + 2]) << 8) | int(stream[start + 3]))
    rng = np.random.RandomState(5)
    outcomes = set()
    for _ in range(2000):
        bad = stream.copy()
        bad[rng.randint(start, len(stream))] = rng.randint(256)
        outcomes.add(run(bad))
    assert outcomes <= {0, -3} and 0 in outcomes


def test_bytes_list_index(tmp_path, golden):
    frames = [bytes(golden[MG.GQN_CASES[i % len(MG.GQN_CASES)] + '_jpeg']) for i in range(10)]
    frames[3] = frames[3][:17]
    cameras = [float(i) for i in range(50)]
    path = str(tmp_path / 'one.tfrecord')
    MG.write_gqn_tfrecord(path, [(frames, cameras)])
    recs = [r.copy() for r in tfrecord.TFRecordReader(path, compression='auto')]
    assert len(recs) == 1
    rec = recs[0]
    off, length = tfrecord.find_bytes_list(rec, 'frames')
    offsets, lengths = np.zeros(16, dtype=np.int64), np.zeros(16, dtype=np.int64)
    count = ctypes.c_int()

    def index(payload_len, slots):
        _lib.call('gx_bytes_list_index', ctypes.c_void_p(rec.ctypes.data + off), payload_len, slots,
                  ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(lengths.ctypes.data), ctypes.byref(count))

    index(length, 16)
    assert count.value == 10
    for k in range(10):
        assert bytes(rec[off + offsets[k]:off + offsets[k] + lengths[k]]) == frames[k]
    index(length, 10)
    assert count.value == 10
    with pytest.raises(GenesisHipError, match='10 values, the caller gave 9 slots'):
        index(length, 9)
    with pytest.raises(GenesisHipError, match='malformed'):
        index(length - 5, 16)


def gqn_cfg(**kw):
    cfg = AttrDict(data_folder='/nowhere/gqn', img_size=64, val_frac=60, num_workers=4, buffer_size=128, K_steps=7, batch_size=32,
                   seed=0, debug=True)
    cfg.update(kw)
    return cfg


def test_gqn_flags_and_splits_with_no_data_read():
    import importlib
    import genesis_amd.gqn_config as Q
    from forge import flags
    # a flag keeps the default of the config that defined it first (one data config per process): define them afresh
    defaults = (('data_folder', 'data/gqn_datasets'), ('img_size', 64), ('val_frac', 60), ('num_workers', 4),
                ('buffer_size', 128), ('K_steps', 7))
    saved = {name: flags.FLAGS.pop(name) for name, _ in defaults if name in flags.FLAGS}
    try:
        Q = importlib.reload(Q)
        for name, default in defaults:
            assert flags.FLAGS[name] == default
    finally:
        flags.FLAGS.update(saved)
    base = '/nowhere/gqn/rooms_ring_camera'
    train = Q.file_list('/nowhere/gqn', 'train', 60)
    assert len(train) == 2160 and train[0] == base + '/train/0001-of-2160.tfrecord' and train[-1] == base + '/train/2160-of-2160.tfrecord'
    test = Q.file_list('/nowhere/gqn', 'test', 60)
    assert len(test) == 240 and test[0] == base + '/test/001-of-240.tfrecord' and test[-1] == base + '/test/240-of-240.tfrecord'
    dt = Q.file_list('/nowhere/gqn', 'devel_train', 60)
    dv = Q.file_list('/nowhere/gqn', 'devel_val', 60)
    assert dt == train[:2124] and dv == train[2124:] and len(dv) == 36
    assert Q.num_frames('train', 60) == 10800000 and Q.num_frames('test', 60) == 1200000
    assert Q.num_frames('devel_train', 60) == 10620000 and Q.num_frames('devel_val', 60) == 180000
    with pytest.raises(ValueError):
        Q.file_list('/nowhere/gqn', 'validation', 60)
    hosts, sizes = Q.host_splits(gqn_cfg())
    assert [h.files for h in hosts] == [dt, dv, test]
    assert [h.batch_size for h in hosts] == [32, 32, 1] and [h.workers for h in hosts] == [4, 4, 1]
    assert [h.shuffle_records for h in hosts] == [128 * 32, 0, 0]
    assert [n // h.batch_size for h, n in zip(hosts, sizes)] == [10620000 // 32, 180000 // 32, 1200000]
    # one process per GPU: every fourth file from the second
    hosts, sizes = Q.host_splits(gqn_cfg(num_workers=40), shard=(1, 4))
    assert [h.files for h in hosts] == [dt[1::4], dv[1::4], test[1::4]]
    assert sizes == (10620000 // 4, 180000 // 4, 1200000 // 4) and hosts[0].workers == 16
    assert Q.file_list('/nowhere/gqn', 'devel_train', 60, shard=(1, 4)) == dt[1::4]
    with pytest.raises(GenesisHipError, match='shard'):
        Q.host_splits(gqn_cfg(), shard=(4, 4))
    # a handful of tiny files
    hosts, sizes = Q.host_splits(gqn_cfg(val_frac=4, batch_size=2), train_files=4, test_files=1, records_per_file=5)
    assert [len(h.files) for h in hosts] == [3, 1, 1] and sizes == (15, 5, 5)
    assert hosts[2].files == ['/nowhere/gqn/rooms_ring_camera/test/1-of-1.tfrecord']


def write_gqn_files(tmp_path, golden):
    """3 train files x 5 records x 10 frames of the golden streams -> (paths, {(file, record, frame): case name})."""
    import genesis_amd.gqn_config as Q
    names = MG.GQN_CASES
    root = tmp_path / 'rooms_ring_camera' / 'train'
    root.mkdir(parents=True)
    which = {}
    files = Q.file_list(str(tmp_path), 'train', 60, train_files=3)
    for fi, path in enumerate(files):
        records = []
        for r in range(5):
            ks = [(7 * fi + 3 * r + f) % len(names) for f in range(10)]
            which.update({(fi, r, f): names[k] for f, k in enumerate(ks)})
            records.append(([bytes(golden[names[k] + '_jpeg']) for k in ks], [0.5] * 50))
        MG.write_gqn_tfrecord(path, records)
    return files, which


def test_gqn_host_stream_without_a_gpu(tmp_path, golden):
    """The host half end to end: order with one and with several readers, shuffling, frame choice, errors."""
    import genesis_amd.gqn_config as Q
    names = MG.GQN_CASES
    files, which = write_gqn_files(tmp_path, golden)

    def pixels(b):
        return [R.decode_pixels(c, q, *b['geometry']) for c, q in zip(b['coef'], b['qtab'])]

    for workers in (1, 3):
        batches = list(Q.HostBatches(files, 4, frame=3, num_workers=workers))
        assert [len(b['coef']) for b in batches] == [4, 4, 4, 3]
        index = np.concatenate([b['index'] for b in batches])
        assert index.tolist() == [[fi, r, 3] for fi in range(3) for r in range(5)]
        for b in batches:
            assert b['geometry'] == (64, 64, 2)
            for ix, px in zip(b['index'], pixels(b)):
                assert np.array_equal(px, golden[which[tuple(ix)] + '_rgb'])
    # shuffled: every record once, the same order for the same seed, another for another seed
    orders = [np.concatenate([b['index'] for b in Q.HostBatches(files, 4, shuffle_records=8, seed=s, num_workers=2)])
              for s in (1, 1, 2)]
    assert sorted(map(tuple, orders[0][:, :2].tolist())) == [(fi, r) for fi in range(3) for r in range(5)]
    assert orders[0].tolist() == orders[1].tolist() and orders[0][:, :2].tolist() != orders[2][:, :2].tolist()
    assert orders[0][:, :2].tolist() != [[fi, r] for fi in range(3) for r in range(5)]
    assert len(set(orders[0][:, 2].tolist())) > 1 and orders[0][:, 2].min() >= 0 and orders[0][:, 2].max() < 10
    # a record whose fourth frame is cut short
    frames = [bytes(golden[names[0] + '_jpeg'])] * 10
    frames[3] = frames[3][:200]
    MG.write_gqn_tfrecord(files[1], [(frames, [0.0] * 50)] * 2)
    with pytest.raises(tfrecord.TFRecordError, match=r'2-of-3\.tfrecord: record 0: frame 3: .*ends early'):
        list(Q.HostBatches(files, 4, frame=3, num_workers=2))
    assert len(list(Q.HostBatches(files, 4, frame=2, num_workers=2))) == 3


def pool_order(stream, N, seed):
    """The shuffle pool restated on lists: fill N rows without a draw, then one randint(N) per further record (the row it
    names is emitted and refilled), then one permutation of the filled rows at the end of the stream."""
    if N <= 1:
        return list(stream)
    rng, pool, out = np.random.RandomState(seed), [], []
    for x in stream:
        if len(pool) < N:
            pool.append(x)
        else:
            j = int(rng.randint(N))
            out.append(pool[j])
            pool[j] = x
    if pool:
        out += [pool[j] for j in rng.permutation(len(pool))]
    return out


@pytest.mark.parametrize('workers', [1, 3])
def test_gqn_shuffled_order_is_the_pools_draw_sequence(tmp_path, golden, workers):
    """Files of 5 records are one chunk each, so the stream into the pool is in file order with any number of readers."""
    import genesis_amd.gqn_config as Q
    files, _ = write_gqn_files(tmp_path, golden)
    stream = [[fi, r, 3] for fi in range(3) for r in range(5)]
    for seed in (0, 1):
        for N in (2, 8, 15, 64):
            batches = list(Q.HostBatches(files, 4, frame=3, shuffle_records=N, seed=seed, num_workers=workers))
            assert [len(b['index']) for b in batches] == [4, 4, 4, 3]
            assert np.concatenate([b['index'] for b in batches]).tolist() == pool_order(stream, N, seed), (seed, N)


def gqn_threads():
    import threading
    return [t.name for t in threading.enumerate() if t.name == 'gqn_merger' or t.name.startswith('gqn_reader_')]


def test_gqn_threads_end_when_the_epoch_is_abandoned_or_fails(tmp_path, golden, monkeypatch):
    import gc
    import genesis_amd.gqn_config as Q
    files, _ = write_gqn_files(tmp_path, golden)
    monkeypatch.setattr(Q, '_QUEUE_BATCHES', 1)             # 15 batches of 1 behind a queue of 1: the merger blocks on it,
    monkeypatch.setattr(Q, '_QUEUE_CHUNKS', 1)              # and so do the readers behind the merger
    monkeypatch.setattr(Q, 'CHUNK_RECORDS', 2)
    it = iter(Q.HostBatches(files, 1, frame=3, num_workers=3))
    assert next(it)['index'].tolist() == [[0, 0, 3]]
    assert 'gqn_merger' in gqn_threads()
    it.close()
    assert gqn_threads() == []
    it = iter(Q.HostBatches(files, 1, frame=3, num_workers=3))
    next(it)
    del it                                                  # dropped, not closed
    gc.collect()
    assert gqn_threads() == []
    # a reader's error raised in the consumer: the merger and all three readers have ended when it arrives
    frames = [bytes(golden[MG.GQN_CASES[0] + '_jpeg'])] * 10
    frames[3] = frames[3][:200]
    MG.write_gqn_tfrecord(files[1], [(frames, [0.0] * 50)] * 2)
    with pytest.raises(tfrecord.TFRecordError, match=r'2-of-3\.tfrecord: record 0: frame 3: .*ends early'):
        list(Q.HostBatches(files, 1, frame=3, num_workers=3))
    assert gqn_threads() == []
