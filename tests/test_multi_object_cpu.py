"""Host side of the multi-object TFRecord loader, without a GPU: CRC-32C, record framing, the tf.Example walk and the
bytes-list unpacker of the C ABI (genesis_amd/csrc/gx_tfrecord.cpp) through genesis_amd/tfrecord.py, and the split /
batch / shard / shuffle arithmetic of genesis_amd/multi_object_config.py on the host record stream.  The fixture files
come from tests/golden/make_golden_multi_object.py, whose encoder (google.protobuf + a table CRC) shares no code with the
reader."""
import ctypes
import io
import os
import os.path as osp
import shutil
import sys

import numpy as np
import pytest

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_multi_object as MG  # noqa: E402

from genesis_amd import _lib, tfrecord  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

FILES = {f[0]: f for f in MG.FILES}


def fixture_path(stem):
    return osp.join(GOLDEN, 'multi_object_%s.tfrecords' % stem)


def raw_stream(stem):
    """The uncompressed record stream of a fixture file."""
    import gzip
    data = open(fixture_path(stem), 'rb').read()
    return gzip.decompress(data) if FILES[stem][7] else data


def decode(records, stem):
    _, _, (H, W), E, _, _, _, _ = FILES[stem]
    images, masks = [], []
    for rec in records:
        images.append(tfrecord.unpack_bytes_list(rec, 'image', np.empty((H, W, 3), dtype=np.uint8)))
        masks.append(tfrecord.unpack_bytes_list(rec, 'mask', np.empty((E, H, W, 1), dtype=np.uint8)))
    return np.stack(images), np.stack(masks)


def test_crc32c_known_vectors():
    assert tfrecord.crc32c(b'123456789') == 0xE3069283
    assert tfrecord.crc32c(bytes(32)) == 0x8A9136AA
    assert tfrecord.crc32c(b'\xff' * 32) == 0x62A8AB43
    assert tfrecord.crc32c(b'') == 0
    c = 0xE3069283
    assert tfrecord.masked_crc32c(b'123456789') == (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xffffffff
    # every alignment and length of the sliced loop against the bytewise table of the fixture generator
    data = np.random.RandomState(0).randint(0, 256, 300).astype(np.uint8)
    for off in range(9):
        for n in (0, 1, 7, 8, 9, 63, 64, 65, 255):
            assert tfrecord.crc32c(data[off:off + n].copy()) == MG.crc32c(data[off:off + n].tobytes())
            a = data[off:off + n]                          # unaligned start inside the array
            assert int(_lib.load().gx_crc32c(ctypes.c_void_p(data.ctypes.data + off), a.size)) == MG.crc32c(a.tobytes())


@pytest.mark.parametrize('stem', sorted(FILES))
def test_fixture_files_decode_record_for_record(stem):
    g = np.load(osp.join(GOLDEN, 'multi_object_records.npz'))
    image, mask = decode(tfrecord.TFRecordReader(fixture_path(stem)), stem)
    assert image.shape[0] == FILES[stem][6]
    assert np.array_equal(image, g[stem + '_image']) and np.array_equal(mask, g[stem + '_mask'])
    gi, gm = MG.file_records(stem)                         # and the generator's seeded arrays are the stored ones
    assert np.array_equal(gi, image) and np.array_equal(gm, mask)


@pytest.mark.parametrize('stem', sorted(FILES))
@pytest.mark.parametrize('chunk', [1 << 22, 4097, 1013, 61])
def test_odd_sized_chunks_give_the_same_records(stem, chunk):
    if chunk == 61 and stem == 'tetrominoes':
        chunk = 331                                        # 624 KB in 61-byte reads only costs time
    want = [bytes(r) for r in tfrecord.TFRecordReader(fixture_path(stem))]
    got = [bytes(r) for r in tfrecord.TFRecordReader(fixture_path(stem), chunk_bytes=chunk, max_scan=3)]
    assert got == want
    got = [bytes(r) for r in tfrecord.TFRecordReader(io.BytesIO(raw_stream(stem)), compression='', chunk_bytes=chunk)]
    assert got == want


def record_spans(raw):
    """(start of the 12-byte header, data length) of every record of an uncompressed stream, parsed in Python."""
    spans, pos = [], 0
    while pos < len(raw):
        n = int.from_bytes(raw[pos:pos + 8], 'little')
        spans.append((pos, n))
        pos += 16 + n
    return spans


def read_all(raw, **kw):
    return [bytes(r) for r in tfrecord.TFRecordReader(io.BytesIO(raw), compression='', **kw)]


def test_corruption_and_truncation_raise_and_name_the_record():
    raw = bytearray(raw_stream('objects_room'))
    spans = record_spans(raw)
    assert len(spans) == 30
    start, n = spans[7]
    bad = bytearray(raw)
    bad[start + 12 + n // 2] ^= 0x40                                       # a data byte of record 7
    with pytest.raises(tfrecord.TFRecordError, match=r'record 7\b.*data bytes'):
        read_all(bytes(bad))
    assert len(read_all(bytes(bad), verify_crc=False)) == 30               # unchecked on request
    bad = bytearray(raw)
    bad[spans[11][0] + 1] ^= 0x01                                          # a length byte of record 11
    with pytest.raises(tfrecord.TFRecordError, match=r'record 11\b.*length'):
        read_all(bytes(bad))
    cut = bytes(raw[:spans[20][0] + 12 + spans[20][1] // 3])               # the file ends inside record 20
    with pytest.raises(tfrecord.TFRecordError, match=r'record 20\b'):
        read_all(cut)
    assert len(read_all(bytes(raw[:spans[20][0]]))) == 20                  # a cut between records is a shorter file


def test_truncated_gzip_raises_and_names_the_record(tmp_path):
    data = open(fixture_path('objects_room'), 'rb').read()
    p = tmp_path / 'cut.tfrecords'
    p.write_bytes(data[:len(data) // 2])
    n = 0
    with pytest.raises(tfrecord.TFRecordError, match=r'record \d+') as e:
        for _ in tfrecord.TFRecordReader(str(p)):
            n += 1
    assert 0 < n < 30 and ('record %d' % n) in str(e.value)


def varint(v):
    out = bytearray()
    while True:
        out.append((v & 0x7f) | (0x80 if v > 0x7f else 0))
        v >>= 7
        if not v:
            return bytes(out)


def ld(field, payload):
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def example(features):
    """A tf.Example from {name: Feature payload}."""
    return ld(1, b''.join(ld(1, ld(1, k.encode()) + ld(2, v)) for k, v in features.items()))


def bytes_feature(values):
    return ld(1, b''.join(ld(1, v) for v in values))


def test_length_two_value_inside_image_is_rejected_by_the_size_check():
    ok = example({'image': bytes_feature([b'\x05', b'\x06', b'\x07', b'\x08'])})
    out = np.zeros(4, dtype=np.uint8)
    assert tfrecord.unpack_bytes_list(ok, 'image', out).tolist() == [5, 6, 7, 8]
    two = example({'image': bytes_feature([b'\x05', b'\x06\x09', b'\x07', b'\x08'])})
    with pytest.raises(tfrecord.TFRecordError, match='holds 5 bytes, expected 4'):
        tfrecord.unpack_bytes_list(two, 'image', out)
    # the general path concatenates values of any length when the total is right, also when the total is 3 x expected / 3
    mixed = example({'image': bytes_feature([b'\x01\x02', b'', b'\x03\x04'])})
    assert tfrecord.unpack_bytes_list(mixed, 'image', out).tolist() == [1, 2, 3, 4]
    # 12 payload bytes for 4 expected, but not the one-byte stride: 3 + 1 bytes in values of other lengths
    same_size = example({'image': ld(1, ld(1, b'\x0a\x01\x07') + ld(1, b'\x09') + ld(7, b'\x00\x00'))})
    assert tfrecord.find_bytes_list(same_size, 'image')[1] == 12
    assert tfrecord.unpack_bytes_list(same_size, 'image', out).tolist() == [0x0a, 0x01, 0x07, 0x09]
    with pytest.raises(tfrecord.TFRecordError):
        tfrecord.unpack_bytes_list(example({'image': bytes_feature([b'\x01'] * 3)}), 'image', out)


def test_walker_skips_other_features_and_refuses_malformed_input():
    import struct
    floats = ld(2, ld(1, struct.pack('<3f', 1.0, 2.0, 3.0)))                                  # packed float_list
    floats_unpacked = ld(2, b''.join(varint(1 << 3 | 5) + struct.pack('<f', v) for v in (1.0, 2.0)))
    ints = ld(3, varint(1 << 3 | 0) + varint(1 << 40) + varint(1 << 3 | 0) + varint((1 << 64) - 1))
    rec = example({'x': floats, 'y': floats_unpacked, 'n': ints, 'mask': bytes_feature([b'\xff', b'\x00']),
                   'image': bytes_feature([b'\x09'])})
    rec = varint(9 << 3 | 1) + bytes(8) + rec + varint(8 << 3 | 5) + bytes(4)                 # unknown top-level fields
    out = np.zeros(2, dtype=np.uint8)
    assert tfrecord.unpack_bytes_list(rec, 'mask', out).tolist() == [255, 0]
    off, n = tfrecord.find_bytes_list(rec, 'image')
    assert rec[off:off + n] == b'\x0a\x01\x09'
    with pytest.raises(_lib.GenesisHipError, match="no feature 'depth'"):
        tfrecord.find_bytes_list(rec, 'depth')
    with pytest.raises(_lib.GenesisHipError, match='not a bytes_list'):
        tfrecord.find_bytes_list(rec, 'x')
    # every truncation of the record is an error or a clean miss, never an over-read; so is a length that runs past the end
    for cut in range(len(rec)):
        try:
            off, n = tfrecord.find_bytes_list(rec[:cut], 'image')
            assert off + n <= cut
        except _lib.GenesisHipError:
            pass
    with pytest.raises(_lib.GenesisHipError, match='malformed'):
        tfrecord.find_bytes_list(varint(1 << 3 | 2) + varint(1000) + b'\x00' * 10, 'image')
    with pytest.raises(_lib.GenesisHipError, match='malformed'):
        tfrecord.find_bytes_list(varint(1 << 3 | 2) + b'\xff' * 11, 'image')                  # a varint that never ends
    with pytest.raises(_lib.GenesisHipError, match='malformed'):
        tfrecord.find_bytes_list(varint(1 << 3 | 3) + b'\x00', 'image')                       # a group
    with pytest.raises(tfrecord.TFRecordError, match='malformed'):
        tfrecord.unpack_bytes_list(example({'image': ld(1, varint(1 << 3 | 2) + varint(50) + b'\x01')}), 'image', out)


# ---- the data config on the host record stream ----
def make_cfg(tmp_path, dataset='objects_room', **kw):
    import genesis_amd.multi_object_config as M
    d = M.DATASETS[dataset]
    dst = str(tmp_path) + d['file']
    os.makedirs(osp.dirname(dst), exist_ok=True)
    shutil.copy(fixture_path(dataset), dst)
    cfg = AttrDict(data_folder=str(tmp_path), dataset=dataset, img_size=-1, dataset_size=-1, num_workers=4, buffer_size=2,
                   K_steps=-1, batch_size=4, seed=0, debug=True)
    cfg.update(kw)
    return cfg


def epoch(host):
    batches = list(host)
    return batches, np.concatenate([b['index'] for b in batches]) if batches else np.zeros(0, dtype=np.int64)


def test_flags_register_with_the_reference_defaults():
    import genesis_amd.multi_object_config as M
    from forge import flags
    want = dict(data_folder='data/multi-object-datasets', dataset='objects_room', img_size=-1, dataset_size=-1, num_workers=4,
                buffer_size=128, K_steps=-1)
    for k, v in want.items():
        assert flags.FLAGS[k] == v, k
    assert M.OBJECTS_ROOM == '/objects_room/objects_room_train.tfrecords'
    assert M.CLEVR == '/clevr_with_masks/clevr_with_masks_train.tfrecords'
    assert M.TETROMINOS == '/tetrominoes/tetrominoes_train.tfrecords'
    assert M.MULTI_DSPRITES == '/multi_dsprites/multi_dsprites_colored_on_colored.tfrecords'
    rules = {k: (d['img_size'], d['K_steps'], d['background_entities'], d['max_frames']) for k, d in M.DATASETS.items()}
    assert rules == {'multi_dsprites': (64, 5, 1, 60000), 'objects_room': (64, 7, 4, 1000000), 'clevr': (128, 11, 1, 70000),
                     'tetrominoes': (32, 4, 1, 60000)}
    assert M.CLEVR_CROP == 192
    # img_size is compared with the frame height before the crop: CLEVR at 240 comes out 192 x 192
    assert M.output_size((240, 320), 240) == ((24, 64, 192, 192), None, 192)
    assert M.output_size((240, 320), 128) == ((24, 64, 192, 192), 128, 128)
    assert M.output_size((240, 320), 192) == ((24, 64, 192, 192), 192, 192)
    assert M.output_size((64, 64), 64) == (None, None, 64) and M.output_size((35, 35), 32) == (None, 32, 32)
    with pytest.raises(NotImplementedError):
        M.configure(AttrDict(dataset='gqn', img_size=-1, K_steps=-1, dataset_size=-1))


def test_split_len_short_last_batch_and_dataset_size(tmp_path):
    import genesis_amd.multi_object_config as M
    g = np.load(osp.join(GOLDEN, 'multi_object_records.npz'))
    cfg = make_cfg(tmp_path)
    (tng, val, tst), sizes = M.host_splits(cfg, val_size=6, test_size=5, shuffle=False)
    assert (cfg.img_size, cfg.K_steps) == (64, 7)
    assert sizes == (1000000 - 11, 6, 5)                    # counted from max_frames, as the reference does
    for host, lo, hi in ((tst, 0, 5), (val, 5, 11), (tng, 11, 30)):
        batches, idx = epoch(host)
        assert idx.tolist() == list(range(lo, hi))
        assert [len(b['index']) for b in batches] == [4] * ((hi - lo) // 4) + ([(hi - lo) % 4] if (hi - lo) % 4 else [])
        for b in batches:
            assert b['input'].dtype == np.uint8 and b['input'].shape[1:] == (64, 64, 3)
            assert b['masks'].dtype == np.uint8 and b['masks'].shape[1:] == (7, 64, 64, 1)
            assert np.array_equal(b['input'], g['objects_room_image'][b['index']])
            assert np.array_equal(b['masks'], g['objects_room_mask'][b['index']])
    # dataset_size cuts the stream: 25 records -> 5 / 6 / 14, and the lengths follow
    cfg = make_cfg(tmp_path, dataset_size=25)
    (tng, val, tst), sizes = M.host_splits(cfg, val_size=6, test_size=5, shuffle=False)
    assert sizes == (14, 6, 5)
    assert epoch(tng)[1].tolist() == list(range(11, 25))
    assert [len(b['index']) for b in epoch(tng)[0]] == [4, 4, 4, 2]
    assert tng.num_records(30) == 14 and val.num_records(30) == 6 and tst.num_records(8) == 5
    with pytest.raises(AssertionError):
        M.host_splits(make_cfg(tmp_path, dataset_size=11), val_size=6, test_size=5)
    cfg = make_cfg(tmp_path, dataset_size=2000000)
    M.configure(cfg)
    assert cfg.dataset_size == 1000000


def test_shards_partition_each_split(tmp_path):
    import genesis_amd.multi_object_config as M
    seen = []
    for rank in range(3):
        cfg = make_cfg(tmp_path)
        (tng, val, tst), _ = M.host_splits(cfg, val_size=6, test_size=5, shard=(rank, 3), shuffle=False)
        idx = epoch(tng)[1]
        assert idx.tolist() == [i for i in range(11, 30) if (i - 11) % 3 == rank]
        assert tng.num_records(30) == len(idx)
        assert epoch(val)[1].tolist() == [i for i in range(5, 11) if (i - 5) % 3 == rank]
        seen.append(idx)
    assert sorted(np.concatenate(seen).tolist()) == list(range(11, 30))
    with pytest.raises(_lib.GenesisHipError, match='shard'):
        M.host_splits(make_cfg(tmp_path), val_size=6, test_size=5, shard=(3, 3))


def test_shuffle_is_seeded_and_every_epoch_a_permutation(tmp_path):
    import genesis_amd.multi_object_config as M
    g = np.load(osp.join(GOLDEN, 'multi_object_records.npz'))

    def train(seed, buffer_size=2):
        cfg = make_cfg(tmp_path, seed=seed, buffer_size=buffer_size)
        return M.host_splits(cfg, val_size=6, test_size=5)[0][0]

    host = train(0)
    assert host.shuffle_records == 8                        # buffer_size * batch_size
    b1, e1 = epoch(host)
    b2, e2 = epoch(host)
    assert e1.tolist() == e2.tolist() and e1.tolist() == epoch(train(0))[1].tolist()
    assert sorted(e1.tolist()) == list(range(11, 30)) and e1.tolist() != list(range(11, 30))
    e3 = epoch(train(1))[1]
    assert sorted(e3.tolist()) == list(range(11, 30)) and e3.tolist() != e1.tolist()
    assert [len(b['index']) for b in b1] == [4, 4, 4, 4, 3]
    for b in b1:                                             # the rows travel with their indices through the pool
        assert np.array_equal(b['input'], g['objects_room_image'][b['index']])
        assert np.array_equal(b['masks'], g['objects_room_mask'][b['index']])
    # a pool of 8 records cannot move a record more than the pool ahead of its turn; a pool larger than the split can
    assert all(int(i) - 11 <= pos + 8 for pos, i in enumerate(e1))
    big = epoch(train(0, buffer_size=100))[1]
    assert sorted(big.tolist()) == list(range(11, 30))


def test_reader_errors_reach_the_consumer_and_the_thread_ends(tmp_path):
    import threading
    import genesis_amd.multi_object_config as M
    cfg = make_cfg(tmp_path)
    path = cfg.data_folder + M.OBJECTS_ROOM
    data = open(path, 'rb').read()
    open(path, 'wb').write(data[:len(data) // 2])
    (tng, val, tst), _ = M.host_splits(cfg, val_size=6, test_size=5, shuffle=False)
    with pytest.raises(tfrecord.TFRecordError, match=r'record \d+'):
        list(tng)
    it = iter(tst)                                           # an epoch abandoned after one batch
    next(it)
    it.close()
    assert not [t for t in threading.enumerate() if t.name == 'multi_object_reader']
    # a file of another geometry fails the size check, with the record named
    cfg = make_cfg(tmp_path, dataset='tetrominoes')
    shutil.copy(fixture_path('objects_room'), cfg.data_folder + M.TETROMINOS)
    (tng, val, tst), _ = M.host_splits(cfg, val_size=6, test_size=5, shuffle=False)
    with pytest.raises(tfrecord.TFRecordError, match=r'record 0: .*expected 3675'):
        list(tst)


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


# (start, stop, shard) and four pool sizes: smaller than the records the split keeps, smaller, equal, larger
@pytest.mark.parametrize('start, stop, shard, pools', [(5, 11, None, (2, 4, 6, 64)), (11, None, None, (2, 8, 19, 64)),
                                                       (11, 30, (1, 2), (2, 4, 9, 64))])
def test_shuffled_order_is_the_pools_draw_sequence(start, stop, shard, pools):
    import genesis_amd.multi_object_config as M
    g = np.load(osp.join(GOLDEN, 'multi_object_records.npz'))
    rank, world = shard or (0, 1)
    stream = [i for i in range(start, 30 if stop is None else stop) if (i - start) % world == rank]
    for seed in (0, 1):
        for N in pools:
            host = M.HostBatches(fixture_path('objects_room'), (64, 64), 7, 'ehw', start, stop, 4, N, seed, shard)
            batches, idx = epoch(host)
            # with `stop` given the pool never has more rows than the split can fill, which sets randint's range
            rows = N if stop is None else max(2, min(N, -(-(stop - start) // world)))
            assert idx.tolist() == pool_order(stream, rows, seed), (seed, N)
            assert [len(b['index']) for b in batches] == [4] * (len(stream) // 4) + [len(stream) % 4] * (len(stream) % 4 > 0)
            for b in batches:
                assert np.array_equal(b['input'], g['objects_room_image'][b['index']])
                assert np.array_equal(b['masks'], g['objects_room_mask'][b['index']])


def test_reader_thread_ends_when_the_epoch_is_abandoned(monkeypatch):
    import gc
    import threading
    import genesis_amd.multi_object_config as M

    def readers():
        return [t for t in threading.enumerate() if t.name == 'multi_object_reader']

    monkeypatch.setattr(M, '_QUEUE_BATCHES', 1)             # 30 batches of 1 behind a queue of 1: the reader blocks on it
    for shuffle_records in (0, 8):
        host = M.HostBatches(fixture_path('objects_room'), (64, 64), 7, 'ehw', 0, None, 1, shuffle_records)
        it = iter(host)
        next(it)
        assert len(readers()) == 1
        it.close()
        assert not readers()
        it = iter(host)
        next(it)
        del it                                              # dropped, not closed
        gc.collect()
        assert not readers()
