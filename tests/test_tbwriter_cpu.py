"""genesis_amd.tbwriter without a GPU: the file name and framing, event order, both decoders (the restatement's and, where it
imports, google.protobuf with message classes built here from the published field numbers), the host picture path against the
restatement byte for byte, histograms, every refusal that needs no device, and the descriptor constants against the header."""
import ctypes
import io
import os
import os.path as osp
import re
import struct

import numpy as np
import pytest
import torch

from genesis_amd import _lib, tbwriter
from genesis_amd import tfrecord
from genesis_amd._lib import GenesisHipError
from genesis_amd.tbwriter import SummaryWriter, read_events
from tests import hist_restatement as HR
from tests import png_restatement as PR
from tests import tbwriter_restatement as R

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes() or (a != a and b != b)


# ---- google.protobuf message classes from the published field numbers ------------------------------------------------------------
def protobuf_event_class():
    pytest.importorskip('google.protobuf')
    from google.protobuf import descriptor_pb2, descriptor_pool
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name='tbwriter_test_%d.proto' % os.getpid(), package='tbwriter_test', syntax='proto3')

    def message(parent, name, fields):
        m = parent.message_type.add() if hasattr(parent, 'message_type') else parent.nested_type.add()
        m.name = name
        for fname, number, ftype, extra in fields:
            f = m.field.add(name=fname, number=number, type=ftype,
                            label=F.LABEL_REPEATED if extra.get('repeated') else F.LABEL_OPTIONAL)
            if 'type_name' in extra:
                f.type_name = extra['type_name']
        return m

    message(fd, 'HistogramProto', [('min', 1, F.TYPE_DOUBLE, {}), ('max', 2, F.TYPE_DOUBLE, {}), ('num', 3, F.TYPE_DOUBLE, {}),
                                   ('sum', 4, F.TYPE_DOUBLE, {}), ('sum_squares', 5, F.TYPE_DOUBLE, {}),
                                   ('bucket_limit', 6, F.TYPE_DOUBLE, dict(repeated=True)),
                                   ('bucket', 7, F.TYPE_DOUBLE, dict(repeated=True))])
    summary = message(fd, 'Summary', [('value', 1, F.TYPE_MESSAGE, dict(repeated=True, type_name='.tbwriter_test.Summary.Value'))])
    message(summary, 'Image', [('height', 1, F.TYPE_INT32, {}), ('width', 2, F.TYPE_INT32, {}), ('colorspace', 3, F.TYPE_INT32, {}),
                               ('encoded_image_string', 4, F.TYPE_BYTES, {})])
    message(summary, 'Value', [('tag', 1, F.TYPE_STRING, {}), ('simple_value', 2, F.TYPE_FLOAT, {}),
                               ('image', 4, F.TYPE_MESSAGE, dict(type_name='.tbwriter_test.Summary.Image')),
                               ('histo', 5, F.TYPE_MESSAGE, dict(type_name='.tbwriter_test.HistogramProto'))])
    message(fd, 'Event', [('wall_time', 1, F.TYPE_DOUBLE, {}), ('step', 2, F.TYPE_INT64, {}), ('file_version', 3, F.TYPE_STRING, {}),
                          ('summary', 5, F.TYPE_MESSAGE, dict(type_name='.tbwriter_test.Summary'))])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    desc = pool.FindMessageTypeByName('tbwriter_test.Event')
    try:
        from google.protobuf import message_factory
        if hasattr(message_factory, 'GetMessageClass'):
            return message_factory.GetMessageClass(desc)
        return message_factory.MessageFactory(pool).GetPrototype(desc)
    except ImportError:      # pragma: no cover
        pytest.skip('google.protobuf has no message factory')


def protobuf_events(path):
    Event = protobuf_event_class()
    with open(path, 'rb') as f:
        return [Event.FromString(r) for r in R.split_records(f.read())]


# ---- framing and order ---------------------------------------------------------------------------------------------------------
def test_file_name_first_event_and_no_truncation(tmp_path, monkeypatch):
    monkeypatch.setattr(tbwriter.time, 'time', lambda: 1700000000.25)
    monkeypatch.setattr(tbwriter.socket, 'gethostname', lambda: 'boxname')
    paths = []
    for k in range(3):      # three writers in the same second
        with SummaryWriter(str(tmp_path / 'run'), filename_suffix='.sfx') as w:
            w.add_scalar('x', float(k), k)
            paths.append(w.path)
    names = [osp.basename(p) for p in paths]
    assert names == ['events.out.tfevents.1700000000.boxname.sfx', 'events.out.tfevents.1700000000.boxname.sfx.1',
                     'events.out.tfevents.1700000000.boxname.sfx.2']
    assert re.fullmatch(r'events\.out\.tfevents\.\d{10}\.boxname\.sfx', names[0])
    for k, p in enumerate(paths):      # none of them lost its contents
        events = R.read_file(p)
        assert events[0]['file_version'] == 'brain.Event:2' and events[0]['wall_time'] == 1700000000.25 and events[0]['values'] == []
        assert [v['simple_value'] for v in events[1]['values']] == [np.float32(k)] and events[1]['step'] == k
    assert sorted(os.listdir(str(tmp_path / 'run'))) == sorted(names)


def test_default_logdir(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(tbwriter.socket, 'gethostname', lambda: 'boxname')
    with SummaryWriter(comment='_c') as w:
        assert re.fullmatch(r'runs[/\\].+_boxname_c', w.logdir) and osp.isfile(w.path)


STEPS = [0, 1, 7, 1 << 32, (1 << 40) + 3, -1, -(1 << 35), None]
SCALARS = [0.0, 1.5, float('inf'), float('-inf'), float('nan'), 1e39, -1e39, np.float64(3.25), np.float32(-2.5), np.int64(7), 10 ** 400,
           torch.tensor(0.125), torch.tensor([9], dtype=torch.int32), np.array([[2.0]]), True, 16777217]


@pytest.fixture
def mixed_file(tmp_path):
    """One file with every kind of event, host values only -> (path, the calls made)."""
    calls = []
    rng = np.random.RandomState(3)
    with SummaryWriter(str(tmp_path)) as w:
        for i, step in enumerate(STEPS):
            w.add_scalar('s/%d' % i, float(i), step, walltime=100.0 + i)
            calls.append(('scalar', 's/%d' % i, np.float32(i), step or 0, 100.0 + i))
        for i, v in enumerate(SCALARS):
            w.add_scalar('v/%d' % i, v, 5)
            with np.errstate(over='ignore'):
                want = np.float32(np.inf) if isinstance(v, int) and v > 1e300 else np.float32(np.asarray(v, dtype=np.float64).reshape(-1)[0]
                                                                                             if not torch.is_tensor(v) else v.item())
            calls.append(('scalar', 'v/%d' % i, want, 5, None))
        img = rng.rand(3, 5, 9).astype(np.float32)
        w.add_image('img/chw', img, 11, walltime=7.5)
        calls.append(('image', 'img/chw', (5, 9, 3), 11, 7.5))
        w.add_image('img/hw', torch.from_numpy(img[0]), dataformats='HW')
        calls.append(('image', 'img/hw', (5, 9, 1), 0, None))
        v = rng.randn(500)
        w.add_histogram('h/host', v, 12)
        calls.append(('histo', 'h/host', v, 12, None))
        w.add_histogram_raw('h/raw', -1.5, 2.5, 10, 3.0, 12.25, [-1.0, 0.0, 3.0], [0, 4, 6], 13, walltime=9.0)
        calls.append(('raw', 'h/raw', (-1.5, 2.5, 10.0, 3.0, 12.25, [-1.0, 0.0, 3.0], [0.0, 4.0, 6.0]), 13, 9.0))
        w.add_scalars_dict({'a': 1.0, 'b': torch.tensor(2.0), 'c': np.float32(3.0)}, 'grp', 14)
        for key, val in (('a', 1.0), ('b', 2.0), ('c', 3.0)):
            calls.append(('scalar', 'grp/' + key, np.float32(val), 14, None))
        assert w.stats['events'] == 1 + len(calls) and w.stats['snapshot_launches'] == 0 and w.stats['pack_launches'] == 0
        path, file_bytes = w.path, w.stats['file_bytes']
    assert osp.getsize(path) == file_bytes
    return path, calls


def test_events_in_call_order_by_every_decoder(mixed_file):
    path, calls = mixed_file
    data = open(path, 'rb').read()
    records = R.split_records(data)                                                      # both checksums, bit by bit
    assert [bytes(r) for r in tfrecord.TFRecordReader(path, compression='')] == records   # ... and by the library's reader
    mine = [R.decode_event(r) for r in records]
    theirs = list(read_events(path))
    assert len(mine) == len(theirs) == 1 + len(calls)
    assert mine[0]['file_version'] == theirs[0]['file_version'] == 'brain.Event:2'
    for e, t, (kind, tag, want, step, wall) in zip(mine[1:], theirs[1:], calls):
        assert e['step'] == t['step'] == step and e['file_version'] is None and 'file_version' not in t
        assert e['wall_time'] == t['wall_time'] and (wall is None or e['wall_time'] == wall)
        assert len(e['values']) == 1 and e['values'][0]['tag'] == tag
        v = e['values'][0]
        if kind == 'scalar':
            assert same_bits(v['simple_value'], want), (tag, v['simple_value'], want)
            assert [x[0] for x in t['scalars']] == [tag] and same_bits(t['scalars'][0][1], want)
            assert t['images'] == [] and t['histograms'] == []
        elif kind == 'image':
            H, W, C = want
            assert (v['image']['height'], v['image']['width'], v['image']['colorspace']) == (H, W, C)
            assert t['images'] == [(tag, v['image'])]
        elif kind == 'histo':
            HR.assert_matches(dict(v['histo'], bucket_limits=v['histo']['bucket_limit'], bucket_counts=v['histo']['bucket']), want, what=tag)
            assert t['histograms'] == [(tag, v['histo'])]
        else:
            h = v['histo']
            assert (h['min'], h['max'], h['num'], h['sum'], h['sum_squares'], h['bucket_limit'], h['bucket']) == want
            assert t['histograms'] == [(tag, h)]
    # the values that must saturate and not raise
    got = {v['tag']: v['simple_value'] for e in mine[1:] for v in e['values'] if 'simple_value' in v}
    assert got['v/5'] == np.inf and got['v/6'] == -np.inf and got['v/10'] == np.inf and got['v/4'] != got['v/4']
    assert got['v/15'] == np.float32(16777216.0) and got['v/12'] == 9.0 and got['v/14'] == 1.0


def test_google_protobuf_reads_the_same(mixed_file):
    path, calls = mixed_file
    events = protobuf_events(path)
    mine = R.read_file(path)
    assert len(events) == len(mine)
    assert events[0].file_version == 'brain.Event:2'
    for pb, e in zip(events, mine):
        assert pb.wall_time == e['wall_time'] and pb.step == e['step'] and len(pb.summary.value) == len(e['values'])
        for pv, v in zip(pb.summary.value, e['values']):
            assert pv.tag == v['tag']
            if 'simple_value' in v:
                assert same_bits(pv.simple_value, v['simple_value'])
            if 'image' in v:
                assert (pv.image.height, pv.image.width, pv.image.colorspace, pv.image.encoded_image_string) == \
                       (v['image']['height'], v['image']['width'], v['image']['colorspace'], v['image']['encoded_image_string'])
            if 'histo' in v:
                h = v['histo']
                for key in ('min', 'max', 'num', 'sum', 'sum_squares'):
                    assert struct.pack('<d', getattr(pv.histo, key)) == struct.pack('<d', h[key])
                assert list(pv.histo.bucket_limit) == h['bucket_limit'] and list(pv.histo.bucket) == h['bucket']
    steps = [pb.step for pb in events[1:1 + len(STEPS)]]
    assert steps == [s or 0 for s in STEPS]


def test_negative_steps_take_ten_bytes():
    assert len(tbwriter._varint(-1)) == 10 and tbwriter._varint(-1) == b'\xff' * 9 + b'\x01'
    assert tbwriter._varint(300) == b'\xac\x02' and tbwriter._varint(0) == b'\x00'
    assert R.masked_crc32c(b'123456789') == tbwriter._masked_crc(b'123456789')
    assert R.crc32c(b'123456789') == 0xe3069283      # the check value of CRC-32C


# ---- pictures on the host path ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 64), (5, 65), (3, 300)]


def decode(png, H, W, C):
    w, h, colour, stream = R.png_parts(png)
    assert (w, h, colour) == (W, H, 2 if C == 3 else 0) and len(stream) == H * (1 + W * C)
    return PR.unfilter(np.frombuffer(stream, np.uint8), H, W, C), stream


@pytest.mark.parametrize('kind', ['fp32', 'uint8', 'int64'])
@pytest.mark.parametrize('C', [1, 3])
def test_host_pictures(tmp_path, kind, C):
    cases = []
    with SummaryWriter(str(tmp_path)) as w:
        for si, (H, W) in enumerate(SHAPES):
            hwc = R.picture(kind, C, H, W, 10 * si + C)
            for dataformats in (('CHW', 'HWC', 'HW') if C == 1 else ('CHW', 'HWC')):
                a = R.as_format(hwc, dataformats)
                tag = '%s/%dx%d/%s' % (kind, H, W, dataformats)
                w.add_image(tag, torch.from_numpy(a) if si % 2 else a, si, dataformats=dataformats)
                cases.append((tag, a, dataformats, H, W))
        path = w.path
    events = R.read_file(path)[1:]
    assert len(events) == len(cases)
    for e, (tag, a, dataformats, H, W) in zip(events, cases):
        v = e['values'][0]
        assert v['tag'] == tag and (v['image']['height'], v['image']['width'], v['image']['colorspace']) == (H, W, C)
        want = R.quantise(a, dataformats)
        assert want.shape == (H, W, C)
        got, stream = decode(v['image']['encoded_image_string'], H, W, C)
        assert np.array_equal(got, want), tag
        assert stream == R.pack_rows(want), tag


def test_pillow_decodes_the_pictures(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    cases = []
    with SummaryWriter(str(tmp_path)) as w:
        for kind in ('fp32', 'uint8', 'int64'):
            for C in (1, 3):
                for si, (H, W) in enumerate(SHAPES):
                    hwc = R.picture(kind, C, H, W, 7 * si + C)
                    w.add_image('p', hwc, dataformats='HWC')
                    cases.append((hwc, H, W, C))
        path = w.path
    for e, (hwc, H, W, C) in zip(list(read_events(path))[1:], cases):
        png = e['images'][0][1]['encoded_image_string']
        pil = Image.open(io.BytesIO(png))
        assert pil.mode == ('RGB' if C == 3 else 'L') and pil.size == (W, H)
        assert np.array_equal(np.asarray(pil).reshape(H, W, C), R.quantise(hwc, 'HWC'))


def test_byte_rule_by_hand():
    x = np.array([[-1.0, 0.0, 0.5, 0.999, 1.0, 2.0, np.nan, 1 / 255, 254.9999 / 255, np.inf, -np.inf, 0.0039]], np.float32)
    want = [0, 0, 127, 254, 255, 255, 0, 1, 254, 255, 0, 0]
    assert R.quantise(x, 'HW').reshape(-1).tolist() == want
    assert tbwriter._quantise_host(x, 'HW').reshape(-1).tolist() == want
    i = np.array([[-5, 0, 7, 255, 256, 1 << 40]], np.int64)
    assert R.quantise(i, 'HW').reshape(-1).tolist() == tbwriter._quantise_host(i, 'HW').reshape(-1).tolist() == [0, 0, 7, 255, 255, 255]
    assert tbwriter._quantise_host(np.array([[1, 300]], np.int32), 'HW').reshape(-1).tolist() == [1, 255]
    assert tbwriter._quantise_host(np.array([[0.5]], np.float64), 'HW').reshape(-1).tolist() == [127]


def test_ties_go_to_the_lowest_filter():
    """A constant row under a different constant row: None costs 40 per byte, Sub 40 once per channel, Up 10 per byte ...; rows
    made so that two filters tie."""
    zeros = np.zeros((2, 6, 1), np.uint8)                       # every filter costs 0: None (0) wins
    assert R.filter_costs(zeros) == [[0] * 5] * 2
    assert tbwriter.pack_rows_host(zeros) == R.pack_rows(zeros) == bytes(14)
    tie = np.array([[[10], [10], [10], [10]], [[20], [20], [20], [20]]], np.uint8)
    costs = R.filter_costs(tie)
    assert costs[0] == [40, 10, 40, 25, 10]      # first row: Sub ties with Paeth; Sub (1) wins
    assert costs[1] == [80, 20, 40, 30, 10]      # second row: Paeth alone
    stream = tbwriter.pack_rows_host(tie)
    assert stream == R.pack_rows(tie) == bytes([1, 10, 0, 0, 0, 4, 10, 0, 0, 0])
    one = np.array([[[200]], [[200]]], np.uint8)               # 1 x 1 rows: row 0 every filter costs 56; row 1: Up ties with Paeth at 0
    assert R.filter_costs(one) == [[56] * 5, [56, 56, 0, 100, 0]]
    stream = tbwriter.pack_rows_host(one)
    assert stream == R.pack_rows(one) == bytes([0, 200, 2, 0])
    forced = tbwriter.pack_rows_host(tie, force_filter=0)
    assert forced == bytes([0, 10, 10, 10, 10, 0, 20, 20, 20, 20])


# ---- histograms ------------------------------------------------------------------------------------------------------------------
def test_host_histogram_equals_the_restatement(tmp_path):
    rng = np.random.RandomState(5)
    cases = [('normal', rng.randn(3000).astype(np.float32)), ('f64', rng.randn(40, 5) * 1e-3), ('zeros', np.zeros(17, np.float32)),
             ('tensor', torch.from_numpy(rng.rand(100).astype(np.float32))), ('ints', np.arange(-5, 6))]
    with SummaryWriter(str(tmp_path)) as w:
        for tag, v in cases:
            w.add_histogram(tag, v, 3)
        w.add_histogram('edges', np.array([0.1, 0.6, 2.0]), 4, bins=[0.0, 0.5, 1.0, 4.0])
        path = w.path
    events = R.read_file(path)[1:]
    for e, (tag, v) in zip(events, cases):
        h = e['values'][0]['histo']
        assert e['values'][0]['tag'] == tag and e['step'] == 3
        values = v.numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64 if np.asarray(v).dtype.kind in 'iu' else None)
        HR.assert_matches(dict(h, bucket_limits=h['bucket_limit'], bucket_counts=h['bucket']), values, what=tag)
    h = events[-1]['values'][0]['histo']
    assert h['bucket_limit'] == [0.0, 0.5, 1.0, 4.0] and h['bucket'] == [0.0, 1.0, 1.0, 1.0] and h['num'] == 3.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('call, message', [
    (lambda w: w.add_scalar('', 1.0), "add_scalar: tag=''"),
    (lambda w: w.add_scalar(None, 1.0), 'add_scalar: tag=None'),
    (lambda w: w.add_scalar('t', torch.zeros(2)), r"add_scalar: value of shape \(2,\) for 't'; expected one element"),
    (lambda w: w.add_scalar('t', np.zeros(3)), 'add_scalar: value of shape'),
    (lambda w: w.add_scalar('t', 'text'), "add_scalar: value='text'"),
    (lambda w: w.add_scalars_dict({'k': torch.zeros(2)}, 'g'), "add_scalars_dict: value of shape .* for 'g/k'"),
    (lambda w: w.add_image('', np.zeros((3, 4, 4))), "add_image: tag=''"),
    (lambda w: w.add_image('t', np.zeros((2, 4, 4))), 'add_image: img of shape .* C = 2 is neither 1 nor 3'),
    (lambda w: w.add_image('t', np.zeros((4, 4, 4)), dataformats='HWC'), 'C = 4 is neither 1 nor 3'),
    (lambda w: w.add_image('t', np.zeros((3, 0, 4))), r'H = 0, W = 4 outside \[1, 4096\]'),
    (lambda w: w.add_image('t', np.zeros((1, 2, 4097), np.uint8)), r'H = 2, W = 4097 outside \[1, 4096\]'),
    (lambda w: w.add_image('t', np.zeros((4097, 2), np.uint8), dataformats='HW'), r'H = 4097, W = 2 outside \[1, 4096\]'),
    (lambda w: w.add_image('t', np.zeros((4, 4))), 'is not CHW'),
    (lambda w: w.add_image('t', np.zeros((3, 4, 4)), dataformats='NCHW'), "dataformats='NCHW'"),
    (lambda w: w.add_image('t', np.zeros((3, 4, 4), np.complex64)), 'img of dtype complex64'),
    (lambda w: w.add_images_device([('t', torch.zeros(3, 4, 4), 'CHW')]), "add_images_device: items: 't' is not a device tensor"),
    (lambda w: w.add_histogram('', np.zeros(3)), "add_histogram: tag=''"),
    (lambda w: w.add_histogram('t', np.zeros(0)), 'add_histogram: values of dtype float64 with 0 elements'),
    (lambda w: w.add_histogram('t', np.zeros(3), bins='auto'), "bins='auto'"),
    (lambda w: w.add_histogram('t', np.zeros(3), max_bins=10), 'max_bins=10'),
    (lambda w: w.add_histogram_raw('t', 0, 1, 2, 3, 4, [1.0, 2.0], [1]), 'bucket_limits has 2 entries, bucket_counts 1'),
])
def test_refusals_write_nothing(tmp_path, call, message):
    with SummaryWriter(str(tmp_path)) as w:
        with pytest.raises(GenesisHipError, match=message):
            call(w)
        assert w.stats['events'] == 1
        path = w.path
    assert len(R.read_file(path)) == 1


@pytest.mark.parametrize('kwargs, message', [
    (dict(scalar_slots=0), 'scalar_slots=0'), (dict(scalar_slots=2.5), 'scalar_slots=2.5'), (dict(compress_level=10), 'compress_level=10'),
])
def test_constructor_refusals(tmp_path, kwargs, message):
    with pytest.raises(GenesisHipError, match=message):
        SummaryWriter(str(tmp_path / 'never'), **kwargs)
    assert not osp.exists(str(tmp_path / 'never'))


def test_closed_writer_refuses_and_close_is_idempotent(tmp_path):
    w = SummaryWriter(str(tmp_path))
    w.add_scalar('a', 1.0)
    w.flush()
    w.close()
    w.close()
    for call in (lambda: w.add_scalar('a', 1.0), lambda: w.add_image('a', np.zeros((1, 2, 2))), lambda: w.add_histogram('a', np.zeros(2)),
                 lambda: w.add_histogram_raw('a', 0, 0, 1, 0, 0, [], []), lambda: w.add_scalars_dict({'k': 1}, 'a'),
                 lambda: w.add_images_device([]), w.flush):
        with pytest.raises(GenesisHipError, match='the writer is closed'):
            call()
    assert len(R.read_file(w.path)) == 2


def test_read_events_names_a_damaged_record(tmp_path):
    with SummaryWriter(str(tmp_path)) as w:
        w.add_scalar('a', 1.0)
        path = w.path
    data = bytearray(open(path, 'rb').read())
    data[-6] ^= 1
    bad = str(tmp_path / 'bad')
    open(bad, 'wb').write(bytes(data))
    with pytest.raises(GenesisHipError, match='record 1: the checksum of the data'):
        list(read_events(bad))
    open(bad, 'wb').write(bytes(data[:-3]))
    with pytest.raises(GenesisHipError, match='record 1 is truncated'):
        list(read_events(bad))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    for prefix, names in (('PNGPACK', ['FP32', 'U8', 'I64', 'D_SRC', 'D_KIND', 'D_C', 'D_H', 'D_W', 'D_PIX_STRIDE', 'D_ROW_STRIDE',
                                       'D_CH_STRIDE', 'D_DST', 'D_ROW0', 'DESC_WORDS', 'MAX_DIM']),
                          ('SCALAR', ['FP32', 'FP64', 'I32', 'I64', 'MAX_REFS'])):
        defs = {k: int(v) for k, v in re.findall(r'#define GX_%s_(\w+) (\d+)' % prefix, header)}
        assert sorted(defs) == sorted(names)
        for name, v in defs.items():
            assert getattr(tbwriter, '%s_%s' % (prefix, name)) == v, name
    words = sorted(getattr(tbwriter, n) for n in dir(tbwriter) if n.startswith('PNGPACK_D_') and n != 'PNGPACK_DESC_WORDS')
    assert words == list(range(len(words))) and len(words) <= tbwriter.PNGPACK_DESC_WORDS
    assert ctypes.sizeof(tbwriter._ScalarRefs) == 32 * 8 + 32 * 4
    assert re.search(r'constexpr int kGxPngMaxDim = %d;' % tbwriter.PNGPACK_MAX_DIM,
                     open(osp.join(REPO, 'genesis_amd', 'csrc', 'gx_common.h')).read())


FAKE = 4096


def _picture(**over):
    row = [0] * tbwriter.PNGPACK_DESC_WORDS
    fields = dict(SRC=FAKE, KIND=tbwriter.PNGPACK_FP32, C=3, H=4, W=5, PIX_STRIDE=1, ROW_STRIDE=5, CH_STRIDE=20, DST=0, ROW0=0)
    fields.update(over)
    for k, v in fields.items():
        row[getattr(tbwriter, 'PNGPACK_D_' + k)] = v
    return row


@pytest.mark.parametrize('rows, kwargs, message', [
    ([_picture()], dict(out=0), 'null pointer'),
    ([_picture()], dict(table_dev=0), 'null pointer'),
    ([_picture()], dict(n=0), 'n_pictures = 0 below 1'),
    ([_picture()], dict(table_words=11), '1 pictures do not fit a table of 11 words'),
    ([_picture(KIND=3)], {}, 'picture 0: unknown kind 3'),
    ([_picture(C=2)], {}, 'picture 0: C = 2 is neither 1 nor 3'),
    ([_picture(H=0)], {}, r'picture 0: H = 0, W = 5 outside \[1, 4096\]'),
    ([_picture(W=4097)], {}, r'picture 0: H = 4, W = 4097 outside \[1, 4096\]'),
    ([_picture(SRC=0)], {}, 'picture 0: null source'),
    ([_picture(SRC=FAKE + 2)], {}, 'picture 0: source 0x1002 is not aligned to its 4-byte elements'),
    ([_picture(SRC=FAKE + 4, KIND=2)], {}, 'picture 0: source 0x1004 is not aligned to its 8-byte elements'),
    ([_picture(PIX_STRIDE=0)], {}, 'picture 0: strides .* must be positive'),
    ([_picture(ROW_STRIDE=-5)], {}, 'picture 0: strides .* must be positive'),
    ([_picture(CH_STRIDE=0)], {}, 'picture 0: strides .* must be positive'),
    ([_picture(DST=1)], {}, 'picture 0: DST = 1, the prefix is 0'),
    ([_picture(), _picture(DST=63, ROW0=4)], {}, 'picture 1: DST = 63, the prefix is 64'),
    ([_picture(), _picture(DST=64, ROW0=5)], {}, 'picture 1: ROW0 = 5, the prefix is 4'),
    ([_picture()], dict(out_bytes=63), 'the streams take 64 bytes, out holds 63'),
])
def test_png_pack_refuses_before_launching(rows, kwargs, message):
    table = np.array([w for row in rows for w in row], np.int64)
    with pytest.raises(GenesisHipError, match=message):
        _lib.call('gx_png_pack', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(kwargs.get('table_dev', FAKE)),
                  kwargs.get('table_words', table.size), kwargs.get('n', len(rows)), ctypes.c_void_p(kwargs.get('out', FAKE)),
                  kwargs.get('out_bytes', 1 << 20), None)


def _refs(n=1, ptr=FAKE, dtype=tbwriter.SCALAR_FP32):
    refs = tbwriter._ScalarRefs()
    for i in range(n):
        refs.ptr[i], refs.dtype[i] = ptr, dtype
    return refs


@pytest.mark.parametrize('refs, n, ring, slots, first, message', [
    (_refs(), 1, 0, 8, 0, 'null pointer'),
    (_refs(), 0, FAKE, 8, 0, r'n = 0 outside \[1, 32\]'),
    (_refs(), 33, FAKE, 64, 0, r'n = 33 outside \[1, 32\]'),
    (_refs(), 1, FAKE + 4, 8, 0, 'ring must be 8-byte aligned'),
    (_refs(2), 2, FAKE, 8, 7, 'slots 7 .. 8 lie outside a ring of 8'),
    (_refs(), 1, FAKE, 8, -1, 'lie outside a ring of 8'),
    (_refs(dtype=4), 1, FAKE, 8, 0, 'value 0: unknown dtype 4'),
    (_refs(ptr=0), 1, FAKE, 8, 0, 'value 0: null address'),
    (_refs(ptr=FAKE + 2), 1, FAKE, 8, 0, 'value 0: address 0x1002 is not aligned to its 4-byte element'),
    (_refs(ptr=FAKE + 4, dtype=tbwriter.SCALAR_I64), 1, FAKE, 8, 0, 'value 0: address 0x1004 is not aligned to its 8-byte element'),
])
def test_scalar_snapshot_refuses_before_launching(refs, n, ring, slots, first, message):
    with pytest.raises(GenesisHipError, match=message):
        _lib.call('gx_scalar_snapshot', ctypes.byref(refs), n, ctypes.c_void_p(ring), slots, first, None)
