"""genesis_amd.tbwriter on the device: gx_png_pack byte for byte against the restatement's pack_rows (filter-type bytes included),
the snapshot semantics of device scalars (gx_scalar_snapshot), visualise_outputs and log_grads_and_weights end to end into an event
file, the equivalence of the host and device picture paths, and the refusals that need a device (all decided on the host)."""
import numpy as np
import pytest
import torch

from genesis_amd import histogram as hist
from genesis_amd import png as gpng
from genesis_amd import tbwriter
from genesis_amd import visualise as vis
from genesis_amd._lib import GenesisHipError
from genesis_amd.tbwriter import SummaryWriter
from tests import png_restatement as PR
from tests import tbwriter_restatement as R
from tests import vis_restatement as V
from tests import visualise_stub as S
from tests.common import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GEOMETRIES = [(1, 1, 1), (3, 1, 1), (1, 1, 5), (3, 5, 1), (3, 4, 63), (3, 4, 64), (3, 4, 65), (1, 3, 257), (3, 2, 1366), (3, 70, 530)]


def images(path):
    """[(tag, step, Summary.Image dict)] of every picture event of a file, by the restatement's decoder."""
    return [(v['tag'], e['step'], v['image']) for e in R.read_file(path) for v in e['values'] if 'image' in v]


def scalars(path):
    return [(v['tag'], e['step'], v['simple_value']) for e in R.read_file(path) for v in e['values'] if 'simple_value' in v]


def inflate(image, C, H, W):
    w, h, colour, stream = R.png_parts(image['encoded_image_string'])
    assert (image['height'], image['width'], image['colorspace']) == (H, W, C) == (h, w, 3 if colour == 2 else 1)
    assert len(stream) == H * (1 + W * C)
    return stream


# ---- gx_png_pack -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def packed(tmp_path_factory):
    """ONE add_images_device call with every geometry in three kinds and layouts and two pictures inside a larger buffer ->
    (the picture events of the file, [(tag, the host source in its layout, dataformats, C, H, W)], the writer's stats)."""
    items, sources = [], []
    for gi, (C, H, W) in enumerate(GEOMETRIES):
        for kind, dataformats in (('fp32', 'CHW'), ('uint8', 'HWC'), ('int64', 'CHW')):
            a = R.as_format(R.picture(kind, C, H, W, 3 * gi + len(kind)), dataformats)
            tag = '%s/%s/%dx%dx%d' % (kind, dataformats, C, H, W)
            items.append((tag, torch.from_numpy(a).to(DEV), dataformats))
            sources.append((tag, a, dataformats, C, H, W))
    # pictures inside a larger atlas: contiguous views that start at an odd element of a flat buffer
    for kind, dataformats, (C, H, W), offset in (('fp32', 'CHW', (3, 6, 37), 5), ('fp32', 'HWC', (3, 5, 21), 1001), ('uint8', 'HW', (1, 9, 33), 3)):
        hwc = R.picture(kind, C, H, W, 77 + offset)
        a = R.as_format(hwc, dataformats)
        flat = torch.zeros(offset + a.size + 11, dtype=torch.from_numpy(a).dtype, device=DEV)
        flat[offset:offset + a.size] = torch.from_numpy(a).reshape(-1).to(DEV)
        view = flat[offset:offset + a.size].view(a.shape)
        assert view.data_ptr() != flat.data_ptr() and view.is_contiguous()
        tag = 'atlas/%s/%s' % (kind, dataformats)
        items.append((tag, view, dataformats))
        sources.append((tag, a, dataformats, C, H, W))
    with SummaryWriter(str(tmp_path_factory.mktemp('packed'))) as w:
        w.add_images_device(items, 21)
        stats, path = dict(w.stats), w.path
    return images(path), sources, stats


def test_png_pack_matches_pack_rows(packed):
    events, sources, stats = packed
    assert stats['pack_launches'] == 1 and stats['d2h_copies'] == 1 and stats['snapshot_launches'] == 0
    assert stats['d2h_bytes'] == sum(H * (1 + W * C) for _, _, _, C, H, W in sources)
    assert [(t, s) for t, s, _ in events] == [(src[0], 21) for src in sources]
    chosen = set()
    for (tag, _, image), (_, a, dataformats, C, H, W) in zip(events, sources):
        want = R.quantise(a, dataformats)
        stream = inflate(image, C, H, W)
        assert stream == R.pack_rows(want), tag
        assert np.array_equal(PR.unfilter(np.frombuffer(stream, np.uint8), H, W, C), want), tag
        chosen.update(stream[r * (1 + W * C)] for r in range(H))
    assert {0, 1, 2, 4} <= chosen      # the contents make None, Sub, Up and Paeth each win somewhere


def test_png_pack_decodes_through_the_projects_own_decoder(packed):
    events, sources, _ = packed
    by_geometry = {}
    for (tag, _, image), src in zip(events, sources):
        by_geometry.setdefault(src[3:], []).append((image['encoded_image_string'], src))
    for (C, H, W), group in by_geometry.items():
        _, u8 = gpng.decode_png_batch([np.frombuffer(p, np.uint8) for p, _ in group], return_u8=True, device=DEV)
        u8 = u8.cpu().numpy()
        for i, (_, (tag, a, dataformats, _, _, _)) in enumerate(group):
            assert np.array_equal(u8[i], R.quantise(a, dataformats)), tag


def test_device_and_host_packing_write_the_same_pictures(tmp_path):
    items = []
    for gi, (C, H, W) in enumerate(GEOMETRIES[:8]):
        kind, dataformats = (('fp32', 'CHW'), ('uint8', 'HWC'), ('int64', 'CHW'), ('fp32', 'HWC'))[gi % 4]
        a = R.as_format(R.picture(kind, C, H, W, 50 + gi), dataformats)
        items.append(('p%d' % gi, torch.from_numpy(a).to(DEV), dataformats))
    half = torch.rand(3, 6, 10, device=DEV).to(torch.float16)      # a dtype that is converted on the device first
    ints = torch.randint(-5, 300, (6, 10), device=DEV, dtype=torch.int32)
    items += [('half', half, 'CHW'), ('int32', ints, 'HW')]
    got = {}
    for device_pack in (False, True):
        with SummaryWriter(str(tmp_path / str(device_pack)), device_pack=device_pack) as w:
            w.add_images_device(items, 2)
            for tag, t, dataformats in items[:3]:
                w.add_image(tag, t, 3, dataformats=dataformats)      # one item each
            assert w.stats['pack_launches'] == (4 if device_pack else 0)
        got[device_pack] = images(w.path)
    assert len(got[True]) == len(items) + 3
    assert got[True] == got[False]      # tags, steps, geometry and encoded_image_string, byte for byte
    assert np.array_equal(PR.unfilter(np.frombuffer(inflate(got[True][-4][2], 1, 6, 10), np.uint8), 6, 10, 1),
                          R.quantise(ints.cpu().numpy(), 'HW'))
    assert np.array_equal(PR.unfilter(np.frombuffer(inflate(got[True][-5][2], 3, 6, 10), np.uint8), 6, 10, 3),
                          R.quantise(half.float().cpu().numpy(), 'CHW'))


# ---- scalars ---------------------------------------------------------------------------------------------------------------------------
def test_a_device_scalar_is_snapshotted_at_call_time(tmp_path):
    with SummaryWriter(str(tmp_path)) as w:
        t = torch.full((1,), 1.25, device=DEV)
        before = dict(w.stats)
        w.add_scalar('a', t, 1)
        t.fill_(-7.5)
        w.add_scalar('a', t, 2)
        assert w.stats['d2h_copies'] == before['d2h_copies'] and w.stats['events'] == before['events']      # nothing read yet
        w.flush()
        assert w.stats['d2h_copies'] == before['d2h_copies'] + 1 and w.stats['snapshot_launches'] == 2
        assert w.stats['d2h_bytes'] == before['d2h_bytes'] + 16
        assert scalars(w.path) == [('a', 1, np.float32(1.25)), ('a', 2, np.float32(-7.5))]
        w.flush()      # nothing pending: no copy
        assert w.stats['d2h_copies'] == before['d2h_copies'] + 1


def mixed_values(n):
    """n one-element device tensors of the four dtypes (0-d, [1] and [1, 1]) and the float32 each must be logged as."""
    out = []
    for i in range(n):
        kind = i % 4
        with np.errstate(over='ignore'):
            if kind == 0:
                t, want = torch.tensor(0.1 * i - 1.0, dtype=torch.float32, device=DEV), np.float32(0.1 * i - 1.0)
            elif kind == 1:
                v = 1e39 if i % 8 == 1 else 1.0 / 3 + i
                t, want = torch.tensor([v], dtype=torch.float64, device=DEV), np.float32(v)
            elif kind == 2:
                t, want = torch.tensor([[-(1 << 31) + i]], dtype=torch.int32, device=DEV), np.float32(-(1 << 31) + i)
            else:
                t, want = torch.tensor((1 << 40) + i, dtype=torch.int64, device=DEV), np.float32((1 << 40) + i)
        out.append((t, want))
    return out


@pytest.mark.parametrize('n, launches', [(1, 1), (32, 1), (33, 2)])
def test_scalars_dict_snapshots_32_values_per_launch(tmp_path, n, launches):
    vals = mixed_values(n)
    with SummaryWriter(str(tmp_path)) as w:
        w.add_scalars_dict({'k%d' % i: t for i, (t, _) in enumerate(vals)}, 'grp', 9)
        for t, _ in vals:
            t.zero_()      # after the snapshot: must not be seen
        assert w.stats['snapshot_launches'] == launches and w.stats['d2h_copies'] == 0
        path = w.path
    got = scalars(path)
    assert [(tag, step) for tag, step, _ in got] == [('grp/k%d' % i, 9) for i in range(n)]
    for (tag, _, v), (_, want) in zip(got, vals):
        assert v.tobytes() == want.tobytes(), (tag, v, want)
    if n > 1:
        assert got[1][2] == np.inf      # 1e39 as a float32


def test_a_full_ring_is_fetched_and_nothing_is_lost(tmp_path):
    with SummaryWriter(str(tmp_path), scalar_slots=4) as w:
        t = torch.zeros((), device=DEV)
        for i in range(9):
            t.fill_(i + 0.5)
            w.add_scalar('r', t, i)
        assert w.stats['d2h_copies'] == 2 and w.stats['events'] == 1 + 8      # two full rings fetched, the ninth value pending
        w.add_scalars_dict({'a': t, 'b': t, 'c': 3.0, 'd': t, 'e': t, 'f': t}, 'g', 10)
        path = w.path
    got = scalars(path)
    assert got[:9] == [('r', i, np.float32(i + 0.5)) for i in range(9)]
    assert got[9:] == [('g/' + k, 10, np.float32(3.0 if k == 'c' else 8.5)) for k in 'abcdef']


def test_file_order_is_call_order_across_kinds(tmp_path):
    with SummaryWriter(str(tmp_path)) as w:
        t = torch.tensor(4.0, device=DEV)
        w.add_scalar('first', t, 1, walltime=10.0)
        t.fill_(5.0)
        w.add_scalar('host', 2.5, 1, walltime=11.0)
        w.add_image('picture', np.zeros((1, 2, 2), np.float32), 1, walltime=12.0)
        w.add_scalar('second', t, 1, walltime=13.0)
        w.add_histogram('histogram', torch.arange(6, dtype=torch.float32, device=DEV), 1, walltime=14.0)
        w.add_scalar('third', t.to(torch.float64), 1, walltime=15.0)
        path = w.path
    events = R.read_file(path)[1:]
    assert [e['values'][0]['tag'] for e in events] == ['first', 'host', 'picture', 'second', 'histogram', 'third']
    assert [e['wall_time'] for e in events] == [10.0, 11.0, 12.0, 13.0, 14.0, 15.0]
    assert [e['values'][0].get('simple_value') for e in events] == [4.0, 2.5, None, 5.0, None, 5.0]


def test_snapshots_on_another_stream_are_waited_for(tmp_path):
    side = torch.cuda.Stream()
    with SummaryWriter(str(tmp_path)) as w:
        with torch.cuda.stream(side):
            t = torch.full((1,), 3.0, device=DEV)
            w.add_scalar('side', t, 1)
        w.flush()
        assert scalars(w.path) == [('side', 1, np.float32(3.0))]
    side.synchronize()


# ---- visualise_outputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.CASES)
def test_visualise_outputs_into_an_event_file(case, tmp_path):
    g = S.load_case(case)
    model = S.StubModel(g, DEV)
    with SummaryWriter(str(tmp_path)) as w:
        vis.visualise_outputs(model, S.make_batch(g), w, 'val', int(g['iter_idx']), palette=V.PALETTE15)
        stats, path = dict(w.stats), w.path
    want = S.recorded_calls(g)
    got = images(path)
    assert [(t, s) for t, s, _ in got] == [(t, int(g['iter_idx'])) for t, _ in want]
    assert stats['pack_launches'] == (2 if model.has_sample else 1) and stats['d2h_copies'] == stats['pack_launches']
    assert model.training
    for (tag, _, image), (_, ref) in zip(got, want):
        C, H, W = ref.shape
        decoded = PR.unfilter(np.frombuffer(inflate(image, C, H, W), np.uint8), H, W, C)
        assert np.array_equal(decoded, R.quantise(ref, 'CHW')), tag


def test_a_palette_overflow_raises_before_any_event(tmp_path):
    g = S.load_case('nosample')
    batch = S.make_batch(g, DEV)
    batch['instances'][2, 0, 3, 3] = 15
    model = S.StubModel(g, DEV)
    with SummaryWriter(str(tmp_path)) as w:
        with pytest.raises(GenesisHipError, match='palette of 15 colours'):
            vis.visualise_outputs(model, batch, w, 'val', 1, palette=V.PALETTE15)
        assert w.stats['events'] == 1 and w.stats['pack_launches'] == 0 and model.training
        path = w.path
    assert len(R.read_file(path)) == 1


# ---- histograms --------------------------------------------------------------------------------------------------------------------
def test_log_grads_and_weights_into_an_event_file(tmp_path):
    import genesis_amd.genesisv2_config as G
    from genesis_amd.compat.attrdict import AttrDict
    gold = Golden('tiny')
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(dict(dynamic_K=False), **dict(gold.cfg, debug=False, multi_gpu=False))))
    model.load_state_dict(gold.weights(model.state_dict()))
    model = model.to(DEV).train()
    x, rand_pixel, eps_k = gold.inputs()
    recon, losses, stats, att_stats, comp_stats = model(x.to(DEV), rand_pixel.to(DEV), torch.stack(eps_k).to(DEV))
    (losses.err.mean(0) + torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()).backward()
    torch.cuda.synchronize()
    h = hist.Histograms()
    for name, param in model.named_parameters():
        h.add('weights/%s' % name, param.data)
        if param.grad is not None:
            h.add('grads/%s' % name, param.grad)
    records = h.compute()
    with SummaryWriter(str(tmp_path)) as w:
        hist.log_grads_and_weights(model, w, 17)
        path = w.path
    events = [e for e in R.read_file(path)[1:] if e['step'] == 17]
    assert len(events) == len(records) > 10
    bits = lambda v: np.float64(v).tobytes()
    for e, r in zip(events, records):
        (v,) = e['values']
        p = v['histo']
        assert v['tag'] == r.tag
        for key, want in (('min', r.min), ('max', r.max), ('num', float(r.num)), ('sum', r.sum), ('sum_squares', r.sum_squares)):
            assert bits(p[key]) == bits(want), (r.tag, key)
        assert [bits(x) for x in p['bucket_limit']] == [bits(x) for x in r.bucket_limits], r.tag
        assert p['bucket'] == [float(c) for c in r.bucket_counts], r.tag


def test_one_file_holds_the_scalars_pictures_and_histograms_of_a_logging_event(tmp_path):
    """The loop's three producers into one writer: heartbeat scalars (device tensors), visualise_outputs, log_grads_and_weights."""
    g = S.load_case('v2')
    net = torch.nn.Linear(5, 3).to(DEV)
    net(torch.ones(2, 5, device=DEV)).sum().backward()
    loss = torch.tensor(2.5, device=DEV)
    with SummaryWriter(str(tmp_path)) as w:
        w.add_scalar('train/loss', loss, 40)
        w.add_scalar('optim/s_per_batch', 0.25, 40)
        vis.visualise_outputs(S.StubModel(g, DEV), S.make_batch(g), w, 'train', 40, palette=V.PALETTE15)
        hist.log_grads_and_weights(net, w, 40)
        w.add_scalar('train/loss', loss * 2, 41)
        path = w.path
    assert len([f for f in tmp_path.iterdir()]) == 1
    events = R.read_file(path)
    kinds = ['version' if e['file_version'] else [k for k in ('simple_value', 'image', 'histo') if k in e['values'][0]][0] for e in events]
    n = len(S.recorded_calls(g))
    assert kinds == ['version', 'simple_value', 'simple_value'] + ['image'] * n + ['histo'] * 4 + ['simple_value']
    assert [e['step'] for e in events[1:]] == [40] * (len(events) - 2) + [41]
    assert [v['tag'] for e in events[-5:-1] for v in e['values']] == ['weights/weight', 'grads/weight', 'weights/bias', 'grads/bias']
    assert [e['values'][0]['simple_value'] for e in (events[1], events[2], events[-1])] == [2.5, 0.25, 5.0]
    assert list(tbwriter.read_events(path))[-1]['scalars'] == [('train/loss', np.float32(5.0))]


# ---- refusals: decided on the host, nothing launched -----------------------------------------------------------------------------------
def test_device_refusals(tmp_path):
    with SummaryWriter(str(tmp_path)) as w:
        for call, message in (
                (lambda: w.add_scalar('t', torch.zeros(2, device=DEV)), r"add_scalar: value of shape \(2,\) for 't'; expected one element"),
                (lambda: w.add_scalar('t', torch.zeros(1, device=DEV, dtype=torch.float16)), 'value of dtype torch.float16'),
                (lambda: w.add_scalar('t', torch.zeros(1, device=DEV, dtype=torch.uint8)), 'value of dtype torch.uint8'),
                (lambda: w.add_image('t', torch.zeros(2, 4, 4, device=DEV)), 'C = 2 is neither 1 nor 3'),
                (lambda: w.add_image('t', torch.zeros(3, 4, 8, device=DEV)[:, :, ::2]), 'is not contiguous'),
                (lambda: w.add_image('t', torch.zeros(4, 4, 3, device=DEV).permute(2, 0, 1)), 'is not contiguous'),
                (lambda: w.add_image('', torch.zeros(3, 4, 4, device=DEV)), "add_image: tag=''"),
                (lambda: w.add_image('t', torch.zeros(1, 1, 4097, device=DEV)), r'W = 4097 outside \[1, 4096\]'),
                (lambda: w.add_images_device([('ok', torch.zeros(3, 4, 4, device=DEV), 'CHW'), ('t', torch.zeros(3, 4, device=DEV), 'CHW')]),
                 'is not CHW'),
                (lambda: w.add_image('t', torch.zeros(3, 4, 4, device=DEV, dtype=torch.bool)), 'img of dtype torch.bool')):
            with pytest.raises(GenesisHipError, match=message):
                call()
        assert w.stats == dict(w.stats, pack_launches=0, snapshot_launches=0, d2h_copies=0, events=1)


def test_add_scalar_under_stream_capture_is_refused_before_launch(tmp_path):
    t = torch.ones(1, device=DEV)
    with SummaryWriter(str(tmp_path)) as w:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = t * 2.0
            with pytest.raises(GenesisHipError, match='add_scalar: value: the current stream is being captured'):
                w.add_scalar('t', y, 1)
            with pytest.raises(GenesisHipError, match='add_image: the current stream is being captured'):
                w.add_image('t', y.view(1, 1, 1), 1)
        t.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert y.item() == 6.0      # the capture ended cleanly and holds the multiplication alone
        assert w.stats['snapshot_launches'] == 0 and w.stats['pack_launches'] == 0 and w.stats['events'] == 1
        w.add_scalar('after', y, 2)
        path = w.path
    assert scalars(path) == [('after', 2, np.float32(6.0))]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two devices')
def test_pictures_on_two_devices_in_one_call(tmp_path):
    with SummaryWriter(str(tmp_path)) as w:
        with pytest.raises(GenesisHipError, match="add_images_device: items: 'b' is on cuda:1, the pictures before it on cuda:0"):
            w.add_images_device([('a', torch.zeros(3, 2, 2, device='cuda:0'), 'CHW'), ('b', torch.zeros(3, 2, 2, device='cuda:1'), 'CHW')])
        assert w.stats['pack_launches'] == 0 and w.stats['events'] == 1
