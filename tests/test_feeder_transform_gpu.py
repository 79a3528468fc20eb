"""The feeder's crop / resample transforms on the device (genesis_amd/feeder.py transform_frames / transform_labels,
DeviceFeeder's crop / resize / dict batches) against what the reference's datasets compute on the host: Pillow's crop +
BILINEAR resize (datasets/shapestacks_config.py:126-130; tests/golden/feeder_pil.npz and live Pillow), np_img_centre_crop +
nearest F.interpolate of the ToTensor batch (multi_object_config.py:181-202) and the instance maps' float round trip
(shapestacks_config.py:155-162).  Bit for bit, no tolerance."""
import os.path as osp
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_feeder as MG  # noqa: E402


def to_tensor(frames_u8):
    return torch.from_numpy(np.ascontiguousarray(frames_u8)).permute(0, 3, 1, 2).float().div(255)   # ToTensor, per batch


def host_nearest(frames, box, size):
    top, left, h, w = box
    x = to_tensor(frames[:, top:top + h, left:left + w])
    return F.interpolate(x, size=size)


def host_labels(labels, box, size):
    top, left, h, w = box
    m = torch.from_numpy(np.ascontiguousarray(labels[:, None, top:top + h, left:left + w])).float()
    return F.interpolate(m, size=size).long()


@pytest.mark.parametrize('case', [c[0] for c in MG.CASES])
def test_bilinear_is_bit_exact_against_the_fixture(case):
    from genesis_amd.feeder import transform_frames
    _, _, box, size = [c for c in MG.CASES if c[0] == case][0]
    g = np.load(osp.join(GOLDEN, 'feeder_pil.npz'))
    frames = MG.feeder_case_frames(case)
    assert MG.checksum(frames) == g[case + '_in_crc']
    got = transform_frames(torch.from_numpy(frames).cuda(), size, crop=box, resize='bilinear').cpu()
    assert got.shape == (frames.shape[0], frames.shape[3]) + tuple(size)
    assert torch.equal(got, to_tensor(g[case + '_out']))


def _pil(frame, box, size):
    if frame.shape[2] != 4:
        return MG.pil_crop_resize(frame, box, size)
    from PIL import Image
    top, left, h, w = box
    im = Image.fromarray(frame, 'RGBA').crop((left, top, left + w, top + h))
    return np.asarray(im.resize((size[1], size[0]), Image.BILINEAR))


@pytest.mark.parametrize('seed', range(8))
def test_bilinear_is_bit_exact_against_live_pillow(seed):
    pytest.importorskip('PIL')
    from genesis_amd.feeder import transform_frames
    rng = np.random.RandomState(100 + seed)
    B = (64, 7, 3, 1, 16, 2, 5, 64)[seed]
    C = (3, 1, 3, 4, 3, 1, 3, 3)[seed]
    Hs, Ws = rng.randint(16, 300, 2)
    h, w = rng.randint(8, Hs + 1), rng.randint(8, Ws + 1)
    box = (rng.randint(0, Hs - h + 1), rng.randint(0, Ws - w + 1), h, w)
    if seed % 3 == 2:                                                              # upsampling
        size = (rng.randint(h, 2 * h + 1), rng.randint(w, 2 * w + 1))
    else:
        size = (max(1, h // rng.randint(1, 17)), max(1, w // rng.randint(1, 17)))
    frames = rng.randint(0, 256, (B, Hs, Ws, C)).astype(np.uint8)
    if C == 4:
        frames[..., 3] = 255                                       # Pillow premultiplies RGBA by alpha: keep it opaque
    want = np.stack([_pil(f, box, size) for f in frames])
    got = transform_frames(torch.from_numpy(frames).cuda(), size, crop=box, resize='bilinear').cpu()
    assert torch.equal(got, to_tensor(want)), (B, Hs, Ws, C, box, size)


@pytest.mark.parametrize('B,Hs,Ws,C,box,size', [(3, 200, 700, 3, (10, 20, 180, 650), (45, 333)),
                                               (1, 120, 2000, 1, (0, 0, 120, 2000), (30, 999)),
                                               (2, 96, 900, 4, (3, 1, 90, 897), (41, 259))])
def test_bilinear_ragged_column_tiles(B, Hs, Ws, C, box, size):
    """Output rows of more than 768 bytes are split into column tiles; these widths leave a shorter last tile
    (333 x 3 -> 167 + 166, 999 -> 500 + 499, 259 x 4 -> 130 + 129)."""
    pytest.importorskip('PIL')
    from genesis_amd.feeder import transform_frames
    frames = np.random.RandomState(Ws + C).randint(0, 256, (B, Hs, Ws, C)).astype(np.uint8)
    if C == 4:
        frames[..., 3] = 255
    want = np.stack([_pil(f, box, size) for f in frames])
    got = transform_frames(torch.from_numpy(frames).cuda(), size, crop=box, resize='bilinear').cpu()
    assert torch.equal(got, to_tensor(want))


def test_out_must_fit():
    from genesis_amd.feeder import GenesisHipError, transform_frames, transform_labels
    frames = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device='cuda')
    labels = torch.zeros(2, 16, 16, dtype=torch.int64, device='cuda')
    for bad in (torch.empty(2, 3, 8, 7, device='cuda'), torch.empty(2, 3, 8, 8, dtype=torch.float64, device='cuda'),
                torch.empty(2, 3, 8, 8), torch.empty(2, 3, 8, 16, device='cuda')[..., ::2]):
        with pytest.raises(GenesisHipError, match='out must be'):
            transform_frames(frames, 8, resize='bilinear', out=bad)
    for bad in (torch.empty(2, 1, 8, 8, dtype=torch.int32, device='cuda'), torch.empty(2, 8, 8, dtype=torch.int64, device='cuda')):
        with pytest.raises(GenesisHipError, match='out must be'):
            transform_labels(labels, 8, out=bad)


def test_shapestacks_batch_is_bit_exact():
    """BASELINE config 4's input: B = 64 frames of 224 x 224 x 3, centre crop 196, PIL bilinear to 64 x 64."""
    pytest.importorskip('PIL')
    from genesis_amd.feeder import centre_box, transform_frames
    frames = np.random.RandomState(7).randint(0, 256, (64, 224, 224, 3)).astype(np.uint8)
    box = centre_box(224, 224, 196)
    want = np.stack([MG.pil_crop_resize(f, box, (64, 64)) for f in frames])
    got = transform_frames(torch.from_numpy(frames).cuda(), 64, crop=box, resize='bilinear').cpu()
    assert torch.equal(got, to_tensor(want))


@pytest.mark.parametrize('B,Hs,Ws,C,crop,size', [(4, 240, 320, 3, 192, 64), (3, 224, 224, 3, 196, 64), (2, 65, 64, 1, 33, 50),
                                                 (2, 64, 96, 3, 64, 128), (1, 7, 9, 3, 5, 3)])
def test_nearest_with_a_crop_is_bit_exact(B, Hs, Ws, C, crop, size):
    from genesis_amd.feeder import centre_box, transform_frames
    frames = np.random.RandomState(B * 10 + C).randint(0, 256, (B, Hs, Ws, C)).astype(np.uint8)
    box = centre_box(Hs, Ws, crop)
    got = transform_frames(torch.from_numpy(frames).cuda(), size, crop=box).cpu()
    assert torch.equal(got, host_nearest(frames, box, (size, size)))


@pytest.mark.parametrize('B,Hs,C,size', [(4, 64, 3, 64), (3, 64, 3, 32), (2, 64, 3, 128), (1, 7, 1, 5), (5, 128, 3, 64)])
def test_nearest_without_a_crop_is_u8hwc_to_f32chw(B, Hs, C, size):
    from genesis_amd.feeder import transform_frames, u8hwc_to_f32chw
    frames = torch.from_numpy(np.random.RandomState(Hs + size).randint(0, 256, (B, Hs, Hs, C)).astype(np.uint8)).cuda()
    assert torch.equal(transform_frames(frames, size), u8hwc_to_f32chw(frames, size))


@pytest.mark.parametrize('dtype', [np.uint8, np.int32, np.int64])
@pytest.mark.parametrize('Hs,Ws,crop,size', [(224, 224, 196, 64), (240, 320, 192, 64), (64, 64, 64, 128), (9, 7, 7, 3)])
def test_labels_are_the_references_float_round_trip(dtype, Hs, Ws, crop, size):
    from genesis_amd.feeder import centre_box, transform_labels
    rng = np.random.RandomState(Hs + size)
    lo, hi = (0, 256) if dtype == np.uint8 else (-3, 1 << 20)          # negative: ignore regions
    labels = rng.randint(lo, hi, (3, Hs, Ws)).astype(dtype)
    if dtype == np.int64:
        labels[0, :4, :4] = (1 << 40) + (1 << 20)                      # a large label an fp32 holds exactly
    box = centre_box(Hs, Ws, crop)
    want = host_labels(labels, box, (size, size))
    got = transform_labels(torch.from_numpy(labels).cuda(), size, crop=box)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    got4 = transform_labels(torch.from_numpy(labels[:, None]).cuda(), size, crop=box)    # [B, 1, H, W] in
    assert torch.equal(got4.cpu(), want)


def shapestacks_batches(n, B=8, seed=3):
    rng = np.random.RandomState(seed)
    return [{'input': rng.randint(0, 256, (B, 224, 224, 3)).astype(np.uint8),
             'instances': rng.randint(0, 7, (B, 224, 224)).astype(np.int64)} for _ in range(n)]


def test_dict_batches_survive_slot_reuse():
    """As test_feeder.py's slot-reuse test, with dict batches through the crop + bilinear path: a long spin on the compute
    stream before every next() keeps each conversion queued while the ring refills; every batch must come out intact."""
    pytest.importorskip('PIL')
    from genesis_amd.feeder import DeviceFeeder, centre_box
    box = centre_box(224, 224, 196)
    batches = shapestacks_batches(7)
    feeder = DeviceFeeder(batches, 64, depth=2, crop=box, resize='bilinear')
    out = []
    for _ in range(len(batches)):
        torch.cuda._sleep(40_000_000)        # ~20 ms of device time queued ahead of the conversion kernels
        out.append(next(feeder))
    with pytest.raises(StopIteration):
        next(feeder)
    torch.cuda.synchronize()
    for d, b in zip(out, batches):
        assert set(d) == {'input', 'instances'}
        want = to_tensor(np.stack([MG.pil_crop_resize(f, box, (64, 64)) for f in b['input']]))
        assert torch.equal(d['input'].cpu(), want)
        assert d['instances'].shape == (8, 1, 64, 64)
        assert torch.equal(d['instances'].cpu(), host_labels(b['instances'], box, (64, 64)))


def test_dict_and_array_batches_with_default_arguments():
    """Dicts without a crop (labels [B,1,H,W] int32 with ignore labels; a dict without instances) and an array batch in
    one feeder: arrays stay arrays, as before."""
    from genesis_amd.feeder import DeviceFeeder
    rng = np.random.RandomState(5)
    batches = [{'input': rng.randint(0, 256, (4, 64, 64, 3)).astype(np.uint8),
                'instances': rng.randint(-1, 5, (4, 1, 64, 64)).astype(np.int32)},
               {'input': rng.randint(0, 256, (4, 64, 64, 3)).astype(np.uint8)},
               rng.randint(0, 256, (4, 64, 64, 3)).astype(np.uint8)]
    out = list(DeviceFeeder(batches, 32))
    assert len(out) == 3
    box = (0, 0, 64, 64)
    assert torch.equal(out[0]['input'].cpu(), host_nearest(batches[0]['input'], box, (32, 32)))
    assert torch.equal(out[0]['instances'].cpu(), host_labels(batches[0]['instances'][:, 0], box, (32, 32)))
    assert set(out[1]) == {'input'} and torch.equal(out[1]['input'].cpu(), host_nearest(batches[1]['input'], box, (32, 32)))
    assert torch.is_tensor(out[2]) and torch.equal(out[2].cpu(), host_nearest(batches[2], box, (32, 32)))


def test_average_ari_on_fed_instances():
    from genesis_amd.feeder import DeviceFeeder, centre_box
    from genesis_amd.metrics import average_ari
    box = centre_box(224, 224, 196)
    batches = shapestacks_batches(2, B=4, seed=11)
    g = torch.Generator().manual_seed(2)
    log_m_k = [torch.randn(4, 1, 64, 64, generator=g).cuda() for _ in range(7)]
    n = 0
    for d, b in zip(DeviceFeeder(batches, 64, crop=box, resize='bilinear'), batches):
        host = host_labels(b['instances'], box, (64, 64)).cuda()
        for fg in (False, True):
            assert average_ari(log_m_k, d['instances'], fg) == average_ari(log_m_k, host, fg)
        n += 1
    assert n == 2
