"""The device half of the multi-object TFRecord loader against the reference's own MultiOjectLoader.__next__ outputs
(tests/golden/multi_object_ref.npz, written by tests/golden/make_golden_multi_object.py): the entity-mask -> instance-map
kernel (gx_entity_masks_to_labels) in both stored layouts, DeviceFeeder's 'masks' dict batches, load(cfg) on the fixture
TFRecord files and one training step on a yielded batch.  Bit for bit, no tolerance."""
import os
import os.path as osp
import shutil
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_multi_object as MG  # noqa: E402

from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

CASE_NAMES = [c[0] for c in MG.CASES]


def ref():
    return np.load(osp.join(GOLDEN, 'multi_object_ref.npz'))


def expected(g, name):
    return torch.from_numpy(g[name + '_input_u8']).float() / 255., torch.from_numpy(g[name + '_instances']).long()


def frames_of(name, g):
    image, mask = MG.case_frames(name)
    assert MG.checksum(image, mask) == g[name + '_in_crc']
    return image, mask


def window(frame, img_size):
    from genesis_amd.multi_object_config import output_size
    crop, size, S = output_size(frame, img_size)
    return crop, size, S


@pytest.mark.parametrize('layout', ['ehw', 'hwe'])
@pytest.mark.parametrize('name', CASE_NAMES)
def test_kernel_is_bit_exact_against_the_reference_loader(name, layout):
    from genesis_amd.feeder import entity_masks_to_labels
    g = ref()
    _, frame, E, bg, img_size, B = MG.case(name)
    _, mask = frames_of(name, g)
    crop, size, S = window(frame, img_size)
    stack = mask if layout == 'ehw' else np.ascontiguousarray(np.transpose(mask, (0, 2, 3, 1, 4)))    # [B,H,W,E,1]
    want = expected(g, name)[1]
    assert want.shape == (B, 1, S, S)
    got = entity_masks_to_labels(torch.from_numpy(stack).cuda(), bg, size, crop, layout)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    # without the stored last axis of 1, and into a caller's buffer that does not start on a 16-byte boundary
    flat = torch.empty(B * S * S + 1, dtype=torch.int64, device='cuda')
    out = flat[1:].view(B, 1, S, S)
    entity_masks_to_labels(torch.from_numpy(stack[..., 0].copy()).cuda(), bg, size, crop, layout, out=out)
    assert torch.equal(out.cpu(), want)


def test_kernel_paths_agree_and_arguments_are_checked():
    from genesis_amd import _lib
    from genesis_amd.feeder import entity_masks_to_labels
    rng = np.random.RandomState(3)
    vals = np.array([0, 1, 254, 255], dtype=np.uint8)
    m = torch.from_numpy(vals[rng.randint(0, 4, (2, 6, 48, 80))]).cuda()
    # host model of the reference's overwrite loop
    def host(stack, bg):
        lab = np.zeros(stack.shape[:1] + stack.shape[2:], dtype=np.int64)
        for o in range(bg, stack.shape[1]):
            lab[stack[:, o] == 255] = o + 1
        return torch.from_numpy(lab[:, None])
    for bg in (0, 2, 5, 6, 9):
        assert torch.equal(entity_masks_to_labels(m, bg).cpu(), host(m.cpu().numpy(), bg))           # 16-byte row path
    for crop in ((0, 16, 48, 32), (5, 16, 40, 48), (0, 8, 48, 32), (1, 3, 30, 33)):                  # aligned and not
        top, left, h, w = crop
        want = host(m.cpu().numpy(), 1)[:, :, top:top + h, left:left + w]
        assert torch.equal(entity_masks_to_labels(m, 1, crop=crop).cpu(), want)
    hwe = m.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(entity_masks_to_labels(hwe, 1, layout='hwe').cpu(), host(m.cpu().numpy(), 1))
    with pytest.raises(_lib.GenesisHipError, match='no CPU path'):
        entity_masks_to_labels(m.cpu(), 1)
    with pytest.raises(_lib.GenesisHipError, match='outside'):
        entity_masks_to_labels(m, 1, crop=(0, 0, 49, 80))
    with pytest.raises(_lib.GenesisHipError, match='layout'):
        entity_masks_to_labels(m, 1, layout='whe')
    for es, ps in ((48 * 80, 2), (2, 6), (0, 1), (1, 0), (48 * 80 + 1, 1)):
        with pytest.raises(_lib.GenesisHipError, match='stride'):
            _lib.call('gx_entity_masks_to_labels', m.data_ptr(), m.data_ptr(), 2, 6, 48, 80, es, ps, 1, 0, 0, 48, 80, 48, 80, None)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_device_feeder_masks_batches_are_bit_exact(name):
    from genesis_amd.feeder import DeviceFeeder
    g = ref()
    _, frame, E, bg, img_size, B = MG.case(name)
    image, mask = frames_of(name, g)
    crop, size, S = window(frame, img_size)
    want_x, want_m = expected(g, name)
    layout = 'hwe' if name.startswith('multi_dsprites') else 'ehw'
    stack = mask if layout == 'ehw' else np.ascontiguousarray(np.transpose(mask, (0, 2, 3, 1, 4)))
    batches = [{'input': image, 'masks': stack}] * 3
    outs = list(DeviceFeeder(batches, size, crop=crop, depth=2, background_entities=bg, mask_layout=layout))
    assert len(outs) == 3
    for o in outs:
        assert sorted(o) == ['input', 'instances']
        assert torch.equal(o['input'].cpu(), want_x) and torch.equal(o['instances'].cpu(), want_m)


def test_device_feeder_masks_arguments():
    from genesis_amd._lib import GenesisHipError
    from genesis_amd.feeder import DeviceFeeder
    image, mask = MG.case_frames('objects_room_64')
    with pytest.raises(GenesisHipError, match='background_entities'):
        DeviceFeeder([{'input': image, 'masks': mask}], 64)
    with pytest.raises(GenesisHipError, match='not both'):
        DeviceFeeder([{'input': image, 'masks': mask, 'instances': mask[:, 0, :, :, 0]}], 64, background_entities=4)
    with pytest.raises(GenesisHipError, match='do not match'):
        DeviceFeeder([{'input': image, 'masks': mask[:, :, :32]}], 64, background_entities=4)
    with pytest.raises(GenesisHipError, match='uint8'):
        DeviceFeeder([{'input': image, 'masks': mask.astype(np.int32)}], 64, background_entities=4)
    # reset() continues on a new iterable with the same ring
    f = DeviceFeeder([{'input': image, 'masks': mask}], 64, depth=2, background_entities=4)
    a = next(f)
    with pytest.raises(StopIteration):
        next(f)
    f.reset([{'input': image, 'masks': mask}])
    b = next(f)
    assert torch.equal(a['instances'], b['instances']) and torch.equal(a['input'], b['input'])


def make_cfg(tmp_path, dataset, **kw):
    import genesis_amd.multi_object_config as M
    dst = str(tmp_path) + M.DATASETS[dataset]['file']
    os.makedirs(osp.dirname(dst), exist_ok=True)
    shutil.copy(osp.join(GOLDEN, 'multi_object_%s.tfrecords' % dataset), dst)
    cfg = AttrDict(data_folder=str(tmp_path), dataset=dataset, img_size=-1, dataset_size=-1, num_workers=4, buffer_size=2,
                   K_steps=-1, batch_size=4, seed=0, debug=True)
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize('dataset', ['objects_room', 'tetrominoes'])
def test_load_yields_the_reference_outputs_of_the_same_records(tmp_path, dataset):
    import genesis_amd.multi_object_config as M
    g = ref()
    want_x, want_m = expected(g, dataset)
    N = want_x.shape[0]
    S = M.DATASETS[dataset]['img_size']
    cfg = make_cfg(tmp_path, dataset)
    loaders = M.load(cfg, val_size=6, test_size=5, shuffle=False)
    assert (cfg.img_size, cfg.K_steps) == (S, M.DATASETS[dataset]['K_steps'])
    bounds = ((11, N), (5, 11), (0, 5))
    for loader, (lo, hi) in zip(loaders, bounds):
        assert loader.batch_size == 4
        for _ in range(2):                                   # two epochs through the same ring
            xs, ms = [], []
            for batch in loader:
                assert sorted(batch) == ['input', 'instances']
                assert batch['input'].is_cuda and batch['input'].dtype == torch.float32
                assert batch['instances'].is_cuda and batch['instances'].dtype == torch.int64
                xs.append(batch['input'].cpu())
                ms.append(batch['instances'].cpu())
            assert [len(x) for x in xs] == [4] * ((hi - lo) // 4) + ([(hi - lo) % 4] if (hi - lo) % 4 else [])
            assert torch.equal(torch.cat(xs), want_x[lo:hi]) and torch.equal(torch.cat(ms), want_m[lo:hi])
        loader.close()
    assert len(loaders[1]) == 6 // 4 and len(loaders[2]) == 5 // 4
    assert len(loaders[0]) == (M.DATASETS[dataset]['max_frames'] - 11) // 4
    # shuffled: the same records in the order of the host stream
    cfg = make_cfg(tmp_path, dataset, seed=3)
    train = M.load(cfg, val_size=6, test_size=5)[0]
    order = np.concatenate([b['index'] for b in train.host])
    assert sorted(order.tolist()) == list(range(11, N)) and order.tolist() != list(range(11, N))
    got_x = torch.cat([b['input'].cpu() for b in train])
    assert torch.equal(got_x, want_x[torch.from_numpy(order)])
    train.close()


def test_a_full_epoch_after_an_abandoned_one_equals_an_untouched_loaders(tmp_path):
    import genesis_amd.multi_object_config as M

    def epoch(loader):
        batches = [(b['input'].cpu(), b['instances'].cpu()) for b in loader]
        return torch.cat([x for x, _ in batches]), torch.cat([m for _, m in batches])

    cfg = make_cfg(tmp_path, 'objects_room', seed=3)
    want_x, want_m = epoch(M.load(cfg, val_size=6, test_size=5)[0])
    assert want_x.shape == (19, 3, 64, 64) and want_m.shape == (19, 1, 64, 64)
    train = M.load(cfg, val_size=6, test_size=5)[0]
    first = next(iter(train))                                # an epoch left after one batch, with the next ones staged
    assert torch.equal(first['input'].cpu(), want_x[:4])
    got_x, got_m = epoch(train)
    assert torch.equal(got_x, want_x) and torch.equal(got_m, want_m)
    train.close()


def test_train_step_on_a_yielded_batch_has_a_finite_elbo(tmp_path):
    import genesis_amd.genesisv2_config as G
    import genesis_amd.multi_object_config as M
    from genesis_amd.trainer import TrainStep
    from oracle import v2_oracle as O
    cfg = make_cfg(tmp_path, 'tetrominoes')
    train = M.load(cfg, val_size=6, test_size=5)[0]
    batch = next(iter(train))
    train.close()
    assert batch['input'].shape == (4, 3, 32, 32) and batch['instances'].shape == (4, 1, 32, 32)
    mcfg = O.make_cfg(K_steps=cfg.K_steps, img_size=cfg.img_size, feat_dim=16)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(mcfg, debug=False, multi_gpu=False))).to('cuda:0').train()
    ts = TrainStep(model, cfg.img_size)
    out = ts.step(batch['input']).cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), out
    assert int(ts.step_t) == 1
