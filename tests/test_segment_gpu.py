"""genesis_amd.segment on the device: `encode` against the full forward pass of the same GENESIS-V2 model (the same kernels on the
same inputs: bit-equal), with dynamic_K at B = 1 and B = 2, without a single decoder launch; `Segmenter` on a model that only
returns stats.log_m_k (the MONet route) against object_table on those planes; and `segment_folder` on five small PNG / JPEG files of
mixed sizes at batch size 2 -- so a short last batch -- against direct Segmenter calls on the same decoded batches with the same
generator seed.  The model is the one of tests/test_evaluate_gpu.py: K_steps = 3, 32 x 32, feat_dim = 16, formula weights, B = 2."""
import os
import os.path as osp
import sys

import numpy as np
import pytest
import torch

from genesis_amd import testing as T
from genesis_amd._lib import GenesisHipError
from genesis_amd.compat.attrdict import AttrDict
from oracle import v2_oracle as O
from tests import objects_restatement as R

sys.path.insert(0, osp.join(osp.dirname(osp.abspath(__file__)), 'golden'))
import make_golden_imagefile as MG  # noqa: E402

pytestmark = pytest.mark.gpu
K, S, D = 3, 32, 16


def make_model(**kw):
    import genesis_amd.genesisv2_config as G
    cfg = O.make_cfg(K_steps=K, img_size=S, feat_dim=D, **kw)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    return model.to('cuda').train()


@pytest.fixture(scope='module')
def model():
    return make_model()


def inputs(B):
    return T.make_input(5, B, S).cuda(), T.draw_noise(6, B, S, D, K)[0].cuda()


def same(a, b):
    return len(a) == len(b) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(a, b))


def check_encode(model, B):
    from genesis_amd.segment import encode
    x, rp = inputs(B)
    with torch.no_grad():
        _, _, stats, _, comp = model(x, rand_pixel=rp, eps=torch.zeros(K, B, D, device='cuda'))
    enc = encode(model, x, rp)
    assert same(enc.log_m_k, stats.log_m_k) and same(enc.mu_k, comp.mu_k) and same(enc.sigma_k, comp.sigma_k)
    assert enc.log_m_k[0].shape == (B, 1, S, S) and enc.mu_k[0].shape == (B, D) and not enc.log_m_k[0].requires_grad
    return enc


def test_encode_equals_the_forward_pass_bit_for_bit(model):
    enc = check_encode(model, 2)
    assert len(enc.log_m_k) == K and enc.steps is None


@pytest.mark.parametrize('B', [1, 2])
def test_encode_with_dynamic_k(B):
    enc = check_encode(make_model(dynamic_K=True), B)
    assert enc.steps is not None and enc.steps.shape == (B,) and 1 <= len(enc.log_m_k) <= K
    if B == 1:
        assert len(enc.log_m_k) == int(enc.steps[0]) + 1


def test_encode_launches_no_decoder_kernel_and_leaves_the_modes(monkeypatch):
    from genesis_amd import functions as fn
    from genesis_amd.segment import encode

    def refuse(*args, **kwargs):
        raise AssertionError('a decoder kernel was launched')
    model = make_model()                                  # (its own: a forward pass is made to fail below)
    monkeypatch.setattr(fn.DecoderFn, 'apply', refuse)
    monkeypatch.setattr(fn.MixtureFn, 'apply', refuse)
    x, rp = inputs(2)
    with pytest.raises(AssertionError, match='a decoder kernel was launched'):      # (the patch bites on the full forward pass)
        model(x, rand_pixel=rp, eps=torch.zeros(K, 2, D, device='cuda'))
    assert model.training and torch.is_grad_enabled()
    enc = encode(model, x, rp)
    assert model.training and torch.is_grad_enabled() and len(enc.log_m_k) == K
    model.eval()
    try:
        with torch.no_grad():
            encode(model, x, rp)
            assert not model.training and not torch.is_grad_enabled()
    finally:
        model.train()
    assert len(encode(model, x).mu_k) == K                 # rand_pixel drawn by the model


class Stub(torch.nn.Module):
    """A model whose forward returns what Segmenter reads of MONet's or GENESIS's: stats.log_m_k."""

    def __init__(self, planes):
        super().__init__()
        self.planes, self.calls, self.modes = planes, 0, []

    def forward(self, x):
        self.calls += 1
        self.modes.append((self.training, torch.is_grad_enabled()))
        stats = AttrDict(log_m_k=self.planes) if self.planes is not None else AttrDict(recon=x)
        return x, AttrDict(), stats, None, None


def test_segmenter_on_a_model_that_only_returns_log_m_k():
    from genesis_amd.objects import object_table
    from genesis_amd.segment import Segmenter
    log_m, x = R.make_inputs(2, 5, 12, 20)
    planes, image = list(torch.from_numpy(log_m).cuda().unsqueeze(2).unbind(0)), torch.from_numpy(x).cuda()
    stub = Stub(planes).train()
    out = Segmenter(stub)(image)
    want = object_table(planes, image)
    assert out.mu is None and out.sigma is None and stub.calls == 1
    assert stub.modes == [(False, False)] and stub.training and torch.is_grad_enabled()      # eval, no grad, and put back
    assert torch.equal(out.table.labels, want.labels) and torch.equal(out.table.geom, want.geom)
    assert torch.equal(out.table.soft.view(torch.int64), want.soft.view(torch.int64)) and out.table.channels == 3
    labels, geom, _ = R.restate(log_m, x)
    assert np.array_equal(out.table.labels.cpu().numpy(), labels) and np.array_equal(out.table.geom.cpu().numpy(), geom)


def test_a_model_without_log_m_k_is_refused():
    from genesis_amd.segment import Segmenter
    with pytest.raises(GenesisHipError, match='returns no stats.log_m_k'):
        Segmenter(Stub(None))(torch.zeros(2, 3, 8, 8, device='cuda'))
    with pytest.raises(GenesisHipError, match='returns no stats.log_m_k'):
        Segmenter(torch.nn.Identity())(torch.zeros(2, 3, 8, 8, device='cuda'))


NAMES = ['j16x16_420_q100', 'p7x9_rgb', 'j7x9_422_q30', 'p145x131_rgb', 'j136x24_444_q75']
FILES = ['f00.jpg', 'f01.png', 'f02.JPEG', 'sub/f03.png', 'sub/f04.jpg']


def test_segment_folder(model, tmp_path):
    from genesis_amd import imagefile
    from genesis_amd.segment import CSV_HEADER, Segmenter
    golden = np.load(MG.NPZ)
    streams = [bytes(golden[n + '_stream']) for n in NAMES]
    src, out = tmp_path / 'pictures', tmp_path / 'out'
    for rel, data in zip(FILES, streams):
        os.makedirs(osp.dirname(str(src / rel)), exist_ok=True)
        with open(str(src / rel), 'wb') as f:
            f.write(data)
    with open(str(src / 'notes.txt'), 'w') as f:
        f.write('not an image')
    seg = Segmenter(model, min_pixels=1, generator=torch.Generator(device='cuda').manual_seed(3))
    files, rows = seg.segment_folder(str(src), str(out), S, batch_size=2, num_workers=2, max_side=264)
    assert files == FILES
    assert sorted(osp.relpath(osp.join(r, n), str(out)) for r, _, ns in os.walk(str(out)) for n in ns) == sorted(
        [f + '.png' for f in FILES] + ['objects.csv'])
    # direct calls on the same decoded batches, in the same order, from the same seed
    direct = Segmenter(model, generator=torch.Generator(device='cuda').manual_seed(3))
    tables = [direct(imagefile.decode_image_batch(streams[a:a + 2], S, max_side=264)).table.cpu() for a in (0, 2, 4)]
    assert [t.labels.shape[0] for t in tables] == [2, 2, 1]
    labels = torch.cat([t.labels for t in tables]).numpy()
    area = torch.cat([t.area for t in tables]).numpy()
    for i, rel in enumerate(FILES):
        with open(str(out / (rel + '.png')), 'rb') as f:
            got = R.read_grey_png(f.read())
        assert got.shape == (S, S) and np.array_equal(got, labels[i]), rel
    with open(str(out / 'objects.csv')) as f:
        lines = f.read().splitlines()
    assert lines[0] == CSV_HEADER and len(lines) == 1 + rows
    cells = [line.split(',') for line in lines[1:]]
    assert all(len(c) == 15 for c in cells)
    assert [c[0] for i, c in enumerate(cells) if i == 0 or cells[i - 1][0] != c[0]] == FILES            # file order, one run each
    for i, rel in enumerate(FILES):
        mine = [c for c in cells if c[0] == rel]
        present = np.flatnonzero(area[i] >= 1)
        assert [int(c[1]) for c in mine] == present.tolist()                     # one row per present slot
        assert [int(c[2]) for c in mine] == area[i][present].tolist() and sum(int(c[2]) for c in mine) == S * S
        assert all(0.0 <= float(c[11]) <= 1.0 and 0.0 <= float(c[12]) <= 1.0 for c in mine)
    # a larger min_pixels lists fewer slots; the label maps stay
    big = Segmenter(model, min_pixels=S * S // 2, generator=torch.Generator(device='cuda').manual_seed(3))
    _, fewer = big.segment_folder(str(src), str(tmp_path / 'out2'), S, batch_size=2, num_workers=2, max_side=264)
    assert fewer == int((area >= S * S // 2).sum()) <= rows
