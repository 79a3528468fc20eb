"""FID on the device (genesis_amd/fid.py, gx_fid.hip) against fp64 and torch's CPU ops: the preprocess, every conv shape
class of the network, the pools, the whole network against the fp64 restatement (tests/fid_restatement.py), batch
invariance of the features, the moment accumulator, and fid_from_model end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fid_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
CANARY = 12345.0


@pytest.fixture(scope='module')
def net_sd():
    from genesis_amd import fid
    sd = R.random_state_dict(fid.expected_shapes(), 0)
    return fid.FIDInception.from_state_dict(sd, DEV), sd


def _reference_preprocess(x):
    q = torch.from_numpy(np.uint8(255 * x.numpy()).astype(np.float32) / 255)
    return F.interpolate(q, size=(299, 299), mode='bilinear', align_corners=False) * 2 - 1


def test_preprocess_bit_exact_against_torch_cpu():
    from genesis_amd import fid
    g = torch.Generator().manual_seed(0)
    k = torch.arange(256, dtype=torch.float32) / 255                  # every k / 255 (255 x truncates to k - 1 for some)
    grid = torch.cat([k, torch.nextafter(k, torch.ones(1)), torch.nextafter(k, torch.zeros(1)).clamp(0, 1)])
    cases = [grid.repeat(2)[:3 * 16 * 32].reshape(1, 3, 16, 32),
             torch.rand(3, 3, 64, 64, generator=g), torch.rand(2, 3, 128, 128, generator=g),
             torch.rand(1, 3, 37, 300, generator=g), torch.rand(1, 3, 299, 299, generator=g)]
    for x in cases:
        got = fid.preprocess(x.to(DEV)).cpu()                           # NHWC
        ref = _reference_preprocess(x).permute(0, 2, 3, 1)
        diff = int((got != ref).sum())
        assert diff == 0, '%s: %d of %d values differ (max %.3g)' % (tuple(x.shape), diff, ref.numel(),
                                                                       float((got - ref).abs().max()))
    x = torch.rand(2, 3, 64, 48, generator=g)                          # quantise=False: the tensor's values as they are
    got = fid.preprocess(x.to(DEV), quantise=False).cpu()
    ref = (F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False) * 2 - 1).permute(0, 2, 3, 1)
    assert torch.equal(got, ref)


CONV_CASES = [  # cin, parts, kh, kw, stride, ph, pw, H, W
    (3, [32], 3, 3, 2, 0, 0, 35, 33),          # Conv2d_1a (Cin = 3: the scalar gather)
    (32, [32], 3, 3, 1, 0, 0, 19, 21),
    (32, [64], 3, 3, 1, 1, 1, 19, 17),
    (64, [80], 1, 1, 1, 0, 0, 23, 17),
    (96, [96], 3, 3, 2, 0, 0, 17, 17),
    (48, [64], 5, 5, 1, 2, 2, 13, 13),
    (128, [128], 1, 7, 1, 0, 3, 11, 11),
    (160, [192], 7, 1, 1, 3, 0, 11, 11),
    (384, [384], 1, 3, 1, 0, 1, 8, 8),
    (384, [384], 3, 1, 1, 1, 0, 8, 8),
    (192, [64, 48, 64], 1, 1, 1, 0, 0, 13, 13),     # A's three stacked 1x1 convs
    (768, [192, 160, 160], 1, 1, 1, 0, 0, 9, 9),   # C's
    (768, [192, 192], 1, 1, 1, 0, 0, 9, 9),        # D's two
]


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: '%dx%d_s%d_p%d%d_cin%d_n%s' % (c[2], c[3], c[4], c[5], c[6], c[0],
                                                                                           '+'.join(map(str, c[1]))))
def test_conv_bias_relu_against_fp64(case):
    """Elementwise: |y - y64| <= 2 (K + 1) 2^-24 (sum_k |w||x| + |b|) (recursive fp32 summation of K products and the
    bias; ReLU is 1-Lipschitz).  The first part goes into channels [c0, c0 + n) of a wider tensor whose other channels
    hold a canary."""
    from genesis_amd import fid
    cin, parts, kh, kw, st, ph, pw, H, W = case
    B = 3
    g = torch.Generator().manual_seed(CONV_CASES.index(case))
    x = torch.randn(B, cin, H, W, generator=g).double()
    ws = [torch.randn(n, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5 for n in parts]
    bs = [0.1 * torch.randn(n, generator=g) for n in parts]
    wp, bias = fid.pack_weights(ws, bs, DEV)
    Ho, Wo = (H + 2 * ph - kh) // st + 1, (W + 2 * pw - kw) // st + 1
    ctot, c0 = parts[0] + 40, 24
    wide = torch.full((B, Ho, Wo, ctot), CANARY, device=DEV)
    outs = fid.conv_bias_relu(x.float().permute(0, 2, 3, 1).contiguous().to(DEV), wp, bias, parts, kh, kw, st, ph, pw,
                              [(wide, c0)] + [None] * (len(parts) - 1))
    K = cin * kh * kw
    for i, (w, b) in enumerate(zip(ws, bs)):
        ref = F.relu(F.conv2d(x.float().double(), w.double(), b.double(), stride=st, padding=(ph, pw)))
        mag = F.conv2d(x.float().double().abs(), w.double().abs(), b.double().abs(), stride=st, padding=(ph, pw))
        got = (outs[i][..., c0:c0 + parts[0]] if i == 0 else outs[i]).double().cpu().permute(0, 3, 1, 2)
        assert got.shape == ref.shape
        bound = 2 * (K + 1) * U * mag
        err = (got - ref).abs()
        assert bool((err <= bound).all()), 'part %d: worst error / bound %.3g' % (i, float((err / bound).max()))
    w0 = wide.cpu()
    assert bool((w0[..., :c0] == CANARY).all()) and bool((w0[..., c0 + parts[0]:] == CANARY).all())


@pytest.mark.parametrize('mode', ['max_s2', 'max_s1p1', 'avg_s1p1', 'global'])
def test_pools_against_fp64(mode):
    from genesis_amd import fid
    B, H, W, C = 2, 17, 15, 48
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(3))
    ref = {'max_s2': lambda t: F.max_pool2d(t, 3, stride=2),
           'max_s1p1': lambda t: F.max_pool2d(t, 3, stride=1, padding=1),
           'avg_s1p1': lambda t: F.avg_pool2d(t, 3, stride=1, padding=1, count_include_pad=False),
           'global': lambda t: t.mean((2, 3), keepdim=True)}[mode](x.double())
    m = {'max_s2': fid.MAXPOOL_S2, 'max_s1p1': fid.MAXPOOL_S1P1, 'avg_s1p1': fid.AVGPOOL_S1P1,
         'global': fid.GLOBAL_AVGPOOL}[mode]
    ctot, c0 = C + 20, 12
    out = torch.full((B, ref.shape[2], ref.shape[3], ctot), CANARY, device=DEV)
    fid.pool(x.permute(0, 2, 3, 1).contiguous().to(DEV), m, out, c0)
    got = out[..., c0:c0 + C].double().cpu().permute(0, 3, 1, 2)
    if mode.startswith('max'):
        assert torch.equal(got, ref)
    else:
        n = 9 if mode == 'avg_s1p1' else H * W
        assert float((got - ref).abs().max()) <= 2 * (n + 1) * U * float(x.abs().max())
    o = out.cpu()
    assert bool((o[..., :c0] == CANARY).all()) and bool((o[..., c0 + C:] == CANARY).all())


def test_whole_network_against_fp64_restatement(net_sd):
    net, sd = net_sd
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    got = net.features(x.to(DEV), dims=(64, 192, 768, 2048), quantise=False)
    ref = R.inception_features(sd, x, quantise=False)
    for d in (64, 192, 768, 2048):
        g = got[d].double().cpu()
        assert g.shape == (4, d)
        rel = float((g - ref[d]).norm() / ref[d].norm())
        print('dims %4d: relative L2 error against fp64 %.3g' % (d, rel))
        assert rel <= 1e-4, (d, rel)


def test_features_are_batch_invariant(net_sd):
    net = net_sd[0]
    imgs = torch.rand(50, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    one = imgs[17:18]
    f1 = net.features(one)
    seven = torch.cat([imgs[:5], one, imgs[40:41]])
    f7 = net.features(seven)
    full = imgs.clone()
    f50 = net.features(full)
    f50b = net.features(full)
    assert torch.equal(f1[0], f7[5]) and torch.equal(f1[0], f50[17])
    assert torch.equal(f7[0], f50[0]) and torch.equal(f7[6], f50[40])
    assert torch.equal(f50, f50b)


def test_moments_against_numpy():
    from genesis_amd import fid

    class _Net(object):
        device = torch.device(DEV)
    g = torch.Generator().manual_seed(6)
    feats = (torch.rand(60, 2048, generator=g) * torch.rand(2048, generator=g) + 0.2).to(DEV)
    runs = []
    for split in ((7, 23, 30), (60,), (7, 23, 30)):
        st = fid.FIDStatistics(_Net(), 2048)
        i = 0
        for n in split:
            st.update_features(feats[i:i + n])
            i += n
        assert st.count == 60
        runs.append(st.compute())
    host = feats.cpu().numpy().astype(np.float64)
    mu, sigma = runs[0]
    assert np.abs(mu - np.mean(host, axis=0)).max() <= 1e-10 * np.abs(mu).max()
    cov = np.cov(host, rowvar=False)
    assert np.abs(sigma - cov).max() <= 1e-10 * np.abs(cov).max()
    for m, s in runs[1:]:                       # bit-identical over runs and over how the images are split
        assert np.array_equal(m, mu) and np.array_equal(s, sigma)


class _Loader(object):
    def __init__(self, imgs, bs):
        self.imgs, self.bs = imgs, bs

    def __iter__(self):
        for i in range(0, self.imgs.shape[0], self.bs):
            yield {'input': self.imgs[i:i + self.bs]}


class _PoolModel(torch.nn.Module):
    """sample(n) serves the next n images of a fixed pool (GenesisV2's own draws depend on the batch size)."""

    def __init__(self, pool):
        super(_PoolModel, self).__init__()
        self.w = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.pool, self.i = pool, 0

    def sample(self, n):
        idx = torch.arange(self.i, self.i + n) % self.pool.shape[0]
        self.i += n
        return self.pool[idx.to(DEV)], None


def test_fid_from_model_end_to_end(tmp_path):
    import genesis_amd.genesisv2_config as G
    from genesis_amd import fid
    from genesis_amd.compat.attrdict import AttrDict
    from oracle import v2_oracle as O
    sd = R.random_state_dict(fid.expected_shapes(), 7)
    path = str(tmp_path / fid.WEIGHTS_FILE)
    torch.save(sd, path)
    loader = _Loader(torch.rand(40, 3, 32, 32, generator=torch.Generator().manual_seed(8)).to(DEV), 10)
    cfg = O.make_cfg(K_steps=3, img_size=32, feat_dim=16)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False))).to(DEV).train()

    torch.manual_seed(9)
    val = fid.fid_from_model(model, loader, batch_size=10, num_images=35, weights=path)
    assert isinstance(val, float) and np.isfinite(val)
    assert model.training

    # by hand: the first 30 loader images, the first three sample(10) draws from the same seed
    net = fid.FIDInception.from_state_dict(path, DEV)
    real, gen = fid.FIDStatistics(net), fid.FIDStatistics(net)
    for b in list(loader)[:3]:
        real.update(b['input'])
    model.eval()
    torch.manual_seed(9)
    for _ in range(3):
        with torch.no_grad():
            gen.update(model.sample(10)[0].contiguous())
    model.train()
    assert real.count == 30 and gen.count == 30
    assert val == fid.frechet_distance(*real.compute(), *gen.compute())

    # batch sizes 5 and 7 both use all 35 images: bit-identical
    pool = torch.rand(35, 3, 32, 32, generator=torch.Generator().manual_seed(10)).to(DEV)
    vals = [fid.fid_from_model(_PoolModel(pool), loader, batch_size=bs, num_images=35, weights=net) for bs in (5, 7)]
    assert np.isfinite(vals[0]) and vals[0] == vals[1], vals
