"""fp64 CPU restatement of the FID Inception forward pass (pytorch_fid's InceptionV3 with resize_input and
normalize_input and the FID blocks), written from the network's layer list with plain torch ops: F.conv2d, BatchNorm on
running statistics (not folded), ReLU, F.max_pool2d / F.avg_pool2d(count_include_pad=False), concatenation in NCHW.
It shares no code with genesis_amd/fid.py.  Also: a random state dict in pytorch_fid's key layout."""
import torch
import torch.nn.functional as F

EPS = 1e-3


def _bc(sd, name, x, stride=1, padding=0):
    """BasicConv2d: conv (no bias) -> BatchNorm2d(eps=1e-3, running statistics) -> ReLU."""
    p = lambda k: sd['%s.%s' % (name, k)].double()        # noqa: E731
    y = F.conv2d(x, p('conv.weight'), stride=stride, padding=padding)
    y = (y - p('bn.running_mean')[:, None, None]) / torch.sqrt(p('bn.running_var') + EPS)[:, None, None]
    return F.relu(y * p('bn.weight')[:, None, None] + p('bn.bias')[:, None, None])


def _avg(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def _mixed_a(sd, n, x):
    b1 = _bc(sd, n + '.branch1x1', x)
    b5 = _bc(sd, n + '.branch5x5_2', _bc(sd, n + '.branch5x5_1', x), padding=2)
    b3 = _bc(sd, n + '.branch3x3dbl_1', x)
    b3 = _bc(sd, n + '.branch3x3dbl_3', _bc(sd, n + '.branch3x3dbl_2', b3, padding=1), padding=1)
    return torch.cat([b1, b5, b3, _bc(sd, n + '.branch_pool', _avg(x))], 1)


def _mixed_b(sd, n, x):
    b3 = _bc(sd, n + '.branch3x3', x, stride=2)
    bd = _bc(sd, n + '.branch3x3dbl_2', _bc(sd, n + '.branch3x3dbl_1', x), padding=1)
    bd = _bc(sd, n + '.branch3x3dbl_3', bd, stride=2)
    return torch.cat([b3, bd, F.max_pool2d(x, 3, stride=2)], 1)


def _mixed_c(sd, n, x):
    b1 = _bc(sd, n + '.branch1x1', x)
    b7 = _bc(sd, n + '.branch7x7_1', x)
    b7 = _bc(sd, n + '.branch7x7_2', b7, padding=(0, 3))
    b7 = _bc(sd, n + '.branch7x7_3', b7, padding=(3, 0))
    bd = _bc(sd, n + '.branch7x7dbl_1', x)
    bd = _bc(sd, n + '.branch7x7dbl_2', bd, padding=(3, 0))
    bd = _bc(sd, n + '.branch7x7dbl_3', bd, padding=(0, 3))
    bd = _bc(sd, n + '.branch7x7dbl_4', bd, padding=(3, 0))
    bd = _bc(sd, n + '.branch7x7dbl_5', bd, padding=(0, 3))
    return torch.cat([b1, b7, bd, _bc(sd, n + '.branch_pool', _avg(x))], 1)


def _mixed_d(sd, n, x):
    b3 = _bc(sd, n + '.branch3x3_2', _bc(sd, n + '.branch3x3_1', x), stride=2)
    b7 = _bc(sd, n + '.branch7x7x3_1', x)
    b7 = _bc(sd, n + '.branch7x7x3_2', b7, padding=(0, 3))
    b7 = _bc(sd, n + '.branch7x7x3_3', b7, padding=(3, 0))
    b7 = _bc(sd, n + '.branch7x7x3_4', b7, stride=2)
    return torch.cat([b3, b7, F.max_pool2d(x, 3, stride=2)], 1)


def _mixed_e(sd, n, x, pool):
    b1 = _bc(sd, n + '.branch1x1', x)
    b3 = _bc(sd, n + '.branch3x3_1', x)
    b3 = torch.cat([_bc(sd, n + '.branch3x3_2a', b3, padding=(0, 1)), _bc(sd, n + '.branch3x3_2b', b3, padding=(1, 0))], 1)
    bd = _bc(sd, n + '.branch3x3dbl_2', _bc(sd, n + '.branch3x3dbl_1', x), padding=1)
    bd = torch.cat([_bc(sd, n + '.branch3x3dbl_3a', bd, padding=(0, 1)), _bc(sd, n + '.branch3x3dbl_3b', bd, padding=(1, 0))], 1)
    return torch.cat([b1, b3, bd, _bc(sd, n + '.branch_pool', pool(x))], 1)


def inception_features(sd, images, quantise=False):
    """images [B, 3, H, W] in [0, 1] -> {64, 192, 768, 2048: fp64 [B, d]}, each pooled to 1 x 1."""
    x = images.float()
    if quantise:
        x = torch.floor((255 * x).clamp(0, 255)) / 255
    x = F.interpolate(x.double(), size=(299, 299), mode='bilinear', align_corners=False)
    x = 2 * x - 1
    gap = lambda t: t.mean((2, 3))            # noqa: E731
    out = {}
    x = _bc(sd, 'Conv2d_1a_3x3', x, stride=2)
    x = _bc(sd, 'Conv2d_2a_3x3', x)
    x = F.max_pool2d(_bc(sd, 'Conv2d_2b_3x3', x, padding=1), 3, stride=2)
    out[64] = gap(x)
    x = _bc(sd, 'Conv2d_4a_3x3', _bc(sd, 'Conv2d_3b_1x1', x))
    x = F.max_pool2d(x, 3, stride=2)
    out[192] = gap(x)
    for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
        x = _mixed_a(sd, n, x)
    x = _mixed_b(sd, 'Mixed_6a', x)
    for n in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
        x = _mixed_c(sd, n, x)
    out[768] = gap(x)
    x = _mixed_d(sd, 'Mixed_7a', x)
    x = _mixed_e(sd, 'Mixed_7b', x, _avg)
    x = _mixed_e(sd, 'Mixed_7c', x, lambda t: F.max_pool2d(t, 3, stride=1, padding=1))
    out[2048] = gap(x)
    return out


def random_state_dict(shapes, seed=0):
    """A state dict in pytorch_fid's key layout for `shapes` ({key: shape} of the conv / BN tensors) plus fc.* and
    num_batches_tracked: He-scaled conv weights and BN statistics near identity, so activations stay O(1) through the
    network.  fp32, as the real weights file."""
    g = torch.Generator().manual_seed(seed)
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)     # noqa: E731
    sd = {}
    for k, shp in shapes.items():
        if k.endswith('conv.weight'):
            fan_in = shp[1] * shp[2] * shp[3]
            sd[k] = torch.randn(*shp, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith('bn.weight'):
            sd[k] = u(shp[0], 0.8, 1.2)
        elif k.endswith('bn.bias'):
            sd[k] = u(shp[0], -0.1, 0.2)
        elif k.endswith('running_mean'):
            sd[k] = u(shp[0], -0.1, 0.1)
        elif k.endswith('running_var'):
            sd[k] = u(shp[0], 0.8, 1.2)
            sd[k[:-len('running_var')] + 'num_batches_tracked'] = torch.tensor(0)
    sd['fc.weight'] = torch.randn(1008, 2048, generator=g) * 0.01
    sd['fc.bias'] = torch.zeros(1008)
    return sd
