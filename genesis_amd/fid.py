"""FID on the device: the drop-in for scripts/compute_fid.py's `fid_from_model` and third_party/pytorch_fid, without
torchvision, image files or a download.

`FIDInception` is pytorch_fid's "FID Inception" (torchvision's Inception-v3 with num_classes=1008, aux_logits=False and
the FID patches of third_party/pytorch_fid/inception.py:166-320), loaded from the pytorch_fid weights file.  Every
BasicConv2d (conv without bias -> BatchNorm2d(eps=1e-3) on running statistics -> ReLU) becomes one folded conv + bias +
ReLU, folded on the host in fp64 and rounded once to fp32.  The forward pass runs on gx_fid.hip: NHWC activations, an
implicit-GEMM conv on the fp32 matrix pipe whose epilogue writes each branch into its channel slice of the block's
concatenation (sibling 1x1 convs of one input in one launch), three pool forms, and an fp64 moment accumulator.  An
image's features do not depend on the batch it is computed in (include/genesis_hip.h), so neither does the FID."""
import ctypes
import os.path as osp

import numpy as np
import torch

from . import _lib
from ._lib import GenesisHipError

WEIGHTS_FILE = 'pt_inception-2015-12-05-6726825d.pth'
BN_EPS = 1e-3
DIMS = (64, 192, 768, 2048)             # pytorch_fid's BLOCK_INDEX_BY_DIM
MAXPOOL_S2, MAXPOOL_S1P1, AVGPOOL_S1P1, GLOBAL_AVGPOOL = 0, 1, 2, 3      # GX_FID_* (include/genesis_hip.h)
MAX_CHUNK = 100                         # images per forward launch sequence (bounds the activation memory)
_IGNORED = ('fc.', 'AuxLogits.')


def layer_table():
    """[(name, cin, cout, kh, kw, stride, ph, pw)] of the 94 BasicConv2d layers (state-dict prefix `name`)."""
    L = []

    def c(name, cin, cout, k=(1, 1), s=1, p=(0, 0)):
        L.append((name, cin, cout, k[0], k[1], s, p[0], p[1]))

    c('Conv2d_1a_3x3', 3, 32, (3, 3), 2)
    c('Conv2d_2a_3x3', 32, 32, (3, 3))
    c('Conv2d_2b_3x3', 32, 64, (3, 3), p=(1, 1))
    c('Conv2d_3b_1x1', 64, 80)
    c('Conv2d_4a_3x3', 80, 192, (3, 3))
    for blk, cin, pf in (('Mixed_5b', 192, 32), ('Mixed_5c', 256, 64), ('Mixed_5d', 288, 64)):
        c(blk + '.branch1x1', cin, 64)
        c(blk + '.branch5x5_1', cin, 48)
        c(blk + '.branch5x5_2', 48, 64, (5, 5), p=(2, 2))
        c(blk + '.branch3x3dbl_1', cin, 64)
        c(blk + '.branch3x3dbl_2', 64, 96, (3, 3), p=(1, 1))
        c(blk + '.branch3x3dbl_3', 96, 96, (3, 3), p=(1, 1))
        c(blk + '.branch_pool', cin, pf)
    c('Mixed_6a.branch3x3', 288, 384, (3, 3), 2)
    c('Mixed_6a.branch3x3dbl_1', 288, 64)
    c('Mixed_6a.branch3x3dbl_2', 64, 96, (3, 3), p=(1, 1))
    c('Mixed_6a.branch3x3dbl_3', 96, 96, (3, 3), 2)
    for blk, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):
        c(blk + '.branch1x1', 768, 192)
        c(blk + '.branch7x7_1', 768, c7)
        c(blk + '.branch7x7_2', c7, c7, (1, 7), p=(0, 3))
        c(blk + '.branch7x7_3', c7, 192, (7, 1), p=(3, 0))
        c(blk + '.branch7x7dbl_1', 768, c7)
        c(blk + '.branch7x7dbl_2', c7, c7, (7, 1), p=(3, 0))
        c(blk + '.branch7x7dbl_3', c7, c7, (1, 7), p=(0, 3))
        c(blk + '.branch7x7dbl_4', c7, c7, (7, 1), p=(3, 0))
        c(blk + '.branch7x7dbl_5', c7, 192, (1, 7), p=(0, 3))
        c(blk + '.branch_pool', 768, 192)
    c('Mixed_7a.branch3x3_1', 768, 192)
    c('Mixed_7a.branch3x3_2', 192, 320, (3, 3), 2)
    c('Mixed_7a.branch7x7x3_1', 768, 192)
    c('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), p=(0, 3))
    c('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), p=(3, 0))
    c('Mixed_7a.branch7x7x3_4', 192, 192, (3, 3), 2)
    for blk, cin in (('Mixed_7b', 1280), ('Mixed_7c', 2048)):
        c(blk + '.branch1x1', cin, 320)
        c(blk + '.branch3x3_1', cin, 384)
        c(blk + '.branch3x3_2a', 384, 384, (1, 3), p=(0, 1))
        c(blk + '.branch3x3_2b', 384, 384, (3, 1), p=(1, 0))
        c(blk + '.branch3x3dbl_1', cin, 448)
        c(blk + '.branch3x3dbl_2', 448, 384, (3, 3), p=(1, 1))
        c(blk + '.branch3x3dbl_3a', 384, 384, (1, 3), p=(0, 1))
        c(blk + '.branch3x3dbl_3b', 384, 384, (3, 1), p=(1, 0))
        c(blk + '.branch_pool', cin, 192)
    return L


def expected_shapes():
    """{state-dict key: shape} of every tensor the network reads."""
    out = {}
    for name, cin, cout, kh, kw, _, _, _ in layer_table():
        out[name + '.conv.weight'] = (cout, cin, kh, kw)
        for p in ('weight', 'bias', 'running_mean', 'running_var'):
            out['%s.bn.%s' % (name, p)] = (cout,)
    return out


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """conv (no bias) -> BatchNorm2d on running statistics as one conv + bias: w' = w s, b' = beta - mean s with
    s = gamma / sqrt(var + eps), in fp64, each rounded once to fp32."""
    w, gamma, beta, mean, var = [torch.as_tensor(t).detach().cpu().double() for t in (w, gamma, beta, mean, var)]
    s = gamma / torch.sqrt(var + eps)
    return (w * s[:, None, None, None]).float(), (beta - mean * s).float()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_weights(ws, biases, device):
    """Folded fp32 weights [Cout, Cin, kh, kw] of sibling convs (same input and kernel shape) -> the operand layout of
    gx_fid_conv_bias_relu: [roundup(N, 64)][roundup(kh kw Cin, 16)] with k = (r kw + s) Cin + c, and the bias [N]."""
    rows = torch.cat([w.permute(0, 2, 3, 1).reshape(w.shape[0], -1) for w in ws], 0)
    N, K = rows.shape
    wp = torch.zeros(-(-N // 64) * 64, -(-K // 16) * 16, dtype=torch.float32)
    wp[:N, :K] = rows
    return wp.to(device), torch.cat(list(biases)).to(device=device, dtype=torch.float32)


def _check_images(x, what):
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise GenesisHipError('%s: expected fp32 device images [B, 3, H, W], got %s %s on %s'
                              % (what, x.dtype, tuple(x.shape), x.device))


def preprocess(images, quantise=True, out=None):
    """fp32 device images [B, 3, H, W] in [0, 1] -> the network input [B, 299, 299, 3] (NHWC): the reference's PNG round
    trip (quantise=True), bilinear 299 x 299 (align_corners=False), 2x - 1; one launch."""
    _check_images(images, 'fid.preprocess')
    x = images.contiguous()
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty(B, 299, 299, 3, device=x.device)
    _lib.call('gx_fid_preprocess', _ptr(x), _ptr(out), B, H, W, int(bool(quantise)), _stream())
    return out


def conv_bias_relu(x, wp, bias, parts, kh, kw, stride=1, ph=0, pw=0, dsts=None):
    """relu(conv(x, w) + b) on NHWC x [B, H, W, Cin] with packed weights (pack_weights).  parts: output channels of each
    stacked conv; dsts: per part (tensor [B, Ho, Wo, Ctot], c0) or None for a new [B, Ho, Wo, part] tensor.  Returns the
    destination tensors."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
        raise GenesisHipError('fid.conv_bias_relu: expected a contiguous fp32 device tensor [B, H, W, C]')
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    N, K = sum(parts), kh * kw * C
    if not 1 <= len(parts) <= 3 or tuple(wp.shape) != (-(-N // 64) * 64, -(-K // 16) * 16) or bias.numel() != N:
        raise GenesisHipError('fid.conv_bias_relu: packed weights %s / bias %d do not fit %d outputs x %d reductions'
                              % (tuple(wp.shape), bias.numel(), N, K))
    dsts = list(dsts) if dsts is not None else [None] * len(parts)
    args = []
    for i, n in enumerate(parts):
        d, c0 = dsts[i] if dsts[i] is not None else (torch.empty(B, Ho, Wo, n, device=x.device), 0)
        if tuple(d.shape[:3]) != (B, Ho, Wo) or not d.is_contiguous() or d.dtype != torch.float32 or c0 + n > d.shape[3]:
            raise GenesisHipError('fid.conv_bias_relu: destination %d %s cannot hold [%d, %d, %d] channels [%d, %d)'
                                  % (i, tuple(d.shape), B, Ho, Wo, c0, c0 + n))
        dsts[i] = (d, c0)
        args += [_ptr(d), d.shape[3], c0, n]
    for _ in range(len(parts), 3):
        args += [None, 0, 0, 0]
    _lib.call('gx_fid_conv_bias_relu', _ptr(x), B, H, W, C, _ptr(wp), _ptr(bias), kh, kw, stride, ph, pw, *args,
              _stream())
    return [d for d, _ in dsts]


def pool(x, mode, out=None, c0=0):
    """NHWC pool (MAXPOOL_S2 / MAXPOOL_S1P1 / AVGPOOL_S1P1 / GLOBAL_AVGPOOL) into channels [c0, c0 + C) of `out`."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
        raise GenesisHipError('fid.pool: expected a contiguous fp32 device tensor [B, H, W, C]')
    B, H, W, C = x.shape
    Ho, Wo = {MAXPOOL_S2: ((H - 3) // 2 + 1, (W - 3) // 2 + 1), GLOBAL_AVGPOOL: (1, 1)}.get(mode, (H, W))
    if out is None:
        out = torch.empty(B, Ho, Wo, C, device=x.device)
    if tuple(out.shape[:3]) != (B, Ho, Wo) or not out.is_contiguous() or c0 + C > out.shape[3]:
        raise GenesisHipError('fid.pool: destination %s cannot hold [%d, %d, %d] channels [%d, %d)'
                              % (tuple(out.shape), B, Ho, Wo, c0, c0 + C))
    _lib.call('gx_fid_pool', _ptr(x), B, H, W, C, int(mode), _ptr(out), out.shape[3], c0, _stream())
    return out


class FIDInception(object):
    """The FID Inception network on the device.  `features(images, dims)` -> fp32 [B, dims] (dims in DIMS, or a tuple of
    them -> {dims: features}), as pytorch_fid's InceptionV3 with resize_input and normalize_input, pooled to 1 x 1 as
    fid_score.py:127-130 does."""

    def __init__(self, folded, device):
        self.folded = folded                        # name -> (fp32 w [Cout, Cin, kh, kw], fp32 b [Cout]) on the host
        self.device = torch.device(device)
        self.spec = {l[0]: l[1:] for l in layer_table()}
        self._packs = {}

    @classmethod
    def from_state_dict(cls, sd_or_path, device=None):
        """pytorch_fid's weights file (pt_inception-2015-12-05-6726825d.pth) or an equivalent dict.  fc.*, AuxLogits.* and
        num_batches_tracked are ignored; any other missing or unexpected key, or a shape mismatch, raises."""
        sd = torch.load(sd_or_path, map_location='cpu') if isinstance(sd_or_path, str) else sd_or_path
        want = expected_shapes()
        keys = [k for k in sd if not k.startswith(_IGNORED) and not k.endswith('num_batches_tracked')]
        missing = sorted(set(want) - set(keys))
        unexpected = sorted(set(keys) - set(want))
        wrong = sorted(k for k in keys if k in want and tuple(sd[k].shape) != want[k])
        if missing or unexpected or wrong:
            raise GenesisHipError('FID Inception state dict does not match the network: missing %s; unexpected %s; '
                                  'wrong shape %s' % (missing, unexpected,
                                                      ['%s %s (want %s)' % (k, tuple(sd[k].shape), want[k]) for k in wrong]))
        folded = {}
        for name in (l[0] for l in layer_table()):
            folded[name] = fold_bn(sd[name + '.conv.weight'], *[sd['%s.bn.%s' % (name, p)] for p in
                                                                 ('weight', 'bias', 'running_mean', 'running_var')])
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        return cls(folded, device)

    # ---- layers ----
    def _packed(self, names):
        if names not in self._packs:
            self._packs[names] = pack_weights([self.folded[n][0] for n in names], [self.folded[n][1] for n in names],
                                              self.device)
        return self._packs[names]

    def _conv(self, x, names, dsts=None):
        names = tuple(names)
        cin, _, kh, kw, s, ph, pw = self.spec[names[0]]
        assert x.shape[3] == cin and all(self.spec[n][0] == cin and self.spec[n][2:] == (kh, kw, s, ph, pw) for n in names)
        wp, b = self._packed(names)
        out = conv_bias_relu(x, wp, b, [self.spec[n][1] for n in names], kh, kw, s, ph, pw, dsts)
        return out if len(names) > 1 else out[0]

    def _block_a(self, x, blk):
        B, H, W, _ = x.shape
        pf = self.spec[blk + '.branch_pool'][1]
        out = torch.empty(B, H, W, 224 + pf, device=x.device)
        _, b5, b3 = self._conv(x, [blk + '.branch1x1', blk + '.branch5x5_1', blk + '.branch3x3dbl_1'], [(out, 0), None, None])
        self._conv(b5, [blk + '.branch5x5_2'], [(out, 64)])
        b3 = self._conv(b3, [blk + '.branch3x3dbl_2'])
        self._conv(b3, [blk + '.branch3x3dbl_3'], [(out, 128)])
        self._conv(pool(x, AVGPOOL_S1P1), [blk + '.branch_pool'], [(out, 224)])
        return out

    def _block_b(self, x, blk):
        B, H, W, C = x.shape
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = torch.empty(B, Ho, Wo, 480 + C, device=x.device)
        self._conv(x, [blk + '.branch3x3'], [(out, 0)])
        t = self._conv(x, [blk + '.branch3x3dbl_1'])
        t = self._conv(t, [blk + '.branch3x3dbl_2'])
        self._conv(t, [blk + '.branch3x3dbl_3'], [(out, 384)])
        pool(x, MAXPOOL_S2, out, 480)
        return out

    def _block_c(self, x, blk):
        B, H, W, _ = x.shape
        out = torch.empty(B, H, W, 768, device=x.device)
        _, t, u = self._conv(x, [blk + '.branch1x1', blk + '.branch7x7_1', blk + '.branch7x7dbl_1'], [(out, 0), None, None])
        t = self._conv(t, [blk + '.branch7x7_2'])
        self._conv(t, [blk + '.branch7x7_3'], [(out, 192)])
        for i in (2, 3, 4):
            u = self._conv(u, [blk + '.branch7x7dbl_%d' % i])
        self._conv(u, [blk + '.branch7x7dbl_5'], [(out, 384)])
        self._conv(pool(x, AVGPOOL_S1P1), [blk + '.branch_pool'], [(out, 576)])
        return out

    def _block_d(self, x, blk):
        B, H, W, C = x.shape
        Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        out = torch.empty(B, Ho, Wo, 512 + C, device=x.device)
        t, u = self._conv(x, [blk + '.branch3x3_1', blk + '.branch7x7x3_1'])
        self._conv(t, [blk + '.branch3x3_2'], [(out, 0)])
        u = self._conv(u, [blk + '.branch7x7x3_2'])
        u = self._conv(u, [blk + '.branch7x7x3_3'])
        self._conv(u, [blk + '.branch7x7x3_4'], [(out, 320)])
        pool(x, MAXPOOL_S2, out, 512)
        return out

    def _block_e(self, x, blk, pool_mode):
        B, H, W, _ = x.shape
        out = torch.empty(B, H, W, 2048, device=x.device)
        _, t, u = self._conv(x, [blk + '.branch1x1', blk + '.branch3x3_1', blk + '.branch3x3dbl_1'], [(out, 0), None, None])
        self._conv(t, [blk + '.branch3x3_2a'], [(out, 320)])
        self._conv(t, [blk + '.branch3x3_2b'], [(out, 704)])
        u = self._conv(u, [blk + '.branch3x3dbl_2'])
        self._conv(u, [blk + '.branch3x3dbl_3a'], [(out, 1088)])
        self._conv(u, [blk + '.branch3x3dbl_3b'], [(out, 1472)])
        self._conv(pool(x, pool_mode), [blk + '.branch_pool'], [(out, 1856)])
        return out

    def _gap(self, x):
        return pool(x, GLOBAL_AVGPOOL).view(x.shape[0], x.shape[3])

    def forward_nhwc(self, x, dims=(2048,)):
        """Network input [B, 299, 299, 3] (preprocess) -> {d: fp32 [B, d]} for every d in dims."""
        last = max(dims)
        out = {}
        h = self._conv(x, ['Conv2d_1a_3x3'])
        h = self._conv(h, ['Conv2d_2a_3x3'])
        h = pool(self._conv(h, ['Conv2d_2b_3x3']), MAXPOOL_S2)
        if 64 in dims:
            out[64] = self._gap(h)
        if last > 64:
            h = self._conv(h, ['Conv2d_3b_1x1'])
            h = pool(self._conv(h, ['Conv2d_4a_3x3']), MAXPOOL_S2)
            if 192 in dims:
                out[192] = self._gap(h)
        if last > 192:
            for blk in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
                h = self._block_a(h, blk)
            h = self._block_b(h, 'Mixed_6a')
            for blk in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
                h = self._block_c(h, blk)
            if 768 in dims:
                out[768] = self._gap(h)
        if last > 768:
            h = self._block_d(h, 'Mixed_7a')
            h = self._block_e(h, 'Mixed_7b', AVGPOOL_S1P1)
            h = self._block_e(h, 'Mixed_7c', MAXPOOL_S1P1)
            out[2048] = self._gap(h)
        return out

    def features(self, images, dims=2048, quantise=True):
        """fp32 device images [B, 3, H, W] in [0, 1] -> fp32 [B, dims] on the device (a tuple of dims -> {d: [B, d]}).
        quantise=True restates the reference's uint8 PNG round trip; False takes the tensor's values as they are."""
        want = tuple(dims) if isinstance(dims, (tuple, list)) else (dims,)
        bad = [d for d in want if d not in DIMS]
        if bad:
            raise GenesisHipError('FID Inception: dims must be in %s, not %s' % (DIMS, bad))
        if self.device.type != 'cuda':
            raise GenesisHipError('FID Inception: the forward pass runs on the HIP device (model loaded on %s)' % self.device)
        _check_images(images, 'FIDInception.features')
        B = images.shape[0]
        parts = {d: [] for d in want}
        with torch.no_grad():
            for i in range(0, B, MAX_CHUNK):
                r = self.forward_nhwc(preprocess(images[i:i + MAX_CHUNK], quantise), want)
                for d in want:
                    parts[d].append(r[d])
        res = {d: (p[0] if len(p) == 1 else torch.cat(p, 0)) for d, p in parts.items()}
        return res if isinstance(dims, (tuple, list)) else res[dims]

    __call__ = features


def default_weights_path():
    return osp.join(torch.hub.get_dir(), 'checkpoints', WEIGHTS_FILE)


def load_fid_inception(path=None, device=None):
    """FIDInception from pytorch_fid's weights file: `path`, else torch.hub.get_dir()/checkpoints/<WEIGHTS_FILE> (where
    pytorch_fid's own download puts it).  Never downloads."""
    path = default_weights_path() if path is None else path
    if not osp.isfile(path):
        raise GenesisHipError('FID Inception weights %s not found at %s: place pytorch_fid\'s weights file there or pass '
                              'its path (nothing is downloaded)' % (WEIGHTS_FILE, path))
    return FIDInception.from_state_dict(path, device)


class FIDStatistics(object):
    """Streaming mean and covariance of the FID features of a set of images (fp64 sums on the device)."""

    def __init__(self, model, dims=2048):
        if dims not in DIMS:
            raise GenesisHipError('FIDStatistics: dims must be in %s, not %r' % (DIMS, dims))
        self.model, self.dims = model, dims
        self.sum = torch.zeros(dims, dtype=torch.float64, device=model.device)
        self.sumsq = torch.zeros(dims, dims, dtype=torch.float64, device=model.device)
        self.count = 0

    def update(self, images):
        """images: fp32 device [B, 3, H, W] in [0, 1], any H and W."""
        self.update_features(self.model.features(images, self.dims))

    def update_features(self, feats):
        feats = feats.contiguous()
        if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dims or not feats.is_cuda:
            raise GenesisHipError('FIDStatistics: expected fp32 device features [B, %d]' % self.dims)
        if feats.shape[0]:
            _lib.call('gx_fid_moments', _ptr(feats), feats.shape[0], self.dims, _ptr(self.sum), _ptr(self.sumsq), _stream())
            self.count += feats.shape[0]

    def compute(self):
        """(mu, sigma) as fp64 numpy: mu as np.mean, sigma the unbiased covariance as np.cov(rowvar=False)."""
        if self.count < 2:
            raise GenesisHipError('FIDStatistics: need at least 2 images, have %d' % self.count)
        n = self.count
        mu = self.sum.cpu().numpy() / n
        sigma = (self.sumsq.cpu().numpy() - n * np.outer(mu, mu)) / (n - 1)
        return mu, sigma


def _trace_sqrt_product(s1, s2):
    """tr sqrt(s1 s2) = sum sqrt(eig(s1^1/2 s2 s1^1/2)) for symmetric positive semi-definite s1, s2 (eigh twice; round-off
    eigenvalues below 0 clamped)."""
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    return float(np.sqrt(np.clip(lam, 0, None)).sum())


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)) (fid_score.py:140-194) in fp64 numpy, no scipy;
    eps I is added to both covariances only when the trace term is not finite, as the reference does."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    try:
        tr = _trace_sqrt_product(sigma1, sigma2)
    except np.linalg.LinAlgError:
        tr = float('nan')
    if not np.isfinite(tr):
        off = np.eye(sigma1.shape[0]) * eps
        tr = _trace_sqrt_product(sigma1 + off, sigma2 + off)
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr)


def _images_of(batch):
    return batch['input'] if isinstance(batch, dict) else batch


def fid_from_model(model, test_loader, batch_size=10, num_images=10000, feat_dim=2048, img_dir=None, weights=None):
    """scripts/compute_fid.py:101-139 on the device: FID between the first `num_images` images of `test_loader`
    (batch['input']) and `num_images` drawn by model.sample(batch_size) in eval() mode, of which each set uses the first
    (num_images // batch_size) * batch_size (fid_score.py:94-103).  `weights`: a FIDInception, a weights-file path or
    a state dict (default: load_fid_inception()).  img_dir is accepted and ignored: no files are written.  Returns the FID
    as a Python float; the model is left in train() mode."""
    model.eval()
    try:
        dev = next(model.parameters()).device
        if isinstance(weights, FIDInception):
            net = weights
        elif weights is None:
            net = load_fid_inception(device=dev)
        else:
            net = FIDInception.from_state_dict(weights, dev)
        used = (num_images // batch_size) * batch_size
        real, gen = FIDStatistics(net, feat_dim), FIDStatistics(net, feat_dim)
        count = 0
        for batch in test_loader:
            x = _images_of(batch)
            take = min(x.shape[0], num_images - count)
            if count < used:
                real.update(x[:min(take, used - count)].to(net.device, torch.float32).contiguous())
            count += take
            if count >= num_images:
                break
        count = 0
        for _ in range(num_images // batch_size + 1):
            if count >= num_images:
                break
            with torch.no_grad():
                img, _ = model.sample(batch_size)
            take = min(img.shape[0], num_images - count)
            if count < used:
                gen.update(img[:min(take, used - count)].to(net.device, torch.float32).contiguous())
            count += take
        m1, s1 = real.compute()
        m2, s2 = gen.compute()
        return frechet_distance(m1, s1, m2, s2)
    finally:
        model.train()
