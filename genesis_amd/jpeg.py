"""Baseline JPEG decoding for the data path (GQN's frames are JPEG strings inside TFRecords: datasets/gqn_config.py,
third_party/tf_gqn/gqn_tfr_provider.py:141-143), split the project's usual way: the serial, bit-by-bit part -- markers
and Huffman codes -- runs in C on the host (genesis_amd/csrc/gx_jpeg.cpp: gx_jpeg_info, gx_jpeg_entropy_decode, no GPU
needed), and everything that touches a pixel -- dequantisation, inverse DCT, chroma upsampling, colour conversion, the
x (1/255) scaling, the nearest resize and the CHW layout -- is ONE HIP launch for the whole batch
(gx_jpeg.hip: gx_jpeg_decode_f32chw).  What crosses PCIe is the quantised int16 coefficients plus 384 bytes of
quantisation tables per frame.

The arithmetic is libjpeg's default decoding path (the slow integer DCT and "fancy" upsampling), bit for bit: the
decoded bytes equal Pillow's (libjpeg-turbo).  Accepted and rejected streams: include/genesis_hip.h."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GenesisHipError, np_ptr as _ptr

MAX_DIM = 128                               # the kernel keeps a frame's three planes in LDS
SAMPLING_NAMES = ('4:4:4', '4:2:2', '4:2:0')
_QTAB = 192                                 # uint16 values of a frame's three tables


class JpegInfo(object):
    """Geometry of one stream: width, height, sampling class (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0), blocks of the three
    padded component planes and the restart interval."""
    __slots__ = ('width', 'height', 'components', 'sampling', 'blocks', 'restart_interval')

    def __init__(self, raw):
        self.width, self.height, self.components, self.sampling = (int(v) for v in raw[:4])
        self.blocks = tuple(int(v) for v in raw[4:7])
        self.restart_interval = int(raw[7])

    @property
    def geometry(self):
        return (self.height, self.width, self.sampling)

    def __repr__(self):
        return 'JpegInfo(%dx%d, %s, blocks %s, restart %d)' % (self.width, self.height, SAMPLING_NAMES[self.sampling],
                                                               list(self.blocks), self.restart_interval)


def jpeg_info(data):
    """JpegInfo of a stream (bytes / uint8 array); raises GenesisHipError for what the decoder does not accept."""
    a = _lib.as_u8(data, 'jpeg')
    raw = np.zeros(8, dtype=np.int32)
    _lib.call('gx_jpeg_info', _ptr(a), a.size, _ptr(raw))
    return JpegInfo(raw)


def plane_blocks(H, W, sampling):
    """Blocks of the padded Y, Cb and Cr planes of an H x W frame (whole MCUs), as gx_jpeg_info reports them."""
    hs, vs = (2 if sampling else 1), (2 if sampling == 2 else 1)
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return (mx * hs * my * vs, mx * my, mx * my)


def entropy_decode(data, coef, qtab):
    """Entropy-decodes one stream into coef (int16, at least blocks * 64 values) and qtab (uint16 [3, 64] or [192]):
    quantised coefficients in natural order, per component plane in block raster order.  -> JpegInfo.  Host only; the C
    call runs without the GIL."""
    a = _lib.as_u8(data, 'jpeg')
    if coef.dtype != np.int16 or not coef.flags.c_contiguous or not coef.flags.writeable:
        raise GenesisHipError('jpeg: coef must be a writable C-contiguous int16 array')
    if qtab.dtype != np.uint16 or qtab.size < _QTAB or not qtab.flags.c_contiguous or not qtab.flags.writeable:
        raise GenesisHipError('jpeg: qtab must be a writable C-contiguous uint16 array of 192 values')
    raw = np.zeros(8, dtype=np.int32)
    _lib.call('gx_jpeg_entropy_decode', _ptr(a), a.size, _ptr(coef), coef.size, _ptr(qtab), _ptr(raw))
    return JpegInfo(raw)


class JpegStaging(object):
    """Host staging for up to `capacity` frames of one geometry (H, W, sampling class): ONE buffer, pinned by default,
    holding the coefficients of every frame and then their quantisation tables, so that a batch crosses PCIe in one copy.
    `decode(i, stream)` entropy-decodes into slot i and may be called from worker threads on different slots at the same
    time; `coef` / `qtab` are numpy views of the buffer ([capacity, blocks * 64] int16, [capacity, 192] uint16)."""

    def __init__(self, capacity, H, W, sampling, pin=True):
        if capacity <= 0:
            raise GenesisHipError('jpeg: staging capacity must be positive, not %r' % (capacity,))
        if not (0 < H <= MAX_DIM and 0 < W <= MAX_DIM) or sampling not in (0, 1, 2):
            raise GenesisHipError('jpeg: frames are at most %d x %d with sampling class 0, 1 or 2; got %d x %d, class %r'
                                  % (MAX_DIM, MAX_DIM, W, H, sampling))
        self.capacity, self.H, self.W, self.sampling = int(capacity), int(H), int(W), int(sampling)
        self.frame_values = sum(plane_blocks(H, W, sampling)) * 64
        self.coef_bytes = self.capacity * self.frame_values * 2          # a multiple of 128: the tables stay aligned
        self.nbytes = self.coef_bytes + self.capacity * _QTAB * 2
        self.buffer = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=bool(pin))
        host = self.buffer.numpy()
        self.coef = host[:self.coef_bytes].view(np.int16).reshape(self.capacity, self.frame_values)
        self.qtab = host[self.coef_bytes:].view(np.uint16).reshape(self.capacity, _QTAB)

    @property
    def geometry(self):
        return (self.H, self.W, self.sampling)

    def decode(self, i, stream):
        info = jpeg_info(stream)                        # the headers first: another geometry may not fit the slot
        if info.geometry != self.geometry:
            what = 'sampling classes' if (info.height, info.width) == (self.H, self.W) else 'sizes'
            raise GenesisHipError('jpeg: mixed %s in a batch: a %d x %d %s frame among %d x %d %s ones'
                                  % (what, info.width, info.height, SAMPLING_NAMES[info.sampling], self.W, self.H,
                                     SAMPLING_NAMES[self.sampling]))
        return entropy_decode(stream, self.coef[i], self.qtab[i])


def _out_size(H, W, img_size):
    if img_size is None:
        return H, W
    if isinstance(img_size, int):
        return img_size, img_size
    return int(img_size[0]), int(img_size[1])


def decode_staged(dev_buffer, capacity, n, geometry, img_size=None, out=None, return_u8=False):
    """The kernel launch on a device copy of a JpegStaging buffer (uint8, the same layout): its first n frames ->
    fp32 [n, 3, S_h, S_w] (and uint8 [n, H, W, 3] with return_u8), on the current stream."""
    H, W, sampling = geometry
    if not dev_buffer.is_cuda:
        raise GenesisHipError('jpeg: the staged coefficients must be on the HIP device; there is no CPU path')
    values = sum(plane_blocks(H, W, sampling)) * 64
    if dev_buffer.dtype != torch.uint8 or dev_buffer.numel() != capacity * (values + _QTAB) * 2 or not 0 < n <= capacity:
        raise GenesisHipError('jpeg: the device buffer does not hold %d staged %d x %d frames' % (capacity, W, H))
    Sh, Sw = _out_size(H, W, img_size)
    if Sh <= 0 or Sw <= 0:
        raise GenesisHipError('jpeg: bad img_size %r' % (img_size,))
    shape = (n, 3, Sh, Sw)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev_buffer.device)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32
          or out.device != dev_buffer.device or not out.is_contiguous()):
        raise GenesisHipError('jpeg: out must be a contiguous float32 tensor of shape %s on %s, not %s %s on %s'
                              % (list(shape), dev_buffer.device, getattr(out, 'dtype', type(out)),
                                 list(getattr(out, 'shape', [])), getattr(out, 'device', None)))
    u8 = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev_buffer.device) if return_u8 else None
    base = dev_buffer.data_ptr()
    _lib.call('gx_jpeg_decode_f32chw', ctypes.c_void_p(base), ctypes.c_void_p(base + capacity * values * 2),
              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(u8.data_ptr()) if return_u8 else None, n, H, W, sampling, Sh, Sw,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return (out, u8) if return_u8 else out


def decode_jpeg_batch(streams, img_size=None, out=None, return_u8=False, device='cuda'):
    """streams: a list of JPEG byte strings / uint8 arrays, all of one size and sampling class (GenesisHipError otherwise)
    -> fp32 device tensor [B, 3, S_h, S_w] in [0, 1] (u8 * (1/255), TensorFlow's convert_image_dtype), S = img_size (an int
    or (S_h, S_w); None: the stored size), resized like F.interpolate(size=S).  return_u8: also the decoded uint8
    [B, H, W, 3] at the stored size, as a second result.  Entropy decoding into pinned staging on the host, one
    host-to-device copy, one kernel launch."""
    streams = list(streams)
    if not streams:
        raise GenesisHipError('jpeg: an empty batch')
    device = torch.device(device)
    if device.type != 'cuda':
        raise GenesisHipError('jpeg: frames are decoded on the HIP device; there is no CPU path')
    if out is not None and isinstance(out, torch.Tensor) and out.device.type != 'cuda':
        raise GenesisHipError('jpeg: out must be on the HIP device, not on %s' % out.device)
    first = jpeg_info(streams[0])
    staging = JpegStaging(len(streams), first.height, first.width, first.sampling)
    for i, s in enumerate(streams):
        staging.decode(i, s)
    dev = staging.buffer.to(device, non_blocking=True)
    return decode_staged(dev, staging.capacity, len(streams), staging.geometry, img_size, out, return_u8)
