"""PNG decoding for the data path (ShapeStacks and Sketchy store one PNG file per frame: datasets/shapestacks_config.py:141,
datasets/sketchy_config.py:91), split like genesis_amd/jpeg.py: the serial part -- the chunk walk, the checksums and zlib's
inflate -- runs in C on the host (genesis_amd/csrc/gx_png.cpp: gx_png_info, gx_png_inflate, no GPU needed), and everything
that touches a pixel runs on the device: ONE HIP launch undoes the scanline filters of the whole batch (gx_png.hip:
gx_png_unfilter), and the feeder's existing kernels (feeder.transform_frames / transform_labels) crop, resample, scale and
lay out.  What crosses PCIe is the inflated, still filtered frame: H * (1 + W * C) bytes.

The decoded bytes equal Pillow's.  Accepted and rejected streams: include/genesis_hip.h.

PngFileLoader is the loader both PNG data configs (shapestacks_config.py, sketchy_config.py) are built on."""
import ctypes
import functools

import numpy as np
import torch

from . import _lib, feeder, loading
from ._lib import GenesisHipError, np_ptr as _ptr
from .loading import read_file

MAX_DIM = 4096                              # kGxPngMaxDim (csrc/gx_common.h): the C entry points reject larger frames themselves
PLANE_RULES = {'byte': 0, 'shapestacks_reference': 1, 'index': 2}


class PngInfo(object):
    """Geometry of one stream: width, height, channels (1 grey, 3 RGB, 4 RGBA), bytes per pixel, colour type, bit depth,
    interlace flag and the size of the inflated, still filtered frame: height * (1 + width * channels)."""
    __slots__ = ('width', 'height', 'channels', 'bytes_per_pixel', 'colour_type', 'bit_depth', 'interlace', 'inflated_size')

    def __init__(self, raw):
        (self.width, self.height, self.channels, self.bytes_per_pixel, self.colour_type, self.bit_depth, self.interlace,
         self.inflated_size) = (int(v) for v in raw[:8])

    @property
    def geometry(self):
        return (self.height, self.width, self.channels)

    def __repr__(self):
        return 'PngInfo(%dx%d, %d channels, colour type %d)' % (self.width, self.height, self.channels, self.colour_type)


def png_info(data):
    """PngInfo of a stream (bytes / uint8 array); raises GenesisHipError for what the decoder does not accept."""
    a = _lib.as_u8(data, 'png')
    raw = np.zeros(8, dtype=np.int32)
    _lib.call('gx_png_info', _ptr(a), a.size, _ptr(raw))
    return PngInfo(raw)


def frame_bytes(H, W, C):
    """Size of an inflated, still filtered H x W x C frame: a filter byte and W * C bytes per row."""
    return H * (1 + W * C)


def inflate(data, dst):
    """Checks one stream (signature, chunks, CRC-32s) and inflates its IDAT data into dst (uint8, at least the frame's
    frame_bytes): still filtered.  -> PngInfo.  Host only; the C call runs without the GIL."""
    a = _lib.as_u8(data, 'png')
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or not dst.flags.writeable:
        raise GenesisHipError('png: dst must be a writable C-contiguous uint8 array')
    raw = np.zeros(8, dtype=np.int32)
    _lib.call('gx_png_inflate', _ptr(a), a.size, _ptr(dst), dst.size, _ptr(raw))
    return PngInfo(raw)


def _check_geometry(H, W, C):
    if not (0 < H <= MAX_DIM and 0 < W <= MAX_DIM) or C not in (1, 3, 4):
        raise GenesisHipError('png: frames are at most %d x %d with 1, 3 or 4 channels; got %d x %d with %r'
                              % (MAX_DIM, MAX_DIM, W, H, C))


class PngStaging(object):
    """Host staging for up to `capacity` frames of one geometry (H, W, C): ONE buffer, pinned by default, of inflated and
    still filtered frames, so that a batch crosses PCIe in one copy.  `decode(i, stream)` checks and inflates into slot i
    and may be called from worker threads on different slots at the same time; `frames` is a numpy view of the buffer
    ([capacity, H * (1 + W * C)] uint8)."""

    def __init__(self, capacity, H, W, C, pin=True):
        if capacity <= 0:
            raise GenesisHipError('png: staging capacity must be positive, not %r' % (capacity,))
        _check_geometry(H, W, C)
        self.capacity, self.H, self.W, self.C = int(capacity), int(H), int(W), int(C)
        self.frame_bytes = frame_bytes(self.H, self.W, self.C)
        self.nbytes = self.capacity * self.frame_bytes
        self.buffer = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=bool(pin))
        self.frames = self.buffer.numpy().reshape(self.capacity, self.frame_bytes)

    @property
    def geometry(self):
        return (self.H, self.W, self.C)

    def decode(self, i, stream):
        # the header first: another geometry may not fit the slot (IHDR is parsed again by the inflate call: 25 bytes)
        info = png_info(stream)
        if info.geometry != self.geometry:
            raise GenesisHipError('png: mixed geometries in a batch: a %d x %d frame with %d channels among %d x %d ones '
                                  'with %d' % (info.width, info.height, info.channels, self.W, self.H, self.C))
        return inflate(stream, self.frames[i])


def unfilter(dev_buffer, capacity, n, geometry, want_u8=True, plane_rule=None):
    """The kernel launch on a device copy of a PngStaging buffer (uint8, the same layout): its first n frames ->
    (uint8 [n, H, W, C] or None, uint8 [n, H, W] or None): the reconstructed bytes, and channel 0 after plane_rule (a key
    of PLANE_RULES; None: no plane).  On the current stream."""
    H, W, C = geometry
    if not isinstance(dev_buffer, torch.Tensor) or not dev_buffer.is_cuda:
        raise GenesisHipError('png: the staged frames must be on the HIP device; there is no CPU path')
    _check_geometry(H, W, C)
    if dev_buffer.dtype != torch.uint8 or dev_buffer.numel() != capacity * frame_bytes(H, W, C) or not 0 < n <= capacity \
            or not dev_buffer.is_contiguous():
        raise GenesisHipError('png: the device buffer does not hold %d staged %d x %d x %d frames' % (capacity, W, H, C))
    if plane_rule is not None and plane_rule not in PLANE_RULES:
        raise GenesisHipError('png: the plane rule must be one of %s, not %r' % (sorted(PLANE_RULES), plane_rule))
    if not want_u8 and plane_rule is None:
        raise GenesisHipError('png: nothing to decode (neither the bytes nor a plane)')
    u8 = torch.empty(n, H, W, C, dtype=torch.uint8, device=dev_buffer.device) if want_u8 else None
    plane = torch.empty(n, H, W, dtype=torch.uint8, device=dev_buffer.device) if plane_rule is not None else None
    _lib.call('gx_png_unfilter', ctypes.c_void_p(dev_buffer.data_ptr()), ctypes.c_void_p(u8.data_ptr()) if want_u8 else None,
              ctypes.c_void_p(plane.data_ptr()) if plane is not None else None, PLANE_RULES.get(plane_rule, 0), n, H, W, C,
              ctypes.c_void_p(torch.cuda.current_stream(dev_buffer.device).cuda_stream))
    return u8, plane


def decode_staged(dev_buffer, capacity, n, geometry, size=None, crop=None, resize='nearest', out=None, return_u8=False):
    """A device copy of a PngStaging buffer -> fp32 [n, C, S_h, S_w] = bytes / 255 (and the uint8 [n, H, W, C] at the
    stored size with return_u8): gx_png_unfilter, then feeder.transform_frames (crop = (top, left, h, w), size, resize
    as there)."""
    u8, _ = unfilter(dev_buffer, capacity, n, geometry)
    x = feeder.transform_frames(u8, size, crop=crop, resize=resize, out=out)
    return (x, u8) if return_u8 else x


def labels_staged(dev_buffer, capacity, n, geometry, rule, size=None, crop=None, out=None):
    """A device copy of a PngStaging buffer of label maps -> int64 [n, 1, S_h, S_w]: channel 0 after `rule` (gx_png_unfilter's
    plane output), then feeder.transform_labels (crop, nearest)."""
    _, plane = unfilter(dev_buffer, capacity, n, geometry, want_u8=False, plane_rule=rule)
    return feeder.transform_labels(plane, size, crop=crop, out=out)


def _stage(streams, device, what):
    streams = list(streams)
    if not streams:
        raise GenesisHipError('png: an empty batch')
    device = torch.device(device)
    if device.type != 'cuda':
        raise GenesisHipError('png: %s are decoded on the HIP device; there is no CPU path' % what)
    first = png_info(streams[0])
    staging = PngStaging(len(streams), first.height, first.width, first.channels)
    for i, s in enumerate(streams):
        staging.decode(i, s)
    return staging, staging.buffer.to(device, non_blocking=True)


def decode_png_batch(streams, size=None, crop=None, resize='nearest', out=None, return_u8=False, device='cuda'):
    """streams: a list of PNG byte strings / uint8 arrays of one geometry (GenesisHipError otherwise) -> fp32 device tensor
    [B, C, S_h, S_w] in [0, 1] (bytes / 255: ToTensor) of the crop window crop = (top, left, h, w) (None: the whole frame)
    resampled to size (an int or (S_h, S_w); None: the window's size) with resize = 'nearest' (F.interpolate) or 'bilinear'
    (Pillow's, bit-exact).  return_u8: also the decoded uint8 [B, H, W, C] at the stored size, as a second result.
    Inflate into pinned staging on the host, one host-to-device copy, the unfilter launch, the feeder's transform.
    Every call allocates its own pinned staging buffer and inflates on the calling thread: a path for a handful of
    streams, evaluation and tests.  Training reads through PngFileLoader, which keeps a ring and reader threads."""
    if out is not None and isinstance(out, torch.Tensor) and out.device.type != 'cuda':
        raise GenesisHipError('png: out must be on the HIP device, not on %s' % out.device)
    staging, dev = _stage(streams, device, 'frames')
    return decode_staged(dev, staging.capacity, staging.capacity, staging.geometry, size, crop, resize, out, return_u8)


def decode_png_labels(streams, rule, size=None, crop=None, device='cuda'):
    """streams: PNG label maps of one geometry -> int64 device tensor [B, 1, S_h, S_w]: channel 0 of every pixel after
    `rule` ('byte', 'shapestacks_reference' or 'index' = byte // 32; PLANE_RULES), the crop window resampled nearest."""
    if rule not in PLANE_RULES:
        raise GenesisHipError('png: the plane rule must be one of %s, not %r' % (sorted(PLANE_RULES), rule))
    staging, dev = _stage(streams, device, 'label maps')
    return labels_staged(dev, staging.capacity, staging.capacity, staging.geometry, rule, size, crop)


class _Ring(object):
    """`depth` pinned PngStaging slots of one geometry with their device copies."""

    def __init__(self, depth, batch_size, geometry, device):
        self.geometry = geometry
        self.staging = [PngStaging(batch_size, *geometry) for _ in range(depth)]
        self.dev = [torch.empty(s.nbytes, dtype=torch.uint8, device=device) for s in self.staging]


class PngFileLoader(loading.FileBatchLoader):
    """Batches of PNG files on the device: {'input': fp32 [B, C, S_h, S_w]} and, with `map_files`, 'instances': int64
    [B, 1, S_h, S_w] (channel 0 of the map PNG of every frame after `label_rule`, cropped like the frame, nearest).
    Length, order, the short last batch, reseeding and how a bad file is reported: loading.FileBatchLoader.

    crop is a window (top, left, h, w), or an int: the centre crop of that size (feeder.centre_box) of whatever size the
    files have.  The reader threads inflate (PngStaging.decode) into the slots of one ring per kind, of the geometry of the
    first file (and the first map); per batch and kind there is one copy and one gx_png_unfilter launch."""

    def __init__(self, files, batch_size, size=None, crop=None, resize='nearest', map_files=None, label_rule='byte',
                 shuffle=True, seed=0, num_workers=4, device='cuda', depth=4, name='png'):
        super().__init__(files, batch_size, shuffle, seed, num_workers, device, depth, name)
        if map_files is not None and len(map_files) != len(files):
            raise GenesisHipError('%s: %d map files for %d frames' % (name, len(map_files), len(files)))
        if label_rule not in PLANE_RULES:
            raise GenesisHipError('%s: the label rule must be one of %s, not %r' % (name, sorted(PLANE_RULES), label_rule))
        self.map_files = None if map_files is None else list(map_files)
        self.size, self.crop, self.resize, self.label_rule = size, crop, resize, label_rule
        self.frame_crop = self.map_crop = None

    def _open_ring(self):
        """-> [the frames' _Ring, the maps' or None]"""
        try:
            g = png_info(read_file(self.files[0])).geometry
            gm = png_info(read_file(self.map_files[0])).geometry if self.map_files is not None else None
        except (GenesisHipError, OSError) as e:
            raise GenesisHipError('%s: %s' % (self.name, e)) from None
        box = (lambda q: feeder.centre_box(q[0], q[1], self.crop)) if isinstance(self.crop, int) else (lambda q: self.crop)
        self.frame_crop, self.map_crop = box(g), (box(gm) if gm is not None else None)
        return [_Ring(self.depth, self.batch_size, q, self.device) if q is not None else None for q in (g, gm)]

    def _jobs(self, s, idx):
        frames, maps = self.ring
        for i, f in enumerate(idx):
            yield self.files[f], functools.partial(frames.staging[s].decode, i)
            if maps is not None:
                yield self.map_files[f], functools.partial(maps.staging[s].decode, i)

    def _stage(self, s, n, results):
        for ring in self.ring:
            if ring is not None:
                ring.dev[s].copy_(ring.staging[s].buffer, non_blocking=True)
        return n

    def _batch(self, s, n):
        frames, maps = self.ring
        batch = {'input': decode_staged(frames.dev[s], self.batch_size, n, frames.geometry, self.size, self.frame_crop,
                                        self.resize)}
        if maps is not None:
            batch['instances'] = labels_staged(maps.dev[s], self.batch_size, n, maps.geometry, self.label_rule, self.size,
                                               self.map_crop)
        return batch
