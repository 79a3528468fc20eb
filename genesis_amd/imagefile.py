"""Loose image files for the data path: a folder of a user's own JPEG and PNG files of ANY size, mixed within one batch --
what the reference's users get from pointing a torchvision dataset at a directory (datasets/apc_config.py:144-147:
Resize(img_size, BILINEAR), CenterCrop(img_size), ToTensor on the PIL image).

Split like genesis_amd/jpeg.py and png.py.  The serial part runs in C on the host, without the GIL: the marker walk and the
Huffman decoder of gx_jpeg.cpp (gx_jpeg_info_any, gx_jpeg_entropy_decode_any: frames up to 4096 x 4096, grey or colour) and
the chunk walk and zlib inflate of gx_png.cpp.  Everything that touches a pixel runs on the device in FOUR launches per batch,
whatever the batch holds (gx_imagefile.hip): gx_jpeg_decode_ragged (blocks -> planes, planes -> pixels),
gx_png_unfilter_ragged and gx_u8_resample_ragged_f32chw, each told about its frames by a per-frame descriptor table.

A batch is staged in ONE byte arena (pinned): the three descriptor tables at the front, then per frame its payload (quantised
coefficients and tables, or the inflated, still filtered PNG rows) and the rows of Pillow's BILINEAR coefficient tables its
output window needs.  Sizes are not known before a header is read, so frames take their place in the arena in the order their
readers get to them.  One copy takes the arena to the device.

The transform, exactly (torchvision's Resize(S) + CenterCrop(S), restated: resize_crop_geometry): a w x h frame is resized WHOLE
to (w', h') = (S, int(S * h / w)) if w <= h else (int(S * w / h), S), and the S x S window at top' = int(round((h' - S) / 2.0)),
left' = int(round((w' - S) / 2.0)) (Python's round: half to even) is the result, as fp32 [3, S, S] = byte / 255.  Grey frames
are replicated to three channels and alpha is dropped, as Pillow's convert('RGB') does before the resize.  The decoded bytes
and the transformed frames equal Pillow's bit for bit (tests/golden/imagefile_pil.npz).  EXIF orientation is ignored, as
Pillow's open ignores it.  Accepted and rejected streams: include/genesis_hip.h."""
import ctypes
import functools
import threading

import numpy as np
import torch

from . import _lib, feeder, loading, png
from ._lib import GenesisHipError, np_ptr as _ptr

MAX_DIM = 4096                              # kGxImageMaxDim (csrc/gx_common.h): the C entry points reject larger frames themselves
MAX_SIZE = 1024                             # img_size, at most (gx_u8_resample_ragged_f32chw's bound on the window)
PNG_MAGIC = b'\x89PNG\r\n\x1a\n'
JPEG_MAGIC = b'\xff\xd8'
SAMPLING_NAMES = ('4:4:4', '4:2:2', '4:2:0')
# descriptor words and tile constants of include/genesis_hip.h (tests/test_imagefile_cpu.py holds them against the header)
JPEGR_WORDS, PNGR_WORDS, RSR_WORDS = 10, 5, 14
JPEGR_BLOCKS_PER_WG, JPEGR_TILE_H, JPEGR_TILE_W = 128, 16, 64
_QTAB_BYTES = 384


def _round16(n):
    return (int(n) + 15) & ~15


class JpegInfoAny(object):
    """Geometry of one JPEG stream as gx_jpeg_info_any reports it: width, height, components (1 grey, 3 colour), sampling
    class (0 = 4:4:4 or grey, 1 = 4:2:2, 2 = 4:2:0), blocks of the padded planes and the restart interval."""
    __slots__ = ('width', 'height', 'components', 'sampling', 'blocks', 'restart_interval')

    def __init__(self, raw):
        self.width, self.height, self.components, self.sampling = (int(v) for v in raw[:4])
        self.blocks = tuple(int(v) for v in raw[4:7])
        self.restart_interval = int(raw[7])

    def __repr__(self):
        return 'JpegInfoAny(%dx%d, %d components, %s, blocks %s, restart %d)' % (
            self.width, self.height, self.components, SAMPLING_NAMES[self.sampling], list(self.blocks), self.restart_interval)


def jpeg_info_any(data):
    """JpegInfoAny of a stream (bytes / uint8 array); raises GenesisHipError for what the decoder does not accept."""
    a = _lib.as_u8(data, 'imagefile')
    raw = np.zeros(8, dtype=np.int32)
    _lib.call('gx_jpeg_info_any', _ptr(a), a.size, _ptr(raw))
    return JpegInfoAny(raw)


def entropy_decode_any(data, coef, qtab):
    """Entropy-decodes one stream into coef (int16, at least blocks * 64 values) and qtab (uint16, 192 values): quantised
    coefficients in natural order, per component plane in block raster order; a grey frame has one plane.  -> JpegInfoAny.
    Host only; the C call runs without the GIL."""
    a = _lib.as_u8(data, 'imagefile')
    if coef.dtype != np.int16 or not coef.flags.c_contiguous or not coef.flags.writeable:
        raise GenesisHipError('imagefile: coef must be a writable C-contiguous int16 array')
    if qtab.dtype != np.uint16 or qtab.size < 192 or not qtab.flags.c_contiguous or not qtab.flags.writeable:
        raise GenesisHipError('imagefile: qtab must be a writable C-contiguous uint16 array of 192 values')
    raw = np.zeros(8, dtype=np.int32)
    _lib.call('gx_jpeg_entropy_decode_any', _ptr(a), a.size, _ptr(coef), coef.size, _ptr(qtab), _ptr(raw))
    return JpegInfoAny(raw)


def stream_kind(data):
    """'png' or 'jpeg' from the magic bytes of a stream (never from a file name)."""
    head = bytes(_lib.as_u8(data, 'imagefile')[:8])
    if head == PNG_MAGIC:
        return 'png'
    if head[:2] == JPEG_MAGIC:
        return 'jpeg'
    raise GenesisHipError('imagefile: neither a PNG nor a JPEG stream (it begins with %s)' % (head.hex() or 'nothing'))


def resize_crop_geometry(H, W, S):
    """torchvision's Resize(S) + CenterCrop(S) on an H x W frame -> (h', w', top', left'): the size the whole frame is resized
    to and where the S x S window lies in it."""
    if H <= 0 or W <= 0 or S <= 0:
        raise GenesisHipError('imagefile: bad sizes (%d x %d -> %d)' % (W, H, S))
    if W <= H:
        w2, h2 = S, int(S * H / W)
    else:
        w2, h2 = int(S * W / H), S
    return h2, w2, int(round((h2 - S) / 2.0)), int(round((w2 - S) / 2.0))


_coeff_cache = {}
_coeff_lock = threading.Lock()


def axis_tables(n_in, n_out):
    """Pillow's BILINEAR tables of one axis (feeder.pil_bilinear_coeffs), computed once per distinct (n_in, n_out)."""
    key = (int(n_in), int(n_out))
    t = _coeff_cache.get(key)
    if t is None:
        t = feeder.pil_bilinear_coeffs(*key)
        with _coeff_lock:
            if len(_coeff_cache) > 4096:        # a folder of many sizes: start over rather than grow without bound
                _coeff_cache.clear()
            _coeff_cache[key] = t
    return t


def window_tables(H, W, S):
    """(h', w', [hb, hw, vb, vw]) of one frame: the rows of the two axis tables that the output window uses -- columns
    left' .. left' + S of W -> w', rows top' .. top' + S of H -> h' -- each an int32 array."""
    h2, w2, top, left = resize_crop_geometry(H, W, S)
    hb, hw = axis_tables(W, w2)
    vb, vw = axis_tables(H, h2)
    return h2, w2, [hb[left:left + S], hw[left:left + S], vb[top:top + S], vw[top:top + S]]


def frame_bound(max_side, S):
    """Bytes of arena that any accepted frame of at most max_side x max_side needs: its payload (4:4:4 coefficients or RGBA
    rows, whichever is larger) and its window tables."""
    blocks = 3 * (-(-max_side // 8)) ** 2
    payload = max(blocks * 128 + _QTAB_BYTES, max_side * (1 + 4 * max_side))
    kmax = 2 * (-(-max_side // S) + 1) + 1
    return _round16(payload) + _round16(4 * S * (4 + 2 * kmax))


class _Frame(object):
    __slots__ = ('kind', 'H', 'W', 'C', 'sampling', 'blocks', 'payload', 'tables', 'h2', 'w2', 'kh', 'kv')


class Arena(object):
    """One batch's staging: a byte buffer (pinned by default) with the descriptor tables of up to `batch` frames at the front
    and a bump allocator behind them, which reader threads share."""

    def __init__(self, batch, nbytes, pin=True):
        self.batch = int(batch)
        self.desc_bytes = _round16(self.batch * (JPEGR_WORDS + PNGR_WORDS + RSR_WORDS) * 8)
        self.nbytes = self.desc_bytes + int(nbytes)
        self.buffer = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=bool(pin))
        self.host = self.buffer.numpy()
        self.lock = threading.Lock()
        self.used = self.desc_bytes

    def reset(self):
        self.used = self.desc_bytes

    def alloc(self, nbytes):
        """Offset of nbytes (rounded up to 16) of the arena, or -1 when it is full."""
        with self.lock:
            at, end = self.used, self.used + _round16(nbytes)
            if end > self.nbytes:
                return -1
            self.used = end
            return at


def frame_need(data, S, max_side):
    """(kind, info, payload bytes, window tables) of one stream: its header is read, nothing is decoded."""
    kind = stream_kind(data)
    info = png.png_info(data) if kind == 'png' else jpeg_info_any(data)
    if info.width > max_side or info.height > max_side:
        raise GenesisHipError('imagefile: a %d x %d frame exceeds max_side = %d' % (info.width, info.height, max_side))
    payload = info.inflated_size if kind == 'png' else sum(info.blocks) * 128 + _QTAB_BYTES
    return kind, info, payload, window_tables(info.height, info.width, S)


def stage_frame(arena, data, S, max_side):
    """Reads one stream's header, takes its place in the arena, decodes the serial half into it and lays its window tables
    behind it.  -> _Frame.  Safe to call from several threads on one arena."""
    data = _lib.as_u8(data, 'imagefile')
    kind, info, payload, (h2, w2, tabs) = frame_need(data, S, max_side)
    tbytes = 4 * sum(t.size for t in tabs)
    at = arena.alloc(_round16(payload) + tbytes)
    if at < 0:
        raise GenesisHipError('imagefile: the %d x %d frame does not fit what is left of the staging arena (%d bytes, sized for '
                              '%d frames of at most max_side = %d)' % (info.width, info.height, arena.nbytes, arena.batch, max_side))
    f = _Frame()
    f.kind, f.H, f.W, f.h2, f.w2, f.payload = kind, info.height, info.width, h2, w2, at
    if kind == 'png':
        f.C, f.sampling, f.blocks = info.channels, 0, 0
        png.inflate(data, arena.host[at:at + payload])
    else:
        f.C, f.sampling, f.blocks = info.components, info.sampling, sum(info.blocks)
        nc = f.blocks * 128
        entropy_decode_any(data, arena.host[at:at + nc].view(np.int16), arena.host[at + nc:at + nc + _QTAB_BYTES].view(np.uint16))
    f.kh, f.kv = tabs[1].shape[1], tabs[3].shape[1]
    f.tables = []
    t = at + _round16(payload)
    for a in tabs:
        arena.host[t:t + 4 * a.size].view(np.int32)[:] = a.reshape(-1)
        f.tables.append(t // 4)
        t += 4 * a.size
    return f


class Layout(object):
    """Where a staged batch's frames go on the device, and its three descriptor tables (int64 views of the arena's front)."""
    __slots__ = ('n', 'jpeg', 'png', 'jt', 'pt', 'rt', 'jt_at', 'pt_at', 'rt_at', 'dst', 'dst_bytes', 'scratch_bytes', 'used', 'S')


def lay_out(arena, frames, S):
    """Writes the descriptor tables of `frames` (in batch order) into the arena's front and plans the resample launch."""
    n = len(frames)
    if not 0 < n <= arena.batch:
        raise GenesisHipError('imagefile: %d frames in an arena for %d' % (n, arena.batch))
    L = Layout()
    L.n, L.S, L.used = n, S, arena.used
    L.jpeg = [i for i, f in enumerate(frames) if f.kind == 'jpeg']
    L.png = [i for i, f in enumerate(frames) if f.kind == 'png']
    words = arena.host[:arena.desc_bytes].view(np.int64)
    L.jt_at, L.pt_at, L.rt_at = 0, len(L.jpeg) * JPEGR_WORDS * 8, (len(L.jpeg) * JPEGR_WORDS + len(L.png) * PNGR_WORDS) * 8
    L.jt = words[:len(L.jpeg) * JPEGR_WORDS].reshape(-1, JPEGR_WORDS)
    L.pt = words[L.pt_at // 8:L.rt_at // 8].reshape(-1, PNGR_WORDS)
    L.rt = words[L.rt_at // 8:L.rt_at // 8 + n * RSR_WORDS].reshape(-1, RSR_WORDS)
    L.dst, at = [], 0
    for f in frames:
        L.dst.append(at)
        at += _round16(f.H * f.W * f.C)
    L.dst_bytes = at
    planes = wg_idct = wg_pix = 0
    for row, i in zip(L.jt, L.jpeg):
        f = frames[i]
        row[:] = (f.H, f.W, f.C, f.sampling, f.payload // 2, (f.payload + f.blocks * 128) // 2, planes, L.dst[i], wg_idct, wg_pix)
        planes += f.blocks * 64
        wg_idct += -(-f.blocks // JPEGR_BLOCKS_PER_WG)
        wg_pix += -(-f.H // JPEGR_TILE_H) * -(-f.W // JPEGR_TILE_W)
    L.scratch_bytes = planes
    for row, i in zip(L.pt, L.png):
        f = frames[i]
        row[:] = (f.H, f.W, f.C, f.payload, L.dst[i])
    for row, f, dst in zip(L.rt, frames, L.dst):
        row[:] = (f.H, f.W, f.C, dst, f.h2, f.w2, f.tables[0], f.tables[1], f.kh, f.tables[2], f.tables[3], f.kv, 0, 0)
    total = ctypes.c_longlong()
    _lib.call('gx_u8_resample_ragged_plan', _ptr(L.rt), n, S, S, ctypes.byref(total))
    return L


def launch(arena, dev, L, frames, out=None, return_u8=False):
    """The four launches on `dev`, a device copy of the arena's first L.used bytes -> fp32 [n, 3, S, S] (and the list of the
    decoded uint8 [H, W, C] views with return_u8), on the current stream."""
    device = dev.device
    shape = (L.n, 3, L.S, L.S)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != device
          or not out.is_contiguous()):
        raise GenesisHipError('imagefile: out must be a contiguous float32 tensor of shape %s on %s, not %s %s on %s'
                              % (list(shape), device, getattr(out, 'dtype', type(out)), list(getattr(out, 'shape', [])),
                                 getattr(out, 'device', None)))
    u8 = torch.empty(L.dst_bytes, dtype=torch.uint8, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    base, host = dev.data_ptr(), arena.host.ctypes.data
    if L.jpeg:
        scratch = torch.empty(L.scratch_bytes, dtype=torch.uint8, device=device)
        _lib.call('gx_jpeg_decode_ragged', ctypes.c_void_p(host + L.jt_at), ctypes.c_void_p(base + L.jt_at), len(L.jpeg),
                  ctypes.c_void_p(base), L.used // 2, ctypes.c_void_p(base), L.used // 2, ctypes.c_void_p(scratch.data_ptr()),
                  L.scratch_bytes, ctypes.c_void_p(u8.data_ptr()), L.dst_bytes, stream)
    if L.png:
        _lib.call('gx_png_unfilter_ragged', ctypes.c_void_p(host + L.pt_at), ctypes.c_void_p(base + L.pt_at), len(L.png),
                  ctypes.c_void_p(base), L.used, ctypes.c_void_p(u8.data_ptr()), L.dst_bytes, stream)
    _lib.call('gx_u8_resample_ragged_f32chw', ctypes.c_void_p(host + L.rt_at), ctypes.c_void_p(base + L.rt_at), L.n,
              ctypes.c_void_p(u8.data_ptr()), L.dst_bytes, ctypes.c_void_p(base), L.used // 4, ctypes.c_void_p(out.data_ptr()),
              L.S, L.S, stream)
    if return_u8:
        return out, [u8[at:at + f.H * f.W * f.C].view(f.H, f.W, f.C) for f, at in zip(frames, L.dst)]
    return out


def _check_size(img_size):
    if not isinstance(img_size, int) or isinstance(img_size, bool) or not 0 < img_size <= MAX_SIZE:
        raise GenesisHipError('imagefile: img_size must be an int in [1, %d], not %r' % (MAX_SIZE, img_size))
    return img_size


def decode_image_batch(streams, img_size, return_u8=False, out=None, device='cuda', max_side=MAX_DIM):
    """streams: a list of PNG and JPEG byte strings / uint8 arrays, of any sizes, in any mixture (the format is recognised by
    the magic bytes) -> fp32 device tensor [B, 3, S, S] in [0, 1]: Resize(S, BILINEAR) + CenterCrop(S) + ToTensor on Pillow's
    convert('RGB') of every frame, bit for bit (the module's docstring states the transform).  return_u8: also the list of the
    decoded uint8 [H, W, C] frames (views of one device arena; C = 1 for grey, 4 for RGBA), as a second result.  out: a
    contiguous fp32 [B, 3, S, S] tensor on the device to write into.  A frame wider or higher than max_side is refused.
    Every call allocates its own pinned arena and decodes on the calling thread: a path for a handful of streams, evaluation
    and tests.  Training reads through ImageFileLoader."""
    S = _check_size(img_size)
    streams = [_lib.as_u8(s, 'imagefile') for s in streams]
    if not streams:
        raise GenesisHipError('imagefile: an empty batch')
    device = torch.device(device)
    if device.type != 'cuda':
        raise GenesisHipError('imagefile: frames are decoded on the HIP device; there is no CPU path')
    if out is not None and isinstance(out, torch.Tensor) and out.device.type != 'cuda':
        raise GenesisHipError('imagefile: out must be on the HIP device, not on %s' % out.device)
    need = 0
    for s in streams:
        _, _, payload, (_, _, tabs) = frame_need(s, S, max_side)
        need += _round16(payload) + _round16(4 * sum(t.size for t in tabs))
    arena = Arena(len(streams), need)
    frames = [stage_frame(arena, s, S, max_side) for s in streams]
    L = lay_out(arena, frames, S)
    dev = arena.buffer[:L.used].to(device, non_blocking=True)
    return launch(arena, dev, L, frames, out, return_u8)


class ImageFileLoader(loading.FileBatchLoader):
    """Batches of image files on the device: {'input': fp32 [B, 3, S, S]}, S = img_size, under the module's transform.
    Length, order, the short last batch, reseeding and how a bad file is reported: loading.FileBatchLoader.
    shard=(rank, world) keeps every world-th file from the rank-th on.

    The reader threads stage (stage_frame) into the pinned arena of a slot; per batch there is one copy of the arena's used
    prefix and the four launches.  An arena holds batch_size frames of at most max_side x max_side (frame_bound): a frame
    above max_side raises GenesisHipError naming the file and max_side."""

    def __init__(self, files, batch_size, img_size, shuffle=True, seed=0, num_workers=4, device='cuda', depth=3, max_side=1024,
                 shard=None, name='imagefile'):
        if not isinstance(max_side, int) or not 0 < max_side <= MAX_DIM:
            raise GenesisHipError('%s: max_side must be an int in [1, %d], not %r' % (name, MAX_DIM, max_side))
        rank, world = loading.parse_shard(shard, name)
        super().__init__(list(files)[rank::world], batch_size, shuffle, seed, num_workers, device, depth, name)
        self.img_size = _check_size(img_size)
        self.max_side = max_side

    def _open_ring(self):
        """-> (the arenas, their device copies)"""
        if self.device.type != 'cuda':
            raise GenesisHipError('%s: frames are decoded on the HIP device; there is no CPU path' % self.name)
        nbytes = self.batch_size * frame_bound(self.max_side, self.img_size)
        arenas = [Arena(self.batch_size, nbytes) for _ in range(self.depth)]
        return arenas, [torch.empty(a.nbytes, dtype=torch.uint8, device=self.device) for a in arenas]

    def _jobs(self, s, idx):
        arena = self.ring[0][s]
        arena.reset()
        decode = functools.partial(stage_frame, arena, S=self.img_size, max_side=self.max_side)
        return [(self.files[f], decode) for f in idx]

    def _stage(self, s, n, frames):
        arenas, dev = self.ring
        L = lay_out(arenas[s], frames, self.img_size)
        dev[s][:L.used].copy_(arenas[s].buffer[:L.used], non_blocking=True)
        return frames, L

    def _batch(self, s, staged):
        arenas, dev = self.ring
        return {'input': launch(arenas[s], dev[s], staged[1], staged[0])}
