"""On-device batch feeder: the reference converts every sample to fp32 on the host
(datasets/multid_config.py:131-135: ToTensor + F.interpolate; multi_object_config.py:176-186) and copies the fp32 batch
to the GPU inside the training loop (train.py:218-220).  Here the uint8 HWC frames are staged in pinned memory, copied
on a side stream one batch ahead (a ring of slots) and converted to the fp32 NCHW batch in [0,1] by one HIP launch, so
the step after compute does not wait on the host."""
import ctypes

import torch

from . import _lib
from ._lib import GenesisHipError
from .loading import SlotEvents


def u8hwc_to_f32chw(frames_u8, img_size=None, out=None):
    """frames_u8: uint8 device tensor [B, Hs, Ws, C] -> float32 [B, C, S, S] (S = img_size or Hs), values / 255,
    nearest-neighbour resampled like F.interpolate(size=S)."""
    if not frames_u8.is_cuda:
        raise GenesisHipError('feeder: frames must be on the HIP device; there is no CPU path')
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous():
        raise GenesisHipError('feeder: expected a contiguous uint8 [B,H,W,C] tensor')
    B, Hs, Ws, C = frames_u8.shape
    H = W = int(img_size) if img_size else Hs
    if img_size is None:
        W = Ws
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=frames_u8.device)
    _lib.call('gx_u8hwc_to_f32chw', ctypes.c_void_p(frames_u8.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, Hs, Ws,
              C, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


_RESAMPLE_MODES = {'nearest': 0, 'bilinear': 1}
_LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}
_coeff_cache = {}


def centre_box(Hs, Ws, crop):
    """The centre-crop window (top, left, h, w) of an Hs x Ws frame, as utils/misc.py:45-56 np_img_centre_crop cuts it:
    top = (Hs - h) // 2, left = (Ws - w) // 2.  `crop` is an int (square) or (h, w).  torchvision's CenterCrop (the PIL
    path of datasets/shapestacks_config.py:126) uses round((Hs - h) / 2.0) instead, which differs only when Hs - h is odd
    (floor vs round half to even); ShapeStacks (224 -> 196) and CLEVR (240 x 320 -> 192) have even differences."""
    h, w = (crop, crop) if isinstance(crop, int) else (int(crop[0]), int(crop[1]))
    if not (0 < h <= Hs and 0 < w <= Ws):
        raise GenesisHipError('feeder: crop %dx%d does not fit a %dx%d frame' % (h, w, Hs, Ws))
    return ((Hs - h) // 2, (Ws - w) // 2, h, w)


def pil_bilinear_coeffs(n_in, n_out):
    """Pillow's BILINEAR coefficient tables of one axis (host, C ABI gx_pil_bilinear_coeffs): bounds int32 [n_out, 2] =
    (first source index, taps), weights int32 [n_out, ksize] with 22 fractional bits."""
    import numpy as np
    ksize = _lib.query('gx_pil_bilinear_ksize', int(n_in), int(n_out))
    if ksize <= 0:
        raise GenesisHipError('feeder: bad resample sizes %d -> %d' % (n_in, n_out))
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    weights = np.zeros((n_out, ksize), dtype=np.int32)
    _lib.call('gx_pil_bilinear_coeffs', int(n_in), int(n_out), ksize, bounds.ctypes.data_as(ctypes.c_void_p),
              weights.ctypes.data_as(ctypes.c_void_p))
    return bounds, weights


def _device_coeffs(Hc, H, Wc, W, device):
    key = (Hc, H, Wc, W, device)
    t = _coeff_cache.get(key)
    if t is None:
        hb, hw = pil_bilinear_coeffs(Wc, W)
        vb, vw = pil_bilinear_coeffs(Hc, H)
        t = tuple(torch.from_numpy(a).to(device) for a in (hb, hw, vb, vw))
        _coeff_cache[key] = t
    return t


def _size_and_box(Hs, Ws, size, crop):
    top, left, Hc, Wc = (0, 0, Hs, Ws) if crop is None else (int(v) for v in crop)
    if size is None:
        H, W = Hc, Wc
    elif isinstance(size, int):
        H = W = size
    else:
        H, W = int(size[0]), int(size[1])
    return top, left, Hc, Wc, H, W


def _check_out(out, shape, dtype, device):
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise GenesisHipError('feeder: out must be a contiguous %s tensor of shape %s on %s, not %s %s on %s'
                              % (dtype, list(shape), device, out.dtype, list(out.shape), out.device))


def transform_frames(frames_u8, size, crop=None, resize='nearest', out=None):
    """frames_u8: uint8 device tensor [B, Hs, Ws, C] -> float32 [B, C, H, W], values / 255, of the crop window
    crop = (top, left, h, w) (None: the whole frame) resampled to size = S or (H, W) (None: the window's size).
    resize='nearest': F.interpolate's default mode (datasets/multi_object_config.py:181-202, CLEVR); 'bilinear': Pillow's
    antialiased BILINEAR resize, which torchvision's Resize applies to a PIL image (datasets/shapestacks_config.py:126-130),
    bit-exact."""
    if not frames_u8.is_cuda:
        raise GenesisHipError('feeder: frames must be on the HIP device; there is no CPU path')
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or not frames_u8.is_contiguous():
        raise GenesisHipError('feeder: expected a contiguous uint8 [B,H,W,C] tensor')
    if resize not in _RESAMPLE_MODES:
        raise GenesisHipError('feeder: resize must be one of %s, not %r' % (sorted(_RESAMPLE_MODES), resize))
    B, Hs, Ws, C = frames_u8.shape
    top, left, Hc, Wc, H, W = _size_and_box(Hs, Ws, size, crop)
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=frames_u8.device)
    _check_out(out, (B, C, H, W), torch.float32, frames_u8.device)
    tables = [None] * 4
    kh = kv = 0
    if resize == 'bilinear' and min(Hc, Wc, H, W) > 0:
        tables = [ctypes.c_void_p(t.data_ptr()) for t in _device_coeffs(Hc, H, Wc, W, frames_u8.device)]
        kh, kv = _lib.query('gx_pil_bilinear_ksize', Wc, W), _lib.query('gx_pil_bilinear_ksize', Hc, H)
    _lib.call('gx_u8hwc_resample_f32chw', ctypes.c_void_p(frames_u8.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, Hs, Ws,
              C, top, left, Hc, Wc, H, W, _RESAMPLE_MODES[resize], tables[0], tables[1], kh, tables[2], tables[3], kv,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


def transform_labels(labels, size, crop=None, out=None):
    """labels: uint8 / int32 / int64 device tensor [B, Hs, Ws] or [B, 1, Hs, Ws] -> int64 [B, 1, H, W]: the crop window
    resampled nearest, as the reference moves instance maps (datasets/shapestacks_config.py:155-162,
    multi_object_config.py:198-203: F.interpolate(cropped.float(), size).long()); equal to it for every label an fp32 holds
    exactly.  crop / size as in transform_frames."""
    if not labels.is_cuda:
        raise GenesisHipError('feeder: labels must be on the HIP device; there is no CPU path')
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if labels.dtype not in _LABEL_DTYPES or labels.dim() != 3 or not labels.is_contiguous():
        raise GenesisHipError('feeder: expected a contiguous uint8 / int32 / int64 [B,H,W] label tensor')
    B, Hs, Ws = labels.shape
    top, left, Hc, Wc, H, W = _size_and_box(Hs, Ws, size, crop)
    if out is None:
        out = torch.empty(B, 1, H, W, dtype=torch.int64, device=labels.device)
    _check_out(out, (B, 1, H, W), torch.int64, labels.device)
    _lib.call('gx_labels_crop_nearest', ctypes.c_void_p(labels.data_ptr()), _LABEL_DTYPES[labels.dtype],
              ctypes.c_void_p(out.data_ptr()), B, Hs, Ws, top, left, Hc, Wc, H, W,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


_MASK_LAYOUTS = ('ehw', 'hwe')


def _mask_dims(shape, layout):
    """(B, E, Hs, Ws) of a mask stack [B,E,H,W] ('ehw') or [B,H,W,E] ('hwe'), either with a trailing axis of 1 as stored."""
    if layout not in _MASK_LAYOUTS:
        raise GenesisHipError('feeder: mask layout must be one of %s, not %r' % (list(_MASK_LAYOUTS), layout))
    shape = tuple(shape)
    if len(shape) == 5 and shape[4] == 1:
        shape = shape[:4]
    if len(shape) != 4:
        raise GenesisHipError('feeder: expected a mask stack [B,E,H,W] or [B,H,W,E] (optionally with a last axis of 1), not %s'
                              % list(shape))
    return shape if layout == 'ehw' else (shape[0], shape[3], shape[1], shape[2])


def entity_masks_to_labels(masks, background_entities, size=None, crop=None, layout='ehw', out=None):
    """masks: uint8 device stack of per-entity masks, [B,E,Hs,Ws] (layout 'ehw': ObjectsRoom, CLEVR, Tetrominoes) or
    [B,Hs,Ws,E] ('hwe': Multi-dSprites as stored, which the reference transposes), optionally with the stored last axis of
    1 -> int64 instance maps [B,1,H,W]: label = o + 1 of the highest entity o >= background_entities whose mask is 255
    there, 0 if none (datasets/multi_object_config.py:188-203), of the crop window resampled nearest as in
    transform_labels.  One HIP launch reads the stack in place."""
    if not masks.is_cuda:
        raise GenesisHipError('feeder: masks must be on the HIP device; there is no CPU path')
    if masks.dtype != torch.uint8 or not masks.is_contiguous():
        raise GenesisHipError('feeder: expected a contiguous uint8 mask stack')
    B, E, Hs, Ws = _mask_dims(masks.shape, layout)
    top, left, Hc, Wc, H, W = _size_and_box(Hs, Ws, size, crop)
    if out is None:
        out = torch.empty(B, 1, H, W, dtype=torch.int64, device=masks.device)
    _check_out(out, (B, 1, H, W), torch.int64, masks.device)
    es, ps = (Hs * Ws, 1) if layout == 'ehw' else (1, E)
    _lib.call('gx_entity_masks_to_labels', ctypes.c_void_p(masks.data_ptr()), ctypes.c_void_p(out.data_ptr()), B, E, Hs, Ws,
              es, ps, int(background_entities), top, left, Hc, Wc, H, W,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


_ROW_DTYPES = {torch.uint8: 0, torch.float32: 1}
_ROW_LABEL_DTYPES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3, torch.float64: 4}
SPRITE_SIZE = 64
MAX_SPRITES_PER_IMAGE = 4


def _gather_args(src, idx, first, B, what):
    if not src.is_cuda:
        raise GenesisHipError('feeder: %s must be on the HIP device; there is no CPU path' % what)
    if idx is not None and (not idx.is_cuda or idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous()):
        raise GenesisHipError('feeder: idx must be a contiguous int64 vector on the HIP device')
    n = src.shape[0] if idx is None else idx.shape[0]
    first = int(first)
    B = n - first if B is None else int(B)
    if first < 0 or B <= 0 or first + B > n:
        raise GenesisHipError('feeder: rows %d .. %d reach outside the %d %s' % (first, first + B, n,
                                                                                'rows stored' if idx is None else 'indices'))
    return first, B, (None if idx is None else ctypes.c_void_p(idx.data_ptr())), (0 if idx is None else int(idx.shape[0]))


def _square(size, Hs, Ws):
    if size is None:
        return Hs, Ws
    return (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))


def rows_gather(src, idx=None, first=0, B=None, size=None, out=None):
    """src: uint8 or float32 device tensor [N, Hs, Ws, C], a whole split as stored -> float32 [B, C, H, W]: the rows
    idx[first : first + B] of it (idx: int64 device vector, e.g. an epoch's permutation; None: the rows first : first + B
    themselves), uint8 / 255 and float32 unchanged (ToTensor's two cases), resampled nearest like F.interpolate(size=) when
    size differs from the stored one.  One HIP launch on the current stream and nothing else: no copy, no synchronisation.
    The values of idx are NOT checked (that would read them back): the caller checks them on the host before uploading."""
    if src.dtype not in _ROW_DTYPES or src.dim() != 4 or not src.is_contiguous():
        raise GenesisHipError('feeder: expected a contiguous uint8 or float32 [N,H,W,C] tensor, not %s %s'
                              % (src.dtype, list(src.shape)))
    first, B, pidx, nidx = _gather_args(src, idx, first, B, 'frames')
    N, Hs, Ws, C = src.shape
    H, W = _square(size, Hs, Ws)
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=src.device)
    _check_out(out, (B, C, H, W), torch.float32, src.device)
    _lib.call('gx_rows_gather_f32chw', ctypes.c_void_p(src.data_ptr()), _ROW_DTYPES[src.dtype], N, pidx, nidx, first,
              ctypes.c_void_p(out.data_ptr()), B, Hs, Ws, C, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


def rows_gather_labels(src, idx=None, first=0, B=None, size=None, out=None):
    """src: uint8 / int32 / int64 / float32 / float64 device tensor [N, Hs, Ws] or [N, Hs, Ws, 1] of label maps -> int64
    [B, 1, H, W]: the same rows as rows_gather, nearest, converted by truncation (datasets/multid_config.py:137-143:
    ToTensor, F.interpolate, .type(LongTensor))."""
    if src.dim() == 4 and src.shape[3] == 1:
        src = src[..., 0]
    if src.dtype not in _ROW_LABEL_DTYPES or src.dim() != 3 or not src.is_contiguous():
        raise GenesisHipError('feeder: expected contiguous uint8 / int32 / int64 / float32 / float64 label maps [N,H,W] or '
                              '[N,H,W,1], not %s %s' % (src.dtype, list(src.shape)))
    first, B, pidx, nidx = _gather_args(src, idx, first, B, 'label maps')
    N, Hs, Ws = src.shape
    H, W = _square(size, Hs, Ws)
    if out is None:
        out = torch.empty(B, 1, H, W, dtype=torch.int64, device=src.device)
    _check_out(out, (B, 1, H, W), torch.int64, src.device)
    _lib.call('gx_rows_gather_labels', ctypes.c_void_p(src.data_ptr()), _ROW_LABEL_DTYPES[src.dtype], N, pidx, nidx, first,
              ctypes.c_void_p(out.data_ptr()), B, Hs, Ws, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return out


def sprites_compose(sprites, first, count, colours, img=None, mask=None):
    """The pasting loop of scripts/generate_multid.py:47-73 for n images in one HIP launch.  sprites: uint8 device stack
    [S, 64, 64] (non-zero = set); first, count: int32 device vectors [n], image i pastes sprites first[i] ..
    first[i] + count[i] - 1 in that order (count 0..4); colours: uint8 device [n, 5, 3], the background and then the
    objects.  -> (img float32 [n, 64, 64, 3] = byte / 255, mask uint8 [n, 64, 64]); the last sprite covering a pixel wins.
    The caller checks first + count against S on the host."""
    n = int(first.shape[0])
    for t, dtype, shape, name in ((sprites, torch.uint8, (sprites.shape[0], SPRITE_SIZE, SPRITE_SIZE), 'sprites'),
                                  (first, torch.int32, (n,), 'first'), (count, torch.int32, (n,), 'count'),
                                  (colours, torch.uint8, (n, MAX_SPRITES_PER_IMAGE + 1, 3), 'colours')):
        if not t.is_cuda:
            raise GenesisHipError('feeder: %s must be on the HIP device; there is no CPU path' % name)
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise GenesisHipError('feeder: %s must be a contiguous %s tensor of shape %s, not %s %s'
                                  % (name, dtype, list(shape), t.dtype, list(t.shape)))
    if img is None:
        img = torch.empty(n, SPRITE_SIZE, SPRITE_SIZE, 3, dtype=torch.float32, device=sprites.device)
    if mask is None:
        mask = torch.empty(n, SPRITE_SIZE, SPRITE_SIZE, dtype=torch.uint8, device=sprites.device)
    _check_out(img, (n, SPRITE_SIZE, SPRITE_SIZE, 3), torch.float32, sprites.device)
    _check_out(mask, (n, SPRITE_SIZE, SPRITE_SIZE), torch.uint8, sprites.device)
    _lib.call('gx_sprites_compose', ctypes.c_void_p(sprites.data_ptr()), int(sprites.shape[0]), ctypes.c_void_p(first.data_ptr()),
              ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(colours.data_ptr()), ctypes.c_void_p(img.data_ptr()),
              ctypes.c_void_p(mask.data_ptr()), n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return img, mask


class DeviceFeeder(object):
    """Iterates fp32 device batches from an iterable of uint8 HWC host batches (numpy arrays or CPU tensors
    [B, H, W, C]).  A ring of `depth` slots (pinned staging buffer + uint8 device buffer); the host->device copy of
    batch i+1 runs on a side stream while batch i is being consumed, and the consumer's stream waits for it with one
    event (copy -> compute).  A slot is refilled only after the host has seen both its copy and the conversion kernels
    that read it complete: loading.SlotEvents, which gives the measurements behind that and behind the deep ring.

    Other datasets' transforms: `crop` = (top, left, h, w) (centre_box) and `resize` ('nearest' / 'bilinear') as in
    transform_frames.  Dict batches {'input': uint8 [B,H,W,C], 'instances': int [B,H,W] or [B,1,H,W]} (as the reference's
    loaders yield them; 'instances' optional) come out as {'input': fp32 [B,C,S,S], 'instances': int64 [B,1,S,S]}: a slot
    then holds both buffers, and its `consumed` event is recorded after both conversions.

    Entity-mask stacks: a dict batch may carry 'masks' instead of 'instances' -- the uint8 stack [B,E,H,W] (mask_layout
    'ehw') or [B,H,W,E] ('hwe'), optionally with the stored last axis of 1, as the multi-object TFRecord datasets hold it
    (genesis_amd/multi_object_config.py).  It crosses PCIe as stored and comes out as 'instances' through
    entity_masks_to_labels with `background_entities`, which must then be given.

    reset(host_batches) starts on a new iterable (the next epoch) and keeps the ring's buffers."""

    def __init__(self, host_batches, img_size, device='cuda', depth=32, crop=None, resize='nearest', background_entities=None,
                 mask_layout='ehw'):
        if resize not in _RESAMPLE_MODES:
            raise GenesisHipError('feeder: resize must be one of %s, not %r' % (sorted(_RESAMPLE_MODES), resize))
        if mask_layout not in _MASK_LAYOUTS:
            raise GenesisHipError('feeder: mask layout must be one of %s, not %r' % (list(_MASK_LAYOUTS), mask_layout))
        self.background_entities = background_entities
        self.mask_layout = mask_layout
        self.it = iter(host_batches)
        self.img_size = img_size
        self.crop = crop
        self.resize = resize
        self.device = torch.device(device)
        self.depth = max(2, int(depth))
        self.pinned = [None] * self.depth
        self.dev_u8 = [None] * self.depth
        self.pinned_lab = [None] * self.depth   # dict batches with 'instances': the label maps' staging / device buffers
        self.dev_lab = [None] * self.depth
        self.keys = [None] * self.depth      # keys of a dict batch in the slot; None: an array batch
        self.events = SlotEvents(self.depth, self.device)
        self.filled = [False] * self.depth
        self.head = 0                        # slot the next __next__ consumes
        self.tail = 0                        # slot the next prefetch fills
        self._prefetch()

    def _prefetch(self):
        try:
            nxt = next(self.it)
        except StopIteration:
            return
        is_dict = isinstance(nxt, dict)
        lab = None
        if is_dict:
            extra = set(nxt) - {'input', 'instances', 'masks'}
            if 'input' not in nxt or extra:
                raise GenesisHipError("feeder: dict batches hold 'input' and optionally 'instances' or 'masks', not %s"
                                      % sorted(extra))
            t = torch.as_tensor(nxt['input'])
            if 'masks' in nxt:
                if 'instances' in nxt:
                    raise GenesisHipError("feeder: a dict batch holds 'instances' or 'masks', not both")
                if self.background_entities is None:
                    raise GenesisHipError("feeder: batches with 'masks' need the background_entities argument")
                lab = torch.as_tensor(nxt['masks'])
                if lab.dtype != torch.uint8:
                    raise GenesisHipError('feeder: entity masks must be uint8, not %s' % lab.dtype)
                mb, _, mh, mw = _mask_dims(lab.shape, self.mask_layout)
                if t.dim() != 4 or (mb, mh, mw) != tuple(t.shape[:3]):
                    raise GenesisHipError('feeder: masks %s do not match the input frames %s' % (list(lab.shape), list(t.shape)))
            if 'instances' in nxt:
                lab = torch.as_tensor(nxt['instances'])
                if lab.dim() == 4 and lab.shape[1] == 1:
                    lab = lab[:, 0]
                if lab.dtype not in _LABEL_DTYPES:
                    if lab.dtype.is_floating_point or lab.dtype == torch.bool:
                        raise GenesisHipError('feeder: instance maps must be integer, not %s' % lab.dtype)
                    lab = lab.to(torch.int32)
                if lab.dim() != 3 or t.dim() != 4 or lab.shape != t.shape[:3]:
                    raise GenesisHipError('feeder: instances must be [B,H,W] or [B,1,H,W] of the input frames [B,H,W,C]')
        else:
            t = torch.as_tensor(nxt)
        if t.dtype != torch.uint8 or t.dim() != 4:
            raise GenesisHipError('feeder: host batches must be uint8 [B,H,W,C]')
        s = self.tail
        self.events.free(s)
        if lab is not None and (self.pinned_lab[s] is None or self.pinned_lab[s].shape != lab.shape
                                or self.pinned_lab[s].dtype != lab.dtype):
            for q in range(self.depth):      # the label ring likewise, all at once
                if self.pinned_lab[q] is None or self.pinned_lab[q].shape != lab.shape or self.pinned_lab[q].dtype != lab.dtype:
                    self.events.free(q)
                    self.pinned_lab[q] = torch.empty(lab.shape, dtype=lab.dtype, pin_memory=True)
                    self.dev_lab[q] = torch.empty(lab.shape, dtype=lab.dtype, device=self.device)
        if self.pinned[s] is None or self.pinned[s].shape != t.shape:
            # the whole ring at once, the first time a batch shape is seen: a pinned allocation costs ~1 ms of host time,
            # and 32 of them spread over the first 32 steps let the device queue run dry (the host needs the whole next
            # segment to get ahead again: 1.5 k -> 2.8 k -> 6.1 k img/s over the first 300 steps, measured)
            for q in range(self.depth):
                if self.pinned[q] is None or self.pinned[q].shape != t.shape:
                    self.events.free(q)
                    self.pinned[q] = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
                    self.dev_u8[q] = torch.empty(t.shape, dtype=torch.uint8, device=self.device)
        self.pinned[s].copy_(t)
        if lab is not None:
            self.pinned_lab[s].copy_(lab)
        with self.events.copying(s):
            self.dev_u8[s].copy_(self.pinned[s], non_blocking=True)
            if lab is not None:
                self.dev_lab[s].copy_(self.pinned_lab[s], non_blocking=True)
        self.keys[s] = tuple(nxt) if is_dict else None
        self.filled[s] = True
        self.tail = (s + 1) % self.depth

    def reset(self, host_batches):
        """Continues with a new iterable of host batches once the current one is exhausted; the ring's buffers stay."""
        if any(self.filled):
            raise GenesisHipError('feeder: reset() before the current batches were all consumed')
        self.it = iter(host_batches)
        self._prefetch()

    def __iter__(self):
        return self

    def __next__(self):
        s = self.head
        if not self.filled[s]:
            raise StopIteration
        with self.events.reading(s):
            if self.crop is None and self.resize == 'nearest':
                x = u8hwc_to_f32chw(self.dev_u8[s], self.img_size)
            else:
                x = transform_frames(self.dev_u8[s], self.img_size, self.crop, self.resize)
            if self.keys[s] is not None:
                x = {'input': x}
                if 'instances' in self.keys[s]:
                    x['instances'] = transform_labels(self.dev_lab[s], x['input'].shape[2:], self.crop)
                elif 'masks' in self.keys[s]:
                    x['instances'] = entity_masks_to_labels(self.dev_lab[s], self.background_entities, x['input'].shape[2:],
                                                            self.crop, self.mask_layout)
        self.filled[s] = False
        self.head = (s + 1) % self.depth
        self._prefetch()          # refills the next free slot while the caller trains on x
        return x
