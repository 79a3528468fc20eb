"""The reference's picture logging with its arguments and tags, composed on the device: `visualise_outputs` (train.py:423-476),
`colour_seg_masks` (utils/misc.py:82-98), torchvision's `make_grid` for the arguments the reference uses, and the pictures of
scripts/visualise_reconstruction.py:86-121 / scripts/visualise_generation.py:84-111 as uint8 sheets (`reconstruction_sheet`,
`generation_sheet`, `save_png`) without matplotlib, torchvision or Pillow.

Every grid of a forward pass is written by ONE gx_vis_compose launch (include/genesis_hip.h) into one atlas -- the mask planes
read in place for exp and argmax, the padding written by the same launch -- and the atlas comes to the host in ONE copy; the
arrays handed to the writer are views of it (the int64 colour grids: exact conversions of such views).

A writer with `add_images_device` (genesis_amd/tbwriter.py) is handed the atlas's device views instead: the pictures are packed for
their PNGs on the device and come to the host as bytes.

Not here: make_grid's normalize / scale_each, scripts/visualise_data.py (add_histogram logging: genesis_amd/histogram.py)."""
import ctypes
import json
import os.path as osp
import struct
import zlib

import numpy as np
import torch

from . import _lib, compat
from ._lib import GenesisHipError
from .metrics import _packed

compat.install()
from forge.experiment_tools import fprint  # noqa: E402

# kinds, modes and descriptor words of gx_vis_compose (tests/test_visualise_cpu.py holds them against include/genesis_hip.h)
COPY, EXP, EXP_MUL, LABEL_COLOUR, ARGMAX_COLOUR, FILL = range(6)
FP32_CHW, U8_HWC = 0, 1
(D_SRC0, D_SRC1, D_STRIDE0, D_STRIDE1, D_DST, D_WORK, D_ITEMS, D_KIND, D_N, D_C, D_H, D_W, D_K, D_NROW, D_PADDING, D_PAD_VALUE,
 D_MODE, D_VEC, D_PACKED, D_CELL0, D_N_GEOM, D_OWN_PAD) = range(22)
DESC_WORDS = 24


def grid_geometry(n, H, W, nrow=8, padding=2):
    """(padding in force, xmaps, ymaps, grid height, grid width) of make_grid for n images of H x W."""
    p = 0 if n == 1 else padding
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return p, xmaps, ymaps, ymaps * (H + p) + p, xmaps * (W + p) + p


# ---- palettes -------------------------------------------------------------------------------------------------------------
_PALETTES = {}      # (bytes, device) -> device tensor [P, 3] uint8


def load_palette(palette='15'):
    """-> uint8 array [P, 3], P <= 256, from the reference's palette name (utils/colour_palette<name>.json relative to the
    working directory, as utils/misc.py:88 opens it), a path to such a file, or a sequence of RGB triples."""
    if isinstance(palette, str):
        tried = [palette, 'utils/colour_palette%s.json' % palette]
        path = next((p for p in tried if osp.isfile(p)), None)
        if path is None:
            raise GenesisHipError('colour palette %r: neither %s nor %s is a file' % (palette, tried[0], tried[1]))
        with open(path) as f:
            try:
                palette = json.load(f)['palette']
            except (ValueError, KeyError, TypeError) as e:
                raise GenesisHipError('colour palette %s: no {"palette": [[r, g, b], ...]} in it (%s)' % (path, e))
    try:
        arr = np.asarray(palette)
    except Exception as e:
        raise GenesisHipError('colour palette: not a sequence of RGB triples (%s)' % e)
    if arr.ndim != 2 or arr.shape[1] != 3 or not 1 <= arr.shape[0] <= 256 or arr.dtype.kind not in 'iu' \
            or arr.min() < 0 or arr.max() > 255:
        raise GenesisHipError('colour palette: expected 1 to 256 RGB triples of integers in [0, 255], got an array of shape %s, '
                              'dtype %s' % (arr.shape, arr.dtype))
    return np.ascontiguousarray(arr, dtype=np.uint8)


def _device_palette(arr, device):
    key = (arr.tobytes(), str(device))
    if key not in _PALETTES:
        _PALETTES[key] = torch.from_numpy(arr.copy()).to(device)
    return _PALETTES[key]


# ---- the atlas: grids collected on the host, written by one launch -----------------------------------------------------------
def _cuda(t, what):
    if not t.is_cuda:
        raise GenesisHipError('%s: the grids are composed on the HIP device; got a tensor on %s' % (what, t.device))
    return t.detach()


def _images(t, what, dtype=torch.float32):
    """A [n, C, H, W] device tensor whose images are contiguous (copied if they are not) -> (tensor, image stride)."""
    t = _cuda(t, what)
    if t.dim() != 4:
        raise GenesisHipError('%s: expected [n, C, H, W], got %s' % (what, tuple(t.shape)))
    if t.dtype != dtype:
        raise GenesisHipError('%s: expected %s, got %s' % (what, dtype, t.dtype))
    if t.numel() == 0:
        raise GenesisHipError('%s: empty tensor %s' % (what, tuple(t.shape)))
    if not t[0].is_contiguous():
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t[0].numel())


class _Atlas(object):
    """Collects grid descriptors; run() uploads them in one copy and fills the atlas in one launch; fetch() brings it to the
    host in one copy.  add() returns the index of the picture for view() / host_view()."""

    def __init__(self, device, palette=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise GenesisHipError('visualise: the grids are composed on the HIP device; there is no CPU path (got %s)' % self.device)
        self.palette = None if palette is None else np.asarray(palette)
        self.rows, self.keep, self.pictures = [], [], []      # descriptors; tensors the launch reads; (dst, shape, mode)
        self.words = self.work = 0
        self.atlas = self.host = None

    def picture(self, n_geom, H, W, nrow, padding, mode):
        """Reserves the words of one grid -> its index."""
        _, _, _, Hg, Wg = grid_geometry(n_geom, H, W, nrow, padding)
        words = 3 * Hg * Wg if mode == FP32_CHW else (3 * Hg * Wg + 3) // 4
        self.pictures.append((self.words, (Hg, Wg), mode))
        self.words += words
        return len(self.pictures) - 1

    def add(self, pic, kind, n, H, W, src0=0, stride0=0, src1=0, stride1=0, C=3, K=0, planes=None, packed=True, nrow=8,
            padding=2, pad_value=0.0, cell0=0, n_geom=None, own_pad=True, aligned=()):
        """One descriptor into picture `pic`.  aligned: every address and stride that 16-byte loads depend on."""
        n_geom = n if n_geom is None else n_geom
        dst, (Hg, Wg), mode = self.pictures[pic]
        HW = H * W
        vec = HW % 4 == 0 and all(a % 16 == 0 for a in aligned)
        row = [0] * DESC_WORDS
        row[D_SRC0], row[D_SRC1], row[D_STRIDE0], row[D_STRIDE1] = int(src0), int(src1), int(stride0), int(stride1)
        row[D_DST], row[D_WORK], row[D_ITEMS] = dst, self.work, n * HW // 4 if vec else n * HW
        row[D_KIND], row[D_N], row[D_C], row[D_H], row[D_W], row[D_K] = kind, n, C, H, W, K
        row[D_NROW], row[D_PADDING] = int(nrow), int(padding)
        row[D_PAD_VALUE] = struct.unpack('<I', struct.pack('<f', float(pad_value)))[0]
        row[D_MODE], row[D_VEC], row[D_PACKED] = mode, int(vec), int(bool(packed))
        row[D_CELL0], row[D_N_GEOM], row[D_OWN_PAD] = cell0, n_geom, int(bool(own_pad))
        self.work += row[D_ITEMS] + (Hg * Wg if own_pad else 0)
        self.rows.append((row, planes))

    # -- the sources ---------------------------------------------------------------------------------------------------------
    def grid(self, kind, t, what, nrow=8, padding=2, pad_value=0.0):
        """A whole make_grid picture (fp32) of one [n, C, H, W] source: COPY, EXP or LABEL_COLOUR."""
        t, stride = _images(t, what, torch.int64 if kind == LABEL_COLOUR else torch.float32)
        n, C, H, W = t.shape
        if kind != COPY and C != 1:
            raise GenesisHipError('%s: expected one channel, got %s' % (what, tuple(t.shape)))
        pic = self.picture(n, H, W, nrow, padding, FP32_CHW)
        self.keep.append(t)
        aligned = () if kind == LABEL_COLOUR else (t.data_ptr(), 0 if n == 1 else 4 * stride)
        self.add(pic, kind, n, H, W, t.data_ptr(), stride, C=C, nrow=nrow, padding=padding, pad_value=pad_value, aligned=aligned)
        return pic

    def planes(self, planes, what):
        """K log-mask planes [B, 1, H, W] as gx_seg_metrics takes them -> (planes, image stride, plane stride or None)."""
        planes = [_cuda(m, what) for m in planes]
        if not 1 <= len(planes) <= 32:
            raise GenesisHipError('%s: %d mask planes; 1 to 32 are supported' % (what, len(planes)))
        shape = planes[0].shape
        if len(shape) != 4 or shape[1] != 1:
            raise GenesisHipError('%s: mask planes must be [B, 1, H, W], got %s' % (what, tuple(shape)))
        for m in planes:
            if m.shape != shape or m.dtype != torch.float32 or m.device != planes[0].device:
                raise GenesisHipError('%s: mask planes differ in shape, dtype or device, or are not fp32' % what)
        B, _, H, W = shape
        stride = planes[0].stride(0) if B > 1 else H * W
        if stride < H * W or any(not m[0].is_contiguous() or (m.stride(0) if B > 1 else H * W) != stride for m in planes):
            planes, stride = [m.contiguous() for m in planes], H * W
        packed = _packed(planes)
        return planes, stride, None if packed is None else packed[0]

    def argmax_grid(self, planes, what, nrow=8, padding=2, pad_value=0.0):
        planes, stride, step = self.planes(planes, what)
        B, _, H, W = planes[0].shape
        K = len(planes)
        pic = self.picture(B, H, W, nrow, padding, FP32_CHW)
        self.keep.extend(planes)
        ptrs = [m.data_ptr() for m in planes]
        aligned = tuple(ptrs) + (0 if B == 1 else 4 * stride,)
        if step is not None:
            self.add(pic, ARGMAX_COLOUR, B, H, W, ptrs[0], stride, 0, step, K=K, nrow=nrow, padding=padding, pad_value=pad_value,
                     aligned=aligned + (0 if K == 1 else 4 * step,))
        else:
            self.add(pic, ARGMAX_COLOUR, B, H, W, 0, stride, K=K, planes=ptrs, packed=False, nrow=nrow, padding=padding,
                     pad_value=pad_value, aligned=aligned)
        return pic

    # -- launch and transfer ---------------------------------------------------------------------------------------------------
    def run(self):
        """One upload of the table, one launch.  -> the device atlas (fp32 words; the last one is the overflow counter)."""
        G = len(self.rows)
        if G == 0:
            raise GenesisHipError('visualise: nothing to compose')
        tail = []
        for row, planes in self.rows:
            if planes is not None:
                row[D_SRC1] = G * DESC_WORDS + len(tail)
                tail.extend(planes)
        table = np.array([w for row, _ in self.rows for w in row] + tail, dtype=np.int64)
        colour = any(row[D_KIND] in (LABEL_COLOUR, ARGMAX_COLOUR) for row, _ in self.rows)
        if colour and self.palette is None:
            raise GenesisHipError('visualise: a colour grid without a palette')
        with torch.cuda.device(self.device):
            pal = _device_palette(self.palette, self.device) if colour else None
            dev_table = torch.from_numpy(table).to(self.device)
            self.atlas = torch.empty(self.words + 1, dtype=torch.float32, device=self.device)
            self.atlas[self.words:].zero_()      # the overflow counter; every other word is written by the launch
            _lib.call('gx_vis_compose', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(dev_table.data_ptr()), table.size, G,
                      ctypes.c_void_p(pal.data_ptr()) if colour else None, len(self.palette) if colour else 0,
                      ctypes.c_void_p(self.atlas.data_ptr()), self.words + 1,
                      ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self.keep = []      # (the allocator hands their memory out again in stream order only)
        return self.atlas

    def view(self, pic, buffer=None):
        """Picture `pic` as a view of the device atlas (or of `buffer`, a copy of it): fp32 [3, Hg, Wg] or uint8 [Hg, Wg, 3]."""
        buffer = self.atlas if buffer is None else buffer
        dst, (Hg, Wg), mode = self.pictures[pic]
        if mode == FP32_CHW:
            return buffer[dst:dst + 3 * Hg * Wg].view(3, Hg, Wg)
        return buffer[dst:dst + (3 * Hg * Wg + 3) // 4].view(torch.uint8)[:3 * Hg * Wg].view(Hg, Wg, 3)

    def fetch(self):
        """run(), then the one device-to-host copy.  -> the number of labels that lay beyond the palette."""
        self.host = self.run().cpu()
        return int(self.host[self.words:].view(torch.int32)[0]) & 0xffffffff

    def fetch_overflow(self):
        """run(), then only the overflow counter comes to the host (4 bytes); the pictures stay on the device for view()."""
        return int(self.run()[self.words:].view(torch.int32).cpu()[0]) & 0xffffffff

    def host_view(self, pic):
        return self.view(pic, self.host)


# ---- make_grid, colour_seg_masks -----------------------------------------------------------------------------------------------
def make_grid(tensor, nrow=8, padding=2, pad_value=0, **kwargs):
    """torchvision.utils.make_grid(tensor, nrow, padding, normalize=False, pad_value) on the device: a [n, C, H, W] fp32 device
    tensor (C = 1 or 3) or a list of [C, H, W] tensors -> a device tensor [3, ymaps (H + padding) + padding,
    xmaps (W + padding) + padding], xmaps = min(nrow, n); [3, H, W] without a border for n = 1.  One launch, padding included.
    Any other keyword (normalize, value_range, scale_each) raises GenesisHipError."""
    if kwargs:
        raise GenesisHipError('make_grid: the keyword %r is not supported (nrow, padding and pad_value are)' % sorted(kwargs)[0])
    if isinstance(tensor, (list, tuple)):
        if not tensor or any(not torch.is_tensor(t) or t.dim() != 3 for t in tensor):
            raise GenesisHipError('make_grid: a list must hold [C, H, W] tensors')
        tensor = torch.stack(list(tensor), 0)
    if not torch.is_tensor(tensor) or tensor.dim() != 4:
        raise GenesisHipError('make_grid: expected a [n, C, H, W] tensor or a list of [C, H, W] tensors')
    if tensor.shape[1] not in (1, 3):
        raise GenesisHipError('make_grid: C = %d is neither 1 nor 3' % tensor.shape[1])
    if int(nrow) < 1 or int(padding) < 0:
        raise GenesisHipError('make_grid: nrow = %s must be at least 1 and padding = %s non-negative' % (nrow, padding))
    atlas = _Atlas(tensor.device)
    pic = atlas.grid(COPY, tensor, 'make_grid', nrow, padding, pad_value)
    atlas.run()
    return atlas.view(pic)


def _label_maps(masks, what):
    if not torch.is_tensor(masks) or masks.dim() not in (3, 4):
        raise GenesisHipError('%s: expected [B, H, W] or [B, 1, H, W] labels, got %s'
                              % (what, tuple(masks.shape) if torch.is_tensor(masks) else type(masks).__name__))
    if masks.dim() == 3:
        masks = masks.unsqueeze(1)
    if masks.shape[1] != 1:
        raise GenesisHipError('%s: expected one channel, got %s' % (what, tuple(masks.shape)))
    if masks.dtype.is_floating_point or masks.dtype.is_complex or masks.dtype == torch.bool:
        raise GenesisHipError('%s: expected integer labels, got %s' % (what, masks.dtype))
    return masks.to(torch.int64)


def colour_seg_masks(masks, palette='15'):
    """utils/misc.py:82-98: integer labels [B, H, W] or [B, 1, H, W] on the device -> int64 [B, 3, H, W], palette[label] per
    pixel, black for negative (ignore) labels.  No host read inside, so a label outside the palette cannot raise here as the
    reference's IndexError does: it gives black, and `visualise_outputs` -- which brings the count of such pixels to the host
    with its pictures -- raises GenesisHipError for it.  palette: see load_palette."""
    pal = load_palette(palette)
    masks = _label_maps(masks, 'colour_seg_masks')
    atlas = _Atlas(masks.device, pal)
    t, stride = _images(masks, 'colour_seg_masks', torch.int64)
    B, _, H, W = t.shape
    atlas.keep.append(t)
    for b in range(B):      # B bare images back to back are [B, 3, H, W]
        atlas.add(atlas.picture(1, H, W, 1, 0, FP32_CHW), LABEL_COLOUR, 1, H, W, t.data_ptr() + 8 * b * stride, H * W, C=1,
                  own_pad=False)      # (a bare image has no padding to write)
    return atlas.run()[:atlas.words].view(B, 3, H, W).to(torch.int64)


# ---- visualise_outputs ---------------------------------------------------------------------------------------------------------
def _log_pictures(atlas, writer, calls, iter_idx, palette_size):
    """Fetches the atlas and makes the recorded writer calls, in order.  A writer that packs pictures on the device
    (genesis_amd.tbwriter: add_images_device) gets the atlas's device views in one call instead, and only the overflow count
    comes to the host here."""
    if not calls:
        return
    on_device = hasattr(writer, 'add_images_device')
    overflow = atlas.fetch_overflow() if on_device else atlas.fetch()
    if overflow:
        raise GenesisHipError('visualise_outputs: %d pixels carry a label or mask index outside the palette of %d colours; '
                              'pass a larger palette' % (overflow, palette_size))
    if on_device:
        writer.add_images_device([(tag, atlas.view(pic).to(torch.int64) if colour else atlas.view(pic), 'CHW')
                                  for tag, pic, colour in calls], iter_idx)
        return
    for tag, pic, colour in calls:
        array = atlas.host_view(pic)
        writer.add_image(tag, array.to(torch.int64) if colour else array, iter_idx)


def visualise_outputs(model, vis_batch, writer, mode, iter_idx, palette='15'):
    """train.py:423-476 with its statement order, tags and arrays: model.eval(); the forward pass of vis_batch['input'][:8] on the
    model's device; add_image of '<mode>_input', '<mode>_recon', '<mode>_instances_gt' (with 'instances' in the batch),
    '<mode>_instances', '<mode>_instances_r', '<mode>_<key>/k<step>' for mx_r_k, x_r_k, log_m_k, log_m_r_k (absent keys
    skipped); then model.sample(batch_size=8, K_steps=model.K_steps) and 'samples', 'gen_<key>/k<step>' for x_k, log_m_k, mx_k --
    or the reference's line when sample raises NotImplementedError.  Every array is a host tensor of the reference's shape and
    dtype (fp32 pictures, int64 colour grids).  All grids of the forward pass come from one launch and one device-to-host copy,
    those of the sample from a second pair; the mask lists are read in place, stats['mx_r_k'] is copied as the model gives it.
    Differences: a label or mask index outside the palette raises GenesisHipError BEFORE any writer call of that forward pass
    (the reference: an IndexError in the middle of them); the model is put back into train mode in a `finally` (the reference
    leaves it in eval mode when the forward pass raises)."""
    pal = load_palette(palette)
    model.eval()
    try:
        _visualise_outputs(model, vis_batch, writer, mode, iter_idx, pal)
    finally:
        model.train()


_SLOT_KEYS = ('mx_r_k', 'x_r_k', 'log_m_k', 'log_m_r_k')      # per-slot pictures of the forward pass, in logging order
_SAMPLE_KEYS = ('x_k', 'log_m_k', 'mx_k')                    # ... and of sample()


def _slot_grids(atlas, calls, stats, keys, prefix):
    """One grid per slot of every list in `stats` named by `keys`: the log-masks through EXP, everything else copied."""
    for key in keys:
        if key in stats:
            for k, plane in enumerate(stats[key]):
                tag = '%s_%s/k%d' % (prefix, key, k)
                calls.append((tag, atlas.grid(EXP if 'log' in key else COPY, plane, tag), False))


def _visualise_outputs(model, vis_batch, writer, mode, iter_idx, pal):
    images = vis_batch['input'][:8]
    on_device = next(model.parameters()).is_cuda
    recon, _, stats, _, _ = model(images.cuda() if on_device else images)
    dev = recon.device
    atlas, calls = _Atlas(dev, pal), []      # calls: (tag, picture, colour grid?) in the reference's logging order
    calls.append((mode + '_input', atlas.grid(COPY, images.to(dev), mode + '_input'), False))
    calls.append((mode + '_recon', atlas.grid(COPY, recon, mode + '_recon'), False))
    if 'instances' in vis_batch:              # ground-truth labels, then each mask field's argmax, through the palette
        tag = mode + '_instances_gt'
        calls.append((tag, atlas.grid(LABEL_COLOUR, _label_maps(vis_batch['instances'][:8].to(dev), tag), tag), True))
    for field, tag in (('log_m_k', mode + '_instances'), ('log_m_r_k', mode + '_instances_r')):
        if field in stats:
            calls.append((tag, atlas.argmax_grid(stats[field], tag), True))
    _slot_grids(atlas, calls, stats, _SLOT_KEYS, mode)
    _log_pictures(atlas, writer, calls, iter_idx, len(pal))

    # the sample: a model without one says so by NotImplementedError (caught around the writer calls too, as in the reference)
    try:
        sample, stats = model.sample(batch_size=8, K_steps=model.K_steps)
        atlas, calls = _Atlas(sample.device, pal), []
        calls.append(('samples', atlas.grid(COPY, sample, 'samples'), False))
        _slot_grids(atlas, calls, stats, _SAMPLE_KEYS, 'gen')
        _log_pictures(atlas, writer, calls, iter_idx, len(pal))
    except NotImplementedError:
        fprint("Sampling not implemented for this model.")


# ---- sheets --------------------------------------------------------------------------------------------------------------------
def _slot_group(planes, b, what, C):
    """Image b of K per-slot tensors [B, C, H, W] as (first address, K, stride) groups: one when the slots are evenly spaced
    views of one buffer, else one per slot."""
    planes = [_images(m, what)[0] for m in planes]
    for m in planes:
        if m.shape != planes[0].shape or m.shape[1] != C:
            raise GenesisHipError('%s: expected K tensors [B, %d, H, W] of one shape, got %s' % (what, C, tuple(m.shape)))
    packed = _packed(planes)
    off = 4 * b * (planes[0].stride(0) if planes[0].shape[0] > 1 else 0)
    if packed is not None and (len(planes) == 1 or packed[0] > 0):
        return planes, [(planes[0].data_ptr() + off, len(planes), packed[0])]
    return planes, [(m.data_ptr() + off, 1, 0) for m in planes]


def _sheet(device, first_col, slot_rows, B, K, H, W, padding, pad_value):
    """first_col: per row a [B, 3, H, W] tensor or None; slot_rows: per row (kind, K tensors, K mask tensors or None).  Image b
    takes the rows b R .. b R + R - 1 of a grid of K + 1 columns.  -> uint8 [Hg, Wg, 3] on the host: one launch, one copy."""
    R = len(slot_rows)
    atlas = _Atlas(device)
    n_geom = B * R * (K + 1)
    pic = atlas.picture(n_geom, H, W, K + 1, padding, U8_HWC)
    common = dict(nrow=K + 1, padding=padding, pad_value=pad_value, n_geom=n_geom)
    own = True      # the first descriptor writes the padding
    for b in range(B):
        for r in range(R):
            cell = (b * R + r) * (K + 1)
            if first_col[r] is None:
                atlas.add(pic, FILL, 1, H, W, cell0=cell, own_pad=own, **common)
            else:
                t, stride = _images(first_col[r], 'sheet')
                atlas.keep.append(t)
                src = t.data_ptr() + 4 * b * stride
                atlas.add(pic, COPY, 1, H, W, src, H * W * t.shape[1], C=t.shape[1], cell0=cell, own_pad=own, aligned=(src,), **common)
            own = False
            kind, xs, ms = slot_rows[r]
            xs, groups = _slot_group(xs, b, 'sheet', 3 if kind != EXP else 1)
            atlas.keep.extend(xs)
            if kind == EXP_MUL:
                ms, mgroups = _slot_group(ms, b, 'sheet', 1)
                atlas.keep.extend(ms)
                if len(groups) != len(mgroups):      # one of the two lists is not packed: a descriptor per slot
                    groups = [(xs[k].data_ptr() + 4 * b * (xs[k].stride(0) if B > 1 else 0), 1, 0) for k in range(K)]
                    mgroups = [(ms[k].data_ptr() + 4 * b * (ms[k].stride(0) if B > 1 else 0), 1, 0) for k in range(K)]
            done = 0
            for gi, (src, n, stride) in enumerate(groups):
                src1, stride1 = (mgroups[gi][0], mgroups[gi][2]) if kind == EXP_MUL else (0, 0)
                atlas.add(pic, kind, n, H, W, src, stride, src1, stride1, C=3 if kind != EXP else 1, cell0=cell + 1 + done,
                          own_pad=False, aligned=(src, src1, 4 * stride, 4 * stride1), **common)
                done += n
    atlas.fetch()
    return atlas.host_view(pic).numpy()


def _check_slots(K, *lists):
    if K < 1 or any(len(l) != K for l in lists if l is not None):
        raise GenesisHipError('sheet: the per-slot lists differ in length')


def reconstruction_sheet(model, x, mask_field=None, padding=2, pad_value=1.0):
    """The picture of scripts/visualise_reconstruction.py:86-121 for the images x [B, 3, H, W] (the script's B is 1): per image
    column 0 = the input over the reconstruction, columns 1 .. K = the slots, rows = mask x RGB, RGB, mask and, when the model
    reports log_s_k, scope; empty cells and the 2-pixel borders hold pad_value.  The masks are stats['log_m_r_k'] for GENESIS-V2
    and stats['log_m_k'] otherwise.  The script decides by the model config's file name; with only the model in hand this goes
    by the module that defines the model's class ('genesisv2' in its name), so a model inside a wrapper (nn.DataParallel, a
    recording proxy) counts as "otherwise": pass mask_field for it.  -> uint8
    [rows, columns, 3] on the host = rint(clamp(v, 0, 1) 255).  One forward pass in the model's current mode, one launch, one copy."""
    x = x.to(next(model.parameters()).device)
    output, _, stats, _, _ = model(x)
    if mask_field is None:
        mask_field = 'log_m_r_k' if 'genesisv2' in type(model).__module__ else 'log_m_k'
    x_k, log_masks = stats['x_r_k'], stats[mask_field]
    log_s_k = stats['log_s_k'] if 'log_s_k' in stats else None
    K = len(x_k)
    _check_slots(K, log_masks, log_s_k or None)
    B, _, H, W = output.shape
    first_col = [x.to(output.device), output, None] + ([None] if log_s_k else [])
    slot_rows = [(EXP_MUL, x_k, log_masks), (COPY, x_k, None), (EXP, log_masks, None)] + ([(EXP, log_s_k, None)] if log_s_k else [])
    return _sheet(output.device, first_col, slot_rows, B, K, H, W, padding, pad_value)


def generation_sheet(model, batch_size, K_steps, padding=2, pad_value=1.0):
    """The picture of scripts/visualise_generation.py:84-111 for model.sample(batch_size, K_steps): per sample column 0 = the
    generated scene, columns 1 .. K = the slots, rows = mask x RGB (stats['mx_k'] as the model gives it), RGB, mask and, with
    log_s_k, scope.  -> uint8 [rows, columns, 3] on the host.  One launch, one copy."""
    y, stats = model.sample(batch_size, K_steps)
    x_k, log_masks, mx_k = stats['x_k'], stats['log_m_k'], stats['mx_k']
    log_s_k = stats['log_s_k'] if 'log_s_k' in stats else None
    K = len(x_k)
    _check_slots(K, log_masks, mx_k, log_s_k or None)
    B, _, H, W = y.shape
    first_col = [y, None, None] + ([None] if log_s_k else [])
    slot_rows = [(COPY, mx_k, None), (COPY, x_k, None), (EXP, log_masks, None)] + ([(EXP, log_s_k, None)] if log_s_k else [])
    return _sheet(y.device, first_col, slot_rows, B, K, H, W, padding, pad_value)


# ---- PNG ---------------------------------------------------------------------------------------------------------------------
def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def save_png(path, array):
    """uint8 [H, W, 3] (RGB) or [H, W] (grey) -> an 8-bit PNG, every row with filter type 0, deflated with zlib."""
    a = array.cpu().numpy() if torch.is_tensor(array) else np.asarray(array)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.size == 0:
        raise GenesisHipError('save_png: expected a non-empty uint8 [H, W, 3] or [H, W] array, got %s of shape %s' % (a.dtype, a.shape))
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + W * (3 if a.ndim == 3 else 1)), np.uint8)      # the filter byte 0, then the row
    rows[:, 1:] = a.reshape(H, -1)
    data = (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0))
            + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _chunk(b'IEND', b''))
    with open(path, 'wb') as f:
        f.write(data)
