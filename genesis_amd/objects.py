"""Per-object tables of a segmentation without ground truth: which slots are present, how large they are, where they lie and how
confident the model is -- what every consumer of a label map computes next, in one launch per batch (gx_object_table,
include/genesis_hip.h) from the K log-mask planes read in place, as `SegMetrics.update` reads them.

    table = object_table(stats.log_m_k, image=x)      # an ObjectTable, everything on the device
    table.labels                                      # uint8 [B, H, W]: argmax over the slots (torch.argmax's rule)
    table.area, table.bbox, table.centroid, table.mean_colour, table.confidence, table.present(min_pixels)
    host = table.cpu()                                # ONE transfer for everything

`geom` (int64 [B, K, 8]: area, x_min, y_min, x_max, y_max, sum_x, sum_y, border bits) is bit-exact; `soft` (fp64 [B, K, 6]: mass,
inside, four colour sums) is summed in a fixed order, so an image's rows are the same bits in whatever batch it arrives.  The
derived quantities are plain torch on these tiny tables and read nothing back to the host."""
import ctypes

import torch

from . import _lib
from ._lib import GenesisHipError
from .metrics import _packed

MAX_SLOTS = 32
MAX_SIDE = 4096
GEOM = ('area', 'x_min', 'y_min', 'x_max', 'y_max', 'sum_x', 'sum_y', 'border')      # the words of a geom row
SOFT = ('mass', 'inside', 'c0', 'c1', 'c2', 'c3')                                    # the words of a soft row
BORDER_LEFT, BORDER_TOP, BORDER_RIGHT, BORDER_BOTTOM = 1, 2, 4, 8


class ObjectTable(object):
    """labels uint8 [B, H, W], geom int64 [B, K, 8], soft fp64 [B, K, 6] (the layouts of gx_object_table), on one device;
    channels: how many colour sums of `soft` are meaningful (0: the table was made without an image)."""

    def __init__(self, labels, geom, soft, channels=0):
        if labels.dim() != 3 or labels.dtype != torch.uint8:
            raise GenesisHipError('ObjectTable: labels must be uint8 [B, H, W], got %s %s' % (labels.dtype, tuple(labels.shape)))
        B = labels.shape[0]
        if geom.dim() != 3 or geom.shape[0] != B or geom.shape[2] != len(GEOM) or geom.dtype != torch.int64:
            raise GenesisHipError('ObjectTable: geom must be int64 [B, K, 8], got %s %s' % (geom.dtype, tuple(geom.shape)))
        if tuple(soft.shape) != (B, geom.shape[1], len(SOFT)) or soft.dtype != torch.float64:
            raise GenesisHipError('ObjectTable: soft must be fp64 [B, K, 6], got %s %s' % (soft.dtype, tuple(soft.shape)))
        if not 0 <= int(channels) <= 4:
            raise GenesisHipError('ObjectTable: channels must be in [0, 4], not %r' % (channels,))
        self.labels, self.geom, self.soft, self.channels = labels, geom, soft, int(channels)

    @property
    def num_slots(self):
        return self.geom.shape[1]

    @property
    def area(self):
        """int64 [B, K]: pixels labelled k."""
        return self.geom[:, :, 0]

    @property
    def bbox(self):
        """int64 [B, K, 4]: (x0, y0, x1, y1), inclusive; (W, H, -1, -1) for an empty slot."""
        return self.geom[:, :, 1:5]

    @property
    def border(self):
        """int64 [B, K]: BORDER_LEFT | BORDER_TOP | BORDER_RIGHT | BORDER_BOTTOM of the image edges the slot touches."""
        return self.geom[:, :, 7]

    @property
    def centroid(self):
        """fp64 [B, K, 2]: (mean column, mean row) of the slot's pixels; NaN for an empty slot."""
        return self.geom[:, :, 5:7].to(torch.float64) / self.area.to(torch.float64).unsqueeze(2)

    @property
    def mass(self):
        """fp64 [B, K]: the slot's mask summed over the whole image."""
        return self.soft[:, :, 0]

    @property
    def confidence(self):
        """fp64 [B, K]: the mean mask value over the slot's own pixels (inside / area); NaN for an empty slot."""
        return self.soft[:, :, 1] / self.area.to(torch.float64)

    @property
    def mean_colour(self):
        """fp64 [B, K, C]: the image's mean over the slot's pixels; NaN for an empty slot, C = 0 without an image."""
        return self.soft[:, :, 2:2 + self.channels] / self.area.to(torch.float64).unsqueeze(2)

    def present(self, min_pixels=1):
        """bool [B, K]: slots with at least min_pixels pixels."""
        return self.area >= int(min_pixels)

    def cpu(self):
        """The table on the host, in ONE transfer."""
        if not self.labels.is_cuda:
            return self
        n_g, n_s = self.geom.numel() * 8, self.soft.numel() * 8
        flat = torch.cat([self.geom.contiguous().view(torch.uint8).reshape(-1), self.soft.contiguous().view(torch.uint8).reshape(-1),
                          self.labels.reshape(-1)]).cpu()
        return ObjectTable(flat[n_g + n_s:].reshape(self.labels.shape), flat[:n_g].view(torch.int64).reshape(self.geom.shape),
                           flat[n_g:n_g + n_s].view(torch.float64).reshape(self.soft.shape), self.channels)


def _check_planes(log_m_k):
    planes = list(log_m_k.unbind(0)) if isinstance(log_m_k, torch.Tensor) else list(log_m_k)
    K = len(planes)
    if not 1 <= K <= MAX_SLOTS:
        raise GenesisHipError('object_table: log_m_k holds %d mask planes; 1 to %d are supported' % (K, MAX_SLOTS))
    if not all(isinstance(m, torch.Tensor) for m in planes):
        raise GenesisHipError('object_table: log_m_k must be a sequence of tensors')
    shape = planes[0].shape
    if len(shape) != 4 or shape[1] != 1 or shape[0] < 1:
        raise GenesisHipError('object_table: log_m_k planes must be [B,1,H,W], got %s' % (tuple(shape),))
    for m in planes:
        if m.shape != shape or m.dtype != torch.float32 or m.device != planes[0].device:
            raise GenesisHipError('object_table: log_m_k planes differ in shape, dtype or device, or are not fp32')
    if not (1 <= shape[2] <= MAX_SIDE and 1 <= shape[3] <= MAX_SIDE):
        raise GenesisHipError('object_table: log_m_k planes of %d x %d; H and W must be in [1, %d]' % (shape[2], shape[3], MAX_SIDE))
    return planes


def _check_image(image, planes):
    B, _, H, W = planes[0].shape
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.dtype != torch.float32:
        raise GenesisHipError('object_table: image must be an fp32 [B,C,H,W] tensor')
    if not 1 <= image.shape[1] <= 4:
        raise GenesisHipError('object_table: image has %d channels; 1 to 4 are supported' % image.shape[1])
    if (image.shape[0], image.shape[2], image.shape[3]) != (B, H, W):
        raise GenesisHipError('object_table: image %s does not match the log_m_k planes %s'
                              % (tuple(image.shape), tuple(planes[0].shape)))
    if image.device != planes[0].device:
        raise GenesisHipError('object_table: image on %s, log_m_k on %s' % (image.device, planes[0].device))


def object_table(log_m_k, image=None):
    """log_m_k: K x [B,1,H,W] fp32 log-masks on the device (a list, or one [K,B,1,H,W] tensor), 1 <= K <= 32 -- evenly strided views
    of one buffer, as stats['log_m_k'] of this project's models, are read in place; K separate tensors through a pointer table; a
    plane whose images are not contiguous is copied.  image: optional fp32 [B,C,H,W], 1 <= C <= 4, for the slots' mean colours.
    -> ObjectTable, on the device; nothing is read back."""
    planes = _check_planes(log_m_k)
    if image is not None:
        _check_image(image, planes)
    if not planes[0].is_cuda:
        raise GenesisHipError('object_table: log_m_k must live on the HIP device; there is no CPU path')
    dev = planes[0].device
    K = len(planes)
    B, _, H, W = planes[0].shape
    HW = H * W
    # every image contiguous, one image stride >= HW for all planes (SegMetrics.update's rule); anything else is copied
    stride = (planes[0].stride(0) if B > 1 else HW, W, 1)
    if stride[0] < HW or any((m.stride(0) if B > 1 else HW, m.stride(2), m.stride(3)) != stride for m in planes):
        planes, stride = [m.contiguous() for m in planes], (HW, W, 1)
    C, x_ptr, x_stride = 0, None, 0
    if image is not None:
        C = image.shape[1]
        if (image.stride(1), image.stride(2), image.stride(3)) != (HW, W, 1) or (B > 1 and image.stride(0) < C * HW):
            image = image.contiguous()
        x_ptr, x_stride = ctypes.c_void_p(image.data_ptr()), image.stride(0) if B > 1 else C * HW
    labels = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    geom = torch.empty(B, K, len(GEOM), dtype=torch.int64, device=dev)
    soft = torch.empty(B, K, len(SOFT), dtype=torch.float64, device=dev)
    packed = _packed(planes)
    if packed is not None:
        base, pstride, table = ctypes.c_void_p(planes[0].data_ptr()), packed[0], None
    else:
        base, pstride, table = None, 0, (ctypes.c_void_p * K)(*[m.data_ptr() for m in planes])
    with torch.cuda.device(dev):
        _lib.call('gx_object_table', base, pstride, stride[0], table, x_ptr, x_stride, C, B, H, W, K,
                  ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(geom.data_ptr()), ctypes.c_void_p(soft.data_ptr()),
                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return ObjectTable(labels, geom, soft, C)
