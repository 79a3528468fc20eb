"""Segmentation metrics of the reference's validation loop on the device: `average_ari` and `average_segcover` with the
signatures and return values of utils/misc.py:101-114 and :173-235 (callers: train.py:542-546,
scripts/compute_seg_metrics.py:113-117, utils/misc.py:135-136).

Both are functions of the per-image contingency table of the two label maps, which one HIP launch produces
(gx_label_contingency, integer atomics in LDS: bit-exact); the remaining arithmetic runs on [B, K, K]-sized device
tensors.  The reference moves every image to the host and loops in Python (numpy argmax + sklearn per image; a
boolean-mask pass over the batch per label pair).

`SegMetrics` does a whole batch of the validation loop in one launch (gx_seg_metrics: argmax over the mask planes read in place,
the table, every score, the batch means) and keeps the running means on the device until `compute()`."""
import ctypes

import torch

from . import _lib
from ._lib import GenesisHipError


def contingency(segA, segB, KA, KB):
    """int32 [B, KA, KB+1]: counts[b,i,j] = #{p: segA[b,p] == i, segB[b,p] == j}; column KB = segB outside [0,KB);
    pixels with segA outside [0,KA) are skipped."""
    if not (segA.is_cuda and segB.is_cuda):
        raise GenesisHipError('metrics: label maps must live on the HIP device; there is no CPU path')
    a = segA.reshape(segA.shape[0], -1).to(torch.int64).contiguous()
    b = segB.reshape(segB.shape[0], -1).to(torch.int64).contiguous()
    if a.shape != b.shape:
        raise GenesisHipError('metrics: label maps differ in shape: %s vs %s' % (tuple(segA.shape), tuple(segB.shape)))
    B, HW = a.shape
    counts = torch.empty(B, KA, KB + 1, dtype=torch.int32, device=a.device)
    _lib.call('gx_label_contingency', ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), B, HW, KA, KB,
              ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return counts


def _num_labels(t):
    return int(t.max().item()) + 1 if t.numel() else 1


def adjusted_rand_from_contingency(c):
    """sklearn.metrics.adjusted_rand_score restated on contingency tables c [B, R, C] (int64):
    pair confusion (tn, fp, fn, tp) from sum n_ij^2 and the squared marginals; 1.0 when fn == fp == 0."""
    c = c.to(torch.int64)
    n = c.sum((1, 2))
    sum_sq = (c * c).sum((1, 2))
    tp = sum_sq - n
    fp = (c.sum(1) ** 2).sum(1) - sum_sq          # column marginals (labels_pred in sklearn's convention)
    fn = (c.sum(2) ** 2).sum(1) - sum_sq
    tn = n * n - fp - fn - sum_sq
    tp, fp, fn, tn = [t.to(torch.float64) for t in (tp, fp, fn, tn)]
    den = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn)
    ari = 2.0 * (tp * tn - fn * fp) / den
    return torch.where((fn == 0) & (fp == 0), torch.ones_like(ari), ari)


def average_ari(log_m_k, instances, foreground_only=False):
    """utils/misc.py:101-114.  log_m_k: K x [B,1,H,W] log-masks; instances: [B,1,H,W] (or [B,H,W]) integer ground truth.
    Returns (mean ARI as a Python float, list of per-image ARI floats)."""
    masks = torch.cat(list(log_m_k), 1)                           # argmax(exp(.)) == argmax(.)
    pred = torch.argmax(masks, dim=1)
    gt = instances.to(masks.device).reshape(pred.shape[0], -1).to(torch.int64)
    K, G = masks.shape[1], _num_labels(gt)
    # rows = ground truth (row 0 = background), columns = prediction
    c = contingency(gt, pred, G, K)[:, :, :K].to(torch.int64)
    if foreground_only:
        c = c[:, 1:, :]
    ari = adjusted_rand_from_contingency(c.transpose(1, 2))       # sklearn: (labels_true=pred, labels_pred=gt)
    lst = [float(v) for v in ari.cpu()]
    return sum(lst) / len(lst), lst


def average_segcover(segA, segB, ignore_background=False):
    """utils/misc.py:173-235: covering of segA by segB, both [B,1,H,W] integer maps; negative labels in segA are
    ignore regions.  Returns (mean_sc.mean(0), scaled_sc.mean(0)) as 0-dim float32 tensors (on the device).

    One tensor expression over the contingency table c[b,i,j] (no loop over label pairs, no host round trip):
        |A_i| = sum_j c[b,i,:]  (column KB holds segB labels < 0),   |B_j, not ignored| = sum_i c[b,i,j],
        IoU[b,i,j] = c / (|A_i| + |B_j| - c)  (0 where the union is empty -- the reference's -100 never wins its running
        maximum, which starts at 0),   best[b,i] = max_j IoU,
        mean covering = sum_i best / #{i: |A_i| > 0},   scaled covering = sum_i |A_i| best / sum_i |A_i|.
    A label that no image of the batch holds contributes 0 to every sum, so "the labels torch.unique returns" needs no
    separate bookkeeping; `ignore_background` drops row 0 from the covered labels (its pixels still count in |B_j|)."""
    assert segA.shape == segB.shape, '%s - %s' % (tuple(segA.shape), tuple(segB.shape))
    assert segA.shape[1] == 1 and segB.shape[1] == 1
    dev = segB.device if segB.is_cuda else segA.device
    segA, segB = segA.to(dev), segB.to(dev)
    labels = torch.stack((segA.max(), segB.max())).clamp_min(0).tolist()      # the table's size: the one host read
    KA, KB = int(labels[0]) + 1, int(labels[1]) + 1
    c = contingency(segA, segB, KA, KB).to(torch.int64)                       # [B, KA, KB+1]
    b_area = c[:, :, :KB].sum(1, keepdim=True)                                # [B, 1, KB]  (background pixels of A count)
    if ignore_background:
        c = c[:, 1:]                                                          # (only A's label 0 is not covered)
    area = c.sum(2)                                                           # [B, KA']
    inter = c[:, :, :KB]
    union = area.unsqueeze(2) + b_area - inter
    iou = torch.where(union == 0, torch.zeros((), device=dev), inter.float() / union.float())
    best = iou.max(2).values if iou.shape[1] else iou.new_zeros(iou.shape[:2])
    mean_sc = best.sum(1) / (area > 0).sum(1).clamp(min=1).float()
    scaled_sc = (area.float() * best).sum(1) / area.sum(1).clamp(min=1).float()
    return mean_sc.mean(0), scaled_sc.mean(0)


_ROW = ('ari', 'ari_fg', 'msc', 'msc_fg', 'ssc', 'ssc_fg')      # columns 0..5 of a gx_seg_metrics row; 6: counted pixels, 7: labels present


def _packed(planes):
    """(plane stride, image stride) in floats if the planes are evenly spaced views of one buffer (log_m.unbind(0) of a
    [K,B,1,H,W] tensor), else None.  The planes are [B,1,H,W] with contiguous images and one common image stride."""
    first = planes[0]
    store, off0 = first.untyped_storage().data_ptr(), first.storage_offset()
    step = planes[1].storage_offset() - off0 if len(planes) > 1 else 0
    if step < 0:
        return None
    for k, m in enumerate(planes):
        if m.untyped_storage().data_ptr() != store or m.storage_offset() != off0 + k * step:
            return None
    return step, first.stride(0)


class SegMetrics:
    """Every segmentation score of the validation loop (train.py:534-559), accumulated on the device: one gx_seg_metrics
    launch per `update`, no host read before `compute`.

    update(log_m_k, instances): K x [B,1,H,W] fp32 log-masks (read in place: evenly strided views of one buffer, as
    stats['log_m_k'] of this project's models, or K separate tensors) and [B,1,H,W] / [B,H,W] integer ground truth.  Labels < 0
    are ignore regions; a label >= max_labels is counted as overflow and makes compute() raise.
    compute(): the one host read.  dict of 'ari', 'ari_fg' (ARI, foreground-only ARI), 'msc', 'msc_fg' (mean segmentation covering,
    without background), 'ssc', 'ssc_fg' (scaled covering) as Python floats -- each the mean over batches of batch means, which is
    what train.py:567 forms as sum(val) / len(val) --, 'num_batches', and with keep_per_image > 0 'per_image': the same six keys as
    float64 arrays over the first keep_per_image images seen, in order.
    reset(): clears the accumulators."""

    def __init__(self, max_labels=32, keep_per_image=0, device='cuda'):
        self.max_labels, self.keep = int(max_labels), int(keep_per_image)
        if self.max_labels < 1 or self.keep < 0:
            raise GenesisHipError('SegMetrics: max_labels must be positive and keep_per_image non-negative')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise GenesisHipError('SegMetrics: the metrics run on the HIP device; there is no CPU path')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._acc = torch.zeros(8, dtype=torch.float64, device=self.device)
        self._state = torch.zeros(4, dtype=torch.int64, device=self.device)      # arrival counter, batches, overflow, log cursor
        self._log = torch.zeros(self.keep, 8, dtype=torch.float64, device=self.device) if self.keep else None
        self._rows = None

    def reset(self):
        self._acc.zero_()
        self._state.zero_()

    def update(self, log_m_k, instances):
        planes = [m if m.is_cuda else m.to(self.device) for m in log_m_k]
        K = len(planes)
        if K < 1:
            raise GenesisHipError('SegMetrics.update: no mask planes')
        shape = planes[0].shape
        if len(shape) != 4 or shape[1] != 1:
            raise GenesisHipError('SegMetrics.update: mask planes must be [B,1,H,W], got %s' % (tuple(shape),))
        B, _, H, W = shape
        HW = H * W
        for m in planes:
            if m.shape != shape or m.dtype != torch.float32 or m.device != planes[0].device:
                raise GenesisHipError('SegMetrics.update: mask planes differ in shape, dtype or device, or are not fp32')
        if planes[0].device != self.device:
            raise GenesisHipError('SegMetrics.update: mask planes on %s, accumulators on %s' % (planes[0].device, self.device))
        # every image contiguous, one image stride >= HW for all planes (any such [B,1,H,W] view of a larger buffer qualifies;
        # anything else, an expanded plane for instance, is copied)
        stride = (planes[0].stride(0) if B > 1 else HW, W, 1)
        if stride[0] < HW or any((m.stride(0) if B > 1 else HW, m.stride(2), m.stride(3)) != stride for m in planes):
            planes, stride = [m.contiguous() for m in planes], (HW, W, 1)
        inst = instances.to(planes[0].device).reshape(instances.shape[0], -1).to(torch.int64).contiguous()
        if inst.shape != (B, HW):
            raise GenesisHipError('SegMetrics.update: instances %s do not match mask planes %s'
                                  % (tuple(instances.shape), tuple(shape)))
        if self._rows is None or self._rows.shape[0] < B:
            self._rows = torch.empty(B, 8, dtype=torch.float64, device=self.device)
        packed = _packed(planes)
        if packed is not None:
            base, pstride, table = ctypes.c_void_p(planes[0].data_ptr()), packed[0], None
        else:
            base, pstride, table = None, 0, (ctypes.c_void_p * K)(*[m.data_ptr() for m in planes])
        _lib.call('gx_seg_metrics', base, pstride, stride[0], table, ctypes.c_void_p(inst.data_ptr()), B, HW, K,
                  self.max_labels, ctypes.c_void_p(self._rows.data_ptr()), ctypes.c_void_p(self._acc.data_ptr()),
                  ctypes.c_void_p(self._state.data_ptr()), ctypes.c_void_p(self._log.data_ptr()) if self.keep else None,
                  self.keep, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def _parts(self):
        """What compute() needs on the host: 8 accumulators, 4 counters (exact in float64), the per-image log."""
        return [self._acc, self._state] + ([self._log] if self.keep else [])

    def compute(self):
        return self._finish(torch.cat([t.reshape(-1).to(torch.float64) for t in self._parts()]).cpu().numpy())

    def _finish(self, host):
        """compute() on values already brought to the host (genesis_amd.evaluate fetches several objects in one transfer)."""
        import numpy as np
        acc, (_, batches, overflow, cursor) = host[:8], (int(v) for v in host[8:12])
        if overflow:
            raise GenesisHipError('SegMetrics: %d pixels carry a ground-truth label >= max_labels = %d; '
                                  'construct SegMetrics with a larger max_labels' % (overflow, self.max_labels))
        if batches == 0:
            raise GenesisHipError('SegMetrics.compute: no batch was seen')
        out = {}
        for c, key in enumerate(_ROW):
            # covering: the reference divides a 0-dim float32 tensor by the count
            out[key] = float(np.float32(acc[c]) / np.float32(batches)) if 'sc' in key else float(acc[c]) / batches
        out['num_batches'] = batches
        if self.keep:
            log = host[12:].reshape(self.keep, 8)[:cursor]
            out['per_image'] = {key: log[:, c].copy() for c, key in enumerate(_ROW)}
        return out
