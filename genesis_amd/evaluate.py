"""The reference's validation code with its arguments and return values, host-bound no longer: `evaluation` (train.py:479-589),
`dataset_ari` (utils/misc.py:117-159) and `seg_metrics_from_model` (the body of scripts/compute_seg_metrics.py:101-131).

Every segmentation score of a batch comes from one gx_seg_metrics launch (genesis_amd.metrics.SegMetrics: the K log-mask planes
read in place, no cat / argmax / label-map round trip), the loss statistics are accumulated on the device in the reference's
operation order, and each function brings its results to the host in ONE transfer at the end.  The only other host reads are the
ones inside the loader and the model (dynamic_K's, for instance).

Not in the reference: reconstruction quality for data without labels -- `evaluation(..., image_quality=True)` and
`reconstruction_quality_from_model` (per-image MSE, RMSE, PSNR, SSIM from one gx_image_quality launch per batch:
genesis_amd.image_quality.ImageQuality), in the same single transfer."""
import datetime
import itertools
import time

import numpy as np
import torch

from . import compat
from .image_quality import KEYS as _QUALITY_KEYS, ImageQuality
from .metrics import SegMetrics

compat.install()
from forge.experiment_tools import fprint  # noqa: E402

MASK_FIELDS = (('log_m_k', ''), ('log_m_r_k', '_r'))      # (key in stats, suffix of its scores in the returned dicts)
_KL_TERMS = (('kl_m_k', 'kl_m'), ('kl_l_k', 'kl_l'))       # per ELBO term: the per-step list, else the [B] tensor, else nothing


def _fetch(tensors):
    """The values of all `tensors` (any float / integer dtype, flattened, in order) as one float64 numpy array: one transfer.
    float32 and the counters (< 2^53) are exact in float64."""
    if not tensors:
        return np.zeros(0)
    dev = next((t.device for t in tensors if t.is_cuda), tensors[0].device)
    return torch.cat([t.detach().to(dev).reshape(-1).to(torch.float64) for t in tensors]).cpu().numpy()


def _on_device(model):
    return next(model.parameters()).is_cuda


def _has(stats, key):
    return hasattr(stats, key) or (isinstance(stats, dict) and key in stats)


def _batch_mean(value):
    """A loss term of one batch as a 0-dim tensor: [B] -> mean; K x [B] -> summed over the steps, then the mean."""
    if isinstance(value, (list, tuple)):
        value = torch.stack(list(value), 1).sum(1)
    return value.mean(0)


def _batch_budget(data_loader, iter_idx, debug, N_eval):
    """(batches to evaluate, the line announcing it, flush it?): five at iteration 0 and in debug runs, N_eval images' worth
    when the loader holds that many, else the whole loader."""
    size = data_loader.batch_size
    if debug or iter_idx == 0:
        return 5, "ITER 0 / DEBUG - eval on 5 batches", True
    if N_eval is not None and N_eval <= size * len(data_loader):
        n = int(N_eval // size)
        return n, f"N_eval = {N_eval}, eval on {n} batches", True
    return len(data_loader), f"Eval on all {len(data_loader)} batches", False


class _MaskScores:
    """One SegMetrics per mask field the model reports, made at the field's first batch; all of them fetched in one transfer."""

    def __init__(self, max_labels):
        self.max_labels, self.metrics, self.updates = max_labels, {}, {}

    def update(self, stats, instances):
        """-> the fields seen for the first time in this call."""
        new = []
        for field, _ in MASK_FIELDS:
            if field not in stats:
                continue
            planes = stats[field]
            if field not in self.metrics:
                dev = planes[0].device if planes[0].is_cuda else 'cuda'      # host planes are moved by update()
                self.metrics[field], self.updates[field] = SegMetrics(max_labels=self.max_labels, device=dev), 0
                new.append(field)
            self.metrics[field].update(planes, instances)
            self.updates[field] += 1
        return new

    def parts(self):
        return [t for m in self.metrics.values() for t in m._parts()]

    def finish(self, host):
        """host: the fetched parts() -> {field: SegMetrics.compute() dict}."""
        return {field: m._finish(host[12 * i:12 * (i + 1)]) for i, (field, m) in enumerate(self.metrics.items())}


def evaluation(model, data_loader, writer, config, iter_idx, N_eval=None, N_seg_metrics=50, max_labels=32, image_quality=False,
               data_range=1.0):
    """train.py:479-589: the statistics of a validation run as a dict of Python floats, logged as 'val/<key>' when `writer` is
    given.  Kept from the reference: the num_batches rule (5 batches at iter_idx == 0 or under config.debug, N_eval // batch_size
    when N_eval fits the loader, else all); per loss key the mean over batches of the batch means (lists of K terms summed over
    the steps first); 'elbo' = err + kl_m + kl_l with whichever of kl_m_k / kl_m and kl_l_k / kl_l the model reports; the
    segmentation scores 'ari', 'ari_fg', 'msc', 'msc_fg' (and '..._r' for log_m_r_k) on the batches with
    b_idx * batch_size < N_seg_metrics only, and the assertion that they cover N_seg_metrics images and less than a batch more
    (not at iter_idx == 0 or under config.debug); 'err_element' from the input's shape; the order of the keys; one batch more
    than needed is drawn from the loader; host batches are moved with .cuda() in place under config.gpu; the printed lines.
    The model ends in train mode, also when the loop raises; the grad mode is put back to what it was on entry (the reference
    leaves it enabled: the same thing for its caller).  Host mask planes are moved to the device by SegMetrics.
    max_labels: bound on the ground-truth labels (genesis_amd.metrics.SegMetrics).
    image_quality=True (not in the reference): every evaluated batch's reconstruction -- the forward's first output -- and
    batch['input'] go through one genesis_amd.image_quality.ImageQuality.update (data range `data_range`, the default window), and
    the result gains 'mse', 'rmse', 'psnr', 'ssim', each the mean over the images, after 'err_element'; they ride in the same
    transfer.  With the default nothing is launched or returned that was not before."""
    model.eval()
    try:
        with torch.no_grad():
            return _evaluation(model, data_loader, writer, config, iter_idx, N_eval, N_seg_metrics, max_labels,
                               ImageQuality(data_range=data_range) if image_quality else None)
    finally:
        model.train()


def _evaluation(model, data_loader, writer, config, iter_idx, N_eval, N_seg_metrics, max_labels, quality=None):
    batch_size = data_loader.batch_size
    num_batches, line, flush = _batch_budget(data_loader, iter_idx, config.debug, N_eval)
    fprint(line, flush)
    started = time.time()
    # key -> [running device sum, terms]; a segmentation key holds None: its place in the returned dict, as the reference's
    # dict gives it at first use.  The sums start from the integer 0, as sum(list) does.
    totals = {}
    scores = _MaskScores(max_labels)
    shape = None

    def add(key, v):
        entry = totals.setdefault(key, [0, 0])
        entry[0], entry[1] = entry[0] + v, entry[1] + 1

    batches = iter(data_loader)
    for b_idx, batch in enumerate(itertools.islice(batches, num_batches)):
        if config.gpu:
            batch.update({key: val.cuda() for key, val in batch.items()})
        recon, losses, stats, _, _ = model(batch['input'])
        shape = batch['input'].shape
        if quality is not None:
            quality.update(recon, batch['input'])
        means = {key: _batch_mean(val) for key, val in losses.items()}
        for key, v in means.items():
            add(key, v)
        elbo = means['err']
        for name in (next((n for n in pair if n in means), None) for pair in _KL_TERMS):
            if name is not None:       # (the reference adds an integer zero for a missing term: the same value)
                elbo = elbo + means[name]
        add('elbo', elbo)
        if 'instances' in batch and b_idx * batch_size < N_seg_metrics:
            for field in scores.update(stats, batch['instances']):
                suffix = dict(MASK_FIELDS)[field]
                totals.update({key + suffix: None for key in ('ari', 'ari_fg', 'msc', 'msc_fg')})
    if next(batches, None) is not None:
        fprint(f"Breaking from eval loop after {num_batches} batches")

    # the one transfer: loss means, err_element, the SegMetrics accumulators
    loss_keys = [key for key, entry in totals.items() if entry is not None]
    values = [totals[key][0] / totals[key][1] for key in loss_keys]
    values.append(values[loss_keys.index('err')] / int(np.prod(shape[1:4])))
    seg_parts = scores.parts()
    host = _fetch(values + seg_parts + (quality._parts() if quality is not None else []))
    loss_host, seg_host = dict(zip(loss_keys + ['err_element'], host)), scores.finish(host[len(values):])

    checked = iter_idx > 0 and not config.debug
    result = {}
    for key, entry in totals.items():
        if entry is not None:
            result[key] = float(loss_host[key])
            continue
        field, suffix = MASK_FIELDS[1] if key.endswith('_r') else MASK_FIELDS[0]
        if checked:
            assert N_seg_metrics <= scores.updates[field] * batch_size < N_seg_metrics + batch_size
        result[key] = seg_host[field][key[:len(key) - len(suffix)]]
    result['err_element'] = float(loss_host['err_element'])
    if quality is not None:
        quality_host = quality._finish(host[len(values) + sum(t.numel() for t in seg_parts):])
        result.update({key: quality_host[key] for key in _QUALITY_KEYS})
    duration = time.time() - started
    fprint(f'Eval duration: {duration:.1f}s, {num_batches / duration:.1f} b/s')
    result.update(duration=float(duration), num_batches=float(num_batches))
    if writer is not None:
        for key, val in result.items():
            writer.add_scalar(f'val/{key}', val, iter_idx)
    return result


def _mean(values):
    values = list(values)
    return sum(values) / len(values)


def dataset_ari(model, data_loader, num_images=300, max_labels=32):
    """utils/misc.py:117-159: (mean ARI, mean foreground ARI) over the first num_images images of the loader, and the per-image
    lists of the LAST batch -- not of the dataset: that is what the reference returns in third and fourth place.
    Returns (0., 0., [0], [0]), with the model left in eval mode, when a batch has no 'instances' or the model no log_m_k.
    One progress line per call instead of one per batch (a line per batch would need a host read per batch); it counts every
    image scored, the FINAL lines the first num_images.  Only the input is moved to the model's device; SegMetrics moves host
    labels and planes itself."""
    fprint("Computing ARI on dataset")
    model.eval()
    sm, scored, last = None, 0, 0
    with torch.no_grad():
        for batch in data_loader:
            if _on_device(model):
                batch['input'] = batch['input'].cuda()
            stats = model(batch['input'])[2]
            if not ('instances' in batch and _has(stats, 'log_m_k')):
                return 0., 0., [0], [0]
            planes = stats['log_m_k']
            last = planes[0].shape[0]
            if sm is None:      # room for every image of the batch that crosses num_images
                sm = SegMetrics(max_labels=max_labels, keep_per_image=num_images + last,
                                device=planes[0].device if planes[0].is_cuda else 'cuda')
            sm.update(planes, batch['instances'])
            scored += last
            if scored >= num_images:
                break

    # one transfer: the log of every image scored and the rows of the last batch
    fixed = 12 + 8 * sm.keep
    host = _fetch(sm._parts() + [sm._rows[:last]])
    per_image = sm._finish(host[:fixed])['per_image']
    every = {key: per_image[key].tolist() for key in ('ari', 'ari_fg')}
    last_rows = host[fixed:].reshape(last, 8)
    stamp = datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S")
    fprint(f"{stamp} | After [{len(every['ari'])} / {num_images}] images: "
           f"ARI {_mean(every['ari']):.4f}, FG ARI {_mean(every['ari_fg']):.4f}")
    kept = {key: vals[:num_images] for key, vals in every.items()}
    averages = {key: _mean(vals) for key, vals in kept.items()}
    for key, label in (('ari', 'ARI'), ('ari_fg', 'FG ARI')):
        fprint(f"FINAL {label} for {len(kept[key])} images: {averages[key]:.4f}")
    model.train()
    return averages['ari'], averages['ari_fg'], last_rows[:, 0].tolist(), last_rows[:, 1].tolist()


def seg_metrics_from_model(model, batches, max_labels=32):
    """The loop of scripts/compute_seg_metrics.py:101-131 over prefetched `batches` ({'input', 'instances'}, any batch size; the
    script's is 1): foreground ARI and foreground mean segmentation covering, each the mean over batches of batch means, for
    log_m_k ('ari_fg', 'msc_fg') and, when the model reports log_m_r_k, for it too ('ari_fg_r', 'msc_fg_r').  Prints the script's
    lines -- the covering ones show a float32 tensor, as the script's do.  The model is left in eval mode, as the script leaves it."""
    model.eval()
    scores = _MaskScores(max_labels)
    with torch.no_grad():
        for x in batches:
            stats = model(x['input'].cuda() if _on_device(model) else x['input'])[2]
            scores.update(stats, x['instances'])
    res = scores.finish(_fetch(scores.parts()))
    out = {}
    for (field, suffix), tag in zip(MASK_FIELDS, ('FG', 'FG-R')):
        if field not in res:
            continue
        out['ari_fg' + suffix], out['msc_fg' + suffix] = res[field]['ari_fg'], res[field]['msc_fg']
        fprint(f"Average {tag} ARI: {out['ari_fg' + suffix]}")
        fprint(f"Average {tag} MSC: {torch.tensor(out['msc_fg' + suffix], dtype=torch.float32)}")
    return out


def reconstruction_quality_from_model(model, batches, data_range=1.0, win_size=11, sigma=1.5, keep_per_image=0):
    """MSE, RMSE, PSNR and SSIM of the model's reconstructions of prefetched `batches` ({'input'}, any batch sizes), the sibling of
    seg_metrics_from_model for data without labels: eval mode, no gradients, one ImageQuality.update per batch and one transfer at
    the end.  Returns ImageQuality.compute()'s dict (means over the images, 'num_images', 'num_batches', and 'per_image' with
    keep_per_image > 0).  The model is left in eval mode."""
    model.eval()
    quality = ImageQuality(data_range=data_range, win_size=win_size, sigma=sigma, keep_per_image=keep_per_image)
    with torch.no_grad():
        for x in batches:
            inp = x['input'].cuda() if _on_device(model) else x['input']
            quality.update(model(inp)[0], inp)
    return quality._finish(_fetch(quality._parts()))
