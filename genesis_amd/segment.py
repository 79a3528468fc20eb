"""Segmentation and per-object latents from a trained model, without the decoder.

GENESIS-V2's masks and posterior come from the UNet encoder, IC-SBP and the slot heads alone; the decoder, the mixture
likelihood and the KL terms that `model(x)` also evaluates contribute nothing to them.  `encode` runs exactly that first half
(GenesisV2._encode: the code `_compute` itself starts with) and `Segmenter` turns its masks into an ObjectTable
(genesis_amd/objects.py: label map, per-slot area, box, centroid, colour, confidence) in one more launch.  Models whose masks
need their whole forward pass (MONet, GENESIS) go through it, without gradients.

    seg = Segmenter(model)
    table, mu, sigma = seg(x)                                   # x fp32 [B,3,H,W] on the device
    seg.segment_folder('photos', 'out', img_size=64)            # out/<file>.png label maps + out/objects.csv

Command line (Forge-style flags, as train.py's):
    python -m genesis_amd.segment --model_config genesis_amd/genesisv2_config.py --model_file model.ckpt-500000 \\
        --data_folder photos --out_dir out --img_size 64 --K_steps 7"""
import collections
import os

import numpy as np
import torch

from . import autostep, objects, tbwriter
from ._lib import GenesisHipError

Encoded = collections.namedtuple('Encoded', 'log_m_k mu_k sigma_k steps')
Segmented = collections.namedtuple('Segmented', 'table mu sigma')
CSV_HEADER = 'file,slot,area,x0,y0,x1,y1,cx,cy,border,mass,confidence,r,g,b'
CSV_NAME = 'objects.csv'


def encode(model, x, rand_pixel=None):
    """The encoder half of a GenesisV2 forward pass, under no_grad: UNet encoder, seg / feat heads and IC-SBP (the model's own
    three-way dispatch), the pooled slot features, z_head and the posterior's mu and sigma.  No decoder, no mixture, no KL, and
    no eps is drawn.  x fp32 [B,3,H,W] on the device; rand_pixel [B,1,H,W] uniform, the IC-SBP seed draws (default: torch.rand).
    -> Encoded(log_m_k, mu_k, sigma_k, steps): K lists of [B,1,H,W] / [B,D] tensors, the very tensors (same kernels, same inputs)
    that model(x, rand_pixel=rand_pixel) returns as stats.log_m_k and comp_stats.mu_k / sigma_k; steps: with dynamic_K the
    per-image step counts [B] (masks of finished images are padded with -1e10; one image: the lists end early), else None.
    The model's training flag and the grad mode are left as found."""
    if not hasattr(model, '_encode'):
        raise GenesisHipError('encode: model must be a GenesisV2 (%s has no encoder-only path)' % type(model).__name__)
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_cuda:
        raise GenesisHipError('encode: x must be a [B,3,H,W] tensor on the HIP device; there is no CPU path')
    with torch.no_grad():
        autostep.arm(model)      # (as forward() does: drops what an unfinished training pass left armed; arms nothing without autograd)
        e = model._encode(x, rand_pixel, None, None, posterior_noise=False)
    return Encoded(list(e['log_m'].unbind(0)), list(e['mu'].unbind(0)), list(e['sigma'].unbind(0)), e['steps'])


def _field(stats, name):
    try:
        return stats[name]
    except (KeyError, TypeError, IndexError):
        return getattr(stats, name, None)


def label_png(labels, level=6):
    """uint8 [H, W] label map -> the bytes of an 8-bit greyscale PNG (tbwriter's encoder: no Pillow)."""
    a = np.ascontiguousarray(labels, dtype=np.uint8)
    if a.ndim != 2:
        raise GenesisHipError('label_png: labels must be [H, W], got %s' % (a.shape,))
    H, W = a.shape
    return tbwriter._png(tbwriter.pack_rows_host(a.reshape(H, W, 1)), H, W, 1, level)


def _num(v):
    return repr(float(v))


def csv_rows(table, files, min_pixels=1):
    """The objects.csv lines (CSV_HEADER's columns, no header) of a host ObjectTable: one per (file, present slot), files in
    order, slots ascending.  Integers as integers, fp64 values with repr (they read back exactly); r, g, b: the mean colour's
    first three channels, empty where the table has fewer."""
    if table.labels.is_cuda:
        raise GenesisHipError('csv_rows: table must be on the host (ObjectTable.cpu())')
    if len(files) != table.labels.shape[0]:
        raise GenesisHipError('csv_rows: %d files for a table of %d images' % (len(files), table.labels.shape[0]))
    geom, present = table.geom.numpy(), table.present(min_pixels).numpy()
    centroid, mass = table.centroid.numpy(), table.mass.numpy()
    confidence, colour = table.confidence.numpy(), table.mean_colour.numpy()
    rows = []
    for b, name in enumerate(files):
        if ',' in name or '"' in name or '\n' in name:
            name = '"' + name.replace('"', '""') + '"'
        for k in np.flatnonzero(present[b]):
            g = geom[b, k]
            rgb = [_num(colour[b, k, c]) if c < table.channels else '' for c in range(3)]
            rows.append(','.join([name, str(int(k)), str(int(g[0])), str(int(g[1])), str(int(g[2])), str(int(g[3])), str(int(g[4])),
                                  _num(centroid[b, k, 0]), _num(centroid[b, k, 1]), str(int(g[7])), _num(mass[b, k]),
                                  _num(confidence[b, k])] + rgb))
    return rows


class Segmenter(object):
    """model -> per-batch object tables.  seg(x): x fp32 [B,C,H,W] on the device -> Segmented(table, mu, sigma): the ObjectTable
    of the batch (object_table(log_m_k, image=x)) and, for a GenesisV2, the posterior's mu / sigma [K,B,D] (None otherwise).
    A GenesisV2 goes through `encode`; any other model whose forward returns stats.log_m_k (MONet, GENESIS) through its full
    forward pass in eval mode without gradients (the training flag is put back); a model without log_m_k is refused.
    min_pixels: the area from which a slot counts as present in segment_folder's objects.csv.
    generator: a torch.Generator for IC-SBP's rand_pixel draws (GenesisV2 only; default: the device's global generator).  The
    draws are made per batch, [B,1,H,W] at once, so with a generator an image's segmentation is reproducible for the same
    batches in the same order -- it depends on the batch composition, not on the image alone."""

    def __init__(self, model, min_pixels=1, generator=None):
        if not isinstance(min_pixels, int) or isinstance(min_pixels, bool) or min_pixels < 1:
            raise GenesisHipError('Segmenter: min_pixels must be a positive int, not %r' % (min_pixels,))
        if generator is not None and not isinstance(generator, torch.Generator):
            raise GenesisHipError('Segmenter: generator must be a torch.Generator, not %s' % type(generator).__name__)
        if not callable(model):
            raise GenesisHipError('Segmenter: model must be callable')
        self.model, self.min_pixels, self.generator = model, min_pixels, generator
        self.encoder_only = hasattr(model, '_encode')

    def _rand_pixel(self, x):
        if self.generator is None:
            return None
        B, _, H, W = x.shape
        return torch.rand(B, 1, H, W, generator=self.generator, device=self.generator.device).to(x.device)

    def __call__(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32:
            raise GenesisHipError('Segmenter: x must be an fp32 [B,C,H,W] tensor')
        if not x.is_cuda:
            raise GenesisHipError('Segmenter: x must live on the HIP device; there is no CPU path')
        image = x if x.shape[1] <= 4 else None
        if self.encoder_only:
            e = encode(self.model, x, self._rand_pixel(x))
            return Segmented(objects.object_table(e.log_m_k, image), torch.stack(e.mu_k), torch.stack(e.sigma_k))
        was_training = getattr(self.model, 'training', None)
        if was_training:
            self.model.eval()
        try:
            with torch.no_grad():
                out = self.model(x)
        finally:
            if was_training:
                self.model.train()
        stats = out[2] if isinstance(out, (tuple, list)) and len(out) > 2 else None
        log_m_k = _field(stats, 'log_m_k') if stats is not None else None
        if log_m_k is None:
            raise GenesisHipError('Segmenter: the forward pass of %s returns no stats.log_m_k; there is nothing to segment'
                                  % type(self.model).__name__)
        return Segmented(objects.object_table(log_m_k, image), None, None)

    def segment_folder(self, folder, out_dir, img_size, batch_size=32, num_workers=4, max_side=1024, device=None):
        """Segments every image file under `folder` (image_folder_config.find_images: .png / .jpg / .jpeg, recursively, sorted), in
        file order, batch_size at a time (the short last batch kept), each under the image-folder transform at img_size.  Writes
        <out_dir>/<relative path>.png, an 8-bit greyscale label map per file, and <out_dir>/objects.csv, one row per (file, slot
        with at least min_pixels pixels) under CSV_HEADER.  One host transfer per batch.  device: default the model's.
        -> (the relative paths, the number of csv rows)."""
        from . import image_folder_config, imagefile
        if not os.path.isdir(folder):
            raise GenesisHipError('segment_folder: folder %s does not exist' % folder)
        files = image_folder_config.find_images(folder)
        if not files:
            raise GenesisHipError('segment_folder: no image files (%s) under %s' % (', '.join(image_folder_config.EXTENSIONS), folder))
        if device is None:
            p = next(iter(self.model.parameters()), None) if hasattr(self.model, 'parameters') else None
            device = p.device if p is not None else 'cuda'
        loader = imagefile.ImageFileLoader([os.path.join(folder, f) for f in files], batch_size, img_size, shuffle=False,
                                           num_workers=num_workers, device=device, max_side=max_side, name='segment_folder')
        os.makedirs(out_dir, exist_ok=True)
        done, rows = 0, 0
        with open(os.path.join(out_dir, CSV_NAME), 'w') as csv:
            csv.write(CSV_HEADER + '\n')
            for batch in loader:
                host = self(batch['input']).table.cpu()                  # the batch's one transfer
                names = files[done:done + host.labels.shape[0]]
                labels = host.labels.numpy()
                for i, name in enumerate(names):
                    path = os.path.join(out_dir, name + '.png')
                    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
                    with open(path, 'wb') as f:
                        f.write(label_png(labels[i]))
                lines = csv_rows(host, names, self.min_pixels)
                csv.write(''.join(line + '\n' for line in lines))
                done, rows = done + len(names), rows + len(lines)
        if done != len(files):
            raise GenesisHipError('segment_folder: %d of %d files were segmented' % (done, len(files)))
        return files, rows


def main(argv=None):
    from . import compat
    compat.install()
    import forge
    from forge import flags
    import forge.experiment_tools as fet
    from . import image_folder_config  # noqa: F401  (registers data_folder, img_size, num_workers, K_steps)
    flags.DEFINE_string('model_config', 'genesis_amd/genesisv2_config.py', 'Path to a model config file.')
    flags.DEFINE_string('model_file', '', 'Path to a checkpoint (model_state_dict) or a bare state_dict.')
    flags.DEFINE_string('out_dir', 'segmentation', 'Folder the label maps and objects.csv are written to.')
    flags.DEFINE_integer('batch_size', 32, 'Images per batch.')
    flags.DEFINE_integer('min_pixels', 1, 'Smallest area of a slot listed in objects.csv.')
    flags.DEFINE_integer('max_side', 1024, 'Largest width or height of a file.')
    flags.DEFINE_integer('seed', -1, 'Seed of the seed-pixel draws; negative: the global generator.')
    flags.DEFINE_boolean('debug', False, 'Debug flag.')
    flags.DEFINE_boolean('multi_gpu', False, 'Multi-GPU flag of the model configs.')
    cfg = forge.config(argv)
    if not cfg.model_file:
        raise SystemExit('segment: --model_file is required')
    # the model config registers its own flags when it is imported: import it (fet.load finds the module again), then parse
    # once more so that its flags are read with their types
    import importlib.util
    import sys
    path = os.path.abspath(cfg.model_config)
    name = '_forge_cfg_' + os.path.splitext(os.path.basename(path))[0]
    spec = importlib.util.spec_from_file_location(name, path)
    sys.modules[name] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sys.modules[name])
    cfg = forge.config(argv)
    model = fet.load(cfg.model_config, cfg)
    state = torch.load(cfg.model_file, map_location='cpu')
    state = state.get('model_state_dict', state)
    model.load_state_dict({(k[7:] if k.startswith('module.') else k): v for k, v in state.items()})
    model = model.to('cuda')
    generator = torch.Generator(device='cuda').manual_seed(cfg.seed) if cfg.seed >= 0 else None
    seg = Segmenter(model, cfg.min_pixels, generator)
    files, rows = seg.segment_folder(cfg.data_folder, cfg.out_dir, cfg.img_size, cfg.batch_size, cfg.num_workers, cfg.max_side)
    fet.fprint('segment: %d files, %d objects -> %s' % (len(files), rows, cfg.out_dir))


if __name__ == '__main__':
    main()
