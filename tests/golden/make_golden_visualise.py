"""Generates tests/golden/visualise_*.npz from the REAL reference function train.py:visualise_outputs (imported through
oracle.ref_import where the reference tree exists), run on the CPU with the stub model and recording writer of
tests/visualise_stub.py.  torchvision is absent here: tests/vis_restatement.py's make_grid (pinned by hand-written arrays in
tests/test_visualise_cpu.py) is installed as torchvision.utils.make_grid; tensorboardX and scripts.compute_fid, which carry no
arithmetic, get empty stand-ins.  utils.misc.colour_seg_masks is the reference's own and opens its own palette file, so the run
happens in the reference's directory.

Inputs: a batch of 10 images (the function takes the first 8), K = 3, 8 x 8 planes made of 4 x 4 blocks with values in sixteenths
(they deflate well), log-masks from a log-softmax, instance maps of 2 x 2 blocks with a -1 ignore region, and recorded sample()
outputs.  Cases: 'v2' (both mask fields, mx_r_k, instances; one slot of log_m_k holds -1e10 as dynamic_K's finished slots do),
'monet' (log_m_k only, no instances), 'nosample' (sample raises NotImplementedError).  Recorded: the inputs, and per writer call
its tag and array ('img_<i>'; shape and dtype are the array's own).  `--out DIR` writes elsewhere (the regeneration test)."""
import os
import os.path as osp
import sys
import types

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
REPO = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import ref_import as R  # noqa: E402
from tests import vis_restatement as V  # noqa: E402
from tests import visualise_stub as S  # noqa: E402

NB, B, K, SIZE, UP, INST_UP = 10, 8, 3, 8, 4, 2
ITER_IDX = 1200
CASES = {  # name: (stat keys, instances, sample, seed)
    'v2': (('mx_r_k', 'x_r_k', 'log_m_k', 'log_m_r_k'), True, True, 31),
    'monet': (('x_r_k', 'log_m_k'), False, True, 32),
    'nosample': (('log_m_k',), True, False, 33),
}


def stand_ins():
    for name, attrs in (('torchvision', {}), ('torchvision.utils', {'make_grid': V.make_grid_torch}),
                        ('tensorboardX', {'SummaryWriter': None}), ('scripts.compute_fid', {'fid_from_model': None})):
        mod = types.ModuleType(name)
        for a, v in attrs.items():
            setattr(mod, a, v)
        sys.modules[name] = mod


def sixteenths(g, *shape):
    return (torch.randint(0, 17, shape, generator=g).float() / 16.0).numpy()


def log_masks(g, n):
    return torch.log_softmax(2.0 * torch.randn(K, n, 1, SIZE // UP, SIZE // UP, generator=g), 0).numpy()


def make_inputs(keys, with_inst, with_sample, seed):
    g = torch.Generator().manual_seed(seed)
    lo = SIZE // UP
    out = {'input': sixteenths(g, NB, 3, lo, lo), 'recon': sixteenths(g, B, 3, lo, lo)}
    for field in ('log_m_k', 'log_m_r_k'):
        if field in keys:
            out[field] = log_masks(g, B)
    if 'log_m_r_k' in keys:
        out['log_m_k'][2, 5] = -1e10                                  # a finished slot of dynamic_K
    if 'x_r_k' in keys:
        out['x_r_k'] = sixteenths(g, K, B, 3, lo, lo)
    if 'mx_r_k' in keys:
        out['mx_r_k'] = (torch.from_numpy(out['x_r_k']) * torch.from_numpy(out['log_m_r_k']).exp()).numpy()
    if with_inst:
        inst = torch.randint(0, 15, (NB, 1, SIZE // INST_UP, SIZE // INST_UP), generator=g)
        inst[:, :, 0, :2] = -1                                        # an ignore region
        inst[0, 0, 1, 0], inst[1, 0, 1, 0] = 0, 14                    # both ends of the palette
        out['instances'] = inst.numpy().astype(np.int8)
    if with_sample:
        out['gen_out'] = sixteenths(g, B, 3, lo, lo)
        out['gen_x_k'] = sixteenths(g, K, B, 3, lo, lo)
        out['gen_log_m_k'] = log_masks(g, B)
        out['gen_mx_k'] = (torch.from_numpy(out['gen_x_k']) * torch.from_numpy(out['gen_log_m_k']).exp()).numpy()
    out.update(K=K, up=UP, inst_up=INST_UP, has_sample=with_sample, iter_idx=ITER_IDX)
    return out


def main():
    out_dir = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else HERE
    R.import_reference()
    stand_ins()
    import train
    train.make_grid = V.make_grid_torch
    os.chdir(R.REFERENCE_ROOT)                                         # utils/colour_palette15.json
    for name, (keys, with_inst, with_sample, seed) in CASES.items():
        out = make_inputs(keys, with_inst, with_sample, seed)
        path = osp.join(out_dir, 'visualise_%s.npz' % name)
        np.savez_compressed(path, **out)
        g = S.load_case(name, out_dir)                                 # what the tests will read
        model, writer = S.StubModel(g), S.Writer()
        train.visualise_outputs(model, S.make_batch(g), writer, 'val', ITER_IDX)
        assert model.training and all(step == ITER_IDX for _, _, step in writer.calls)
        out['tags'] = np.array([c[0] for c in writer.calls])
        for i, (_, array, _) in enumerate(writer.calls):
            out['img_%02d' % i] = array.detach().numpy()
        np.savez_compressed(path, **out)
        print(name, osp.getsize(path), 'bytes', len(writer.calls), 'pictures')


if __name__ == '__main__':
    main()
