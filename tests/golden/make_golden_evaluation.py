"""Generates tests/golden/evaluation_*.npz from the REAL reference functions train.py:evaluation and
utils/misc.py:dataset_ari (imported through oracle.ref_import where the reference tree exists; sklearn supplies
adjusted_rand_score), run on the stub model and loader of tests/evaluation_stub.py: seeded losses and blocky log-masks /
instance maps, B = 4, K = 4, 16 x 16, six batches.  train.py's imports that are absent here and carry no arithmetic
(torchvision.utils, tensorboardX, scripts.compute_fid) get empty stand-ins in this script's own sys.modules.

Cases: the num_batches rule three ways (iter_idx = 0: five batches; N_eval = 16; all batches), both loss forms ([B] tensors and
lists of K tensors [B]), kl_l_k / kl_l, with / without log_m_r_k, N_seg_metrics = 10 (the gate closes after three batches and the
reference's two assertions hold), and one case without 'instances'.  Recorded: the inputs, the returned dict, the scalars the
writer received; for the instance-bearing cases also dataset_ari(num_images=10) and, for seg_metrics_from_model, the means over
all six batches of the reference's foreground average_ari / average_segcover per mask field."""
import os.path as osp
import sys
import types

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
REPO = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import ref_import as R  # noqa: E402
from tests import evaluation_stub as S  # noqa: E402

B, K, SIZE, NB = 4, 4, 16, 6
MASK_UP, INST_UP = 4, 2
CASES = {  # name: (iter_idx, N_eval, loss keys, log_m_r_k, instances, seed)
    'iter0': (0, None, ('err', 'kl_l_k', 'kl_m'), True, True, 21),
    'neval16': (7, 16, ('err', 'kl_l', 'kl_m'), False, True, 22),
    'all': (7, None, ('err', 'kl_l_k', 'kl_m_k', 'aux'), True, True, 23),
    'noinst': (7, None, ('err', 'kl_l_k', 'kl_m'), True, False, 24),
}
N_SEG_METRICS = 10
NUM_IMAGES = 10


def stand_ins():
    for name, attrs in (('torchvision', ()), ('torchvision.utils', ('make_grid',)), ('tensorboardX', ('SummaryWriter',)),
                        ('scripts.compute_fid', ('fid_from_model',))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod


def make_inputs(loss_keys, with_r, with_inst, seed):
    g = torch.Generator().manual_seed(seed)
    out = {'loss_keys': np.array(loss_keys)}
    for k in loss_keys:
        shape = (NB, K, B) if k in S.LIST_LOSSES else (NB, B)
        out['loss/' + k] = (torch.rand(shape, generator=g) * (200.0 if k == 'err' else 3.0)).numpy()
    inst = torch.randint(0, 4, (NB, B, 1, SIZE // INST_UP, SIZE // INST_UP), generator=g)
    inst[:, 0][inst[:, 0] == 3] = 0                                   # a label absent from image 0 of every batch
    low = inst[..., ::MASK_UP // INST_UP, ::MASK_UP // INST_UP]         # the masks follow the instances at half their resolution
    for field in ('log_m_k', 'log_m_r_k')[:2 if with_r else 1]:
        logits = torch.randn(NB, K, B, 1, SIZE // MASK_UP, SIZE // MASK_UP, generator=g)
        for k in range(K):
            logits[:, k] += 2.0 * (low == k).float()
        out[field] = torch.log_softmax(logits, 1).numpy()
    if with_inst:
        out['instances'] = inst.numpy().astype(np.int8)
    out.update(B=B, mask_up=MASK_UP, inst_up=INST_UP, num_loader_batches=NB, input_shape=np.array([B, 3, SIZE, SIZE]))
    return out


def foreground_scores(misc, planes, inst):
    """(foreground ARI, foreground mean covering) of one batch from the reference's two metric functions."""
    labels = torch.cat(planes, 1).argmax(1, keepdim=True)
    return misc.average_ari(planes, inst, True)[0], misc.average_segcover(inst, labels, True)[0]


def main():
    R.import_reference()
    stand_ins()
    import train
    import utils.misc as misc
    for name, (iter_idx, n_eval, loss_keys, with_r, with_inst, seed) in CASES.items():
        out = make_inputs(loss_keys, with_r, with_inst, seed)
        out.update(iter_idx=iter_idx, N_eval=-1 if n_eval is None else n_eval, N_seg_metrics=N_SEG_METRICS)
        path = osp.join(HERE, 'evaluation_%s.npz' % name)
        np.savez_compressed(path, **out)
        g = S.load_case(name)                                          # what the tests will read
        config, _, _, _ = S.eval_args(g)
        model, writer = S.StubModel(g), S.Writer()
        ret = train.evaluation(model, S.make_loader(g), writer, config, iter_idx, n_eval, N_SEG_METRICS)
        assert model.training and torch.is_grad_enabled()
        out['ret_keys'] = np.array(list(ret.keys()))
        out['ret_vals'] = np.array([ret[k] for k in ret], np.float64)
        out['writer_tags'] = np.array([c[0] for c in writer.calls])
        out['writer_vals'] = np.array([c[1] for c in writer.calls], np.float64)
        out['writer_steps'] = np.array([c[2] for c in writer.calls], np.int64)
        if with_inst:
            avg, avg_fg, lst, lst_fg = misc.dataset_ari(S.StubModel(g), S.make_loader(g), NUM_IMAGES)
            out.update(num_images=NUM_IMAGES, dari_avg=np.float64(avg), dari_avg_fg=np.float64(avg_fg),
                       dari_list=np.array(lst, np.float64), dari_list_fg=np.array(lst_fg, np.float64))
            model, means = S.StubModel(g), {}
            for x in S.make_loader(g):             # foreground scores of every batch and mask field, then their plain means
                stats = model(x['input'])[2]
                for field in ('log_m_k', 'log_m_r_k'):
                    if field in stats:
                        means.setdefault(field, []).append(foreground_scores(misc, stats[field], x['instances']))
            for field, rows in means.items():
                r = '_r' if field == 'log_m_r_k' else ''
                for key, col in zip(('ari_fg', 'msc_fg'), zip(*rows)):
                    out['sm_' + key + r] = np.float64(float(sum(col) / len(col)))
        np.savez_compressed(path, **out)
        print(name, osp.getsize(path), 'bytes', dict(zip(out['ret_keys'], out['ret_vals'])))


if __name__ == '__main__':
    main()
