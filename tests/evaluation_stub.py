"""The stub model and loader behind tests/golden/evaluation_*.npz (tests/golden/make_golden_evaluation.py records what the
reference's train.evaluation and utils.misc.dataset_ari return for them; the tests replay the same objects through
genesis_amd.evaluate).  The model's forward hands out recorded losses and masks batch after batch; nothing is computed here."""
import os.path as osp

import numpy as np
import torch

from genesis_amd.compat.attrdict import AttrDict

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
CASES = ('iter0', 'neval16', 'all', 'noinst')
INSTANCE_CASES = ('iter0', 'neval16', 'all')
LIST_LOSSES = ('kl_l_k', 'kl_m_k')      # stored [batches, K, B]: lists of K tensors [B]; every other loss is stored [batches, B]


def load_case(name):
    return np.load(osp.join(GOLDEN, 'evaluation_%s.npz' % name), allow_pickle=False)


def _up(a, f):
    """[..., h, w] -> [..., f h, f w] by repetition (the fixtures store blocky planes at their block resolution)."""
    return torch.from_numpy(np.ascontiguousarray(a)).repeat_interleave(f, -2).repeat_interleave(f, -1)


class Loader(list):
    """A list of batches with the two attributes evaluation() reads from a DataLoader."""

    def __init__(self, batches, batch_size):
        super().__init__(batches)
        self.batch_size = batch_size


class StubModel:
    """forward() returns the recorded (losses, stats) of call 0, 1, 2, ...; packed=True hands out the mask planes as views of
    one [K,B,1,H,W] buffer (as the project's models do), else as K separate tensors."""

    def __init__(self, g, device='cpu', packed=False, fail_at=None):
        self.device, self.calls, self.training, self.fail_at = torch.device(device), 0, True, fail_at
        self.seen = []                      # (training, grad enabled) at every forward
        self.param = torch.nn.Parameter(torch.zeros(1, device=self.device))
        self.loss_keys = [str(k) for k in g['loss_keys']]
        self.losses = {k: torch.from_numpy(g['loss/' + k]).to(self.device) for k in self.loss_keys}
        self.masks = {}
        for field in ('log_m_k', 'log_m_r_k'):
            if field in g.files:
                m = _up(g[field], int(g['mask_up'])).to(self.device)          # [batches, K, B, 1, H, W]
                self.masks[field] = m if packed else [[p.clone() for p in mb.unbind(0)] for mb in m]

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def parameters(self):
        return iter([self.param])

    def __call__(self, x):
        i, self.calls = self.calls, self.calls + 1
        self.seen.append((self.training, torch.is_grad_enabled()))
        if self.fail_at is not None and i == self.fail_at:
            raise RuntimeError('stub forward fails at call %d' % i)
        losses = AttrDict()
        for k in self.loss_keys:
            v = self.losses[k][i]
            losses[k] = list(v.unbind(0)) if k in LIST_LOSSES else v
        stats = AttrDict()
        for field, m in self.masks.items():
            stats[field] = list(m[i].unbind(0)) if torch.is_tensor(m) else list(m[i])
        return None, losses, stats, None, None


def make_loader(g, device='cpu'):
    n, B = int(g['num_loader_batches']), int(g['B'])
    shape = tuple(int(v) for v in g['input_shape'])
    batches = []
    for i in range(n):
        batch = {'input': torch.zeros(shape, device=device)}
        if 'instances' in g.files:
            batch['instances'] = _up(g['instances'][i], int(g['inst_up'])).to(torch.int64).to(device)
        batches.append(batch)
    return Loader(batches, B)


class Writer:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, float(value), int(step)))


def eval_args(g):
    """(config, iter_idx, N_eval, N_seg_metrics) of the recorded evaluation() call."""
    n_eval = int(g['N_eval'])
    return AttrDict(debug=False, gpu=False), int(g['iter_idx']), (None if n_eval < 0 else n_eval), int(g['N_seg_metrics'])
