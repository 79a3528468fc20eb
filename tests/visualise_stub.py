"""The stub model and writer behind tests/golden/visualise_*.npz (tests/golden/make_golden_visualise.py records what the
reference's train.visualise_outputs hands to the writer for them; the tests replay the same objects through
genesis_amd.visualise).  forward() and sample() hand out recorded tensors; nothing is computed here."""
import os.path as osp

import numpy as np
import torch

from genesis_amd.compat.attrdict import AttrDict

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), 'golden')
CASES = ('v2', 'monet', 'nosample')
STAT_KEYS = ('mx_r_k', 'x_r_k', 'log_m_k', 'log_m_r_k')       # stored [K, B, C, h, w]
SAMPLE_KEYS = ('x_k', 'log_m_k', 'mx_k')                      # stored as 'gen_<key>'


def load_case(name, directory=GOLDEN):
    return np.load(osp.join(directory, 'visualise_%s.npz' % name), allow_pickle=False)


def _up(a, f):
    """[..., h, w] -> [..., f h, f w] by repetition (the fixtures store blocky planes at their block resolution)."""
    return torch.from_numpy(np.ascontiguousarray(a)).repeat_interleave(f, -2).repeat_interleave(f, -1)


def _slots(t, packed):
    """[K, B, C, H, W] -> the list of K tensors a model returns: views of the one buffer, or K tensors of their own."""
    return list(t.unbind(0)) if packed else [p.clone() for p in t.unbind(0)]


class StubModel:
    def __init__(self, g, device='cpu', packed=False, fail=False):
        self.device, self.training, self.fail, self.packed = torch.device(device), True, fail, packed
        self.param = torch.nn.Parameter(torch.zeros(1, device=self.device))
        self.K_steps = int(g['K'])
        up = int(g['up'])
        self.recon = _up(g['recon'], up).to(self.device)
        self.stats = {k: _up(g[k], up).to(self.device) for k in STAT_KEYS if k in g.files}
        self.has_sample = bool(g['has_sample'])
        if self.has_sample:
            self.sample_out = _up(g['gen_out'], up).to(self.device)
            self.sample_stats = {k: _up(g['gen_' + k], up).to(self.device) for k in SAMPLE_KEYS if 'gen_' + k in g.files}
        self.seen = []                      # (what, training) at every forward / sample

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def parameters(self):
        return iter([self.param])

    def __call__(self, x):
        self.seen.append(('forward', self.training, tuple(x.shape), x.device.type))
        if self.fail:
            raise RuntimeError('stub forward fails')
        stats = AttrDict()
        for k, t in self.stats.items():
            stats[k] = _slots(t, self.packed)
        return self.recon, None, stats, None, None

    def sample(self, batch_size, K_steps):
        self.seen.append(('sample', self.training, batch_size, K_steps))
        if not self.has_sample:
            raise NotImplementedError
        stats = AttrDict()
        for k, t in self.sample_stats.items():
            stats[k] = _slots(t, self.packed)
        return self.sample_out, stats


def make_batch(g, device='cpu'):
    up = int(g['up'])
    batch = {'input': _up(g['input'], up).to(device)}
    if 'instances' in g.files:
        batch['instances'] = _up(g['instances'], int(g['inst_up'])).to(torch.int64).to(device)
    return batch


class Writer:
    def __init__(self):
        self.calls = []

    def add_image(self, tag, array, step):
        self.calls.append((tag, array, int(step)))


def recorded_calls(g):
    """[(tag, array)] in the order the reference's writer received them."""
    return [(str(tag), g['img_%02d' % i]) for i, tag in enumerate(g['tags'])]
