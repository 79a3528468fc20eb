"""Records the reference runs of the two live-import checks (test_live_against_reference_import in
tests/test_oracle_vs_golden.py and tests/test_monet_oracle.py) from the REAL reference, so that the checks also run where
the reference tree is absent: the state_dict of the reference's own randomly initialised model, the input and the
reference's forward outputs, exactly as the tests' live_reference_run produces them.

    python tests/golden/make_golden_live.py      # -> tests/golden/live_v2.npz, tests/golden/live_monet.npz
"""
import os.path as osp
import sys

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
REPO = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, REPO)

from genesis_amd import testing as T  # noqa: E402
from oracle import ref_import as R  # noqa: E402
from tests import test_monet_oracle, test_oracle_vs_golden  # noqa: E402


def template(sd):
    """sd with every value zeroed that formula_state_dict does not copy (it copies the buffers 'std' / num_batches_tracked and
    log_sigma); checked: both give the same weights."""
    kept = lambda k: k == 'std' or k.endswith('num_batches_tracked') or k.endswith('log_sigma')  # noqa: E731
    t = {k: v.clone() if kept(k) else torch.zeros_like(v) for k, v in sd.items()}
    a, b = T.formula_state_dict(sd), T.formula_state_dict(t)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    return t


def record(name, run, mods):
    sd, x, outs = run(mods)
    sd = template(sd)
    arrays = {'sd_keys': np.array(list(sd.keys())), 'x': x.numpy()}
    arrays.update({'sd/' + k: v.detach().numpy() for k, v in sd.items()})
    arrays.update({'out/' + k: v.detach().numpy() for k, v in outs.items()})
    path = osp.join(HERE, 'live_%s.npz' % name)
    np.savez_compressed(path, **arrays)
    print('wrote %s' % path)


if __name__ == '__main__':
    mods = R.import_reference()
    record('v2', test_oracle_vs_golden.live_reference_run, mods)
    record('monet', test_monet_oracle.live_reference_run, mods)
