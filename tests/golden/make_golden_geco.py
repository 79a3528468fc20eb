"""Generates tests/golden/geco_series.npz from the REAL reference class utils/geco.py:GECO (imported through
oracle.ref_import where the reference tree is present): error series and the `beta` / `err_ema` its loss() leaves after each
call.  Recorded results only.

main      300 errors (float32): 3 x goal falling in a straight line to 0.8 x goal at step 100 (the moving average crosses the
          goal near step 100), then goal x (1 - 0.2 exp(-(t - 100) / 150) cos(2 pi (t - 100) / 40)): an oscillation around the
          goal whose amplitude shrinks, slow enough for the moving average (alpha 0.9) to cross the goal about every 20 steps,
          in both directions.  Driven twice, with speedup = 10 and with speedup = None.
lo_clamp  beta_init 1e-9, four errors of 1e6 x goal at step size 1: the factor underflows, beta lands on beta_min.
hi_clamp  four errors of 0 at step size 1, speedup 10: the factor overflows, beta lands on beta_max and stays there.
Keys: <case>_err, <case>_beta, <case>_ema (float32 [T]; <case> = main_su10, main_none, lo_clamp, hi_clamp -- the two main cases
share main_err) and the scalars goal, step_size, alpha, speedup."""
import os.path as osp
import sys

import numpy as np
import torch

HERE = osp.dirname(osp.abspath(__file__))
REPO = osp.dirname(osp.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import ref_import as R  # noqa: E402

GOAL, STEP_SIZE, ALPHA, SPEEDUP = 1737.25, 4e-5, 0.9, 10


def main_series():
    t = np.arange(300, dtype=np.float64)
    down = 3.0 - 2.2 * t / 100.0
    u = t - 100.0
    wave = 1.0 - 0.2 * np.exp(-u / 150.0) * np.cos(2 * np.pi * u / 40.0)
    return (GOAL * np.where(t < 100, down, wave)).astype(np.float32)


def drive(geco_cls, errs, **kw):
    g = geco_cls(**kw)
    betas, emas = [], []
    for e in errs:
        g.loss(torch.tensor(float(e), dtype=torch.float32), torch.tensor(0.0))
        betas.append(float(g.beta)); emas.append(float(g.err_ema))
    return np.array(betas, dtype=np.float32), np.array(emas, dtype=np.float32)


def main():
    GECO = R.import_reference()['geco'].GECO
    errs = main_series()
    out = {'goal': np.float64(GOAL), 'step_size': np.float64(STEP_SIZE), 'alpha': np.float64(ALPHA),
           'speedup': np.float64(SPEEDUP), 'main_err': errs}
    for name, su in (('main_su10', SPEEDUP), ('main_none', None)):
        out[name + '_beta'], out[name + '_ema'] = drive(GECO, errs, goal=GOAL, step_size=STEP_SIZE, alpha=ALPHA, speedup=su)
    lo = np.full(4, 1e6 * GOAL, dtype=np.float32)
    out['lo_clamp_err'] = lo
    out['lo_clamp_beta'], out['lo_clamp_ema'] = drive(GECO, lo, goal=GOAL, step_size=1.0, alpha=ALPHA, beta_init=1e-9,
                                                      speedup=SPEEDUP)
    hi = np.zeros(4, dtype=np.float32)
    out['hi_clamp_err'] = hi
    out['hi_clamp_beta'], out['hi_clamp_ema'] = drive(GECO, hi, goal=GOAL, step_size=1.0, alpha=ALPHA, speedup=SPEEDUP)
    np.savez_compressed(osp.join(HERE, 'geco_series.npz'), **out)
    ema = out['main_su10_ema'].astype(np.float64)
    print('crossings of the goal by the moving average: %d; beta range %.3e .. %.3e (speedup) / %.3e .. %.3e (none); clamps %s %s'
          % (int(np.sum(np.diff(np.sign(GOAL - ema)) != 0)), out['main_su10_beta'].min(), out['main_su10_beta'].max(),
             out['main_none_beta'].min(), out['main_none_beta'].max(), out['lo_clamp_beta'], out['hi_clamp_beta']))


if __name__ == '__main__':
    main()
