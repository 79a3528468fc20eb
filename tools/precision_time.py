"""ms per TrainStep(graph=True) step at the three matmul precision levels (genesis_amd.set_matmul_precision: 'highest' | 'high' |
'medium') for the metric configuration (GENESIS-V2, K = 7, 64 x 64, B = 32), config 5 (K = 11, 128 x 128, B = 32), MONet config 4
and GENESIS config 3 (K = 7, 64 x 64, B = 32).  A fresh model and loop per (config, level): the first step captures the graph;
then `--steps` replayed steps are timed with HIP events, `--reps` times, the median reported.

    python tools/precision_time.py [--steps 30] [--reps 5] [--configs metric,cfg5,monet4,genesis3] [--levels ...] [--out table.md]"""
import argparse
import json
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
import torch  # noqa: E402

import genesis_amd  # noqa: E402
from genesis_amd import _lib, testing as T  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402
from genesis_amd.trainer import TrainStep  # noqa: E402

CONFIGS = {
    'metric': ('v2', dict(K_steps=7, img_size=64, feat_dim=64), 32),
    'cfg5': ('v2', dict(K_steps=11, img_size=128, feat_dim=64), 32),
    'monet4': ('monet', dict(K_steps=7, img_size=64), 32),
    'genesis3': ('genesis', dict(K_steps=7, img_size=64), 32),
}


def build(fam, kw):
    if fam == 'v2':
        from oracle import v2_oracle as O
        import genesis_amd.genesisv2_config as G
    elif fam == 'monet':
        from oracle import monet_oracle as O
        import genesis_amd.monet_config as G
    else:
        from oracle import genesis_oracle as O
        import genesis_amd.genesis_config as G
    cfg = O.make_cfg(**kw)
    torch.manual_seed(0)
    return G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False))).cuda().train(), cfg['img_size']


def time_level(name, level, steps, reps):
    fam, kw, B = CONFIGS[name]
    genesis_amd.set_matmul_precision(level)
    model, S = build(fam, kw)
    x = T.make_input(1, B, S).cuda()
    ts = TrainStep(model, S, graph=True)
    out = ts.step(x)                         # capture + one step
    for _ in range(3):
        out = ts.step(x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        for _ in range(steps):
            out = ts.step(x)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    elbo = float(out[0])
    ts.close()
    del ts, model
    torch.cuda.empty_cache()
    ms.sort()
    return ms[len(ms) // 2], ms, elbo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--configs', default='metric,cfg5,monet4,genesis3')
    ap.add_argument('--levels', default='highest,high,medium', help='(one level per process: a rocprofv3 pass of its own)')
    ap.add_argument('--out', default=None, help='markdown table (+ .json next to it)')
    a = ap.parse_args()
    rows, raw = [], {}
    try:
        for name in a.configs.split(','):
            res = {}
            for level in a.levels.split(','):
                med, ms, elbo = time_level(name, level, a.steps, a.reps)
                res[level] = med
                raw['%s/%s' % (name, level)] = dict(ms_per_step=med, reps=ms, last_elbo=elbo)
                print('%-9s %-8s %8.3f ms/step  (reps %s; last ELBO %.4f)' % (name, level, med, ' '.join('%.3f' % v for v in ms), elbo),
                      flush=True)
            rows.append((name, res))
    finally:
        _lib.load().gx_matmul_precision(-1)
    lines = ['| config | highest ms/step | high ms/step | medium ms/step | medium saves vs high |', '|---|---|---|---|---|']
    for name, r in rows:
        if len(r) < 3:
            continue
        lines.append('| %s | %.3f | %.3f | %.3f | %+.1f %% |' % (name, r['highest'], r['high'], r['medium'],
                                                               100.0 * (r['high'] - r['medium']) / r['high']))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('TrainStep(graph=True), B = 32, median of %d x %d steps (tools/precision_time.py)\n\n' % (a.reps, a.steps))
            f.write('\n'.join(lines) + '\n')
        with open(osp.splitext(a.out)[0] + '.json', 'w') as f:
            json.dump(raw, f, indent=1)


if __name__ == '__main__':
    main()
