"""ms per TrainStep(graph=True) step for every combination of matmul level (genesis_amd.set_matmul_precision) and tap-conv mode
(genesis_amd.set_tapconv_precision: 'default' | 'medium') -- the configurations of tools/precision_time.py (B = 32).  A fresh model
and loop per (config, level, mode): the first step captures the graph; then `--steps` replayed steps are timed with HIP events,
`--reps` times, the median reported.

    python tools/tapconv_precision_time.py [--steps 30] [--reps 5] [--configs metric,cfg5,monet4,genesis3]
                                           [--levels high,medium] [--taps default,medium] [--out table.md]"""
import argparse
import json
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
import genesis_amd  # noqa: E402
from genesis_amd import _lib  # noqa: E402
from precision_time import time_level  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--configs', default='metric,cfg5,monet4,genesis3')
    ap.add_argument('--levels', default='high,medium')
    ap.add_argument('--taps', default='default,medium')
    ap.add_argument('--out', default=None, help='markdown table (+ .json next to it)')
    a = ap.parse_args()
    levels, taps = a.levels.split(','), a.taps.split(',')
    rows, raw = [], {}
    try:
        for name in a.configs.split(','):
            res = {}
            for level in levels:
                for tap in taps:
                    genesis_amd.set_tapconv_precision(tap)
                    med, ms, elbo = time_level(name, level, a.steps, a.reps)
                    res[(level, tap)] = med
                    raw['%s/%s/tap-%s' % (name, level, tap)] = dict(ms_per_step=med, reps=ms, last_elbo=elbo)
                    print('%-9s %-8s tap %-8s %8.3f ms/step  (reps %s; last ELBO %.4f)'
                          % (name, level, tap, med, ' '.join('%.3f' % v for v in ms), elbo), flush=True)
            rows.append((name, res))
    finally:
        _lib.load().gx_matmul_precision(-1)
        _lib.load().gx_tapconv_precision(-1)
    cols = [(lv, t) for lv in levels for t in taps]
    base = cols[0]
    lines = ['| config | ' + ' | '.join('%s / tap %s ms/step' % c for c in cols) + ' |', '|---' * (len(cols) + 1) + '|']
    for name, r in rows:
        cells = ['%.3f (%+.1f %%)' % (r[c], 100.0 * (r[c] - r[base]) / r[base]) if c != base else '%.3f' % r[c] for c in cols]
        lines.append('| %s | %s |' % (name, ' | '.join(cells)))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('TrainStep(graph=True), B = 32, median of %d x %d steps (tools/tapconv_precision_time.py); in brackets: '
                    'change against %s / tap %s\n\n' % (a.reps, a.steps, base[0], base[1]))
            f.write('\n'.join(lines) + '\n')
        with open(osp.splitext(a.out)[0] + '.json', 'w') as f:
            json.dump(raw, f, indent=1)


if __name__ == '__main__':
    main()
