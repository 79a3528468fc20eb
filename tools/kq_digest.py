"""SHA-256 digests of the transposed-conv kernels' outputs (forward, forward with GroupNorm statistics, data gradient) on the
16-bit matrix pipe, at the shapes of tests/test_kq_schedule_gpu.py.  A change of the kernels' SCHEDULE (staging order, buffering,
occupancy) leaves every accumulator's MFMAs and their order alone, so the outputs stay bit for bit what they were: run this on the
build BEFORE such a change and commit what it writes; the test then compares the build it runs on against the record.

    python tools/kq_digest.py [--out tests/golden/kq_schedule_digests.json]

The record also names the torch version and the device: the test skips the comparison, and says so, where either differs."""
import argparse
import hashlib
import json
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (N, Cin, Cout, Hin): the smallest shapes at which the ends of the staging pipeline can go wrong
SHAPES = [
    (3, 16, 64, 8),      # one chunk: a prefetch two phases ahead runs off the end at once; four images per tile, the last group ragged
    (2, 32, 64, 16),     # two chunks, one tile per image
    (5, 64, 64, 32),     # four chunks, four tiles per image
    (260, 16, 64, 16),   # 260 tiles: the split tail (q_split_tail), half-work workgroups
    (2, 48, 40, 64),     # four staging rounds, exact planes, ragged output channels
]
MODES = (1, 2)           # gx_kq_precision: six bf16 piece products, three fp16 piece products
GROUPS = 8
OUTPUTS = ('y', 'mean', 'rstd', 'dx')


def rnd(*shape, seed=0, scale=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def inputs(N, Cin, Cout, Hin):
    """CPU-seeded operands of one shape: x, w, bias, gamma, beta, dy."""
    return dict(x=rnd(N, Cin, Hin, Hin, seed=171), w=rnd(Cin, Cout, 5, 5, seed=172, scale=0.05), b=rnd(Cout, seed=173, scale=0.3),
                gamma=1 + 0.2 * rnd(Cout, seed=174), beta=0.1 * rnd(Cout, seed=175), dy=rnd(N, Cout, 2 * Hin, 2 * Hin, seed=176))


def run(t, mode, dev='cuda'):
    """The three entry points at gx_kq_policy(2), gx_kq_precision(mode) (the caller restores both): y, y with statistics, mean, rstd, dx."""
    from genesis_amd import _lib, hip_ops as hip
    _lib.call('gx_kq_policy', 2)
    _lib.call('gx_kq_precision', mode)
    d = {k: v.to(dev) for k, v in t.items()}
    y = hip.deconv5x5s2_fwd(d['x'], d['w'], d['b'])
    y2, mean, rstd = hip.deconv5x5s2_gn_stats_fwd(d['x'], d['w'], d['b'], d['gamma'], d['beta'], GROUPS, 1e-5)
    dx = hip.deconv5x5s2_dgrad(d['dy'], d['w'])
    return dict(y=y, y2=y2, mean=mean, rstd=rstd, dx=dx)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def key(shape):
    return ','.join(str(v) for v in shape)


def main():
    import torch
    from genesis_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=osp.join(ROOT, 'tests', 'golden', 'kq_schedule_digests.json'))
    a = ap.parse_args()
    _lib.load()
    rec = {'torch': torch.__version__, 'device': torch.cuda.get_device_name(0), 'digests': {}}
    try:
        for shape in SHAPES:
            t = inputs(*shape)
            rec['digests'][key(shape)] = {}
            for mode in MODES:
                o = run(t, mode)
                assert torch.equal(o['y'], o['y2']), (shape, mode)
                rec['digests'][key(shape)][str(mode)] = {k: digest(o[k]) for k in OUTPUTS}
    finally:
        _lib.call('gx_kq_precision', -1)
        _lib.call('gx_kq_policy', 1)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d shapes x %d forms on %s, torch %s' % (a.out, len(SHAPES), len(MODES), rec['device'], rec['torch']))


if __name__ == '__main__':
    main()
