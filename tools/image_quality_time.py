"""Time of the reconstruction-quality metrics per batch, in one process on the device:
  (a) genesis_amd.image_quality.ImageQuality.update (one gx_image_quality launch, fp64, no host read);
  (b) the same four per-image quantities composed from torch ops in fp64: five grouped F.conv2d calls with the 2-D Gaussian window
      for the five maps, the elementwise SSIM expression, the means, the squared error, PSNR;
  (c) the same composition in fp32,
at B = 32 for 3 x 64 x 64 and 3 x 128 x 128 -- wall clock around `--calls` calls ended by one synchronize, the three alternating in
every round, the median over the rounds -- with the kernel launches of one call of each (torch.profiler, after the timing has been
written) and the largest difference between (a) and (b) on the timed inputs.  For scale it copies evaluation()'s time per batch,
forward included, from profiles/eval_time.json (B = 32, 64 x 64).  The baseline is the torch composition, not the code under test.

The measurement runs in ONE child process under a time limit; if it fails or runs out of time this script reports that and
stops: there is no second attempt.
Usage: python tools/image_quality_time.py [--calls 200] [--rounds 5] [--limit 300] [--json profiles/image_quality_time.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def wall(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def torch_rows(pred, target, g2, L, dtype):
    """[B, 4] (mse, rmse, psnr, ssim) from torch ops in `dtype`; g2: the 2-D window as a depthwise weight [C, 1, n, n]."""
    import torch
    import torch.nn.functional as F
    x, y = pred.to(dtype), target.to(dtype)
    C = x.shape[1]
    d = x - y
    mse = (d * d).flatten(1).mean(1)
    psnr = 10.0 * torch.log10((L * L) / mse)
    mx, my = F.conv2d(x, g2, groups=C), F.conv2d(y, g2, groups=C)
    mxx, myy, mxy = F.conv2d(x * x, g2, groups=C), F.conv2d(y * y, g2, groups=C), F.conv2d(x * y, g2, groups=C)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mxmy, mx2, my2 = mx * my, mx * mx, my * my
    ssim = ((2.0 * mxmy + C1) * (2.0 * (mxy - mxmy) + C2)) / ((mx2 + my2 + C1) * ((mxx - mx2) + (myy - my2) + C2))
    return torch.stack([mse, mse.sqrt(), psnr, ssim.flatten(1).mean(1)], 1)


def count_launches(fn):
    """Kernel launches of one call (device events of torch.profiler that are neither copies nor memsets)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len([n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()])


def measure(a):
    import torch
    from genesis_amd.image_quality import ImageQuality, gaussian_window, image_quality
    B, C, L = 32, 3, 1.0
    res = {'B': B, 'C': C, 'win_size': 11, 'sigma': 1.5, 'calls': a.calls, 'rounds': a.rounds,
           'timing': 'wall clock around `calls` calls ended by one synchronize; variants alternate in every round; median (min, max) us',
           'shapes': {}}
    try:
        with open(os.path.join(REPO, 'profiles', 'eval_time.json')) as f:
            ev = json.load(f)['evaluation_10_batches']['evaluation_ms']
        res['evaluation_per_batch_us_from_eval_time_json'] = 1e3 * min(ev) / 10
    except (OSError, KeyError, ValueError) as e:
        res['evaluation_per_batch_us_from_eval_time_json'] = None
        print('eval_time.json not read: %s' % e, flush=True)
    g = gaussian_window()
    fns = {}
    for S in (64, 128):
        gen = torch.Generator().manual_seed(S)
        target = torch.rand(B, C, S, S, generator=gen)
        pred = (target + 0.1 * torch.randn(B, C, S, S, generator=gen)).clamp(0, 1).cuda()
        target = target.cuda()
        iq = ImageQuality()
        w64 = torch.from_numpy(g[:, None] * g[None, :]).cuda().expand(C, 1, 11, 11).contiguous()
        w32 = w64.float()
        variants = {'update': lambda iq=iq, p=pred, t=target: iq.update(p, t),
                    'torch_fp64': lambda p=pred, t=target, w=w64: torch_rows(p, t, w, L, torch.float64),
                    'torch_fp32': lambda p=pred, t=target, w=w32: torch_rows(p, t, w, L, torch.float32)}
        entry = {}
        rows = image_quality(pred, target)
        for name, dtype, w in (('torch_fp64', torch.float64, w64), ('torch_fp32', torch.float32, w32)):
            diff = (torch_rows(pred, target, w, L, dtype).double() - rows).abs().max(0).values.tolist()
            entry['max_abs_diff_%s_vs_update' % name] = dict(zip(('mse', 'rmse', 'psnr', 'ssim'), diff))
        for fn in variants.values():      # warm-up: code objects, library algorithm choices, the allocator
            for _ in range(5):
                fn()
        one = {name: wall(fn, 3) for name, fn in variants.items()}
        calls = {name: max(5, min(a.calls, int(0.5 / max(t, 1e-7)))) for name, t in one.items()}      # <= 0.5 s a window
        times = {name: [] for name in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                times[name].append(1e6 * wall(fn, calls[name]))
        for name, v in times.items():
            entry[name + '_us'] = {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'calls_per_window': calls[name]}
        entry['torch_fp64_over_update'] = entry['torch_fp64_us']['median'] / entry['update_us']['median']
        entry['torch_fp32_over_update'] = entry['torch_fp32_us']['median'] / entry['update_us']['median']
        res['shapes']['%dx%dx%d' % (C, S, S)] = entry
        fns[S] = variants
        print(S, json.dumps(entry), flush=True)

    def dump():
        if a.json:
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)
    dump()                                     # the times are kept whatever the launch count below does
    for S, variants in fns.items():
        entry = res['shapes']['%dx%dx%d' % (C, S, S)]
        entry['launches_per_call'] = {name: count_launches(fn) for name, fn in variants.items()}
        print(S, 'launches', entry['launches_per_call'], flush=True)
    dump()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--limit', type=int, default=300, help='seconds the measuring child may take')
    ap.add_argument('--json', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--calls', str(a.calls), '--rounds', str(a.rounds)]
    if a.json:
        cmd += ['--json', a.json]
    try:
        rc = subprocess.run(cmd, timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit('image_quality_time: the measurement did not finish within %d s; not repeated' % a.limit)
    if rc != 0:
        raise SystemExit('image_quality_time: the measurement ended with status %d; not repeated' % rc)


if __name__ == '__main__':
    main()
