"""Wall time and kernel launches of one picture-logging call, before and after genesis_amd.visualise, on the metric configuration's
model (GENESIS-V2, K = 7, 64 x 64) at B = 8 with a writer that discards what it gets:
  (a) baseline: picture logging as the loop did it until now (the operations of train.py:423-476 and utils/misc.py:82-98, host
      reads included, written here in this project's own words) on the device, with make_grid's layout built from torch ops; its
      writer brings every grid to the host first, as any TensorBoard writer must;
  (b) genesis_amd.visualise.visualise_outputs (two gx_vis_compose launches, two device-to-host copies);
  (c) the forward pass and sample() alone, which both contain.
Times: warm-up calls, then the median of `--reps` single calls, each between two synchronisations (the calls contain host reads, so
event timing alone would flatter (a)).  Launches per call: every variant runs once and twice under `rocprofv3 --kernel-trace` (no
counters) in a process of its own, after one warm-up call; the difference of the two kernel counts is one call's, and the
kernels that visualise_outputs launches beyond (c) are listed by name ('picture_kernels').

Every measurement runs in ONE child process under a time limit; a child that fails or runs out of time ends the script: there is
no second attempt.
Usage: python tools/visualise_time.py [--reps 20] [--warmup 3] [--no-trace] [--limit 300] [--json path]"""
import argparse
import collections
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, K, SIZE = 8, 7, 64
VARIANTS = ('baseline', 'visualise_outputs', 'model_only')


def torch_make_grid(images, nrow=8, padding=2, pad_value=0.0):
    """make_grid's layout with torch ops: one filled canvas, then one copy per image into its cell."""
    import torch
    if images.shape[1] == 1:
        images = torch.cat([images] * 3, 1)
    n, _, H, W = images.shape
    if n == 1:
        return images[0]
    cols = min(nrow, n)
    rows = -(-n // cols)
    canvas = images.new_full((3, rows * (H + padding) + padding, cols * (W + padding) + padding), pad_value)
    for i in range(n):
        top, left = (i // cols) * (H + padding) + padding, (i % cols) * (W + padding) + padding
        canvas[:, top:top + H, left:left + W].copy_(images[i])
    return canvas


def baseline_label_colours(labels, palette):
    """Integer labels [B, 1, H, W] -> int64 [B, 3, H, W] with the operations and host reads of the reference's colour mapper: one
    read of the largest label; then per label up to it a comparison, a read of whether the label occurs at all and, if it does,
    one masked write per colour channel; the three channel planes concatenated at the end."""
    import torch
    planes = [torch.zeros_like(labels) for _ in range(3)]
    for label in range(int(labels.max().item()) + 1):
        here = labels == label
        if bool(here.any()):
            for plane, value in zip(planes, palette[label]):
                plane[here] = value
    return torch.cat(planes, 1)


def baseline_pictures(batch, recon, stats, mode, palette):
    """(tag, images) of the forward pass in logging order, each made only when the caller asks for it: the operations the
    reference runs per picture -- cat + argmax + colour mapping for the segmentations, exp for every log-mask plane."""
    import torch
    yield mode + '_input', batch['input'][:8]
    yield mode + '_recon', recon
    if 'instances' in batch:
        yield mode + '_instances_gt', baseline_label_colours(batch['instances'][:8], palette)
    for field, suffix in (('log_m_k', '_instances'), ('log_m_r_k', '_instances_r')):
        if field in stats:
            winner = torch.argmax(torch.cat(stats[field], 1), 1, True)
            yield mode + suffix, baseline_label_colours(winner, palette)
    for key in ('mx_r_k', 'x_r_k', 'log_m_k', 'log_m_r_k'):
        for k, plane in enumerate(stats[key] if key in stats else ()):
            yield '%s_%s/k%d' % (mode, key, k), plane.exp() if key.startswith('log') else plane


def baseline_sample_pictures(sample, stats):
    yield 'samples', sample
    for key in ('x_k', 'log_m_k', 'mx_k'):
        for k, plane in enumerate(stats[key] if key in stats else ()):
            yield 'gen_%s/k%d' % (key, k), plane.exp() if key.startswith('log') else plane


def baseline_visualise(model, batch, writer, mode, step, palette):
    """Picture logging the way the loop did it until now, in this project's words: eval mode, the forward pass of the first eight
    images, then picture by picture its torch ops, a torch-op make_grid and the writer call (which fetches the grid); the same
    for sample(); train mode again."""
    model.eval()
    recon, _, stats, _, _ = model(batch['input'][:8])
    for tag, images in baseline_pictures(batch, recon, stats, mode, palette):
        writer.add_image(tag, torch_make_grid(images), step)
    sample, sample_stats = model.sample(batch_size=8, K_steps=model.K_steps)
    for tag, images in baseline_sample_pictures(sample, sample_stats):
        writer.add_image(tag, torch_make_grid(images), step)
    model.train()


class DiscardingWriter(object):
    """Brings a device array to the host (what a TensorBoard writer does first) and drops it."""
    calls = 0

    def add_image(self, tag, array, step):
        self.calls += 1
        if array.is_cuda:
            array.cpu()


def setup():
    import torch
    from genesis_amd import testing as T
    from genesis_amd import visualise as vis
    from genesis_amd.compat.attrdict import AttrDict
    import genesis_amd.genesisv2_config as G
    from oracle import v2_oracle as O
    cfg = O.make_cfg(K_steps=K, img_size=SIZE, feat_dim=64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    model = model.to('cuda').train()
    g = torch.Generator().manual_seed(0)
    batch = {'input': torch.rand(B, 3, SIZE, SIZE, generator=g).cuda(),
             'instances': torch.randint(0, 8, (B, 1, SIZE // 4, SIZE // 4), generator=g).repeat_interleave(4, 2)
             .repeat_interleave(4, 3).cuda()}
    palette = [[(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256] for i in range(15)]
    writer = DiscardingWriter()

    def model_only():
        model.eval()
        model(batch['input'][:8])
        model.sample(batch_size=8, K_steps=model.K_steps)
        model.train()

    return {'baseline': lambda: baseline_visualise(model, batch, writer, 'val', 1, palette),
            'visualise_outputs': lambda: vis.visualise_outputs(model, batch, writer, 'val', 1, palette=palette),
            'model_only': model_only}, writer


def measure(a):
    import torch
    fns, writer = setup()
    res = {'shape': dict(B=B, K=K, H=SIZE, W=SIZE), 'reps': a.reps, 'warmup': a.warmup}
    with torch.no_grad():
        for name in VARIANTS:
            for _ in range(a.warmup):
                fns[name]()
            before, times = writer.calls, []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fns[name]()
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            res[name] = {'median_ms': statistics.median(times), 'min_ms': min(times), 'max_ms': max(times),
                         'pictures_per_call': (writer.calls - before) // a.reps}
            print(name, res[name], flush=True)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


def trace_child(a):
    """One warm-up call, then `--trace-calls` calls of one variant: the process rocprofv3 watches."""
    import torch
    fns, _ = setup()
    with torch.no_grad():
        for _ in range(1 + a.trace_calls):
            fns[a.trace_child]()
    torch.cuda.synchronize()


def run_child(cmd, limit, what):
    try:
        rc = subprocess.run(cmd, timeout=limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit('visualise_time: %s did not finish within %d s; not repeated' % (what, limit))
    if rc != 0:
        raise SystemExit('visualise_time: %s ended with status %d; not repeated' % (what, rc))


def kernel_rows(directory):
    """Kernel name -> launches in the trace rocprofv3 left under `directory`."""
    files = glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit('visualise_time: rocprofv3 left no kernel trace in %s' % directory)
    names = collections.Counter()
    for path in files:
        with open(path, newline='') as f:
            names.update(row.get('Kernel_Name', '?') for row in csv.DictReader(f))
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300, help='seconds each child process may take')
    ap.add_argument('--no-trace', action='store_true', help='times only, no rocprofv3 runs')
    ap.add_argument('--json', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--trace-child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--trace-calls', type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    if a.trace_child:
        return trace_child(a)
    me = os.path.abspath(__file__)
    tmp = tempfile.mkdtemp(prefix='visualise_time_')
    try:
        times = os.path.join(tmp, 'times.json')
        run_child([sys.executable, me, '--child', '--reps', str(a.reps), '--warmup', str(a.warmup), '--json', times], a.limit,
                  'the timing run')
        with open(times) as f:
            res = json.load(f)
        if not a.no_trace:
            if shutil.which('rocprofv3') is None:
                raise SystemExit('visualise_time: rocprofv3 is not on the PATH (use --no-trace for the times alone)')
            per_call = {}
            for name in VARIANTS:
                counts = []
                for calls in (1, 2):
                    out = os.path.join(tmp, '%s_%d' % (name, calls))
                    run_child(['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', out, '-o', 'vt', '--', sys.executable, me,
                               '--trace-child', name, '--trace-calls', str(calls)], a.limit, 'the kernel trace of ' + name)
                    counts.append(kernel_rows(out))
                per_call[name] = counts[1] - counts[0]
                res[name]['kernel_launches_per_call'] = sum(per_call[name].values())
                print(name, 'kernel launches per call:', res[name]['kernel_launches_per_call'], flush=True)
            extra = per_call['visualise_outputs'] - per_call['model_only']
            res['visualise_outputs']['picture_kernels'] = {k[:160]: v for k, v in sorted(extra.items())}
            print('picture kernels:', res['visualise_outputs']['picture_kernels'], flush=True)
            for name in VARIANTS[:2]:
                res[name]['kernel_launches_for_pictures'] = (res[name]['kernel_launches_per_call']
                                                             - res['model_only']['kernel_launches_per_call'])
        for name in VARIANTS[:2]:
            res[name]['median_ms_for_pictures'] = res[name]['median_ms'] - res['model_only']['median_ms']
        res['ratio_of_medians'] = res['baseline']['median_ms'] / res['visualise_outputs']['median_ms']
        print(json.dumps(res), flush=True)
        if a.json:
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
