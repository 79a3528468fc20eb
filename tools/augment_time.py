"""What does augmenting a resident batch cost?  One launch of gx_cache_gather_aug (genesis_amd/augment.py: flip, crop,
brightness and colour all on, with labels) against the pair it replaces, gx_cache_gather_f32 + gx_cache_gather_labels, on the
same stores and the same index vector: B = 32, frames of 3 x 64 x 64 and 3 x 128 x 128, a store of `--rows` random frames.
Prints one JSON line per shape with microseconds per BATCH, medians over `--repeats` alternating windows of `--calls` batches:

    eager      device events around `--calls` calls from Python, output allocation included: what a loader's consumer
               sees; at these sizes it is the host's launch rate rather than the kernels
    graph      the same calls captured once in a HIP graph and replayed: the device's time for the launches back to back

Kernel times proper come from a profiler run of this script (rocprofv3 --kernel-trace --stats -- python tools/augment_time.py).
Needs a GPU.

    python tools/augment_time.py [--rows 2048] [--calls 200] [--repeats 5] [--json profiles/augment_time.json]"""
import argparse
import json
import os.path as osp
import statistics
import sys

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

from genesis_amd import augment, data_cache  # noqa: E402

BATCH = 32
SHAPES = ((3, 64, 64), (3, 128, 128))


def window_us(run, calls):
    """Microseconds per call of run(i), i < calls, between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        run(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls


def captured(run, calls):
    """run(0 .. calls) captured in one graph -> a function of i that replays all of them (to be timed with calls = 1)."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(calls):
            run(i)
    return lambda _: graph.replay()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2048)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('augment_time: needs a GPU; there is nothing to measure without one')
    if args.rows < BATCH:
        raise SystemExit('augment_time: --rows must be at least %d' % BATCH)
    aug = augment.Augment(flip=0.5, min_side=0.4, brightness=0.3, colour=0.2, seed=1)
    rng = np.random.RandomState(0)
    results = []
    for shape in SHAPES:
        C, H, W = shape
        frames = data_cache.new_store(args.rows, C * H * W, 'cuda')
        labels = data_cache.new_store(args.rows, 2 * H * W, 'cuda')
        frames.copy_(torch.from_numpy(rng.randint(0, 256, size=tuple(frames.shape)).astype(np.uint8)))
        labels.copy_(torch.from_numpy(rng.randint(0, 8, size=tuple(labels.shape)).astype(np.uint8)))
        idx = torch.from_numpy(rng.permutation(args.rows).astype(np.int64)).cuda()
        batches = args.rows // BATCH

        def one(i):
            return augment.gather(frames, labels, shape, aug, 1, idx, (i % batches) * BATCH, BATCH)

        def pair(i):
            first = (i % batches) * BATCH
            return (data_cache.gather_frames(frames, shape, idx, first, BATCH),
                    data_cache.gather_labels(labels, (H, W), idx, first, BATCH))

        runs = {'aug': one, 'pair': pair}
        for run in runs.values():                                  # warm: code objects, the allocator's blocks
            window_us(run, args.calls)
        graphs = {name: captured(run, args.calls) for name, run in runs.items()}
        for g in graphs.values():
            window_us(g, 1)
        eager = {name: [] for name in runs}
        graph = {name: [] for name in runs}
        for _ in range(args.repeats):                              # alternating, so that drift lands on both
            for name in runs:
                eager[name].append(window_us(runs[name], args.calls))
                graph[name].append(window_us(graphs[name], 1) / args.calls)
        line = dict(what='augment_time', shape=list(shape), batch=BATCH, rows=args.rows, calls=args.calls, labels=True,
                    augment=repr(aug), bytes_written=BATCH * H * W * (4 * C + 8))
        for kind, table in (('eager', eager), ('graph', graph)):
            for name in runs:
                line['%s_%s_us' % (kind, name)] = dict(median=statistics.median(table[name]), min=min(table[name]),
                                                       max=max(table[name]))
            line['%s_aug_over_pair' % kind] = line['%s_aug_us' % kind]['median'] / line['%s_pair_us' % kind]['median']
        results.append(line)
        print(json.dumps(line), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
