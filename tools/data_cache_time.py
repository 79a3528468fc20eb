"""What does keeping the decoded split on the device (genesis_amd/data_cache.py) buy?  On the mixed folder of
tools/imagefolder_time.py (256 x 256 and 640 x 480 frames, JPEG and PNG), at 64 x 64 and 128 x 128 output, 16 reader threads,
batch 32, prints one JSON line each:

    plain      images/s delivered by image_folder_config's train loader, `--repeats` epochs after one that allocates its ring
    filling    images/s delivered by CachedLoader's filling epoch over the same (warmed) loader: `--repeats` fresh wrappers,
               each timed over its one filling epoch, the store's allocation, the counters' read and the print included
    resident   images/s delivered by resident epochs (each uploads its permutation), `--repeats` windows of at least
               `--window` seconds
    step       images/s of TrainStep on the metric configuration (GENESIS-V2, K = 7, 64 x 64, batch 32, HIP graph), same run
    driven     images/s of that TrainStep fed from a CachedLoader at 64 x 64: epoch 1 (filling), then resident epochs (windows
               as above)
    check      the two requirements, decided on the medians of this run:
               resident_feeds_step   the resident rate at 64 x 64 exceeds the step's rate
               filling_keeps_up      per size, the filling rate is not below the plain rate by more than the plain loader's
                                     own spread (max - min over its repeats)

Every rate is a host clock around work that ends in a device synchronise.  Needs a GPU and Pillow (to encode the folder).

    python tools/data_cache_time.py [--frames 2050] [--repeats 3] [--steps 100] [--window 0.5] [--json profiles/data_cache_time.json]"""
import argparse
import json
import os.path as osp
import statistics
import sys
import tempfile
import time

import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.dirname(osp.abspath(__file__)))
import imagefolder_time as IT  # noqa: E402

from genesis_amd.compat.attrdict import AttrDict  # noqa: E402
from genesis_amd.data_cache import CachedLoader  # noqa: E402

WORKERS, BATCH = 16, 32


def plain_loader(folder, S):
    import genesis_amd.image_folder_config as F
    return F.load(AttrDict(data_folder=folder, img_size=S, num_workers=WORKERS, K_steps=7, batch_size=BATCH, seed=0, max_side=640))[0]


def epoch_rate(loader, consume=None):
    """images/s of one epoch of `loader`, the device drained at its end; consume(batch) is the work done per batch."""
    n, t0 = 0, time.perf_counter()
    for b in loader:
        n += len(b['input'])
        if consume is not None:
            consume(b['input'])
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0), n


def window_rate(loader, seconds, consume=None):
    """images/s of whole epochs of a resident loader, repeated until `seconds` have passed."""
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for b in loader:
            n += len(b['input'])
            if consume is not None:
                consume(b['input'])
        torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def make_step():
    import genesis_amd.genesisv2_config as G
    from genesis_amd.trainer import TrainStep
    cfg = AttrDict(K_steps=7, img_size=64, feat_dim=64, kernel='gaussian', semiconv=True, dynamic_K=False, klm_loss=False,
                   detach_mr_in_klm=True, pixel_bound=True, autoreg_prior=True, pixel_std1=0.7, pixel_std2=0.7, debug=False,
                   multi_gpu=False)
    torch.manual_seed(0)
    ts = TrainStep(G.load(cfg).to('cuda').train(), 64, lr=1e-4, graph=True)
    g = torch.Generator().manual_seed(1234)
    batches = [torch.rand(BATCH, 3, 64, 64, generator=g).cuda() for _ in range(4)]
    ts.prepare(batches[0])
    for i in range(40):
        ts.step(batches[i % 4])
    torch.cuda.synchronize()
    return ts, batches


def step_rate(ts, batches, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ts.step(batches[i % 4])
    torch.cuda.synchronize()
    return BATCH * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2050, help='files of the synthetic folder (two go to val and test)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of each resident window')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('data_cache_time: needs a GPU; there is nothing to measure without one')
    if (args.frames - 2) % BATCH:
        raise SystemExit('data_cache_time: --frames minus 2 must be a multiple of %d (the graph step takes whole batches)' % BATCH)
    results = []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    median = statistics.median
    rates = {}
    with tempfile.TemporaryDirectory() as folder:
        IT.write_folder(folder, IT.synthetic_streams(), IT.KINDS, args.frames)
        for S in (64, 128):
            plain, filling, resident = [], [], []
            for _ in range(args.repeats):               # alternating: a plain epoch and a filling epoch of the same warmed loader
                loader = plain_loader(folder, S)
                epoch_rate(loader)                      # allocates the pinned ring, starts the threads
                plain.append(epoch_rate(loader)[0])
                wrapped = CachedLoader(loader, shuffle=True, name='mixed %d' % S)
                rate, n = epoch_rate(wrapped)
                filling.append(rate)
                if wrapped.cache_state != 'resident':
                    raise SystemExit('data_cache_time: %s' % wrapped.cache_state)
                window_rate(wrapped, 0.1)               # warm: the gather's code object, the allocator's blocks
                resident.append(window_rate(wrapped, args.window))
                wrapped.close()
            rates[S] = dict(plain=median(plain), filling=median(filling), resident=median(resident), spread=max(plain) - min(plain))
            report(what='plain', img_size=S, threads=WORKERS, images=n, images_per_s=plain, median=rates[S]['plain'],
                   spread=rates[S]['spread'])
            report(what='filling', img_size=S, threads=WORKERS, images=n, images_per_s=filling, median=rates[S]['filling'])
            report(what='resident', img_size=S, images=n, images_per_s=resident, median=rates[S]['resident'])
        ts, batches = make_step()
        steps = [step_rate(ts, batches, args.steps) for _ in range(args.repeats)]
        step = median(steps)
        report(what='step', images_per_s=steps, median=step, config='GENESIS-V2 K=7 64x64 feat_dim 64 batch 32, HIP graph')
        loader = plain_loader(folder, 64)
        epoch_rate(loader)                              # as above: the filling epoch runs over a warmed loader
        wrapped = CachedLoader(loader, shuffle=True, name='mixed 64, driven')
        first = epoch_rate(wrapped, ts.step)[0]
        second = [window_rate(wrapped, args.window, ts.step) for _ in range(args.repeats)]
        report(what='driven', img_size=64, epoch_1_filling=first, epoch_2_resident=second, median_epoch_2=median(second),
               state=wrapped.cache_state)
        wrapped.close()
    report(what='check',
           resident_over_step=rates[64]['resident'] / step, resident_feeds_step=bool(rates[64]['resident'] > step),
           filling_over_plain={str(S): rates[S]['filling'] / rates[S]['plain'] for S in rates},
           filling_keeps_up={str(S): bool(rates[S]['filling'] >= rates[S]['plain'] - rates[S]['spread']) for S in rates})
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
