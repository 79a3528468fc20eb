"""What the last hop of logging costs with genesis_amd.tbwriter, on the metric configuration's model (GENESIS-V2, K = 7, 64 x 64) at
B = 8, in one run:

  pictures  one logging event of visualise_outputs (55 pictures) into a SummaryWriter, three ways that alternate inside a round:
            'device_pack'  the writer as it is: the atlas stays on the device, one gx_png_pack launch and one copy of bytes per atlas;
            'host_pack'    the path before the writer had add_images_device: the fp32 atlas is fetched and the same writer packs
                           the pictures on the host (the same bytes for the same pictures: tests/test_tbwriter_gpu.py; sample() draws
                           anew in every call, so the two files of this run differ in their sampled pictures);
            'model_only'   the forward pass and sample() alone, which both contain.
            Per event: wall time between two synchronisations (median of `--reps` after `--warmup`), bytes copied device to host,
            bytes appended to the file, and -- computed once, outside the timing -- the file bytes with filter type 0 forced for
            every row, so that what the row heuristic buys is known, and the host's time for deflating and framing the event's
            streams alone (zlib level 6), with and without the heuristic.
  scalars   one heartbeat's scalars (train.py:290-311 with K = 7: 28 one-element device tensors derived from the step's output)
            with a TrainStep graph replay queued in front, two ways: 'float_per_scalar' reads every tensor with float() and logs
            the number, which is what tensorboardX's add_scalar does; 'snapshot' hands the device tensors to add_scalar.  The time
            is the host's, from before the first call to the return of the last (the replay is still running when 'snapshot'
            returns: that is the point); 'snapshot_flush' is the later flush() with its one copy, after the step has finished.

Times need the device: the script fails without one.
Usage: python tools/tbwriter_time.py [--reps 20] [--warmup 3] [--json path]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, K, SIZE = 8, 7, 64


class HostPath(object):
    """A SummaryWriter seen through add_image alone, as visualise_outputs saw every writer before add_images_device: it is handed
    host views of the fetched fp32 atlas.  Counts the bytes of that fetch (the views' fp32 words; colour grids arrive as int64
    conversions of fp32 views) and keeps the arrays of the last event."""

    def __init__(self, writer):
        self.writer, self.fetched, self.arrays = writer, 0, []

    def add_image(self, tag, array, step):
        self.fetched += 4 * array.numel()
        self.arrays.append(array)
        self.writer.add_image(tag, array, step)


def build():
    import torch
    from genesis_amd import testing as T
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
    return model, batch


def summary(times):
    return {'median_ms': statistics.median(times), 'min_ms': min(times), 'max_ms': max(times)}


def pictures(model, batch, tmp, a):
    import torch
    from genesis_amd import tbwriter
    from genesis_amd import visualise as vis
    palette = [[(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256] for i in range(15)]
    dev = tbwriter.SummaryWriter(os.path.join(tmp, 'device'), device_pack=True)
    host = HostPath(tbwriter.SummaryWriter(os.path.join(tmp, 'host'), device_pack=False))

    def model_only():
        model.eval()
        model(batch['input'][:8])
        model.sample(batch_size=8, K_steps=model.K_steps)
        model.train()

    fns = {'device_pack': lambda: vis.visualise_outputs(model, batch, dev, 'val', 1, palette=palette),
           'host_pack': lambda: vis.visualise_outputs(model, batch, host, 'val', 1, palette=palette),
           'model_only': model_only}
    times = {name: [] for name in fns}
    with torch.no_grad():
        for name, fn in fns.items():
            for _ in range(a.warmup):
                fn()
        counters = {'device_pack': dict(dev.stats), 'host_pack': dict(host.writer.stats, fetched=host.fetched)}
        for _ in range(a.reps):
            for name, fn in fns.items():
                if name == 'host_pack':
                    host.arrays = []      # (keeps the arrays of the last event only)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0))
    res = {name: summary(t) for name, t in times.items()}
    d, h = counters['device_pack'], counters['host_pack']
    res['device_pack'].update(
        pictures_per_event=(dev.stats['events'] - d['events']) // a.reps,
        pack_launches_per_event=(dev.stats['pack_launches'] - d['pack_launches']) // a.reps,
        # (the writer's copies, and the 4-byte overflow count visualise_outputs reads per atlas)
        d2h_copies_per_event=(dev.stats['d2h_copies'] - d['d2h_copies'] + dev.stats['pack_launches'] - d['pack_launches']) // a.reps,
        d2h_bytes_per_event=(dev.stats['d2h_bytes'] - d['d2h_bytes']) // a.reps + 4 * (dev.stats['pack_launches'] - d['pack_launches']) // a.reps,
        file_bytes_per_event=(dev.stats['file_bytes'] - d['file_bytes']) // a.reps)
    res['host_pack'].update(
        pictures_per_event=(host.writer.stats['events'] - h['events']) // a.reps,
        d2h_bytes_per_event=(host.fetched - h['fetched']) // a.reps + 4 * res['device_pack']['pack_launches_per_event'],
        file_bytes_per_event=(host.writer.stats['file_bytes'] - h['file_bytes']) // a.reps)
    # the same event with filter type 0 in every row: the PNGs alone change
    # ... and where the host's time goes: deflating and framing the event's streams (zlib level 6), timed alone
    chosen = forced = 0
    deflate = {'row_heuristic': 0.0, 'filter_0_forced': 0.0}
    assert len(host.arrays) == res['host_pack']['pictures_per_event']
    for array in host.arrays:
        u8 = tbwriter._quantise_host(array.numpy(), 'CHW')
        H, W, C = u8.shape
        for key, stream in (('row_heuristic', tbwriter.pack_rows_host(u8)), ('filter_0_forced', tbwriter.pack_rows_host(u8, force_filter=0))):
            t0 = time.perf_counter()
            size = len(tbwriter._png(stream, H, W, C, 6))
            deflate[key] += 1e3 * (time.perf_counter() - t0)
            if key == 'row_heuristic':
                chosen += size
            else:
                forced += size
    res['png_bytes_per_event'] = {'row_heuristic': chosen, 'filter_0_forced': forced}
    res['host_deflate_ms_per_event'] = deflate
    res['file_bytes_per_event_filter_0_forced'] = res['host_pack']['file_bytes_per_event'] - chosen + forced
    for name in ('device_pack', 'host_pack'):
        res[name]['median_ms_beyond_model'] = res[name]['median_ms'] - res['model_only']['median_ms']
    dev.close()
    host.writer.close()
    return res


def heartbeat_values(out, n):
    """n one-element device tensors derived from the step's output, as the loop derives its scalars (err / num_elements, ...)."""
    return [out[i % out.numel()] * (1.0 + i) for i in range(n)]


def scalars(model, batch, tmp, a):
    import torch
    from genesis_amd import tbwriter
    from genesis_amd.trainer import TrainStep
    n = 14 + 2 * K
    step = TrainStep(model, SIZE, graph=True)
    x = batch['input']
    for _ in range(a.warmup + 1):      # (the first call captures the graph)
        step.step(x)
    torch.cuda.synchronize()
    writers = {name: tbwriter.SummaryWriter(os.path.join(tmp, name)) for name in ('float_per_scalar', 'snapshot')}
    times = {'float_per_scalar': [], 'snapshot': [], 'snapshot_flush': [], 'step_alone': []}
    for it in range(a.warmup + a.reps):
        for name, w in writers.items():
            torch.cuda.synchronize()
            values = heartbeat_values(step.step(x), n)      # the replay and the derivations are queued, not finished
            t0 = time.perf_counter()
            if name == 'snapshot':
                for i, v in enumerate(values):
                    w.add_scalar('train/s%d' % i, v, it)
            else:
                for i, v in enumerate(values):
                    w.add_scalar('train/s%d' % i, float(v), it)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            w.flush()
            t3 = time.perf_counter()
            if it >= a.warmup:
                times[name].append(1e3 * (t1 - t0))
                if name == 'snapshot':
                    times['snapshot_flush'].append(1e3 * (t3 - t2))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step.step(x)
        torch.cuda.synchronize()
        if it >= a.warmup:
            times['step_alone'].append(1e3 * (time.perf_counter() - t0))
    res = {name: summary(t) for name, t in times.items()}
    res['scalars_per_heartbeat'] = n
    s = writers['snapshot'].stats
    res['snapshot'].update(snapshot_launches_per_heartbeat=s['snapshot_launches'] // (a.warmup + a.reps),
                           d2h_copies_per_heartbeat=s['d2h_copies'] // (a.warmup + a.reps))
    res['float_per_scalar']['blocking_reads_per_heartbeat'] = n
    for w in writers.values():
        w.close()
    step.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('tbwriter_time: no HIP device; times are not taken on the host')
    tmp = tempfile.mkdtemp(prefix='tbwriter_time_')
    try:
        model, batch = build()
        res = {'shape': dict(B=B, K=K, H=SIZE, W=SIZE), 'reps': a.reps, 'warmup': a.warmup}
        res['pictures'] = pictures(model, batch, tmp, a)
        print('pictures', res['pictures'], flush=True)
        res['scalars'] = scalars(model, batch, tmp, a)
        print('scalars', res['scalars'], flush=True)
        print(json.dumps(res), flush=True)
        if a.json:
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
