"""How fast the multi-object TFRecord loader (genesis_amd/multi_object_config.py) feeds a training step.

Writes a synthetic GZIP TFRecord file of each dataset's geometry (ObjectsRoom, Multi-dSprites, Tetrominoes, CLEVR with
masks: one byte per bytes_list value, as the real files) to a temporary directory and measures
  reader      host records/s of the reader alone, no GPU: 'scan' = inflate + framing + both CRCs, 'decode' = that plus
              the tf.Example walk and the unpacking into uint8 batches (HostBatches, file order), 'shuffled' = through
              the shuffle pool
  end_to_end  images/s of load(cfg)'s train loader driving TrainStep.step over whole epochs, against the same steps on a
              resident batch (the rate the step alone sustains)
  kernel      gx_entity_masks_to_labels on one batch: bytes moved (mask bytes of the entities read + int64 written) and
              HIP-event time per launch; kernel time without launch gaps comes from
                  rocprofv3 --kernel-trace --stats --output-format csv -d OUTDIR -o mof -- \\
                      python tools/multi_object_feed_time.py --kernel-only
              whose *_kernel_stats.csv --rocprof-csv merges into the JSON.
A single GZIP stream is inflated by one thread, so expect the reader, not the GPU, to bound CLEVR.  The host numbers
belong to whatever CPU runs the script.  Synthetic frames (flat rectangles plus noise) inflate at their own rate; real files
will differ.
Usage: python tools/multi_object_feed_time.py [--datasets a,b] [--records N] [--batch B] [--epochs N] [--no-device]
           [--kernel-only] [--rocprof-csv path] [--json profiles/multi_object_feed_time.json]"""
import argparse
import csv
import json
import os
import struct
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def varint(v):
    out = bytearray()
    while True:
        out.append((v & 0x7f) | (0x80 if v > 0x7f else 0))
        v >>= 7
        if not v:
            return bytes(out)


def ld(field, payload):
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def one_byte_values(a):
    w = np.empty((a.size, 3), dtype=np.uint8)
    w[:, 0], w[:, 1], w[:, 2] = 0x0A, 0x01, a.reshape(-1)
    return w.tobytes()


def synth_record(rng, frame, entities, layout):
    H, W = frame
    image = np.empty((H, W, 3), dtype=np.uint8)
    image[:] = rng.randint(0, 256, 3)
    mask = np.zeros((entities, H, W), dtype=np.uint8)
    mask[0] = 255
    for o in range(1, entities):
        y0, x0, h, w = rng.randint(0, H // 2), rng.randint(0, W // 2), rng.randint(4, H // 2), rng.randint(4, W // 2)
        image[y0:y0 + h, x0:x0 + w] = rng.randint(0, 256, 3)
        mask[:o, y0:y0 + h, x0:x0 + w] = 0
        mask[o, y0:y0 + h, x0:x0 + w] = 255
    image = (image.astype(np.int16) + rng.randint(-6, 7, image.shape)).clip(0, 255).astype(np.uint8)     # sensor-like noise
    if layout == 'hwe':
        mask = np.ascontiguousarray(mask.transpose(1, 2, 0))
    feats = {'image': ld(1, one_byte_values(image)), 'mask': ld(1, one_byte_values(mask)),
             'x': ld(2, ld(1, rng.rand(entities).astype('<f4').tobytes()))}
    return ld(1, b''.join(ld(1, ld(1, k.encode()) + ld(2, v)) for k, v in feats.items()))


def write_file(path, d, records, seed=0):
    from genesis_amd import tfrecord
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    z = zlib.compressobj(6, zlib.DEFLATED, 16 + zlib.MAX_WBITS)
    raw = 0
    with open(path, 'wb') as f:
        for _ in range(records):
            data = synth_record(rng, d['frame'], d['entities'], d['layout'])
            head = struct.pack('<Q', len(data))
            rec = head + struct.pack('<I', tfrecord.masked_crc32c(head)) + data + struct.pack('<I', tfrecord.masked_crc32c(data))
            raw += len(rec)
            f.write(z.compress(rec))
        f.write(z.flush())
    return raw, os.path.getsize(path)


def make_cfg(folder, dataset, batch, records):
    from genesis_amd.compat.attrdict import AttrDict
    return AttrDict(data_folder=folder, dataset=dataset, img_size=-1, dataset_size=records, num_workers=4, buffer_size=128,
                    K_steps=-1, batch_size=batch, seed=0, debug=True)


def reader_rates(path, cfg, records):
    import genesis_amd.multi_object_config as M
    from genesis_amd import tfrecord
    out = {}
    t = time.perf_counter()
    n = sum(1 for _ in tfrecord.TFRecordReader(path))
    out['scan_records_per_s'] = n / (time.perf_counter() - t)
    for key, shuffle in (('decode_records_per_s', False), ('shuffled_records_per_s', True)):
        (train, _, _), _ = M.host_splits(cfg, val_size=0, test_size=0, shuffle=shuffle)
        t = time.perf_counter()
        n = sum(len(b['index']) for b in train)
        out[key] = n / (time.perf_counter() - t)
        assert n == records
    return out


def end_to_end(cfg, records, epochs):
    import genesis_amd.genesisv2_config as G
    import genesis_amd.multi_object_config as M
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd.trainer import TrainStep
    from forge import flags
    train = M.load(cfg, val_size=0, test_size=0)[0]
    mcfg = AttrDict(dict(flags.FLAGS))
    mcfg.update(dict(cfg, debug=False, multi_gpu=False))
    torch.manual_seed(0)
    model = G.load(mcfg).to('cuda:0').train()
    ts = TrainStep(model, cfg.img_size)
    steps = images = 0
    resident = None
    for e in range(epochs + 1):                     # the first epoch warms up (allocations, weight cache)
        if e == 1:
            torch.cuda.synchronize()
            t = time.perf_counter()
            steps = images = 0
        for batch in train:
            if batch['input'].shape[0] != cfg.batch_size:
                continue
            resident = batch['input']
            ts.step(resident)
            steps += 1
            images += resident.shape[0]
    torch.cuda.synchronize()
    fed = images / (time.perf_counter() - t)
    train.close()
    x = resident.clone()
    for _ in range(5):
        ts.step(x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        ts.step(x)
    torch.cuda.synchronize()
    res = steps * x.shape[0] / (time.perf_counter() - t)
    return {'steps': steps, 'fed_images_per_s': fed, 'resident_images_per_s': res, 'fed_share_of_resident': fed / res,
            'img_size': int(cfg.img_size), 'K_steps': int(cfg.K_steps)}


def kernel_time(d, batch, img_size, iters=200, warmup=20):
    import genesis_amd.multi_object_config as M
    from genesis_amd.feeder import entity_masks_to_labels
    crop, size, S = M.output_size(d['frame'], img_size)
    H, W = d['frame']
    shape = (batch,) + M.mask_shape(d['frame'], d['entities'], d['layout'])
    m = torch.from_numpy(np.random.RandomState(0).choice(np.array([0, 255], dtype=np.uint8), shape)).cuda()
    out = torch.empty(batch, 1, S, S, dtype=torch.int64, device='cuda')
    run = lambda: entity_masks_to_labels(m, d['background_entities'], size, crop, d['layout'], out=out)   # noqa: E731
    for _ in range(warmup):
        run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        run()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / iters
    # a pixel that is sampled reads at most its foreground entities' bytes; every output pixel writes 8
    nbytes = batch * S * S * ((d['entities'] - d['background_entities']) + 8)
    return {'mask_shape': list(shape), 'out': [batch, 1, S, S], 'bytes_upper_bound': nbytes, 'us_per_launch_hip_events': us,
            'bytes_per_s': nbytes / (us * 1e-6)}


def merge_rocprof(results, path):
    rows = [r for r in csv.DictReader(open(path)) if 'entity_masks_to_labels' in r.get('Name', '')]
    results['rocprofv3_kernel_stats'] = [{k: r[k] for k in ('Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'MinNs', 'MaxNs')
                                          if k in r} for r in rows]


def main():
    import genesis_amd.multi_object_config as M
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', default='objects_room,multi_dsprites,tetrominoes,clevr')
    ap.add_argument('--records', type=int, default=0, help='records per file (0: 2048, CLEVR 192)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--no-device', action='store_true')
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--rocprof-csv', default=None)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    results = {}
    if a.json and os.path.exists(a.json):
        results = json.load(open(a.json))
    if a.rocprof_csv:
        merge_rocprof(results, a.rocprof_csv)
    else:
        for name in a.datasets.split(','):
            d = M.DATASETS[name]
            r = results.setdefault(name, {})
            if not a.no_device:
                r['kernel'] = kernel_time(d, a.batch, d['img_size'])
                print(name, 'kernel', r['kernel'], flush=True)
            if a.kernel_only:
                continue
            records = a.records or (192 if name == 'clevr' else 2048)
            with tempfile.TemporaryDirectory() as tmp:
                cfg = make_cfg(tmp, name, a.batch, records)
                raw, packed = write_file(tmp + d['file'], d, records)
                r['file'] = {'records': records, 'raw_bytes': raw, 'gzip_bytes': packed, 'batch_size': a.batch}
                r['reader'] = reader_rates(tmp + d['file'], cfg, records)
                print(name, 'reader', r['reader'], flush=True)
                if not a.no_device:
                    r['end_to_end'] = end_to_end(cfg, records, a.epochs)
                    print(name, 'end_to_end', r['end_to_end'], flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == '__main__':
    main()
