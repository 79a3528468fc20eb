"""Can the GQN loader feed the training step?  Writes synthetic GQN-shaped TFRecord files (ten 64 x 64 4:2:0 JPEG frames
of quality 95 per record, as TensorFlow's encode_jpeg defaults give) into a temporary folder and prints, one JSON line each:

    entropy   frames/s of gx_jpeg_entropy_decode on one host thread (and Pillow's full decode beside it, when Pillow is there)
    kernel    microseconds of gx_jpeg_decode_f32chw per batch of 32 (HIP events)
    loader    images/s of genesis_amd.gqn_config's train loader over one epoch at 1, 4 and 16 reader threads
    step      images/s of TrainStep on the metric configuration (GENESIS-V2, K = 7, 64 x 64, batch 32), same run
    ratio     loader images/s at the best thread count <= 16 over the step's images/s

Frames come from Pillow when it is installed, otherwise from the 64 x 64 4:2:0 streams of tests/golden/jpeg_pil.npz.

    python tools/gqn_feed_time.py [--files 16] [--records 600] [--steps 100] [--json path]"""
import argparse
import io
import json
import os.path as osp
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tests', 'golden'))
import make_golden_jpeg as MG  # noqa: E402

from genesis_amd import jpeg  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402


def synthetic_streams(n=64):
    try:
        import PIL  # noqa: F401
    except ImportError:
        g = np.load(MG.NPZ)
        return [bytes(g[name + '_jpeg']) for name in MG.GQN_CASES], 'fixture streams'
    return [MG.encode(MG.content_image('mixed', 64, 64, 100 + i), 2, 95) for i in range(n)], 'Pillow, quality 95, 4:2:0'


def time_entropy(streams, seconds=1.0):
    coef = np.zeros(96 * 64, dtype=np.int16)
    qtab = np.zeros(192, dtype=np.uint16)
    arrays = [np.frombuffer(s, dtype=np.uint8) for s in streams]
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for a in arrays:
            jpeg.entropy_decode(a, coef, qtab)
        n += len(arrays)
    return n / (time.perf_counter() - t0)


def time_pillow(streams, seconds=1.0):
    try:
        from PIL import Image
    except ImportError:
        return None
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for s in streams:
            np.asarray(Image.open(io.BytesIO(s)).convert('RGB'))
        n += len(streams)
    return n / (time.perf_counter() - t0)


def time_kernel(streams, batch=32, iters=200):
    staging = jpeg.JpegStaging(batch, 64, 64, 2)
    for i in range(batch):
        staging.decode(i, streams[i % len(streams)])
    dev = staging.buffer.cuda()
    out = torch.empty(batch, 3, 64, 64, device='cuda')
    for _ in range(20):
        jpeg.decode_staged(dev, batch, batch, staging.geometry, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        jpeg.decode_staged(dev, batch, batch, staging.geometry, out=out)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def time_loader(folder, files, records, workers, batch=32):
    import genesis_amd.gqn_config as Q
    cfg = AttrDict(data_folder=folder, img_size=64, val_frac=files, num_workers=workers, buffer_size=128, K_steps=7,
                   batch_size=batch, seed=0, debug=True)
    train = Q.load(cfg, train_files=files, test_files=1, records_per_file=records)[0]
    rates = []
    for _ in range(2):                          # the first epoch allocates the pinned ring
        n, t0 = 0, time.perf_counter()
        for b in train:
            n += len(b['input'])
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    train.close()
    return rates[-1], n


def time_step(steps, batch=32):
    import genesis_amd.genesisv2_config as G
    from genesis_amd.trainer import TrainStep
    cfg = AttrDict(K_steps=7, img_size=64, feat_dim=64, kernel='gaussian', semiconv=True, dynamic_K=False, klm_loss=False,
                   detach_mr_in_klm=True, pixel_bound=True, autoreg_prior=True, pixel_std1=0.7, pixel_std2=0.7, debug=False,
                   multi_gpu=False)
    torch.manual_seed(0)
    model = G.load(cfg).to('cuda').train()
    ts = TrainStep(model, 64, lr=1e-4, graph=True)
    g = torch.Generator().manual_seed(1234)
    batches = [torch.rand(batch, 3, 64, 64, generator=g).cuda() for _ in range(4)]
    ts.prepare(batches[0])
    for i in range(40):
        ts.step(batches[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        ts.step(batches[i % 4])
    torch.cuda.synchronize()
    return batch * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=16, help='train files written (one of them becomes the validation split)')
    ap.add_argument('--records', type=int, default=600, help='records per file')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import genesis_amd.gqn_config as Q
    results = []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    streams, origin = synthetic_streams()
    report(what='frames', origin=origin, streams=len(streams), mean_bytes=float(np.mean([len(s) for s in streams])))
    report(what='entropy', frames_per_s_per_thread=time_entropy(streams), pillow_full_decode_per_s_per_thread=time_pillow(streams))
    report(what='kernel', us_per_batch_of_32=time_kernel(streams))
    with tempfile.TemporaryDirectory() as folder:
        import os
        for split, n in (('train', args.files), ('test', 1)):
            os.makedirs(osp.join(folder, Q.DATASET, split))
            for fi, path in enumerate(Q.file_list(folder, split, args.files, args.files, 1)):
                rec = [([streams[(fi + 7 * r + f) % len(streams)] for f in range(10)], [0.0] * 50)
                       for r in range(args.records if split == 'train' else 1)]
                MG.write_gqn_tfrecord(path, rec)
        best = 0.0
        for workers in (1, 4, 16):
            rate, n = time_loader(folder, args.files, args.records, workers)
            best = max(best, rate)
            report(what='loader', threads=workers, images_per_s=rate, images=n)
    step = time_step(args.steps)
    report(what='step', images_per_s=step, config='GENESIS-V2 K=7 64x64 feat_dim 64 batch 32, HIP graph')
    report(what='ratio', loader_over_step=best / step)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
