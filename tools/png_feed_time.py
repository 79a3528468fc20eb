"""Can the PNG loaders feed the training step?  Writes a synthetic ShapeStacks tree (224 x 224 RGB frames with their maps)
once with smooth and once with noisy frames, and a Sketchy tree of 128 x 128 frames, into a temporary folder and prints,
one JSON line each:

    inflate   frames/s of gx_png_inflate on one host thread (and Pillow's full Image.open(...).load() beside it, when
              Pillow is there), per kind of frame
    kernel    microseconds of gx_png_unfilter per batch of 32 (HIP events around back-to-back launches), per kind
    loader    images/s of the config's train loader over one epoch at 1, 4 and 16 reader threads, per kind
    step      images/s of TrainStep on the metric configuration (GENESIS-V2, K = 7, 64 x 64, batch 32), same run
    ratio     per kind, loader images/s at the best thread count <= 16 over the step's images/s

Frames are Pillow-encoded (its adaptive filter choice) when Pillow is installed; otherwise the smooth 224 and the 128 frame
are the streams of tests/golden/png_pil.npz and the noisy one is assembled with the row filters cycling 0..4.

    python tools/png_feed_time.py [--frames 512] [--steps 100] [--json path]"""
import argparse
import io
import json
import os
import os.path as osp
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tests', 'golden'))
import make_golden_png as MG  # noqa: E402

from genesis_amd import png  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

KINDS = ('smooth224', 'noisy224', 'mixed128')


def synthetic_streams():
    g = np.load(MG.NPZ)
    noise = MG.content_image('noise', 224, 224, 3, 4242)
    try:
        import PIL  # noqa: F401
        noisy, origin = MG.pil_encode(noise), 'Pillow (adaptive filters)'
    except ImportError:
        noisy, origin = MG.assemble(noise, MG.row_filters(224, MG.CYCLE)), 'fixture streams; noisy: filters cycling 0..4'
    return {'smooth224': bytes(g['pil_smooth224_png']), 'noisy224': noisy, 'mixed128': bytes(g['pil_mixed128_png']),
            'map': bytes(g['ss_map_png'])}, origin


def time_inflate(stream, seconds=1.0):
    a = np.frombuffer(stream, dtype=np.uint8)
    dst = np.zeros(png.png_info(a).inflated_size, dtype=np.uint8)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(16):
            png.inflate(a, dst)
        n += 16
    return n / (time.perf_counter() - t0)


def time_pillow(stream, seconds=1.0):
    try:
        from PIL import Image
    except ImportError:
        return None
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(16):
            Image.open(io.BytesIO(stream)).load()
        n += 16
    return n / (time.perf_counter() - t0)


def time_kernel(stream, batch=32, iters=100):
    info = png.png_info(stream)
    staging = png.PngStaging(batch, *info.geometry)
    for i in range(batch):
        staging.decode(i, stream)
    dev = staging.buffer.cuda()
    for _ in range(10):
        png.unfilter(dev, batch, batch, staging.geometry)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        png.unfilter(dev, batch, batch, staging.geometry)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def write_shapestacks(folder, frame, mapfile, frames, per_scenario=64):
    scenarios = ['env_synthetic-h=2-vcom=0-vpsf=0-v=%d' % i for i in range(-(-frames // per_scenario))]
    os.makedirs(osp.join(folder, 'splits', 'default'))
    for mode in ('train', 'eval', 'test'):
        with open(osp.join(folder, 'splits', 'default', mode + '.txt'), 'w') as f:
            f.write(''.join(s + '\n' for s in (scenarios if mode == 'train' else scenarios[:1])))
    left = frames
    for s in scenarios:
        os.makedirs(osp.join(folder, 'recordings', s))
        os.makedirs(osp.join(folder, 'iseg', s))
        for cam in range(min(per_scenario, left)):
            with open(osp.join(folder, 'recordings', s, 'rgb-w=0-f=0-l=0-c=unique-cam_%d-mono-0.png' % cam), 'wb') as f:
                f.write(frame)
            with open(osp.join(folder, 'iseg', s, 'iseg-w=0-f=0-l=0-c=original-cam_%d-mono-0.map' % cam), 'wb') as f:
                f.write(mapfile)
        left -= per_scenario


def write_sketchy(folder, frame, frames, per_episode=64):
    for mode, n in (('train', frames), ('valid', 1), ('test', 1)):
        for e in range(-(-n // per_episode)):
            os.makedirs(osp.join(folder, 'processed', mode, 'ep%d' % e))
            for i in range(min(per_episode, n - e * per_episode)):
                with open(osp.join(folder, 'processed', mode, 'ep%d' % e, 'ep%d_%d.png' % (e, i)), 'wb') as f:
                    f.write(frame)


def time_loader(kind, folder, workers, batch=32):
    if kind == 'mixed128':
        import genesis_amd.sketchy_config as K
        train = K.load(AttrDict(data_folder=folder, img_size=128, num_workers=workers, K_steps=10, batch_size=batch, seed=0,
                                debug=True))[0]
    else:
        import genesis_amd.shapestacks_config as S
        train = S.load(AttrDict(data_folder=folder, split_name='default', img_size=64, shuffle_test=False, num_workers=workers,
                                load_instances=True, copy_to_tmp=False, K_steps=9, batch_size=batch, seed=0, debug=True))[0]
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
    ap.add_argument('--frames', type=int, default=512, help='frames of every synthetic train split')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    results = []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    streams, origin = synthetic_streams()
    report(what='frames', origin=origin, bytes={k: len(streams[k]) for k in KINDS})
    for kind in KINDS:
        report(what='inflate', kind=kind, frames_per_s_per_thread=time_inflate(streams[kind]),
               pillow_full_decode_per_s_per_thread=time_pillow(streams[kind]))
    for kind in KINDS:
        report(what='kernel', kind=kind, us_per_batch_of_32=time_kernel(streams[kind]))
    best = {}
    for kind in KINDS:
        with tempfile.TemporaryDirectory() as folder:
            if kind == 'mixed128':
                write_sketchy(folder, streams[kind], args.frames)
            else:
                write_shapestacks(folder, streams[kind], streams['map'], args.frames)
            for workers in (1, 4, 16):
                rate, n = time_loader(kind, folder, workers)
                best[kind] = max(best.get(kind, 0.0), rate)
                report(what='loader', kind=kind, threads=workers, images_per_s=rate, images=n,
                       instances=kind != 'mixed128')
    step = time_step(args.steps)
    report(what='step', images_per_s=step, config='GENESIS-V2 K=7 64x64 feat_dim 64 batch 32, HIP graph')
    for kind in KINDS:
        report(what='ratio', kind=kind, loader_over_step=best[kind] / step)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
