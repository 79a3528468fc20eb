"""Can the image-folder loader feed the training step?  Writes a synthetic folder into a temporary directory -- 256 x 256 and
640 x 480 frames, as JPEG (quality 90, 4:2:0) and as PNG, encoded by Pillow -- and prints, one JSON line each:

    frames    bytes of the four kinds of file
    loader    images/s of genesis_amd.image_folder_config's train loader over one epoch of the mixed folder, at 64 x 64 and
              128 x 128 output with 4 and 16 reader threads (the second epoch: the first allocates the pinned ring)
    kinds     the same at 64 x 64 and 16 threads for a folder of ONE kind of file, which says where the time goes
    pillow    images/s of a Pillow thread pool on the same CPUs and the same mixed folder: open, convert('RGB'), resize
              (BILINEAR), crop, np.asarray -- what a torchvision dataset's workers do, without the batch collation
    step      images/s of TrainStep on the metric configuration (GENESIS-V2, K = 7, 64 x 64, batch 32), same run
    ratio     the loader's best rate at 64 x 64 over the Pillow pool's and over the step's

    python tools/imagefolder_time.py [--frames 512] [--steps 100] [--json path]"""
import argparse
import io
import json
import os
import os.path as osp
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tests', 'golden'))
import make_golden_imagefile as MG  # noqa: E402

from genesis_amd import imagefile  # noqa: E402
from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

KINDS = ('jpeg256', 'jpeg640x480', 'png256', 'png640x480')


def synthetic_streams():
    from PIL import Image
    out = {}
    for i, (W, H) in enumerate(((256, 256), (640, 480))):
        img = MG.content_image('mixed', H, W, 3, 5150 + i)
        tag = '256' if W == 256 else '640x480'
        out['jpeg' + tag] = MG.encode_jpeg(img, 2, 90)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format='PNG')
        out['png' + tag] = buf.getvalue()
    return out


def write_folder(folder, streams, kinds, frames):
    for i in range(frames):
        kind = kinds[i % len(kinds)]
        sub = osp.join(folder, 'train' if i >= 2 else ('val', 'test')[i], 'd%d' % (i % 8))
        os.makedirs(sub, exist_ok=True)
        with open(osp.join(sub, 'f%05d.%s' % (i, 'jpg' if kind.startswith('jpeg') else 'png')), 'wb') as f:
            f.write(streams[kind])


def time_loader(folder, S, workers, batch=32):
    import genesis_amd.image_folder_config as F
    train = F.load(AttrDict(data_folder=folder, img_size=S, num_workers=workers, K_steps=7, batch_size=batch, seed=0,
                            max_side=640))[0]
    rates = []
    for _ in range(2):
        n, t0 = 0, time.perf_counter()
        for b in train:
            n += len(b['input'])
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    train.close()
    return rates[-1], n


def time_pillow(folder, S, workers):
    from PIL import Image
    import genesis_amd.image_folder_config as F
    files = [osp.join(folder, f) for f in F.split_files(folder, 'train')]

    def one(path):
        im = Image.open(path).convert('RGB')
        h2, w2, top, left = imagefile.resize_crop_geometry(im.height, im.width, S)
        return np.asarray(im.resize((w2, h2), Image.BILINEAR).crop((left, top, left + S, top + S)))

    with ThreadPoolExecutor(workers) as pool:
        list(pool.map(one, files[:64]))
        t0 = time.perf_counter()
        n = sum(1 for _ in pool.map(one, files))
        return n / (time.perf_counter() - t0)


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
    ap.add_argument('--frames', type=int, default=512, help='files of the synthetic folder')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    results = []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    streams = synthetic_streams()
    report(what='frames', bytes={k: len(streams[k]) for k in KINDS})
    best = 0.0
    with tempfile.TemporaryDirectory() as folder:
        write_folder(folder, streams, KINDS, args.frames)
        for S in (64, 128):
            for workers in (4, 16):
                rate, n = time_loader(folder, S, workers)
                best = max(best, rate) if S == 64 else best
                report(what='loader', folder='mixed', img_size=S, threads=workers, images_per_s=rate, images=n)
        pillow = {w: time_pillow(folder, 64, w) for w in (4, 16)}
        for w in (4, 16):
            report(what='pillow', folder='mixed', img_size=64, threads=w, images_per_s=pillow[w])
    for kind in KINDS:
        with tempfile.TemporaryDirectory() as folder:
            write_folder(folder, streams, (kind,), args.frames)
            rate, n = time_loader(folder, 64, 16)
            report(what='kinds', folder=kind, img_size=64, threads=16, images_per_s=rate, images=n)
    step = time_step(args.steps)
    report(what='step', images_per_s=step, config='GENESIS-V2 K=7 64x64 feat_dim 64 batch 32, HIP graph')
    report(what='ratio', loader_over_pillow=best / max(pillow.values()), loader_over_step=best / step)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
