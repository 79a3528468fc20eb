"""Can the Multi-dSprites loaders feed the training step?  Generates a synthetic split with genesis_amd.generate_multid on a
procedural sprite bank (tests/multid_bank.py), stores it as the generator does (float32 frames, float64 masks) in a temporary
folder and prints, one JSON line each:

    generate  images/s of generate() (host draws + gx_sprites_compose + copies back), sprites from an ndarray
    upload    seconds and GB/s to make the training split resident (frames, then masks narrowed to uint8 on the way)
    loader    images/s of the config's train loader over one epoch, resident and mem_map, batch 32, with instances
    step      images/s of TrainStep on the metric configuration (GENESIS-V2, K = 7, 64 x 64, batch 32), same run
    fed       images/s of that TrainStep when every batch comes from the loader, per mode
    ratio     per mode, loader images/s over the step's images/s

    python tools/multid_feed_time.py [--frames 50000] [--steps 100] [--json path]"""
import argparse
import json
import os.path as osp
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tests'))
import multid_bank  # noqa: E402

from genesis_amd.compat.attrdict import AttrDict  # noqa: E402

MODES = (('resident', False), ('mem_map', True))


def data_cfg(folder, mem_map, batch=32):
    return AttrDict(data_folder=folder, unique_colours=False, load_instances=True, img_size=64, num_workers=4, mem_map=mem_map,
                    K_steps=5, batch_size=batch, seed=0, debug=True)


def write_splits(folder, frames, sprites):
    import genesis_amd.generate_multid as G
    import genesis_amd.multid_config as M
    G.MAX_SPRITE_INDEX = len(sprites) - 1
    random.seed(0)
    G.generate(sprites, 256)                                    # allocations and the first launch
    t0 = time.perf_counter()
    images, masks = G.generate(sprites, frames)
    rate = frames / (time.perf_counter() - t0)
    for mode, n in zip(M.MODES, (frames, 64, 64)):
        path = osp.join(folder, M.file_name(mode, False))
        np.save(path, images[:n])
        np.save(M.mask_path(path), masks[:n])
    return rate, images.nbytes + masks.nbytes


def time_upload(folder):
    import genesis_amd.multid_config as M
    path = osp.join(folder, M.file_name('training', False))
    M.MultidLoader(path, 32).close()                            # the files into the page cache, the allocator warmed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loader = M.MultidLoader(path, 32)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    stored = loader.frames.nbytes + loader.masks.nbytes
    held = loader.dev_frames.numel() * loader.dev_frames.element_size() + loader.dev_masks.numel() * loader.dev_masks.element_size()
    loader.close()
    return dt, stored, held


def time_loader(train):
    rates = []
    for _ in range(2):                                          # the first epoch allocates (the ring, the batches)
        n, t0 = 0, time.perf_counter()
        for b in train:
            n += len(b['input'])
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    return rates[-1], n


def make_step(batch=32):
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
    return ts, batches


def time_step(ts, batches, steps):
    t0 = time.perf_counter()
    for i in range(steps):
        ts.step(batches[i % 4])
    torch.cuda.synchronize()
    return len(batches[0]) * steps / (time.perf_counter() - t0)


def time_fed(ts, train, steps):
    """The step fed by the loader: whole batches only (the graph is captured at one batch size), epochs as they come."""
    def batches():
        while True:
            for b in train:
                if len(b['input']) == train.batch_size:
                    yield b['input']
    it = batches()
    for _ in range(20):
        ts.step(next(it))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(next(it))
    torch.cuda.synchronize()
    return train.batch_size * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50000, help='frames of the synthetic training split')
    ap.add_argument('--sprites', type=int, default=4096, help='sprites of the synthetic bank')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    results = []

    def report(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    import genesis_amd.multid_config as M
    sprites = multid_bank.first_sprites(args.sprites)
    with tempfile.TemporaryDirectory() as folder:
        rate, nbytes = write_splits(folder, args.frames, sprites)
        report(what='generate', images_per_s=rate, images=args.frames, sprites_in_bank=args.sprites, output_bytes=nbytes)
        dt, stored, held = time_upload(folder)
        report(what='upload', seconds=dt, frames=args.frames, stored_bytes=stored, resident_bytes=held, stored_gb_per_s=stored / dt / 1e9)
        ts, batches = make_step()
        step = time_step(ts, batches, args.steps)
        report(what='step', images_per_s=step, config='GENESIS-V2 K=7 64x64 feat_dim 64 batch 32, HIP graph')
        for name, mem_map in MODES:
            train = M.load(data_cfg(folder, mem_map))[0]
            loader_rate, n = time_loader(train)
            report(what='loader', mode=name, images_per_s=loader_rate, images=n, instances=True, batch=32)
            fed = time_fed(ts, train, args.steps)
            report(what='fed', mode=name, images_per_s=fed, fed_over_resident_input=fed / step)
            report(what='ratio', mode=name, loader_over_step=loader_rate / step)
            train.close()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
