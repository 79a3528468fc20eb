"""Device crop + resample (genesis_amd.feeder.transform_frames / transform_labels) against the reference's host path for one
batch of ShapeStacks-shaped frames (B = 64, 224 x 224 x 3, centre crop 196, PIL bilinear to 64 x 64) and one of CLEVR-shaped
frames (B = 64, 240 x 320 x 3, centre crop 192, nearest to 64 x 64).

Device: HIP events around `--iters` back-to-back launches on resident uint8 frames (after `--warmup`), per launch; achieved
bytes/s = (uint8 crop-window bytes read + fp32 bytes written) / time, against HBM.  Host: the reference's per-image transform on
one thread (PIL crop + resize + ToTensor for ShapeStacks, centre crop + fp32 / 255 + nearest F.interpolate for CLEVR),
PNG decode excluded; the host numbers belong to whatever CPU runs the script.  Kernel times without launch gaps: run the
device part alone under rocprofv3, e.g.
    rocprofv3 --kernel-trace --stats -d OUTDIR -o ftt -- python tools/feeder_transform_time.py --no-host
Usage: python tools/feeder_transform_time.py [--iters N] [--warmup N] [--no-host] [--no-device] [--json path]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

HBM_PEAK = 8.0e12          # bytes/s, MI355X spec (~6.3e12 achievable)

SHAPES = [  # name, frames [B, Hs, Ws, C], crop, size, resize
    ('shapestacks', (64, 224, 224, 3), 196, 64, 'bilinear'),
    ('clevr', (64, 240, 320, 3), 192, 64, 'nearest'),
]


def device_time(frames, labels, box, size, resize, iters, warmup):
    from genesis_amd.feeder import transform_frames, transform_labels
    x = torch.from_numpy(frames).cuda()
    lab = torch.from_numpy(labels).cuda()
    out = torch.empty(x.shape[0], x.shape[3], size, size, device='cuda')
    lab_out = torch.empty(x.shape[0], 1, size, size, dtype=torch.int64, device='cuda')
    runs = {'frames': lambda: transform_frames(x, size, crop=box, resize=resize, out=out),
            'labels': lambda: transform_labels(lab, size, crop=box, out=lab_out)}
    nbytes = {'frames': x.shape[0] * box[2] * box[3] * x.shape[3] + out.numel() * 4,
              'labels': lab.shape[0] * box[2] * box[3] * lab.element_size() + lab_out.numel() * 8}
    res = {}
    for what, run in runs.items():
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / iters
        rate = nbytes[what] / (us * 1e-6)
        res[what] = dict(us_per_batch=us, bytes=nbytes[what], bytes_per_s=rate, hbm_peak_share=rate / HBM_PEAK)
    return res


def host_time(name, frames, box, size, reps):
    top, left, h, w = box
    if name == 'shapestacks':
        from PIL import Image
        imgs = [Image.fromarray(f) for f in frames]

        def run():
            ts = []
            for im in imgs:   # transforms.CenterCrop(196), Resize(64) (PIL bilinear), ToTensor()
                r = np.asarray(im.crop((left, top, left + w, top + h)).resize((size, size), Image.BILINEAR))
                ts.append(torch.from_numpy(r.copy()).permute(2, 0, 1).float().div(255))
            return torch.stack(ts)
    else:
        def run():  # multi_object_config.py:181-189 on the batch: centre crop, NCHW fp32 / 255, nearest resize
            x = torch.from_numpy(np.ascontiguousarray(frames[:, top:top + h, left:left + w]))
            return F.interpolate(x.permute(0, 3, 1, 2).float().div(255), size=size)
    run()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-device', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from genesis_amd.feeder import centre_box
    torch.set_num_threads(1)
    results = {}
    for name, shape, crop, size, resize in SHAPES:
        rng = np.random.RandomState(0)
        frames = rng.randint(0, 256, shape).astype(np.uint8)
        labels = rng.randint(0, 7, shape[:3]).astype(np.uint8)
        box = centre_box(shape[1], shape[2], crop)
        r = dict(shape=list(shape), crop=list(box), size=size, resize=resize)
        if not a.no_device:
            if not torch.cuda.is_available():
                raise SystemExit('no GPU: the device timing needs one (--no-device times the host path alone)')
            r['device'] = device_time(frames, labels, box, size, resize, a.iters, a.warmup)
            d, l = r['device']['frames'], r['device']['labels']
            print('%-12s device %-8s %8.2f us/batch  %5.2f MB  %7.1f GB/s  (%.1f %% of HBM peak)   labels (uint8) %6.2f us/batch'
                  % (name, resize, d['us_per_batch'], d['bytes'] / 1e6, d['bytes_per_s'] / 1e9, 100 * d['hbm_peak_share'],
                     l['us_per_batch']), flush=True)
        if not a.no_host:
            r['host_ms_per_batch'] = host_time(name, frames, box, size, a.host_reps)
            print('%-12s host, one thread   %8.2f ms/batch  (%.0f us/image)' % (name, r['host_ms_per_batch'],
                                                                              r['host_ms_per_batch'] * 1e3 / shape[0]), flush=True)
        results[name] = r
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
