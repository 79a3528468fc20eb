"""Images per second of the encoder-only segmentation path against the full forward pass, in one process and on the same batches:
  (a) Segmenter.__call__ (genesis_amd.segment: encode + one gx_object_table launch; label map, object table, mu and sigma),
  (b) the full no-grad model(x) followed by stats.instance_seg (the decoder, the mixture and the KL terms included; an int64
      argmax and no table),
and the share of gx_object_table in (a): object_table alone on the planes of one encode, event-timed.
Configurations: the metric configuration (GENESIS-V2, B = 32, K = 7, 64 x 64, feat_dim 64) and K = 11 at 128 x 128 (B = 32).
Both paths draw rand_pixel with torch.rand on the device and launch eagerly (without autograd model(x) replays no graph).
Wall clock around `--calls` calls ended by one synchronize, `--reps` windows per path, alternating; the best of each counts.

The measurement runs in ONE child process under a time limit; if it fails or runs out of time this script reports that and
stops: there is no second attempt.
Usage: python tools/segment_time.py [--calls 200] [--reps 3] [--limit 400] [--json profiles/segment_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = (('metric_K7_64', dict(K_steps=7, img_size=64, feat_dim=64), 32), ('K11_128', dict(K_steps=11, img_size=128, feat_dim=64), 32))


def wall(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def measure(a):
    import torch
    from genesis_amd import testing as T
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd.objects import object_table
    from genesis_amd.segment import Segmenter, encode
    import genesis_amd.genesisv2_config as G
    from oracle import v2_oracle as O
    res = {'calls': a.calls, 'reps': a.reps, 'configs': {}}
    for name, kw, B in CONFIGS:
        cfg = O.make_cfg(**kw)
        S = kw['img_size']
        torch.manual_seed(0)
        model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
        model.load_state_dict(T.formula_state_dict(model.state_dict()))
        model = model.to('cuda').eval()
        g = torch.Generator().manual_seed(1)
        batches = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(4)]
        seg = Segmenter(model, generator=torch.Generator(device='cuda').manual_seed(2))
        state = {'i': 0}

        def batch():
            state['i'] += 1
            return batches[state['i'] % len(batches)]

        def encoder_only():
            return seg(batch()).table.labels

        def full_forward():
            with torch.no_grad():
                out = model(batch())
            return out[2].instance_seg

        r = {'B': B, 'K': kw['K_steps'], 'img_size': S}
        paths = (('segmenter', encoder_only), ('full_forward_instance_seg', full_forward))
        for _, fn in paths:
            fn()
            fn()
        windows = {key: [] for key, _ in paths}
        for _ in range(a.reps):                  # alternating windows: both paths see the same minutes of a shared machine
            for key, fn in paths:
                windows[key].append(1e3 * wall(fn, a.calls))
        for key, _ in paths:
            ms = windows[key]
            r[key + '_ms_per_batch'] = ms
            r[key + '_images_per_s'] = B / (min(ms) * 1e-3)
            print(name, key, ['%.2f ms' % v for v in ms], '%.0f images/s' % r[key + '_images_per_s'], flush=True)
        planes = encode(model, batches[0]).log_m_k
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        object_table(planes, batches[0])
        times = []
        for _ in range(a.reps):
            start.record()
            for _ in range(a.calls):
                object_table(planes, batches[0])
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop) / a.calls)
        r['object_table_ms_per_batch'] = times
        r['ratio_segmenter_over_full'] = r['segmenter_images_per_s'] / r['full_forward_instance_seg_images_per_s']
        r['object_table_share_of_segmenter'] = min(times) / min(r['segmenter_ms_per_batch'])
        print(name, 'encoder-only path: %.2f x the full forward; gx_object_table %.3f ms = %.1f %% of it'
              % (r['ratio_segmenter_over_full'], min(times), 100 * r['object_table_share_of_segmenter']), flush=True)
        res['configs'][name] = r
        del model, seg
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=400, help='seconds the measuring child may take')
    ap.add_argument('--json', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--calls', str(a.calls), '--reps', str(a.reps)]
    if a.json:
        cmd += ['--json', a.json]
    try:
        rc = subprocess.run(cmd, timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit('segment_time: the measurement did not finish within %d s; not repeated' % a.limit)
    if rc != 0:
        raise SystemExit('segment_time: the measurement ended with status %d; not repeated' % rc)


if __name__ == '__main__':
    main()
