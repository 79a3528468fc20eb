"""Throughput of the on-device FID (genesis_amd/fid.py): feature images/s of the FID Inception at B = 50 and 100 (HIP
events around `--iters` back-to-back FIDStatistics.update calls on resident 64 x 64 images, after `--warmup`), against
the fp32 matrix-pipe ceiling, and the time of compute() + frechet_distance at 2048 dims.  Random weights in pytorch_fid's
layout (the arithmetic does not depend on the values).  Kernel times without launch gaps: run it under rocprofv3, e.g.
    rocprofv3 --kernel-trace --stats -d OUTDIR -o fid -- python tools/fid_time.py --iters 3 --no-distance
Usage: python tools/fid_time.py [--iters N] [--warmup N] [--no-distance] [--json path]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

FP32_MFMA_PEAK = 157.3e12          # flop/s, MI355X spec (MI355X_MICROARCH: 155 measured)


def conv_macs_per_image(net):
    """Multiply-adds of one image's forward pass, counted from the shapes every conv launch sees."""
    from genesis_amd import fid
    macs = [0]
    real = fid.conv_bias_relu

    def count(x, wp, bias, parts, kh, kw, stride=1, ph=0, pw=0, dsts=None):
        B, H, W, C = x.shape
        Ho, Wo = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
        macs[0] += B * Ho * Wo * sum(parts) * C * kh * kw
        return real(x, wp, bias, parts, kh, kw, stride, ph, pw, dsts)
    fid.conv_bias_relu = count
    try:
        net.features(torch.rand(1, 3, 64, 64, device='cuda'))
    finally:
        fid.conv_bias_relu = real
    return macs[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-distance', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: the timing needs one')
    from genesis_amd import fid
    from tests.fid_restatement import random_state_dict
    net = fid.FIDInception.from_state_dict(random_state_dict(fid.expected_shapes(), 0), 'cuda')
    macs = conv_macs_per_image(net)
    ceiling = FP32_MFMA_PEAK / (2.0 * macs)
    res = dict(macs_per_image=macs, fp32_mfma_ceiling_img_per_s=ceiling)
    print('FID Inception: %.3f G multiply-adds per image; fp32-MFMA ceiling %.0f img/s' % (macs / 1e9, ceiling), flush=True)
    for B in (50, 100):
        imgs = torch.rand(B, 3, 64, 64, device='cuda')
        st = fid.FIDStatistics(net, 2048)
        for _ in range(a.warmup):
            st.update(imgs)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            st.update(imgs)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        rate = B / (ms * 1e-3)
        res['B%d' % B] = dict(ms_per_batch=ms, img_per_s=rate, ceiling_share=rate / ceiling,
                              achieved_tflops=2.0 * macs * rate / 1e12)
        print('B = %3d: %8.2f ms per batch (features + moments), %7.0f img/s, %.1f %% of the fp32-MFMA ceiling '
              '(%.1f TF/s)' % (B, ms, rate, 100 * rate / ceiling, 2.0 * macs * rate / 1e12), flush=True)
    if not a.no_distance:
        st = fid.FIDStatistics(net, 2048)
        st.update_features(torch.rand(200, 2048, device='cuda'))
        st2 = fid.FIDStatistics(net, 2048)
        st2.update_features(torch.rand(200, 2048, device='cuda') * 1.1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fid.frechet_distance(*st.compute(), *st2.compute())
        dt = time.perf_counter() - t0
        res['compute_and_distance_s'] = dt
        print('compute() x 2 + frechet_distance (2048 dims): %.2f s (FID %.4f)' % (dt, v), flush=True)
        rate = res['B100']['img_per_s']
        res['fid_10k_plus_10k_s_excl_sample'] = 20000 / rate + dt
        print('10 000 + 10 000 image FID, excluding sample(): %.1f s' % res['fid_10k_plus_10k_s_excl_sample'], flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
