"""Times the sample-quality launches (genesis_amd/sample_quality.py, gx_manifold.hip) at N = M = 10 000, D = 2048: the two
k-NN radius passes, the two count passes, the KID sums at S = 100 and m = 1000, their total, and the achieved fp64 rate
against the operation count the shapes give.  Beside each one, in the same call and alternating with it, a plain torch fp64
formulation on the same device (cdist + kthvalue + comparisons, chunked so that it fits; matmul for KID), whose integer
results are compared with the kernels'.  A window is `--reps` back-to-back calls between two HIP events; `--warmup`
unrecorded rounds, then the median (and the range) of `--iters` rounds, kernel and torch windows alternating.  Last the
FID Inception feature pass on 64 x 64 images, the share of an evaluation that matters.
Usage: python tools/sample_quality_time.py [--n N] [--m M] [--dims D] [--iters N] [--reps N] [--warmup N] [--no-features] [--json path]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

FP64_VECTOR_PEAK = 78.6e12         # flop/s, MI355X spec
CHUNK = 1000                       # query rows per torch chunk: CHUNK x N fp64 = 80 MB at N = 10 000


def timed(fn, reps=1):
    """(ms per call, the last result) of `reps` back-to-back calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, out


def torch_radii(X, k):
    X64, out = X.double(), []
    for i0 in range(0, X.shape[0], CHUNK):
        d = torch.cdist(X64[i0:i0 + CHUNK], X64).square_()
        r = torch.arange(d.shape[0], device=X.device)
        d[r, r + i0] = float('inf')
        out.append(d.kthvalue(k, dim=1).values)
    return torch.cat(out)


def torch_counts(Q, R, rad):
    Q64, R64, hits = Q.double(), R.double(), []
    covered = torch.zeros(R.shape[0], dtype=torch.bool, device=R.device)
    for i0 in range(0, Q.shape[0], CHUNK):
        inside = torch.cdist(Q64[i0:i0 + CHUNK], R64).square_() <= rad[None, :]
        hits.append(inside.sum(1))
        covered |= inside.any(0)
    return torch.cat(hits).int(), covered.int()


def torch_kid_sums(real, fake, ix, iy):
    R64, F64, D, out = real.double(), fake.double(), real.shape[1], []
    for s in range(ix.shape[0]):
        x, y = F64[ix[s].long()], R64[iy[s].long()]
        kxx, kyy, kxy = ((a @ b.T / D + 1.0) ** 3 for a, b in ((x, x), (y, y), (x, y)))
        out.append(torch.stack([kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()]))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--m', type=int, default=10000)
    ap.add_argument('--dims', type=int, default=2048)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-features', action='store_true')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: the timing needs one')
    from genesis_amd import sample_quality as SQ
    N, M, D, k, S = a.n, a.m, a.dims, 3, 100
    g = torch.Generator(device='cuda').manual_seed(0)
    W = torch.randn(6, D, device='cuda', generator=g)                 # low intrinsic dimension, as pool features have
    real = (torch.randn(N, 6, device='cuda', generator=g) @ W + 0.05 * torch.randn(N, D, device='cuda', generator=g)).abs()
    fake = ((0.8 * torch.randn(M, 6, device='cuda', generator=g) + 0.3) @ W
            + 0.05 * torch.randn(M, D, device='cuda', generator=g)).abs()
    msub = min(N, M, 1000)
    ix, iy = (torch.from_numpy(v).cuda() for v in SQ.kid_indices(N, M, msub, S, 0))
    rad_r, rad_f = SQ.knn_radii(real, k), SQ.knn_radii(fake, k)
    tiles = -(-msub // 64)
    kid_pairs = S * (2 * (tiles * (tiles + 1) // 2) + tiles * tiles) * 64 * 64      # the pairs of the tiles that run
    items = [   # name, kernel call, torch call, fp64 operations
        ('radii real  [N x N]', lambda: SQ.knn_radii(real, k), lambda: torch_radii(real, k), 3.0 * N * N * D),
        ('radii fake  [M x M]', lambda: SQ.knn_radii(fake, k), lambda: torch_radii(fake, k), 3.0 * M * M * D),
        ('counts fake in real', lambda: SQ.manifold_counts(fake, real, rad_r), lambda: torch_counts(fake, real, rad_r),
         3.0 * N * M * D),
        ('counts real in fake', lambda: SQ.manifold_counts(real, fake, rad_f), lambda: torch_counts(real, fake, rad_f),
         3.0 * N * M * D),
        ('KID sums S=%d m=%d' % (S, msub), lambda: SQ.kid_sums(real, fake, ix, iy), lambda: torch_kid_sums(real, fake, ix, iy),
         2.0 * kid_pairs * D),
    ]
    res = dict(N=N, M=M, D=D, k=k, kid_subsets=S, kid_subset_size=msub, iters=a.iters, reps=a.reps, items={})
    total_k = total_t = 0.0
    for name, ours, theirs, ops in items:
        tk, tt = [], []
        for it in range(a.warmup + a.iters):
            ms_k, out_k = timed(ours, a.reps)
            ms_t, out_t = timed(theirs, a.reps)
            if it >= a.warmup:
                tk.append(ms_k)
                tt.append(ms_t)
        mk, mt = statistics.median(tk), statistics.median(tt)
        if name.startswith('counts'):
            diff = int((out_k[0] != out_t[0]).sum()) + int((out_k[1] != out_t[1]).sum())
            check = 'integer results differ in %d places' % diff if diff else 'integer results equal'
        else:
            rel = float(((out_k - out_t).abs() / out_t.abs()).max())
            check = 'largest relative difference %.2g' % rel
        rate = ops / (mk * 1e-3)
        res['items'][name] = dict(kernel_ms=mk, kernel_ms_all=tk, torch_ms=mt, torch_ms_all=tt, fp64_ops=ops,
                                  kernel_tflops=rate / 1e12, vector_peak_share=rate / FP64_VECTOR_PEAK, check=check)
        print('%-22s kernel %8.2f ms (%.2f .. %.2f)  %5.1f Tflop/s fp64 = %4.1f %% of the vector peak | torch %8.2f ms '
              '(%.2f .. %.2f) | %s' % (name, mk, min(tk), max(tk), rate / 1e12, 100 * rate / FP64_VECTOR_PEAK, mt, min(tt),
                                       max(tt), check), flush=True)
        total_k += mk
        total_t += mt
    res['total_kernel_ms'], res['total_torch_ms'] = total_k, total_t
    print('total: kernels %.1f ms, torch fp64 formulation %.1f ms' % (total_k, total_t), flush=True)
    ms, out = timed(lambda: SQ.sample_quality(real, fake))
    res['sample_quality_ms'] = ms
    print('sample_quality() as called (k = 3 and k = 5: three radius and three count passes, KID, one read): %.1f ms  %s'
          % (ms, {n: round(v, 5) for n, v in out.items()}), flush=True)
    if not a.no_features:
        from genesis_amd import fid
        from tests.fid_restatement import random_state_dict
        net = fid.FIDInception.from_state_dict(random_state_dict(fid.expected_shapes(), 0), 'cuda')
        imgs = torch.rand(100, 3, 64, 64, device='cuda')
        net.features(imgs)
        ms = statistics.median(timed(lambda: net.features(imgs), a.reps)[0] for _ in range(3))
        res['features_ms_per_100_images'] = ms
        res['features_s_for_all_images'] = ms * 1e-3 * (N + M) / 100
        print('FID Inception features: %.1f ms per 100 images of 64 x 64 -> %.1f s for %d + %d images; the all-pairs kernels '
              'are %.2f %% of that' % (ms, res['features_s_for_all_images'], N, M,
                                       100 * total_k * 1e-3 / res['features_s_for_all_images']), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
