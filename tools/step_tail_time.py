"""What the schedule and the averaged weights cost inside the optimiser launch, at the metric model's parameter count (GENESIS-V2,
K = 7, 64 x 64: the flat fp32 group of TrainStep and its one fp64 element), in one run.

Variants, each on buffers of its own: gx_adam_step_pair (the launch of a default TrainStep, zero_grads = 1) and gx_adam_step_pair_ex
with a constant schedule, with warm-up + cosine, with a constant schedule + EMA and with warm-up + cosine + EMA.  A window is `--reps`
launches back to back on one stream between two HIP events (no host work between them); the variants alternate inside a round and the
figure of a variant is the median over `--rounds` rounds of the window's time per launch, its spread their minimum and maximum.
Accesses per fp32 element: 8 for the plain launch (read p, g, m, v; write p, g, m, v), 11 with the EMA (the average is read and
written, and p' is read back by the thread that has just stored it, from cache); the achieved GB/s counts 8 and 10 (the algorithm's
own traffic) next to the chip's float4 copy rate.
Usage: python tools/step_tail_time.py [--rounds 9] [--reps 60] [--warmup 20] [--json path]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SIZE = 7, 64
HBM_COPY_GB_S = 6290.0
LR, B1, B2, EPS = 1e-4, 0.9, 0.999, 1e-8


def parameter_count():
    """(n32, n64) of the flat buffers TrainStep builds for the metric model."""
    import torch
    from genesis_amd import testing as T
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd.trainer import TrainStep
    import genesis_amd.genesisv2_config as G
    from oracle import v2_oracle as O
    cfg = O.make_cfg(K_steps=K, img_size=SIZE, feat_dim=64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    ts = TrainStep(model.to('cuda').train(), SIZE)
    n = (ts.n32, ts.n64)
    ts.close()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from genesis_amd import _lib
    from genesis_amd.schedule import LRSchedule
    if not torch.cuda.is_available():
        raise SystemExit('step_tail_time needs a GPU: nothing is measured without one')
    n32, n64 = parameter_count()
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cosine = LRSchedule('cosine', warmup_iters=1000, decay_iters=500000, min_lr=1e-6)
    variants = {'gx_adam_step_pair': None, 'ex_constant': (LRSchedule('constant'), False), 'ex_cosine': (cosine, False),
                'ex_constant_ema': (LRSchedule('constant'), True), 'ex_cosine_ema': (cosine, True)}
    gen = torch.Generator().manual_seed(0)
    state = {}
    for name, v in variants.items():
        f32 = [torch.randn(n32, generator=gen).cuda() for _ in range(5)]
        f64 = [torch.randn(max(n64, 1), generator=gen, dtype=torch.float64).cuda() for _ in range(5)]
        for g in (f32, f64):
            g[2].mul_(0.01); g[3].abs_().mul_(1e-4)
        state[name] = dict(f32=f32, f64=f64, step=torch.full((), 2000, dtype=torch.int64, device='cuda'),
                           tail=torch.zeros(2, dtype=torch.float64, device='cuda'),
                           words=v[0].words(LR) if v else None, ema=bool(v and v[1]))

    def launch(name):
        s = state[name]
        a32, a64 = s['f32'], s['f64']
        p64 = [P(t) if n64 else None for t in a64]
        if s['words'] is None:
            _lib.call('gx_adam_step_pair', P(a32[0]), P(a32[1]), P(a32[2]), P(a32[3]), n32, p64[0], p64[1], p64[2], p64[3], n64,
                      P(s['step']), LR, B1, B2, EPS, 1.0, 1, stream)
        else:
            _lib.call('gx_adam_step_pair_ex', P(a32[0]), P(a32[1]), P(a32[2]), P(a32[3]), n32, p64[0], p64[1], p64[2], p64[3], n64,
                      P(s['step']), ctypes.c_void_p(s['words'].ctypes.data), None, B1, B2, EPS, 1.0, None,
                      P(a32[4]) if s['ema'] else None, p64[4] if s['ema'] else None, 0.999, 0, P(s['tail']), 1, stream)

    for name in variants:
        for _ in range(a.warmup):
            launch(name)
    torch.cuda.synchronize()
    rounds = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                launch(name)
            e1.record()
            e1.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / a.reps)
    out = {'n32': n32, 'n64': n64, 'rounds': a.rounds, 'reps_per_window': a.reps, 'warmup': a.warmup, 'variants': {}}
    for name, r in rounds.items():
        per = 10.0 if state[name]['ema'] else 8.0
        nbytes = per * (4.0 * n32 + 8.0 * n64)
        med = statistics.median(r)
        out['variants'][name] = {'median_us': 1e3 * med, 'min_us': 1e3 * min(r), 'max_us': 1e3 * max(r), 'accesses_per_element': per,
                                 'algorithmic_bytes': nbytes, 'GB_per_s': nbytes / (med * 1e-3) / 1e9,
                                 'share_of_float4_copy_rate': nbytes / (med * 1e-3) / 1e9 / HBM_COPY_GB_S}
    base = out['variants']['gx_adam_step_pair']['median_us']
    for name, v in out['variants'].items():
        v['ratio_to_plain'] = v['median_us'] / base
    text = json.dumps(out, indent=1)
    print(text)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
