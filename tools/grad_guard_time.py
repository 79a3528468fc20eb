"""What the gradient guard costs, on the metric configuration (GENESIS-V2, B = 32, K = 7, 64 x 64), in one run:

  step      the median time of a TrainStep(graph=True) step with the guard off, with skip_nonfinite alone and with a binding
            max_grad_norm (a thousandth of the first step's norm, so that it binds in every step): `--rounds` rounds, the variants alternating inside a round, `--steps` replayed
            steps per variant and round between two synchronisations; the figure of a variant is the median over the rounds of the
            round's time per step, its spread their minimum and maximum.  `--parent-tree DIR` (a built checkout of the parent
            commit) adds the parent's own step measured the same way in a child process of its own, before and after, so that the
            guard-off step can be compared with it back to back against the parent's own run-to-run spread.
  guard     gx_grad_guard alone (its two launches between two HIP events, median of `--reps`): on the model's real gradient
            buffers, on 2^24 fp32 elements, where launch cost no longer dominates, and on 2^27 (512 MB: more than the chip's
            last-level cache holds from one repetition to the next), with the achieved input GB/s next to the HBM rates of the
            chip (8.0 TB/s specified, 6.3 TB/s achieved by a float4 copy).
  drop_in   genesis_amd.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ after one iteration of the unchanged loop, the same
            gradients and the same binding max_norm: milliseconds per call (host clock between two synchronisations, median of
            `--reps`) and kernel launches per call (counted by torch.profiler in a pass of its own; null when it is unavailable).

Every measurement runs in a child process under a time limit; a child that fails or runs out of time ends the script: there is no
second attempt.
Usage: python tools/grad_guard_time.py [--rounds 7] [--steps 40] [--reps 30] [--warmup 5] [--limit 420] [--parent-tree DIR] [--json path]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, SIZE = 32, 7, 64
LARGE = 1 << 24
HUGE = 1 << 27
BINDING = 1e-3      # max_grad_norm of the clipped variant over the first step's norm: it binds in every timed step
HBM_SPEC_GB_S, HBM_COPY_GB_S = 8000.0, 6290.0


def build_model():
    import torch
    from genesis_amd import testing as T
    from genesis_amd.compat.attrdict import AttrDict
    import genesis_amd.genesisv2_config as G
    from oracle import v2_oracle as O
    cfg = O.make_cfg(K_steps=K, img_size=SIZE, feat_dim=64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    return model.to('cuda').train()


def batch():
    import torch
    return torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).cuda()


def summary(per_round):
    return {'median_ms': statistics.median(per_round), 'min_ms': min(per_round), 'max_ms': max(per_round), 'rounds_ms': per_round}


def time_steps(variants, x, a):
    """variants: {name: TrainStep}.  Alternating rounds -> {name: summary of ms per step}."""
    import torch
    for ts in variants.values():
        for _ in range(a.warmup + 1):          # (the first call captures the graph)
            ts.step(x)
    torch.cuda.synchronize()
    rounds = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, ts in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ts.step(x)
            torch.cuda.synchronize()
            rounds[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    return {name: summary(r) for name, r in rounds.items()}


def measure_parent_step(a):
    """The step of whatever tree is first on sys.path (the parent's), no guard arguments: one variant, the same protocol."""
    from genesis_amd.trainer import TrainStep
    res = time_steps({'step': TrainStep(build_model(), SIZE, graph=True)}, batch(), a)['step']
    print(json.dumps(res), flush=True)


def guard_ms(guard, a, gscale=1.0, max_norm=1.0):
    import torch
    for _ in range(a.warmup):
        guard.run(gscale, max_norm)
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        guard.run(gscale, max_norm)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    nbytes = sum(t.numel() * t.element_size() for t in guard.tensors)
    ms = statistics.median(times)
    gbs = nbytes / (1e6 * ms)
    return {'median_ms': ms, 'min_ms': min(times), 'max_ms': max(times), 'segments': len(guard.tensors), 'chunks': guard.work,
            'elements': sum(t.numel() for t in guard.tensors), 'input_bytes': nbytes, 'input_GB_per_s': gbs,
            'share_of_hbm_spec': gbs / HBM_SPEC_GB_S, 'share_of_float4_copy_rate': gbs / HBM_COPY_GB_S}


def count_launches(fn):
    """Device kernels launched by one call of fn, by torch.profiler; None when the profiler cannot be used."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
                and not str(e.name).startswith(('Memcpy', 'Memset')))
        return n or None
    except Exception as err:      # noqa: BLE001  (a missing tracer is no reason to lose the timings)
        print('torch.profiler unavailable: %s' % err, flush=True)
        return None


def measure_drop_in(a):
    import torch
    import genesis_amd
    model = build_model()
    x = batch()
    _, losses, _, _, _ = model(x)          # one iteration of the unchanged loop: the gradients stay in .grad
    (losses.err.mean(0) + torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()).backward()
    torch.cuda.synchronize()
    params = list(model.parameters())
    saved = [p.grad.clone() for p in params]
    norm = float(torch.nn.utils.clip_grad_norm_(params, 1e30))
    max_norm = 0.5 * norm

    def restore():
        for p, g in zip(params, saved):
            p.grad.copy_(g)
    variants = {'torch.nn.utils.clip_grad_norm_': lambda: torch.nn.utils.clip_grad_norm_(params, max_norm),
                'genesis_amd.clip_grad_norm_': lambda: genesis_amd.clip_grad_norm_(params, max_norm)}
    res = {'parameters': len(params), 'elements': sum(p.numel() for p in params), 'grad_norm': norm, 'max_norm': max_norm}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            restore()
            fn()
        times = []
        for _ in range(a.reps):
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        restore()
        res[name] = {'median_ms': statistics.median(times), 'min_ms': min(times), 'max_ms': max(times),
                     'launches_per_call': count_launches(fn)}
        print(name, res[name], flush=True)
    from genesis_amd import grad_guard
    res['segments_of_the_drop_in'] = int(next(reversed(grad_guard._CACHE.values())).table.shape[0])
    res['ratio_of_medians'] = res['torch.nn.utils.clip_grad_norm_']['median_ms'] / res['genesis_amd.clip_grad_norm_']['median_ms']
    return res


def measure(a):
    import torch
    from genesis_amd import grad_guard
    from genesis_amd.trainer import TrainStep
    x = batch()
    res = {'shape': dict(B=B, K=K, H=SIZE, W=SIZE), 'rounds': a.rounds, 'steps_per_round': a.steps, 'reps': a.reps, 'warmup': a.warmup}
    probe = TrainStep(build_model(), SIZE, graph=False, skip_nonfinite=True)
    probe.step(x)
    norm = float(probe.grad_norm)
    res['grad_norm_first_step'] = norm
    res['guard_on_model_gradients'] = guard_ms(probe._guard, a, 1.0, 0.5 * norm)
    res['guard_on_model_gradients']['n32'], res['guard_on_model_gradients']['n64'] = probe.n32, probe.n64
    probe.close()
    big = 0.02 * torch.randn(LARGE, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
    res['guard_16M'] = guard_ms(grad_guard.GradGuard([big]), a)
    del big
    # (64 MB fit the chip's 256 MB last-level cache and every repetition re-reads them: 2^27 elements, 512 MB, do not)
    huge = torch.full((HUGE,), 0.02, device='cuda')
    res['guard_128M'] = guard_ms(grad_guard.GradGuard([huge]), a)
    del huge
    for key in ('guard_on_model_gradients', 'guard_16M', 'guard_128M'):
        print(key, res[key], flush=True)
    variants = {'guard_off': TrainStep(build_model(), SIZE, graph=True),
                'skip_nonfinite': TrainStep(build_model(), SIZE, graph=True, skip_nonfinite=True),
                'max_grad_norm_binding': TrainStep(build_model(), SIZE, graph=True, max_grad_norm=BINDING * norm, skip_nonfinite=True)}
    res['step'] = time_steps(variants, x, a)
    res['step']['max_grad_norm'] = BINDING * norm
    res['step']['clip_coef_last_step'] = float(variants['max_grad_norm_binding'].clip_coef)
    res['step']['grad_norm_last_step'] = float(variants['max_grad_norm_binding'].grad_norm)
    res['step']['skipped_steps'] = int(variants['max_grad_norm_binding'].skipped_steps)
    off = res['step']['guard_off']['median_ms']
    for name in ('skip_nonfinite', 'max_grad_norm_binding'):
        res['step'][name]['over_guard_off_us'] = 1e3 * (res['step'][name]['median_ms'] - off)
    print('step', res['step'], flush=True)
    for ts in variants.values():
        ts.close()
    res['drop_in'] = measure_drop_in(a)
    print(json.dumps(res), flush=True)
    return res


def child(cmd, limit, env=None):
    try:
        p = subprocess.run(cmd, timeout=limit, env=env, stdout=subprocess.PIPE)
    except subprocess.TimeoutExpired:
        raise SystemExit('grad_guard_time: a measurement did not finish within %d s; not repeated' % limit)
    sys.stdout.write(p.stdout.decode())
    if p.returncode != 0:
        raise SystemExit('grad_guard_time: a measurement ended with status %d; not repeated' % p.returncode)
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--limit', type=int, default=420, help='seconds a child process may take')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit: its step is timed too')
    ap.add_argument('--json', default=None)
    ap.add_argument('--child', default=None, choices=['all', 'parent'], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == 'parent':
        sys.path.insert(0, os.path.abspath(a.parent_tree))
        return measure_parent_step(a)
    sys.path.insert(0, REPO)
    if a.child == 'all':
        return measure(a)
    common = ['--rounds', str(a.rounds), '--steps', str(a.steps), '--reps', str(a.reps), '--warmup', str(a.warmup)]
    me = [sys.executable, os.path.abspath(__file__)]
    parent_cmd = me + ['--child', 'parent', '--parent-tree', a.parent_tree or ''] + common
    parent = []
    if a.parent_tree:
        parent.append(child(parent_cmd, a.limit))
    res = child(me + ['--child', 'all'] + common, a.limit)
    if a.parent_tree:
        parent.append(child(parent_cmd, a.limit))
        res['step']['parent_commit_before_and_after'] = parent
        res['step']['guard_off_minus_parent_us'] = 1e3 * (res['step']['guard_off']['median_ms']
                                                          - statistics.mean(p['median_ms'] for p in parent))
        res['step']['parent_run_to_run_us'] = 1e3 * abs(parent[0]['median_ms'] - parent[1]['median_ms'])
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
