"""Wall time and device-to-host copies of one weight-and-gradient histogram logging event, before and after genesis_amd.histogram,
on the metric configuration's model (GENESIS-V2, K = 7, 64 x 64) after one training iteration (forward, loss.backward()), with a
writer that discards what it gets:
  (a) baseline: the logging done the way tensorboardX does it -- per tensor `.cpu().numpy().astype(float)`, numpy.histogram on the
      default table of 1549 edges, min / max / sum / dot and the trimming, written here in this project's own words;
  (b) genesis_amd.histogram.log_grads_and_weights (one table upload, one gx_hist_multi call, one device-to-host copy).
Times: warm-up calls, then the median of `--reps` single calls, each between two synchronisations (both variants contain host
reads, so event timing alone would flatter them).  Copies are counted where they are made.
The kernels alone (gx_hist_multi's memset node and two launches between two HIP events, the table already on the device; median of
`--reps`): the whole parameter set (every weight and gradient, one call), and one segment of the largest parameter's size filled
with N(0, 0.02) values against the same segment ZERO-FILLED -- the contention case, every lane of every wave on one bin -- and
the same pair at 2^24 elements, where the call's fixed cost no longer hides the cost of an element.

Every measurement runs in ONE child process under a time limit; a child that fails or runs out of time ends the script: there is
no second attempt.
Usage: python tools/histogram_time.py [--reps 20] [--warmup 3] [--limit 300] [--json path]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, K, SIZE = 32, 7, 64
LARGE = 1 << 24


class DiscardingWriter(object):
    calls = 0

    def add_histogram_raw(self, *args, **kwargs):
        self.calls += 1


class Copies(object):
    """Counts the device-to-host copies of the baseline where it makes them."""
    n = 0

    def fetch(self, t):
        self.n += 1
        return t.detach().cpu().numpy()


def baseline_histogram(values, edges):
    """One tensor the way tensorboardX's make_histogram treats it, on the host."""
    import numpy as np
    v = values.astype(float).reshape(-1)
    counts, limits = np.histogram(v, bins=edges)
    filled = np.flatnonzero(counts)
    first, last = (int(filled[0]), int(filled[-1])) if filled.size else (0, -1)
    kept = counts[first - 1:last + 1] if first > 0 else np.concatenate(([0], counts[:last + 1]))
    return (v.min(), v.max(), v.size, v.sum(), v.dot(v), limits[first:last + 2].tolist(), kept.tolist())


def baseline_log(model, writer, copies, edges, step):
    for name, param in model.named_parameters():
        writer.add_histogram_raw('weights/' + name, *baseline_histogram(copies.fetch(param.data), edges), step)
        if param.grad is not None:
            writer.add_histogram_raw('grads/' + name, *baseline_histogram(copies.fetch(param.grad), edges), step)


def setup():
    import torch
    from genesis_amd import testing as T
    from genesis_amd.compat.attrdict import AttrDict
    import genesis_amd.genesisv2_config as G
    from oracle import v2_oracle as O
    cfg = O.make_cfg(K_steps=K, img_size=SIZE, feat_dim=64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    model = model.to('cuda').train()
    x = torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(0)).cuda()
    _, losses, _, _, _ = model(x)      # one iteration of the unchanged loop: the gradients stay in .grad
    (losses.err.mean(0) + torch.stack(losses.kl_l_k, dim=1).mean(dim=0).sum()).backward()
    torch.cuda.synchronize()
    return model


def kernel_ms(tensors, reps, warmup):
    """gx_hist_multi alone on `tensors` against the default table: median ms between two HIP events."""
    import numpy as np
    import torch
    from genesis_amd import _lib
    from genesis_amd import histogram as hist
    dev = tensors[0].device
    edges = hist._device_edges(hist.default_bins(), dev)
    S, nb = len(tensors), hist.default_bins().size - 1
    table, work = np.zeros((S, hist.DESC_WORDS), np.int64), 0
    for i, t in enumerate(tensors):
        table[i] = (t.data_ptr(), t.numel(), hist.FP32 if t.dtype == torch.float32 else hist.FP64, work)
        work += -(-t.numel() // hist.CHUNK)
    dev_table = torch.from_numpy(table).to(dev)
    out = torch.empty(7 * S + (S * nb + 1) // 2, dtype=torch.int64, device=dev)
    ws_bytes = _lib.query('gx_hist_multi_ws_bytes', work)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = ctypes.c_void_p

    def call():
        _lib.call('gx_hist_multi', p(table.ctypes.data), p(dev_table.data_ptr()), table.size, S, p(edges.data_ptr()), nb + 1,
                  p(out.data_ptr() + 56 * S), p(out.data_ptr()), p(out.data_ptr() + 32 * S), p(ws.data_ptr()), ws_bytes, stream)
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    elements = sum(t.numel() for t in tensors)
    nbytes = sum(t.numel() * t.element_size() for t in tensors)
    ms = statistics.median(times)
    return {'median_ms': ms, 'min_ms': min(times), 'max_ms': max(times), 'segments': S, 'workgroups': work, 'elements': elements,
            'ns_per_element': 1e6 * ms / elements, 'input_GB_per_s': nbytes / (1e6 * ms)}


def measure(a):
    import torch
    from genesis_amd import histogram as hist
    model = setup()
    writer, copies, edges = DiscardingWriter(), Copies(), hist.default_bins()
    tensors = []
    for _, param in model.named_parameters():
        tensors.append(param.data)
        if param.grad is not None:
            tensors.append(param.grad)
    res = {'shape': dict(B=B, K=K, H=SIZE, W=SIZE), 'reps': a.reps, 'warmup': a.warmup, 'tensors': len(tensors),
           'elements': sum(t.numel() for t in tensors), 'largest_parameter': max(t.numel() for t in tensors)}
    variants = {'baseline': lambda: baseline_log(model, writer, copies, edges, 1),
                'log_grads_and_weights': lambda: hist.log_grads_and_weights(model, writer, 1)}
    for name, fn in variants.items():
        for _ in range(a.warmup):
            fn()
        calls, n0, times = writer.calls, copies.n, []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        res[name] = {'median_ms': statistics.median(times), 'min_ms': min(times), 'max_ms': max(times),
                     'writer_calls_per_event': (writer.calls - calls) // a.reps,
                     'device_to_host_copies_per_event': (copies.n - n0) // a.reps if name == 'baseline' else 1}
        print(name, res[name], flush=True)
    res['ratio_of_medians'] = res['baseline']['median_ms'] / res['log_grads_and_weights']['median_ms']
    n = res['largest_parameter']
    g = torch.Generator(device='cuda').manual_seed(0)
    res['kernels_whole_parameter_set'] = kernel_ms(tensors, a.reps, a.warmup)
    res['kernels_one_segment_normal'] = kernel_ms([0.02 * torch.randn(n, device='cuda', generator=g)], a.reps, a.warmup)
    res['kernels_one_segment_zeros'] = kernel_ms([torch.zeros(n, device='cuda')], a.reps, a.warmup)
    res['zeros_over_normal_per_element'] = (res['kernels_one_segment_zeros']['ns_per_element']
                                            / res['kernels_one_segment_normal']['ns_per_element'])
    # a parameter-sized segment is a few dozen workgroups, and the call's fixed cost hides what an element costs: the same pair at
    # 2^24 elements, where the workgroups fill the chip many times over
    res['kernels_16M_normal'] = kernel_ms([0.02 * torch.randn(LARGE, device='cuda', generator=g)], a.reps, a.warmup)
    res['kernels_16M_zeros'] = kernel_ms([torch.zeros(LARGE, device='cuda')], a.reps, a.warmup)
    res['zeros_over_normal_per_element_16M'] = res['kernels_16M_zeros']['ns_per_element'] / res['kernels_16M_normal']['ns_per_element']
    for key in ('kernels_whole_parameter_set', 'kernels_one_segment_normal', 'kernels_one_segment_zeros', 'kernels_16M_normal',
                'kernels_16M_zeros'):
        print(key, res[key], flush=True)
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300, help='seconds the child process may take')
    ap.add_argument('--json', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return measure(a)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--reps', str(a.reps), '--warmup', str(a.warmup)]
    if a.json:
        cmd += ['--json', a.json]
    try:
        rc = subprocess.run(cmd, timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit('histogram_time: the measurement did not finish within %d s; not repeated' % a.limit)
    if rc != 0:
        raise SystemExit('histogram_time: the measurement ended with status %d; not repeated' % rc)


if __name__ == '__main__':
    main()
