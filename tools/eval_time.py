"""Time of the validation metrics per batch, before and after genesis_amd.metrics.SegMetrics, in one process:
  (a) the sequence the loop ran until now for one mask field (train.py:542-548): cat + argmax, average_ari twice,
      average_segcover twice (genesis_amd.metrics: several launches and six host reads -- two per average_ari call, one per
      average_segcover call);
  (b) SegMetrics.update (one gx_seg_metrics launch, no host read),
at B = 32, K = 7, 64 x 64, labels < 8 -- wall clock around `--calls` calls ended by one synchronize ((a) contains host reads, so
event timing alone would flatter it) -- and the same pair for a 10-batch evaluation of the metric configuration's model
(GENESIS-V2, K = 7, 64 x 64, B = 32; both mask fields scored on every batch): a run of the former kind, average_ari /
average_segcover per batch and mask field and a host read per statistic, against genesis_amd.evaluate.evaluation.

The measurement runs in ONE child process under a time limit; if it fails or runs out of time this script reports that and
stops: there is no second attempt.
Usage: python tools/eval_time.py [--calls 200] [--reps 3] [--limit 300] [--json path]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def wall(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def former_scores(M, planes, inst):
    """What a batch of one mask field cost until now: the four numbers from genesis_amd.metrics' two functions."""
    import torch
    labels = torch.argmax(torch.cat(planes, 1), 1, True)
    return (M.average_ari(planes, inst)[0], M.average_ari(planes, inst, True)[0],
            M.average_segcover(inst, labels)[0], M.average_segcover(inst, labels, True)[0])


def former_evaluation(model, loader, M):
    """A validation run as INTEGRATION.md described it until now: eager forwards, per-batch loss means kept as device tensors,
    former_scores per mask field, and one host read per statistic at the end."""
    import torch
    from genesis_amd.evaluate import MASK_FIELDS, _batch_mean
    model.eval()
    kept = {}
    with torch.no_grad():
        for batch in loader:
            out = model(batch['input'])
            for key, val in out[1].items():
                kept.setdefault(key, []).append(_batch_mean(val))
            for field, suffix in MASK_FIELDS:
                four = former_scores(M, out[2][field], batch['instances'])
                for key, v in zip(('ari', 'ari_fg', 'msc', 'msc_fg'), four):
                    kept.setdefault(key + suffix, []).append(v)
    model.train()
    return {key: float(sum(vals) / len(vals)) for key, vals in kept.items()}


def measure(a):
    import torch
    from genesis_amd import metrics as M
    from genesis_amd import testing as T
    from genesis_amd.compat.attrdict import AttrDict
    from genesis_amd.evaluate import evaluation
    import genesis_amd.genesisv2_config as G
    from oracle import v2_oracle as O
    B, K, S, labels = 32, 7, 64, 8
    g = torch.Generator().manual_seed(0)
    inst = torch.randint(0, labels, (B, 1, S // 4, S // 4), generator=g).repeat_interleave(4, 2).repeat_interleave(4, 3).cuda()
    log_m = torch.log_softmax(torch.randn(K, B, 1, S, S, generator=g), 0).cuda()
    planes = list(log_m.unbind(0))

    def current():
        former_scores(M, planes, inst)

    sm = M.SegMetrics(max_labels=labels)
    res = {'shape': dict(B=B, K=K, H=S, W=S, max_labels=labels), 'calls': a.calls}
    for name, fn in (('current_sequence', current), ('seg_metrics_update', lambda: sm.update(planes, inst))):
        fn()
        res[name + '_us_per_batch'] = [1e6 * wall(fn, a.calls) for _ in range(a.reps)]
        print(name, ['%.1f us' % v for v in res[name + '_us_per_batch']], flush=True)
    res['ratio'] = min(res['current_sequence_us_per_batch']) / min(res['seg_metrics_update_us_per_batch'])
    print('update is %.1f x faster per batch' % res['ratio'], flush=True)

    cfg = O.make_cfg(K_steps=7, img_size=64, feat_dim=64)
    torch.manual_seed(0)
    model = G.load(AttrDict(dict(cfg, debug=False, multi_gpu=False)))
    model.load_state_dict(T.formula_state_dict(model.state_dict()))
    model = model.to('cuda').train()
    batches = [{'input': torch.rand(B, 3, S, S, generator=g).cuda(),
                'instances': torch.randint(0, labels, (B, 1, S // 4, S // 4), generator=g).repeat_interleave(4, 2)
                .repeat_interleave(4, 3).cuda()} for _ in range(10)]

    class Loader(list):
        batch_size = B
    loader, config = Loader(batches), AttrDict(debug=False, gpu=True)
    ev = {}
    for name, fn in (('former', lambda: former_evaluation(model, loader, M)),
                     ('evaluation', lambda: evaluation(model, loader, None, config, 1, None, 10 * B, max_labels=labels))):
        fn()
        ev[name + '_ms'] = [1e3 * wall(fn, 1) for _ in range(a.reps)]
        print(name, ['%.1f ms' % v for v in ev[name + '_ms']], flush=True)
    ev['ratio'] = min(ev['former_ms']) / min(ev['evaluation_ms'])
    ev['note'] = '10 batches, forward included; both mask fields scored on every batch'
    res['evaluation_10_batches'] = ev
    print('evaluation() is %.2f x faster' % ev['ratio'], flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--limit', type=int, default=300, help='seconds the measuring child may take')
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
        raise SystemExit('eval_time: the measurement did not finish within %d s; not repeated' % a.limit)
    if rc != 0:
        raise SystemExit('eval_time: the measurement ended with status %d; not repeated' % rc)


if __name__ == '__main__':
    main()
