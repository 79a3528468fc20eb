"""The staging schedule of the 16-bit-pipe transposed-conv kernels (double-buffered parity planes in the data gradient, weight
slices two phases ahead: DESIGN.md finding 59) changes WHEN operands reach LDS, never which MFMAs an accumulator sees or their
order.  So at the smallest shapes where the ends of that pipeline can go wrong the outputs (a) stay inside the error bars of the
existing bf16-pipe test and (b) are bit for bit what the build before the change produced (tools/kq_digest.py wrote their SHA-256
digests into tests/golden/kq_schedule_digests.json)."""
import functools
import importlib.util
import json
import os.path as osp

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

hip = pytest.importorskip('genesis_amd.hip_ops')

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('kq_digest', osp.join(ROOT, 'tools', 'kq_digest.py'))
kd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kd)

with open(osp.join(ROOT, 'tests', 'golden', 'kq_schedule_digests.json')) as _f:
    RECORD = json.load(_f)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """Operands and the fp64 conv_transpose2d forward / data gradient of one shape: computed once, shared, never written to."""
    t = kd.inputs(*shape)
    xr = t['x'].double().requires_grad_()
    ref = F.conv_transpose2d(xr, t['w'].double(), t['b'].double(), 2, 2, 1)
    ref.backward(t['dy'].double())
    return t, ref.detach(), xr.grad.detach()


def rel(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize('shape', kd.SHAPES, ids=kd.key)
def test_schedule_keeps_error_bars_and_bits(shape):
    from genesis_amd import _lib
    t, ref, dref = reference(shape)
    err, errd, got = {}, {}, {}
    try:
        for mode in (0, 1, 2):      # fp32 pipe (the yardstick of the bars), six bf16 piece products (untouched), three fp16 piece products
            o = kd.run(t, mode)
            assert torch.equal(o['y'], o['y2']), 'forward with and without statistics differ (form %d)' % mode
            err[mode], errd[mode] = rel(o['y'], ref), rel(o['dx'], dref)
            got[mode] = {k: kd.digest(o[k]) for k in kd.OUTPUTS}
    finally:
        _lib.call('gx_kq_precision', -1)
        _lib.call('gx_kq_policy', 1)
    print('deconv %s: relative L2 error fp32 pipe %.3e, bf16 x 6 %.3e, fp16 x 3 %.3e; data gradient %.3e / %.3e / %.3e'
          % (kd.key(shape), err[0], err[1], err[2], errd[0], errd[1], errd[2]))
    # (a) the bars of test_transposed_conv_on_the_bf16_pipe_keeps_fp32_accuracy
    for mode in (1, 2):
        assert err[mode] <= 1.5 * err[0] + 1e-7 and err[mode] < 2e-5, err
        assert errd[mode] <= 1.5 * errd[0] + 1e-7 and errd[mode] < 2e-5, errd
    # (b) bit for bit the outputs of the build the record was taken on
    here = (torch.__version__, torch.cuda.get_device_name(0))
    if here != (RECORD['torch'], RECORD['device']):
        print('bitwise comparison skipped: the record is from torch %s on %s, this is torch %s on %s'
              % (RECORD['torch'], RECORD['device'], here[0], here[1]))
        return
    for mode in (1, 2):
        assert got[mode] == RECORD['digests'][kd.key(shape)][str(mode)], 'form %d: outputs differ from the recorded build' % mode
