"""genesis_amd.metrics.SegMetrics (gx_seg_metrics: argmax, contingency table, ARI and covering, batch accumulation in one
launch) against the two yardsticks the project already has: average_ari / average_segcover of the same module and the
reference's own values in tests/golden/metrics_*.npz.  Tolerances are those of tests/test_metrics.py: ARI 1e-12 (rtol and atol),
covering 2e-7 relative."""
import glob
import os.path as osp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = osp.dirname(osp.abspath(__file__))
GOLDENS = sorted(osp.basename(p)[8:-4] for p in glob.glob(osp.join(HERE, 'golden', 'metrics_*.npz')))
ARI = dict(rtol=1e-12, atol=1e-12)
COVER = dict(rtol=2e-7)


def make_case(B, K, H, W, G, seed, ignore=False):
    """K separate log-mask planes [B,1,H,W] correlated with a random instance map [B,1,H,W] of labels < G (on the device)."""
    g = torch.Generator().manual_seed(seed)
    inst = torch.randint(0, G, (B, 1, H, W), generator=g)
    inst[0][inst[0] == G - 1] = 0                                       # a label absent from image 0
    logits = torch.randn(B, K, H, W, generator=g)
    for k in range(min(K, G)):
        logits[:, k:k + 1] += 2.0 * (inst == k).float()
    if ignore:
        inst[:, :, :max(1, H // 4), :] = -1
    log_m = torch.log_softmax(logits, 1)
    return [log_m[:, k:k + 1].contiguous().cuda() for k in range(K)], inst.cuda()


def existing(planes, inst, ari=True):
    """The batch means (and per-image ARI lists) of the functions SegMetrics replaces."""
    from genesis_amd import metrics as M
    inst4 = inst.reshape(inst.shape[0], 1, *planes[0].shape[2:])
    out = {}
    if ari:
        out['ari'], out['ari_list'] = M.average_ari(planes, inst4)
        out['ari_fg'], out['ari_fg_list'] = M.average_ari(planes, inst4, True)
    ins_seg = torch.argmax(torch.cat(planes, 1), 1, True)
    out['msc'], out['ssc'] = M.average_segcover(inst4, ins_seg)
    out['msc_fg'], out['ssc_fg'] = M.average_segcover(inst4, ins_seg, True)
    return out


def check(got, want, ari=True):
    if ari:
        for key in ('ari', 'ari_fg'):
            np.testing.assert_allclose(got[key], want[key], err_msg=key, **ARI)
    for key in ('msc', 'msc_fg', 'ssc', 'ssc_fg'):
        np.testing.assert_allclose(got[key], float(want[key]), err_msg=key, **COVER)


def run(planes, inst, **kw):
    from genesis_amd.metrics import SegMetrics
    sm = SegMetrics(**kw)
    sm.update(planes, inst)
    return sm.compute()


@pytest.mark.parametrize('case', GOLDENS)
@pytest.mark.parametrize('packed', [False, True])
def test_reference_goldens(case, packed):
    g = np.load(osp.join(HERE, 'golden', 'metrics_%s.npz' % case))
    log_m = torch.from_numpy(g['log_m']).cuda()                           # [K,B,1,H,W]
    planes = list(log_m.unbind(0)) if packed else [p.clone() for p in log_m.unbind(0)]
    out = run(planes, torch.from_numpy(g['inst']).cuda(), keep_per_image=log_m.shape[1])
    assert out['num_batches'] == 1
    for fg, key in ((0, 'ari'), (1, 'ari_fg')):
        if 'ari_mean_fg%d' % fg in g:
            np.testing.assert_allclose(out['per_image'][key], g['ari_list_fg%d' % fg], **ARI)
            np.testing.assert_allclose(out[key], g['ari_mean_fg%d' % fg], **ARI)
    for bg, suffix in ((0, ''), (1, '_fg')):
        np.testing.assert_allclose(out['msc' + suffix], float(g['sc_mean_bg%d' % bg]), **COVER)
        np.testing.assert_allclose(out['ssc' + suffix], float(g['sc_scaled_bg%d' % bg]), **COVER)


@pytest.mark.parametrize('B,K,H,W,G', [(3, 4, 35, 35, 4),       # ragged plane (Tetrominoes): the 4-byte path
                                       (2, 3, 1, 1, 2),         # one pixel
                                       (1, 5, 16, 16, 4),       # one image
                                       (2, 1, 8, 8, 3),         # one plane: every pixel predicted 0
                                       (3, 11, 12, 20, 6),      # K = 11, more planes than the inner unroll
                                       (2, 7, 64, 64, 5)])      # several passes of the 256 threads, 16-byte path
def test_shapes_against_the_existing_functions(B, K, H, W, G):
    planes, inst = make_case(B, K, H, W, G, seed=B * 100 + K)
    want = existing(planes, inst)
    out = run(planes, inst, keep_per_image=B)
    check(out, want)
    np.testing.assert_allclose(out['per_image']['ari'], want['ari_list'], **ARI)
    np.testing.assert_allclose(out['per_image']['ari_fg'], want['ari_fg_list'], **ARI)
    # planes as views of one buffer: the same launch arithmetic, so the same bits
    packed = torch.stack(planes)
    assert run(list(packed.unbind(0)), inst) == {k: v for k, v in out.items() if k != 'per_image'}
    # [B,H,W] instances
    assert run(planes, inst[:, 0]) == {k: v for k, v in out.items() if k != 'per_image'}


def test_unaligned_base_takes_the_scalar_path():
    planes, inst = make_case(2, 4, 16, 16, 4, seed=5)
    want = run(planes, inst)
    K, B, HW = 4, 2, 256
    flat = torch.zeros(K * B * HW + 1, device='cuda')
    view = flat[1:].view(K, B, 1, 16, 16)                                # 4 bytes past a 16-byte boundary
    view.copy_(torch.stack(planes))
    assert view.data_ptr() % 16 == 4
    assert run(list(view.unbind(0)), inst) == want                       # packed, unaligned
    separate = []
    for p in planes:                                                     # a table of unaligned planes
        buf = torch.zeros(B * HW + 3, device='cuda')
        buf[3:].view(B, 1, 16, 16).copy_(p)
        separate.append(buf[3:].view(B, 1, 16, 16))
    assert run(separate, inst) == want
    # image stride above HW: planes cut out of a [B, K, H, W] tensor
    bk = torch.stack(planes, 1)[:, :, 0].contiguous()                    # [B, K, H, W]
    assert run([bk[:, k:k + 1] for k in range(K)], inst) == want


def test_ties_go_to_the_lowest_plane():
    H = W = 8
    planes = [torch.full((1, 1, H, W), -1.0, device='cuda') for _ in range(4)]
    planes[0][..., :4] = 0.0                       # left half: planes 0 and 2 tie -> 0
    planes[2][...] = 0.0                           # right half: plane 2 alone
    inst = torch.zeros(1, 1, H, W, dtype=torch.int64, device='cuda')
    inst[..., 4:] = 1
    out = run(planes, inst)
    assert out['ari'] == 1.0 and out['msc'] == 1.0 and out['ssc'] == 1.0      # any other choice on the left merges the halves
    check(out, existing(planes, inst))


def test_finished_slots_and_nan_planes():
    planes, inst = make_case(3, 5, 16, 16, 4, seed=9)
    planes[3].fill_(-1e10)                         # dynamic_K's finished slots
    planes[4].fill_(-1e10)
    for p in planes:
        p[2, :, 8:] = -1e10                        # a region where every plane ties: index 0
    check(run(planes, inst), existing(planes, inst))
    planes[1][0] = float('nan')                    # NaN ranks above every number ...
    planes[2][0, :, :4] = float('nan')             # ... and the first NaN wins
    planes[4][1, :, 5] = float('nan')
    pred = torch.argmax(torch.cat(planes, 1), 1)
    assert bool((pred[0] == 1).all()) and bool((pred[1, 5] == 4).all())
    check(run(planes, inst), existing(planes, inst))


def test_background_only_image_and_ignore_regions():
    from genesis_amd import metrics as M
    planes, inst = make_case(3, 4, 16, 16, 4, seed=11)
    inst[1] = 0
    want = existing(planes, inst)
    out = run(planes, inst, keep_per_image=3)
    check(out, want)
    assert out['per_image']['ari_fg'][1] == M.average_ari(planes, inst, True)[1][1] == 1.0
    planes, inst = make_case(3, 5, 32, 32, 4, seed=13, ignore=True)      # -1 rows: covering only, as the goldens compare
    check(run(planes, inst), existing(planes, inst, ari=False), ari=False)


def test_three_updates_with_a_short_last_batch():
    from genesis_amd.metrics import SegMetrics
    sm, sm5 = SegMetrics(keep_per_image=8), SegMetrics(keep_per_image=5)
    wants = []
    for i, B in enumerate((3, 3, 2)):
        planes, inst = make_case(B, 4, 20, 20, 5, seed=30 + i)
        sm.update(planes, inst)
        sm5.update(planes, inst)
        wants.append(existing(planes, inst))
    out = sm.compute()
    assert out['num_batches'] == 3
    mean = {k: sum(w[k] for w in wants) / len(wants) for k in ('ari', 'ari_fg', 'msc', 'msc_fg', 'ssc', 'ssc_fg')}
    check(out, mean)
    for key in ('ari', 'ari_fg'):
        lst = sum((w[key + '_list'] for w in wants), [])
        np.testing.assert_allclose(out['per_image'][key], lst, **ARI)
        np.testing.assert_array_equal(sm5.compute()['per_image'][key], out['per_image'][key][:5])      # bounded by its capacity
    again = sm.compute()                                                 # compute() leaves the accumulators alone
    assert all(again[k] == out[k] for k in out if k != 'per_image')
    # reset(): empty again, then as a fresh object
    sm.reset()
    with pytest.raises(Exception, match='no batch'):
        sm.compute()
    planes, inst = make_case(2, 4, 20, 20, 5, seed=32)
    sm.update(planes, inst)
    fresh = run(planes, inst, keep_per_image=8)
    again = sm.compute()
    assert again['num_batches'] == 1 and all(again[k] == fresh[k] for k in ('ari', 'ari_fg', 'msc', 'msc_fg', 'ssc', 'ssc_fg'))
    np.testing.assert_array_equal(again['per_image']['ari'], fresh['per_image']['ari'])


def test_refusals():
    from genesis_amd._lib import GenesisHipError
    from genesis_amd.metrics import SegMetrics
    with pytest.raises(GenesisHipError, match='no batch'):
        SegMetrics().compute()
    planes, inst = make_case(2, 4, 8, 8, 4, seed=40)
    sm = SegMetrics(max_labels=3)                                        # labels 0..3 present: 3 overflows
    sm.update(planes, inst)
    with pytest.raises(GenesisHipError, match='max_labels'):
        sm.compute()
    assert run(planes, inst, max_labels=4) == run(planes, inst)          # the table's height does not enter the scores
    big = [planes[0]] * 33
    with pytest.raises(GenesisHipError, match=r'K = 33'):
        SegMetrics().update(big, inst)
    with pytest.raises(GenesisHipError, match='64 KiB'):
        SegMetrics(max_labels=1 << 13).update(planes, inst)
    with pytest.raises(GenesisHipError):
        SegMetrics().update(planes, inst[:1])


def test_update_makes_no_host_read():
    """update() under torch's sync debug mode 'error', which turns every synchronising call into an exception (a build without
    that mode would capture one update in a graph instead: a capture admits no host read either)."""
    from genesis_amd.metrics import SegMetrics
    planes, inst = make_case(3, 4, 16, 16, 4, seed=50)
    packed = list(torch.stack(planes).unbind(0))
    want = existing(planes, inst)
    sm = SegMetrics(keep_per_image=6)
    torch.cuda.synchronize()
    supported = True
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()
            supported = False                                            # the mode did not catch a plain host read
        except RuntimeError:
            pass
        if supported:
            sm.update(planes, inst)
            sm.update(packed, inst[:, 0])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not supported:
        sm.update(planes, inst)                                          # (allocations made outside the capture)
        sm.reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sm.update(planes, inst)
        graph.replay()
        graph.replay()
    out = sm.compute()
    assert out['num_batches'] == 2
    check(out, want)
