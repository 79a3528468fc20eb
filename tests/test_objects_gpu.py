"""gx_object_table / genesis_amd.objects.object_table on the device against tests/objects_restatement.py.

Exactness.  `labels` and `geom` are integers: bit-exact.
Tolerance of `soft`: relative 1e-11 wherever the restated value is positive, exactly 0 where it is 0 (NaN where it is NaN: a NaN
log-mask).  Derivation: all terms are non-negative, so nothing cancels.  Kernel and restatement differ by the order of summation,
at most N 2^-53 relative for N terms, plus about 1 ulp of exp per term on either side: at most (N + 4) 2^-53 = 1.8e-12 at
N = 16384, the largest plane here.  (Checked on the host: reordering 16384 such terms moves the sum by 1.3e-15 relative.)  The
colour sums add fp32 values converted exactly, so only the order term applies to them.

Shapes (B, K, H, W): (1,1,1,1), (2,3,5,7), (3,7,13,29) ragged, H W % 4 != 0, the 4-byte loads; (2,32,16,16) K at its cap; (2,7,64,64)
and (1,11,128,128) the models' sizes; a workgroup strides over 256 threads x 4 pixels = 1024 pixels: (1,4,30,34) = 1020 is no
multiple of it, (1,4,4,257) = 1028 (16-byte loads) and (2,4,25,41) = 1025 (4-byte loads) lie just above it.  One restatement per
shape, shared by every test that needs it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd._lib import GenesisHipError
from tests import objects_restatement as R

pytestmark = pytest.mark.gpu
RTOL = 1e-11
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 7, 13, 29), (2, 32, 16, 16), (2, 7, 64, 64), (1, 11, 128, 128), (1, 4, 30, 34), (1, 4, 4, 257),
          (2, 4, 25, 41)]


@functools.lru_cache(maxsize=None)
def case(shape, C=3):
    """(log_m [K,B,H,W], x [B,C,H,W], labels, geom, soft): the shared inputs and their restatement, computed once."""
    log_m, x = R.make_inputs(*shape, C=C)
    out = (log_m, x) + R.restate(log_m, x)
    for a in out:
        a.setflags(write=False)
    return out


def packed(log_m):
    """K evenly strided views of one [K,B,1,H,W] buffer, as a model's stats.log_m_k."""
    return list(torch.tensor(log_m).cuda().unsqueeze(2).unbind(0))


def separate(log_m):
    """K tensors of their own."""
    return [torch.tensor(m).cuda().unsqueeze(1) for m in log_m]


def bits(t):
    return (t.soft.contiguous().view(torch.int64), t.geom, t.labels)


def same_bits(a, b):
    return all(torch.equal(p, q) for p, q in zip(bits(a), bits(b)))


def check(table, labels, geom, soft, channels):
    host = table.cpu()
    assert host.labels.dtype == torch.uint8 and host.geom.dtype == torch.int64 and host.soft.dtype == torch.float64
    assert np.array_equal(host.labels.numpy(), labels)
    assert np.array_equal(host.geom.numpy(), geom)
    got, want = host.soft.numpy(), soft.copy()
    want[:, :, 2 + channels:] = 0.0
    nan, zero = np.isnan(want), want == 0.0
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[zero], want[zero])                          # exactly 0 where the restatement is 0
    pos = ~nan & ~zero
    assert (want[pos] > 0).all()
    err = np.abs(got[pos] - want[pos]) / want[pos]
    print('soft: %d positive values, largest relative error %.3g' % (pos.sum(), err.max() if err.size else 0.0))
    assert (err <= RTOL).all()


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_kernel_against_the_restatement(shape):
    from genesis_amd.objects import object_table
    log_m, x, labels, geom, soft = case(shape)
    planes, image = packed(log_m), torch.tensor(x).cuda()
    table = object_table(planes, image)
    assert table.labels.is_cuda and table.labels.shape == (shape[0], shape[2], shape[3]) and table.channels == 3
    check(table, labels, geom, soft, 3)
    # agreement with the existing argmax, and K separate tensors (the pointer table) give the same bits as the packed planes
    assert torch.equal(table.labels.long(), torch.argmax(torch.stack(planes).squeeze(2), 0))
    assert same_bits(object_table(separate(log_m), image), table)
    assert same_bits(object_table(torch.stack(planes), image), table)


@pytest.mark.parametrize('shape', [(3, 7, 13, 29), (2, 7, 64, 64), (1, 4, 4, 257)], ids=str)
def test_base_offset_by_four_bytes_and_image_stride_above_hw(shape):
    from genesis_amd.objects import object_table
    log_m, x, labels, geom, soft = case(shape)
    B, K, H, W = shape
    HW = H * W
    image = torch.tensor(x).cuda()
    want = object_table(packed(log_m), image)
    src = torch.tensor(log_m).cuda().reshape(K, B, HW)
    # a base 4 bytes behind a 16-byte boundary: the 4-byte loads, in the pixel order of the 16-byte loads -- the same bits
    buf = torch.empty(K * B * HW + 1, device='cuda')
    off = buf[1:].view(K, B, 1, H, W)
    off.copy_(src.view(K, B, 1, H, W))
    assert off.data_ptr() % 16 == 4
    table = object_table(list(off.unbind(0)), image)
    check(table, labels, geom, soft, 3)
    assert same_bits(table, want)
    # an image stride above H W (the planes of a wider buffer), multiple of 4 floats and not
    for pad in (8, 3):
        wide = torch.full((K, B, HW + pad), float('nan'), device='cuda')
        wide[:, :, :HW] = src
        views = [torch.as_strided(wide, (B, 1, H, W), (HW + pad, HW, W, 1), k * B * (HW + pad)) for k in range(K)]
        assert views[0].stride(0) == HW + pad or B == 1
        assert same_bits(object_table(views, image), want)
    # the image as a view of a wider buffer: read in place through its image stride
    xw = torch.zeros(B, 3 * HW + 5, device='cuda')
    xw[:, :3 * HW] = image.reshape(B, -1)
    assert same_bits(object_table(packed(log_m), torch.as_strided(xw, (B, 3, H, W), (3 * HW + 5, HW, W, 1))), want)
    # planes that are no evenly strided images (a transposed view) are copied
    tr = [m.transpose(2, 3).contiguous().transpose(2, 3) for m in packed(log_m)]
    assert same_bits(object_table(tr, image), want)


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (2, 7, 64, 64)], ids=str)
def test_image_argument(shape):
    from genesis_amd.objects import object_table
    planes = packed(case(shape)[0])
    none = object_table(planes)
    log_m, _, labels, geom, soft = case(shape, 3)
    check(none, labels, geom, soft, 0)
    assert none.channels == 0 and none.mean_colour.shape == (shape[0], shape[1], 0)
    for C in (1, 3, 4):
        _, x, labels, geom, soft = case(shape, C)
        table = object_table(planes, torch.tensor(x).cuda())
        check(table, labels, geom, soft, C)
        assert table.channels == C and torch.equal(table.geom, none.geom) and torch.equal(table.soft[:, :, :2].contiguous().view(torch.int64),
                                                                                       none.soft[:, :, :2].contiguous().view(torch.int64))


@pytest.mark.parametrize('shape', [(3, 7, 13, 29), (3, 7, 64, 64)], ids=str)
def test_an_images_rows_do_not_depend_on_its_batch(shape):
    from genesis_amd.objects import object_table
    log_m, x = case(shape)[:2]
    dev_m, dev_x = torch.tensor(log_m).cuda(), torch.tensor(x).cuda()

    def run(order):
        idx = torch.tensor(order, device='cuda')
        return object_table(list(dev_m[:, idx].unsqueeze(2).unbind(0)), dev_x[idx])

    alone, first, last = run([1]), run([1, 0, 2]), run([0, 2, 1])
    for t, i in ((first, 0), (last, 2)):
        assert torch.equal(t.labels[i], alone.labels[0]) and torch.equal(t.geom[i], alone.geom[0])
        assert torch.equal(t.soft[i].contiguous().view(torch.int64), alone.soft[0].contiguous().view(torch.int64))
    assert not torch.equal(first.geom[1], first.geom[0])


def test_derived_quantities_stay_on_the_device_and_cpu_is_one_copy():
    from genesis_amd.objects import object_table
    shape = (3, 7, 13, 29)
    log_m, x, labels, geom, soft = case(shape)
    table = object_table(packed(log_m), torch.tensor(x).cuda())
    area = geom[:, :, 0].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        centroid, conf = geom[:, :, 5:7] / area[:, :, None], soft[:, :, 1] / area
    for got in (table.area, table.bbox, table.border, table.centroid, table.mass, table.confidence, table.mean_colour, table.present(2)):
        assert got.is_cuda
    assert np.array_equal(table.area.cpu().numpy(), geom[:, :, 0]) and np.array_equal(table.bbox.cpu().numpy(), geom[:, :, 1:5])
    assert np.array_equal(table.centroid.cpu().numpy(), centroid, equal_nan=True)
    np.testing.assert_allclose(table.confidence.cpu().numpy(), conf, rtol=RTOL, equal_nan=True)
    assert np.array_equal(table.present(2).cpu().numpy(), geom[:, :, 0] >= 2)
    host = table.cpu()
    assert not host.labels.is_cuda and host.channels == 3 and same_bits(host, type(host)(table.labels.cpu(), table.geom.cpu(), table.soft.cpu(), 3))
    assert torch.isnan(host.centroid[0, shape[1] - 1]).all()          # the slot that wins nowhere


def _call(**over):
    K, B, H, W = 3, 2, 4, 8
    t = _call.tensors
    a = dict(base=t['planes'].data_ptr(), pstride=B * H * W, istride=H * W, table=None, x=t['x'].data_ptr(), xstride=3 * H * W, C=3, B=B,
             H=H, W=W, K=K, labels=t['labels'].data_ptr(), geom=t['geom'].data_ptr(), soft=t['soft'].data_ptr())
    a.update(over)
    p = lambda v: None if v is None else (v if isinstance(v, ctypes.Array) else ctypes.c_void_p(v))      # noqa: E731
    _lib.call('gx_object_table', p(a['base']), a['pstride'], a['istride'], p(a['table']), p(a['x']), a['xstride'], a['C'], a['B'], a['H'],
              a['W'], a['K'], p(a['labels']), p(a['geom']), p(a['soft']), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_c_abi_refusals_return_the_error_code_before_any_launch():
    K, B, H, W = 3, 2, 4, 8
    _call.tensors = dict(planes=torch.zeros(K, B, 1, H, W, device='cuda'), x=torch.ones(B, 3, H, W, device='cuda'),
                         labels=torch.full((B, H, W), 77, dtype=torch.uint8, device='cuda'),
                         geom=torch.full((B, K, 8), -5, dtype=torch.int64, device='cuda'),
                         soft=torch.full((B, K, 6), -5.0, dtype=torch.float64, device='cuda'))
    t = _call.tensors
    ptrs = [t['planes'][k].data_ptr() for k in range(K)]
    null_plane = (ctypes.c_void_p * K)(ptrs[0], None, ptrs[2])
    for over, match in ((dict(base=None), 'either base'), (dict(table=(ctypes.c_void_p * K)(*ptrs)), 'either base'),
                        (dict(base=None, table=null_plane), 'plane 1 is null'),
                        (dict(labels=None), 'labels, geom or soft'), (dict(geom=None), 'labels, geom or soft'), (dict(soft=None), 'labels, geom or soft'),
                        (dict(K=0), r'K = 0 outside \[1, 32\]'), (dict(K=33), r'K = 33 outside \[1, 32\]'),
                        (dict(B=0), 'B = 0 below 1'), (dict(H=0), 'H = 0 or W'), (dict(W=0), 'or W = 0'),
                        (dict(H=4097), 'H = 4097'), (dict(W=4097), 'W = 4097'),
                        (dict(C=0), r'C = 0 outside \[1, 4\]'), (dict(C=5), r'C = 5 outside \[1, 4\]'),
                        (dict(istride=H * W - 1), 'image_stride 31 below H W = 32'), (dict(pstride=-1), 'negative plane_stride'),
                        (dict(xstride=3 * H * W - 1), 'x_image_stride 95 below C H W = 96')):
        with pytest.raises(GenesisHipError, match=match) as e:
            _call(**over)
        assert '(-1)' in str(e.value)                                    # GX_EINVAL
    torch.cuda.synchronize()
    assert bool((t['labels'] == 77).all()) and bool((t['geom'] == -5).all()) and bool((t['soft'] == -5.0).all())      # nothing ran
    _call(C=5, x=None)                                                   # without an image C is not looked at
    _call()
    torch.cuda.synchronize()
    assert not bool(t['labels'].any()) and t['geom'][0, 0].tolist() == [32, 0, 0, 7, 3, 112, 48, 15]
    assert t['soft'][1].tolist() == [[32.0, 32.0, 32.0, 32.0, 32.0, 0.0], [32.0, 0.0, 0.0, 0.0, 0.0, 0.0], [32.0, 0.0, 0.0, 0.0, 0.0, 0.0]]
