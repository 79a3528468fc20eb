"""Object tables without a device: tests/objects_restatement.py against hand-written 4 x 5 cases with known tables, what the shared
input maker promises, every Python-side refusal of genesis_amd.objects / genesis_amd.segment (raised before a device is touched),
the header's declaration of gx_object_table, and the objects.csv lines and label-PNG bytes of an ObjectTable built from restated
arrays (the PNG read back by tests/objects_restatement.py: zlib and tests/png_restatement.py)."""
import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd._lib import GenesisHipError
from tests import objects_restatement as R

H, W = 4, 5
LABELS_A = np.array([[0, 0, 1, 1, 1],
                     [0, 2, 1, 1, 1],
                     [0, 0, 0, 1, 1],
                     [0, 0, 0, 0, 1]])
# area, x_min, y_min, x_max, y_max, sum_x, sum_y, border (1 column 0, 2 row 0, 4 column W - 1, 8 row H - 1)
GEOM_A = np.array([[10, 0, 0, 3, 3, 10, 19, 1 | 2 | 8],
                   [9, 2, 0, 4, 3, 29, 10, 2 | 4 | 8],
                   [1, 1, 1, 1, 1, 1, 1, 0]], np.int64)


def case_a():
    """Three slots, mask 0.8 on the slot's own pixels and 0.1 elsewhere; the image holds the column in channel 0 and the row in
    channel 1, so the colour sums are sum_x and sum_y."""
    log_m = np.where(LABELS_A[None] == np.arange(3)[:, None, None], np.float32(np.log(0.8)), np.float32(np.log(0.1)))
    log_m = log_m.astype(np.float32)[:, None]                                    # [K, 1, H, W]
    py, px = np.divmod(np.arange(H * W), W)
    x = np.stack([px, py]).reshape(1, 2, H, W).astype(np.float32)
    return log_m, x


def host_table(log_m, x):
    from genesis_amd.objects import ObjectTable
    labels, geom, soft = R.restate(log_m, x)
    return ObjectTable(torch.from_numpy(labels), torch.from_numpy(geom), torch.from_numpy(soft), 0 if x is None else x.shape[1])


def test_restatement_on_a_hand_written_case():
    log_m, x = case_a()
    labels, geom, soft = R.restate(log_m, x)
    assert labels.dtype == np.uint8 and np.array_equal(labels[0], LABELS_A)
    assert geom.dtype == np.int64 and np.array_equal(geom[0], GEOM_A)
    area = GEOM_A[:, 0].astype(np.float64)
    m_in, m_out = float(np.exp(np.float64(np.float32(np.log(0.8))))), float(np.exp(np.float64(np.float32(np.log(0.1)))))
    np.testing.assert_allclose(soft[0, :, 0], area * m_in + (20 - area) * m_out, rtol=1e-14)
    np.testing.assert_allclose(soft[0, :, 1], area * m_in, rtol=1e-14)
    assert np.array_equal(soft[0, :, 2], GEOM_A[:, 5]) and np.array_equal(soft[0, :, 3], GEOM_A[:, 6])
    assert np.array_equal(soft[0, :, 4:], np.zeros((3, 2)))
    assert np.array_equal(R.restate(log_m)[2][0, :, 2:], np.zeros((3, 4)))        # no image: no colour sums


def test_restatement_ties_nans_infinities_and_empty_slots():
    log_m = np.zeros((4, 1, H, W), np.float32)          # four equal planes: the lowest k wins everywhere
    log_m[1] = -np.inf
    labels, geom, soft = R.restate(log_m)
    assert not labels.any()
    empty = [0, W, H, -1, -1, 0, 0, 0]
    assert geom[0].tolist() == [[20, 0, 0, 4, 3, 40, 30, 15], empty, empty, empty]
    assert soft[0, :, 0].tolist() == [20.0, 0.0, 20.0, 20.0] and soft[0, :, 1].tolist() == [20.0, 0.0, 0.0, 0.0]
    log_m[2, 0, 2, 3] = log_m[3, 0, 2, 3] = np.nan      # a NaN ranks above every number and the first one wins
    log_m[1, 0, 0, 0] = 1.0
    log_m[3, 0, 3, 4] = -1e10
    labels, geom, soft = R.restate(log_m)
    assert labels[0, 2, 3] == 2 and labels[0, 0, 0] == 1 and labels.sum() == 3
    assert geom[0].tolist() == [[18, 0, 0, 4, 3, 37, 28, 15], [1, 0, 0, 0, 0, 0, 0, 3], [1, 3, 2, 3, 2, 3, 2, 0], empty]
    assert soft[0, 0].tolist() == [20.0, 18.0, 0, 0, 0, 0] and soft[0, 1, 0] == float(np.exp(np.float64(1.0))) == soft[0, 1, 1]
    assert np.isnan(soft[0, 2, 0]) and np.isnan(soft[0, 2, 1]) and np.isnan(soft[0, 3, 0]) and soft[0, 3, 1] == 0.0


def test_the_input_maker_keeps_its_promises():
    B, K, HH, WW = 3, 7, 13, 29
    log_m, x = R.make_inputs(B, K, HH, WW)
    assert log_m.dtype == np.float32 and log_m.shape == (K, B, HH, WW) and x.dtype == np.float32 and x.min() >= 0.0
    labels, geom, soft = R.restate(log_m, x)
    top = np.nanmax(log_m, axis=0)
    with np.errstate(invalid='ignore'):
        assert ((log_m[0] == top) & (log_m[1] == top)).reshape(B, -1).sum(1).min() >= 10             # exact ties, every image
    assert np.isnan(log_m[1, B - 1]).sum() >= 10 and np.isnan(log_m[:, B - 1]).sum(0).max() == 2         # NaNs; two at one pixel
    assert (log_m[K - 1, 0] == -1e10).all() and np.isneginf(log_m[K - 1, 1]).all()
    assert geom[0, K - 1].tolist() == [0, WW, HH, -1, -1, 0, 0, 0] and soft[0, K - 1, 0] == 0.0 == soft[1, K - 1, 0]
    assert geom[0, 2].tolist() == [1, WW // 2, HH // 2, WW // 2, HH // 2, WW // 2, HH // 2, 0]          # one pixel
    assert geom[0, 0, 7] == 15 and geom[0, 0, 1:5].tolist() == [0, 0, WW - 1, HH - 1]                   # all four borders
    assert (geom[:, :, 0].sum(1) == HH * WW).all()
    assert np.isnan(soft[B - 1, 1, 0]) and np.isfinite(soft[:B - 1]).all()
    small = R.make_inputs(1, 1, 1, 1)
    assert R.restate(*small)[1].tolist() == [[[1, 0, 0, 0, 0, 0, 0, 15]]]


def test_derived_quantities_of_a_host_table():
    log_m, x = case_a()
    t = host_table(log_m, x)
    assert t.cpu() is t and t.num_slots == 3
    assert t.area.tolist() == [[10, 9, 1]] and t.bbox[0].tolist() == GEOM_A[:, 1:5].tolist() and t.border[0].tolist() == [11, 14, 0]
    assert t.centroid[0].tolist() == [[1.0, 1.9], [29 / 9, 10 / 9], [1.0, 1.0]]
    assert t.mean_colour.shape == (1, 3, 2) and torch.equal(t.mean_colour, t.centroid)
    np.testing.assert_allclose(t.confidence[0].numpy(), 0.8, rtol=1e-7)
    assert t.present().tolist() == [[True, True, True]] and t.present(2).tolist() == [[True, True, False]]
    e = host_table(np.zeros((2, 1, H, W), np.float32), None)
    assert e.mean_colour.shape == (1, 2, 0) and torch.isnan(e.centroid[0, 1]).all() and torch.isnan(e.confidence[0, 1])
    assert e.present().tolist() == [[True, False]]


def planes(K=3, B=2, HH=4, WW=5, dtype=torch.float32):
    return [torch.zeros(B, 1, HH, WW, dtype=dtype) for _ in range(K)]


@pytest.mark.parametrize('make,match', [
    (lambda: ([], None), 'log_m_k holds 0 mask planes'),
    (lambda: (planes(33), None), 'log_m_k holds 33 mask planes'),
    (lambda: ([torch.zeros(2, 4, 5)] * 2, None), r'log_m_k planes must be \[B,1,H,W\]'),
    (lambda: ([torch.zeros(2, 2, 4, 5)] * 2, None), r'log_m_k planes must be \[B,1,H,W\]'),
    (lambda: (planes() + [torch.zeros(2, 1, 4, 6)], None), 'log_m_k planes differ'),
    (lambda: (planes(dtype=torch.float64), None), 'log_m_k planes differ in shape, dtype or device, or are not fp32'),
    (lambda: ([np.zeros((2, 1, 4, 5), np.float32)], None), 'log_m_k must be a sequence of tensors'),
    (lambda: ([torch.zeros(1, 1, 1, 4097).expand(1, 1, 2, 4097)], None), r'log_m_k planes of 2 x 4097'),
    (lambda: (planes(), torch.zeros(2, 3, 4, 5, dtype=torch.float64)), 'image must be an fp32'),
    (lambda: (planes(), torch.zeros(3, 4, 5)), 'image must be an fp32'),
    (lambda: (planes(), torch.zeros(2, 5, 4, 5)), 'image has 5 channels'),
    (lambda: (planes(), torch.zeros(2, 3, 5, 4)), 'image .* does not match the log_m_k planes'),
    (lambda: (planes(), torch.zeros(1, 3, 4, 5)), 'image .* does not match the log_m_k planes'),
    (lambda: (planes(), None), 'log_m_k must live on the HIP device'),
    (lambda: (torch.zeros(3, 2, 1, 4, 5), torch.zeros(2, 3, 4, 5)), 'log_m_k must live on the HIP device'),
])
def test_object_table_refusals_need_no_device(make, match):
    from genesis_amd.objects import object_table
    log_m_k, image = make()
    with pytest.raises(GenesisHipError, match=match):
        object_table(log_m_k, image)


def test_object_table_and_segmenter_refusals_on_host_objects():
    from genesis_amd.objects import ObjectTable
    from genesis_amd.segment import Segmenter, csv_rows, encode, label_png
    lab, geom, soft = torch.zeros(1, 4, 5, dtype=torch.uint8), torch.zeros(1, 3, 8, dtype=torch.int64), torch.zeros(1, 3, 6, dtype=torch.float64)
    for args, match in (((lab.int(), geom, soft), 'labels must be uint8'), ((lab, geom[:, :, :7], soft), 'geom must be int64'),
                        ((lab, geom, soft[:, :2]), 'soft must be fp64'), ((lab, geom, soft.float()), 'soft must be fp64'),
                        ((lab, geom, soft, 5), 'channels must be in')):
        with pytest.raises(GenesisHipError, match=match):
            ObjectTable(*args)
    model = torch.nn.Linear(2, 2)
    for kw, match in ((dict(min_pixels=0), 'min_pixels'), (dict(min_pixels=1.5), 'min_pixels'), (dict(generator=7), 'generator')):
        with pytest.raises(GenesisHipError, match=match):
            Segmenter(model, **kw)
    with pytest.raises(GenesisHipError, match='model must be callable'):
        Segmenter(object())
    seg = Segmenter(model)
    with pytest.raises(GenesisHipError, match='x must be an fp32'):
        seg(torch.zeros(2, 3, 8))
    with pytest.raises(GenesisHipError, match='x must live on the HIP device'):
        seg(torch.zeros(2, 3, 8, 8))
    with pytest.raises(GenesisHipError, match='model must be a GenesisV2'):
        encode(model, torch.zeros(2, 3, 8, 8))
    with pytest.raises(GenesisHipError, match='folder .* does not exist'):
        seg.segment_folder('/nonexistent/folder/of/pictures', '/nonexistent/out', 8)
    with pytest.raises(GenesisHipError, match='2 files for a table of 1 images'):
        csv_rows(ObjectTable(lab, geom, soft), ['a', 'b'])
    with pytest.raises(GenesisHipError, match=r'labels must be \[H, W\]'):
        label_png(np.zeros((1, 4, 5), np.uint8))


def test_encode_refuses_a_host_tensor_before_the_model_runs():
    from genesis_amd.compat.attrdict import AttrDict
    import genesis_amd.genesisv2_config as G
    from genesis_amd.segment import encode
    from oracle import v2_oracle as O
    model = G.load(AttrDict(dict(O.make_cfg(K_steps=3, img_size=32, feat_dim=16), debug=False, multi_gpu=False)))
    with pytest.raises(GenesisHipError, match='x must be a .* tensor on the HIP device'):
        encode(model, torch.zeros(2, 3, 32, 32))


def test_header_declares_gx_object_table():
    ret, args = _lib.parse_header()['gx_object_table']
    assert ret == 'int' and len(args) == 15
    assert [n for _, n in args] == ['base', 'plane_stride', 'image_stride', 'planes', 'x', 'x_image_stride', 'C', 'B', 'H', 'W', 'K',
                                    'labels', 'geom', 'soft', 'stream']
    assert args[3][0] == 'const float* const*' and args[11][0] == 'unsigned char*' and args[12][0] == 'long long*'


def test_csv_rows_of_a_restated_table():
    from genesis_amd.segment import CSV_HEADER, csv_rows
    assert CSV_HEADER == 'file,slot,area,x0,y0,x1,y1,cx,cy,border,mass,confidence,r,g,b'
    log_m, x = case_a()
    t = host_table(log_m, x)
    rows = csv_rows(t, ['sub/a b.png'])
    mass, conf = t.mass[0].tolist(), t.confidence[0].tolist()
    assert rows == ['sub/a b.png,0,10,0,0,3,3,1.0,1.9,11,%r,%r,1.0,1.9,' % (mass[0], conf[0]),
                    'sub/a b.png,1,9,2,0,4,3,%r,%r,14,%r,%r,%r,%r,' % (29 / 9, 10 / 9, mass[1], conf[1], 29 / 9, 10 / 9),
                    'sub/a b.png,2,1,1,1,1,1,1.0,1.0,0,%r,%r,1.0,1.0,' % (mass[2], conf[2])]
    assert all(len(r.split(',')) == len(CSV_HEADER.split(',')) for r in rows)
    assert [float(v) for v in rows[1].split(',')[10:12]] == [mass[1], conf[1]]          # repr reads back exactly
    assert [r.split(',')[1] for r in csv_rows(t, ['f'], min_pixels=2)] == ['0', '1']
    assert csv_rows(t, ['a,"b".jpg'])[2].startswith('"a,""b"".jpg",2,1,')
    assert csv_rows(host_table(log_m, None), ['f'])[2].endswith(',,,')                  # no image: no colours


def test_label_png_bytes_read_back():
    from genesis_amd.segment import label_png
    log_m, x = R.make_inputs(2, 32, 9, 14)
    t = host_table(log_m, x)
    for b in range(2):
        got = R.read_grey_png(label_png(t.labels[b].numpy()))
        assert got.dtype == np.uint8 and np.array_equal(got, t.labels[b].numpy())
    assert np.array_equal(R.read_grey_png(label_png(LABELS_A.astype(np.uint8))), LABELS_A)
    assert int(t.labels.max()) > 3          # (more than a few grey levels in play)
