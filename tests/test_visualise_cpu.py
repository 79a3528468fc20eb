"""genesis_amd.visualise without a GPU: the numpy restatement of make_grid against hand-written arrays, save_png through Pillow,
the refusals that happen before any launch, the descriptor constants against the header, and the committed fixtures against a
fresh run of the reference's own visualise_outputs where the reference tree is present."""
import ctypes
import os.path as osp
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from genesis_amd import _lib
from genesis_amd import visualise as vis
from genesis_amd._lib import GenesisHipError
from oracle import ref_import as R
from tests import vis_restatement as V
from tests import visualise_stub as S

REPO = osp.dirname(osp.dirname(osp.abspath(__file__)))


def _images(n):
    """n images of 2 x 3 pixels, one channel: pixel (r, c) of image i = 10 i + 3 r + c + 1."""
    return np.array([[[[10 * i + 3 * r + c + 1 for c in range(3)] for r in range(2)]] for i in range(n)], np.float32)


def test_restated_make_grid_n1_is_the_bare_image():
    want = np.array([[[1, 2, 3], [4, 5, 6]]] * 3, np.float32)
    assert np.array_equal(V.make_grid(_images(1), pad_value=9.0), want)
    rgb = np.arange(18, dtype=np.float32).reshape(1, 3, 2, 3)
    assert np.array_equal(V.make_grid(rgb), rgb[0])


def test_restated_make_grid_n3_by_hand():
    P = 9
    channel = [[P] * 17,
               [P] * 17,
               [P, P, 1, 2, 3, P, P, 11, 12, 13, P, P, 21, 22, 23, P, P],
               [P, P, 4, 5, 6, P, P, 14, 15, 16, P, P, 24, 25, 26, P, P],
               [P] * 17,
               [P] * 17]
    want = np.array([channel] * 3, np.float32)
    got = V.make_grid(_images(3), pad_value=9.0)
    assert got.shape == (3, 6, 17) and got.dtype == np.float32
    assert np.array_equal(got, want)


def test_restated_make_grid_n11_by_hand():
    """Eight to a row, a short second row whose unused cells are padding: '.' = pad value, a hex digit = that image."""
    e = '.' * 42
    picture = [e, e,
               '..000..111..222..333..444..555..666..777..',
               '..000..111..222..333..444..555..666..777..',
               e, e,
               '..888..999..aaa' + '.' * 27,
               '..888..999..aaa' + '.' * 27,
               e, e]
    images = np.stack([np.full((3, 2, 3), i + 1, np.float32) for i in range(11)])
    want = np.array([[0.5 if ch == '.' else int(ch, 16) + 1 for ch in row] for row in picture], np.float32)
    got = V.make_grid(images, pad_value=0.5)
    assert got.shape == (3, 10, 42)
    for c in range(3):
        assert np.array_equal(got[c], want)
    # nrow = 4, no padding: three rows of four cells, the last cell empty
    got = V.make_grid(images, nrow=4, padding=0, pad_value=0.5)
    rows = ['000111222333', '444555666777', '888999aaa...']
    want = np.array([[0.5 if ch == '.' else int(ch, 16) + 1 for ch in rows[r // 2]] for r in range(6)], np.float32)
    assert got.shape == (3, 6, 12) and np.array_equal(got[1], want)


def test_grid_geometry_matches_the_restatement():
    for n in (1, 3, 8, 11):
        for nrow, padding in ((8, 2), (4, 0), (4, 2)):
            p, xmaps, ymaps, Hg, Wg = vis.grid_geometry(n, 5, 7, nrow, padding)
            assert V.make_grid(np.zeros((n, 3, 5, 7), np.float32), nrow, padding).shape == (3, Hg, Wg)


def test_restated_colour_seg_masks():
    palette = V.load_palette()
    assert len(palette) == 15
    masks = np.array([[[-1, 0], [14, 3]]])
    got = V.colour_seg_masks(masks)
    assert got.shape == (1, 3, 2, 2) and got.dtype == np.int64
    assert got[0, :, 0, 0].tolist() == [0, 0, 0] and got[0, :, 0, 1].tolist() == palette[0]
    assert got[0, :, 1, 0].tolist() == palette[14] and got[0, :, 1, 1].tolist() == palette[3]
    with pytest.raises(IndexError):
        V.colour_seg_masks(np.array([[[15]]]))


def test_descriptor_constants_match_the_header():
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define GX_VIS_(\w+) (\d+)', header)}
    for name in ('COPY', 'EXP', 'EXP_MUL', 'LABEL_COLOUR', 'ARGMAX_COLOUR', 'FILL', 'FP32_CHW', 'U8_HWC', 'DESC_WORDS'):
        assert defs[name] == getattr(vis, name), name
    words = {k[2:]: v for k, v in defs.items() if k.startswith('D_') and k != 'DESC_WORDS'}
    assert len(words) == 22 and sorted(words.values()) == list(range(22))
    for name, v in words.items():
        assert getattr(vis, 'D_' + name) == v, name


@pytest.mark.parametrize('shape', [(1, 1, 3), (5, 7, 3), (1, 1), (5, 7)])
def test_save_png_round_trip_through_pillow(tmp_path, shape):
    from PIL import Image
    a = np.random.RandomState(sum(shape)).randint(0, 256, shape).astype(np.uint8)
    path = str(tmp_path / 'a.png')
    vis.save_png(path, a)
    with Image.open(path) as im:
        assert im.mode == ('RGB' if len(shape) == 3 else 'L')
        assert np.array_equal(np.asarray(im), a)


def test_save_png_refuses_other_arrays(tmp_path):
    for bad in (np.zeros((2, 2), np.float32), np.zeros((2, 2, 4), np.uint8), np.zeros((0, 2), np.uint8)):
        with pytest.raises(GenesisHipError, match='save_png'):
            vis.save_png(str(tmp_path / 'b.png'), bad)


def test_refusals_before_any_launch():
    with pytest.raises(GenesisHipError, match='normalize'):
        vis.make_grid(torch.zeros(2, 3, 4, 4), normalize=True)
    with pytest.raises(GenesisHipError, match='scale_each'):
        vis.make_grid(torch.zeros(2, 3, 4, 4), nrow=4, scale_each=False)
    with pytest.raises(GenesisHipError, match='neither 1 nor 3'):
        vis.make_grid(torch.zeros(2, 2, 4, 4))
    with pytest.raises(GenesisHipError, match='HIP device'):
        vis.make_grid(torch.zeros(2, 3, 4, 4))                       # a host tensor: there is no CPU path
    labels = torch.zeros(1, 2, 2, dtype=torch.int64)
    for bad in ([[1, 2]], [[1, 2, 300]], [[0.5, 0.5, 0.5]], [], 'no_such_palette', [[1, 2, 3]] * 257):
        with pytest.raises(GenesisHipError, match='palette'):
            vis.colour_seg_masks(labels, palette=bad)
    for bad in (torch.zeros(2, 2, dtype=torch.int64), torch.zeros(1, 1, 1, 2, 2, dtype=torch.int64)):
        with pytest.raises(GenesisHipError, match=r'\[B, H, W\]'):
            vis.colour_seg_masks(bad, palette=V.PALETTE15)
    with pytest.raises(GenesisHipError, match='integer labels'):
        vis.colour_seg_masks(torch.zeros(1, 2, 2), palette=V.PALETTE15)
    assert vis.load_palette(V.PALETTE15).tolist() == V.load_palette()


def _descriptor(**over):
    """One valid COPY descriptor of 2 images of 3 x 4 x 4 (fake addresses: validation reads no device memory)."""
    row = [0] * vis.DESC_WORDS
    fields = dict(SRC0=4096, STRIDE0=48, DST=0, WORK=0, ITEMS=32, KIND=vis.COPY, N=2, C=3, H=4, W=4, K=0, NROW=8, PADDING=2,
                  MODE=vis.FP32_CHW, VEC=0, PACKED=1, CELL0=0, N_GEOM=2, OWN_PAD=1)
    fields.update(over)
    for k, v in fields.items():
        row[getattr(vis, 'D_' + k)] = v
    return row


def _compose(rows, atlas_words, tail=()):
    table = np.array([w for row in rows for w in row] + list(tail), np.int64)
    _lib.call('gx_vis_compose', ctypes.c_void_p(table.ctypes.data), ctypes.c_void_p(4096), table.size, len(rows),
              ctypes.c_void_p(4096), 15, ctypes.c_void_p(4096), atlas_words, None)


@pytest.mark.parametrize('over, words, message', [
    (dict(KIND=4, K=33, C=1), 10 ** 6, r'K = 33 outside \[1, 32\]'),
    (dict(KIND=4, K=0, C=1), 10 ** 6, r'K = 0 outside \[1, 32\]'),
    (dict(C=2), 10 ** 6, 'C = 2 is neither 1 nor 3'),
    (dict(NROW=0), 10 ** 6, 'nrow = 0'),
    (dict(PADDING=-1), 10 ** 6, 'padding = -1'),
    (dict(), 3 * 8 * 14, 'pass the atlas'),               # the grid needs 3 x 8 x 14 words and the counter one more
    (dict(DST=-1), 10 ** 6, 'pass the atlas'),
    (dict(SRC0=0), 10 ** 6, 'null source'),
    (dict(KIND=2, SRC1=0), 10 ** 6, 'null mask source'),
    (dict(KIND=9), 10 ** 6, 'unknown kind'),
    (dict(MODE=2), 10 ** 6, 'unknown mode'),
    (dict(VEC=1, ITEMS=8, SRC0=4100), 10 ** 6, '16-byte loads'),
    (dict(ITEMS=31), 10 ** 6, 'ITEMS'),
    (dict(WORK=5), 10 ** 6, 'WORK'),
    (dict(CELL0=1), 10 ** 6, 'bad dims'),
])
def test_compose_refuses_before_launching(over, words, message):
    """Every descriptor error is a GX_EINVAL with a message, raised from the host copy of the table: no GPU is touched."""
    with pytest.raises(GenesisHipError, match=message):
        _compose([_descriptor(**over)], words)


def test_compose_checks_pointer_tables_and_the_prefix():
    good = _descriptor()
    with pytest.raises(GenesisHipError, match='WORK = 0, the prefix is 144'):       # 32 source items + 8 x 14 grid pixels
        _compose([good, _descriptor(DST=336)], 10 ** 6)
    argmax = dict(KIND=vis.ARGMAX_COLOUR, K=2, C=1, PACKED=0, SRC0=0, SRC1=vis.DESC_WORDS)
    with pytest.raises(GenesisHipError, match='plane 1 is null'):
        _compose([_descriptor(**argmax)], 10 ** 6, tail=(4096, 0))
    with pytest.raises(GenesisHipError, match='outside the table'):
        _compose([_descriptor(**argmax)], 10 ** 6, tail=(4096,))


@pytest.mark.skipif(not R.reference_available(), reason='the reference tree is not present')
def test_fixtures_regenerate_from_the_live_reference(tmp_path):
    """tests/golden/make_golden_visualise.py, run afresh on the reference's own train.visualise_outputs (in a process of its
    own: it installs stand-in modules and changes directory), gives the committed arrays bit for bit."""
    script = osp.join(REPO, 'tests', 'golden', 'make_golden_visualise.py')
    subprocess.run([sys.executable, script, '--out', str(tmp_path)], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    for case in S.CASES:
        old, new = S.load_case(case), S.load_case(case, str(tmp_path))
        assert sorted(old.files) == sorted(new.files)
        for key in old.files:
            assert old[key].dtype == new[key].dtype and old[key].shape == new[key].shape, (case, key)
            assert np.array_equal(old[key], new[key], equal_nan=old[key].dtype.kind == 'f'), (case, key)


def test_fixture_contents():
    """What the reference handed to its writer: the tags and their order, fp32 pictures and int64 colour grids."""
    g = S.load_case('v2')
    tags = [t for t, _ in S.recorded_calls(g)]
    assert tags[:6] == ['val_input', 'val_recon', 'val_instances_gt', 'val_instances', 'val_instances_r', 'val_mx_r_k/k0']
    assert tags[17] == 'samples' and tags[-1] == 'gen_mx_k/k2' and len(tags) == 27
    for tag, a in S.recorded_calls(g):
        assert a.shape == (3, 12, 82)
        assert a.dtype == (np.int64 if 'instances' in tag else np.float32), tag
    assert [t for t, _ in S.recorded_calls(S.load_case('nosample'))] == [
        'val_input', 'val_recon', 'val_instances_gt', 'val_instances', 'val_log_m_k/k0', 'val_log_m_k/k1', 'val_log_m_k/k2']
    assert 'val_instances_gt' not in [t for t, _ in S.recorded_calls(S.load_case('monet'))]
