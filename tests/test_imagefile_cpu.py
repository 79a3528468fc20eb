"""The host half of the loose-image-file path (genesis_amd/imagefile.py, image_folder_config.py) without a GPU: the C entropy
decoder for frames of any size, grey or colour (gx_jpeg_info_any, gx_jpeg_entropy_decode_any), followed by the numpy
restatement of the pixel arithmetic (tests/jpeg_restatement.py, extended here to one-component frames) against Pillow's
decoded pixels (tests/golden/imagefile_pil.npz, written by tests/golden/make_golden_imagefile.py) at zero tolerance; hostile
streams between guard bytes; the transform's sizes, window and table rows against Pillow's resize-then-crop; the staging
arena and the descriptor tables; the refusals; the argument checks of the three device entry points, which run before any
launch; the folder config's flags, splits and list files."""
import ctypes
import os
import os.path as osp
import random
import re
import sys

import numpy as np
import pytest

HERE = osp.dirname(osp.abspath(__file__))
GOLDEN = osp.join(HERE, 'golden')
sys.path.insert(0, GOLDEN)
sys.path.insert(0, HERE)
import jpeg_restatement as R  # noqa: E402
import make_golden_imagefile as MG  # noqa: E402
import png_restatement as PR  # noqa: E402

from genesis_amd import _lib, imagefile, jpeg, png  # noqa: E402
from genesis_amd._lib import GenesisHipError  # noqa: E402

REPO = osp.dirname(HERE)
GX_OK, GX_EINVAL, GX_EDATA = 0, -1, -3


@pytest.fixture(scope='module', autouse=True)
def flags_left_as_found():
    """A data config registers its flags when it is first imported, and the first definition of a name keeps its default:
    importing image_folder_config here must not decide the defaults the other data configs' tests see later."""
    from genesis_amd import compat
    compat.install()
    from forge import flags
    saved = dict(flags.FLAGS)
    yield
    flags.FLAGS.clear()
    flags.FLAGS.update(saved)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(MG.NPZ))


def decode_pixels_any(coef, qtab, info):
    """uint8 [H, W, 3] or, for a one-component frame, [H, W]: jpeg_restatement, extended to grey."""
    H, W = info.height, info.width
    if info.components == 3:
        return R.decode_pixels(coef, qtab, H, W, info.sampling)
    bh, bw = -(-H // 8), -(-W // 8)
    blk = np.asarray(coef)[:bh * bw * 64].astype(np.int64).reshape(-1, 8, 8) * np.asarray(qtab).reshape(3, 64)[0].astype(np.int64).reshape(8, 8)
    cols = R.idct_pass(blk.transpose(0, 2, 1), 11).transpose(0, 2, 1)
    px = np.clip(R.idct_pass(cols, 18) + 128, 0, 255)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:H, :W].astype(np.uint8)


def host_decode(stream):
    info = imagefile.jpeg_info_any(stream)
    coef = np.full(sum(info.blocks) * 64, 0x5555, dtype=np.int16)
    qtab = np.zeros(192, dtype=np.uint16)
    got = imagefile.entropy_decode_any(stream, coef, qtab)
    assert (got.width, got.height, got.components, got.sampling, got.blocks) == \
        (info.width, info.height, info.components, info.sampling, info.blocks)
    return info, decode_pixels_any(coef, qtab, info)


def pil_two_pass(u8, S):
    """Pillow's resize-then-crop from the project's table rows (imagefile.window_tables), in numpy: uint8 [S, S, 3]."""
    img = u8[:, :, None] if u8.ndim == 2 else u8
    img = np.repeat(img, 3, axis=2) if img.shape[2] == 1 else img[:, :, :3]
    H, W = img.shape[:2]
    h2, w2, (hb, hw, vb, vw) = imagefile.window_tables(H, W, S)
    assert hb.shape == (S, 2) and vb.shape == (S, 2) and hw.shape[0] == S and vw.shape[0] == S

    def one_pass(src, bounds, weights):           # along axis 0 of src
        out = np.empty((S,) + src.shape[1:], dtype=np.uint8)
        for i in range(S):
            first, n = int(bounds[i, 0]), int(bounds[i, 1])
            acc = (src[first:first + n].astype(np.int64) * weights[i, :n].astype(np.int64).reshape(-1, 1, 1)).sum(axis=0) + (1 << 21)
            out[i] = np.clip(acc >> 22, 0, 255)
        return out

    inter = one_pass(img.transpose(1, 0, 2), hb, hw).transpose(1, 0, 2)       # [H, S, 3]
    return one_pass(inter, vb, vw)


def test_the_fixture_covers_what_the_kernels_can_get_wrong(golden):
    assert osp.getsize(MG.NPZ) < 1000 * 1000
    sizes = {(c[1], c[2]) for c in MG.JPEG_CASES}
    assert sizes == {(1, 1), (16, 16), (7, 9), (136, 24), (24, 136), (145, 131), (264, 40), (131, 145), (200, 200), (520, 16),
                     (16, 520), (2056, 8)}
    assert {c[3] for c in MG.JPEG_CASES} == {0, 1, 2, None} and {c[4] for c in MG.JPEG_CASES} == {30, 75, 100}
    assert sum(bool(c[6]) for c in MG.JPEG_CASES) >= 1
    by = {(c[1], c[2]): c[3] for c in MG.JPEG_CASES}
    assert (by[(145, 131)], by[(264, 40)], by[(131, 145)], by[(200, 200)]) == (2, 1, 0, None)
    assert {(c[1], c[2], c[3]) for c in MG.PNG_CASES} == {(w, h, c) for (w, h) in ((7, 9), (145, 131), (520, 16)) for c in (1, 3, 4)} | {(9, 700, 4)}
    for name in MG.PNG_NAMES:
        assert set(MG.png_row_filters(golden[name + '_stream']).tolist()) == {0, 1, 2, 3, 4}, name
    # three or more bands / tiles of every kernel on each axis (the constants: the GPU test's docstring)
    assert 145 > 2 * imagefile.JPEGR_TILE_W and 131 > 2 * imagefile.JPEGR_TILE_H and 136 // 8 * 3 * 3 > imagefile.JPEGR_BLOCKS_PER_WG
    # the transform: upscales, an identity pass, an odd h' - S
    geo = [(n, S) + imagefile.resize_crop_geometry(*MG.case_size(n), S) for n in MG.CASE_NAMES for S in MG.SIZES]
    assert any(min(MG.case_size(n)) < S for n, S, *_ in geo)
    assert any(S in MG.case_size(n) for n, S, *_ in geo)
    assert any((h2 - S) % 2 == 1 or (w2 - S) % 2 == 1 for _, S, h2, w2, _, _ in geo)
    for name in MG.REFUSED:
        assert name in golden


def test_generator_and_module_state_the_same_transform():
    for H in (1, 7, 8, 9, 64, 131, 145, 520):
        for W in (1, 7, 8, 16, 63, 65, 136, 2056):
            for S in (1, 8, 20, 64):
                assert imagefile.resize_crop_geometry(H, W, S) == MG.resize_crop_geometry(H, W, S)
    # Python's round is half to even: 5 -> 2, 7 -> 4
    assert imagefile.resize_crop_geometry(13, 8, 8)[2:] == (2, 0) and imagefile.resize_crop_geometry(15, 8, 8)[2:] == (4, 0)


@pytest.mark.parametrize('name', MG.JPEG_NAMES)
def test_entropy_decoder_any_and_restatement_equal_pillow(golden, name):
    _, W, H, sampling, _, _, rst = MG.JPEG_CASES[MG.JPEG_NAMES.index(name)]
    info, px = host_decode(golden[name + '_stream'])
    assert (info.height, info.width) == (H, W) and info.restart_interval == rst
    assert (info.components, info.sampling) == ((1, 0) if sampling is None else (3, sampling))
    want_blocks = (-(-H // 8) * -(-W // 8), 0, 0) if sampling is None else jpeg.plane_blocks(H, W, sampling)
    assert info.blocks == want_blocks
    want = golden[name + '_u8']
    assert px.shape == want.shape
    assert int((px != want).sum()) == 0


def test_old_entry_points_keep_their_limits(golden):
    with pytest.raises(GenesisHipError, match='larger than'):
        jpeg.jpeg_info(golden['j145x131_420_q75_stream'])
    with pytest.raises(GenesisHipError, match='greyscale'):
        jpeg.jpeg_info(golden['j200x200_grey_q75_stream'])
    assert jpeg.jpeg_info(golden['j16x16_420_q100_stream']).geometry == (16, 16, 2)


def _sof(stream):
    at = bytes(stream).find(b'\xff\xc0')
    assert at > 0
    return at


def test_refusals_name_the_case(golden):
    base = golden['j16x16_420_q100_stream']
    sof = _sof(base)
    with pytest.raises(GenesisHipError, match='progressive'):
        imagefile.jpeg_info_any(golden['refuse_progressive'])
    with pytest.raises(GenesisHipError, match='four components'):
        imagefile.jpeg_info_any(golden['refuse_cmyk'])
    wide = base.copy()
    wide[sof + 11] = 0x12                               # H x V of the first component: 4:4:0
    with pytest.raises(GenesisHipError, match='sampling factors 1x2'):
        imagefile.jpeg_info_any(wide)
    wide[sof + 11] = 0x41                               # 4:1:1
    with pytest.raises(GenesisHipError, match='sampling factors 4x1'):
        imagefile.jpeg_info_any(wide)
    dqt = bytes(base).find(b'\xff\xdb')
    q16 = base.copy()
    q16[dqt + 4] |= 0x10
    with pytest.raises(GenesisHipError, match='16-bit quantisation'):
        imagefile.jpeg_info_any(q16)
    arith = base.copy()
    arith[sof + 1] = 0xC9
    with pytest.raises(GenesisHipError, match='arithmetic'):
        imagefile.jpeg_info_any(arith)
    big = base.copy()
    big[sof + 5:sof + 7] = (0x10, 0x01)                 # height 4097
    with pytest.raises(GenesisHipError, match='larger than the 4096 x 4096'):
        imagefile.jpeg_info_any(big)
    big[sof + 5:sof + 7] = (0x10, 0x00)                 # 4096: accepted
    assert imagefile.jpeg_info_any(big).height == 4096
    sos = bytes(base).find(b'\xff\xda')
    single = base.copy()
    single[sos + 4] = 1                                 # Ns: a scan of one of the three components
    with pytest.raises(GenesisHipError, match='one interleaved scan'):
        imagefile.jpeg_info_any(single)
    with pytest.raises(GenesisHipError, match='ends early'):
        imagefile.entropy_decode_any(base[:len(base) - 40], np.zeros(6 * 64, dtype=np.int16), np.zeros(192, dtype=np.uint16))
    with pytest.raises(GenesisHipError, match='the buffer holds'):
        imagefile.entropy_decode_any(base, np.zeros(5 * 64, dtype=np.int16), np.zeros(192, dtype=np.uint16))
    # the staging path: by magic bytes, then by header
    arena = imagefile.Arena(4, 1 << 20, pin=False)
    with pytest.raises(GenesisHipError, match='palette'):
        imagefile.stage_frame(arena, golden['refuse_palette'], 8, 4096)
    with pytest.raises(GenesisHipError, match='16-bit samples'):
        imagefile.stage_frame(arena, golden['refuse_png16'], 8, 4096)
    with pytest.raises(GenesisHipError, match='progressive'):
        imagefile.stage_frame(arena, golden['refuse_progressive'], 8, 4096)
    with pytest.raises(GenesisHipError, match='four components'):
        imagefile.stage_frame(arena, golden['refuse_cmyk'], 8, 4096)
    with pytest.raises(GenesisHipError, match='neither a PNG nor a JPEG'):
        imagefile.stage_frame(arena, b'GIF89a, say', 8, 4096)
    with pytest.raises(GenesisHipError, match=r'145 x 131 frame exceeds max_side = 144'):
        imagefile.stage_frame(arena, golden['p145x131_rgb_stream'], 8, 144)
    with pytest.raises(GenesisHipError, match='does not fit what is left of the staging arena'):
        imagefile.stage_frame(imagefile.Arena(1, 1024, pin=False), golden['p145x131_rgb_stream'], 8, 4096)
    assert arena.used == arena.desc_bytes               # a refused frame takes no room


@pytest.mark.parametrize('name', ['j7x9_422_q30', 'j24x136_420_q75_rst'])
def test_hostile_streams_stay_inside_their_buffers(golden, name):
    """Every prefix and seeded single-byte corruptions: GX_OK or GX_EDATA, and nothing written outside coef[:capacity] and
    qtab[:192], which sit between guard words."""
    stream = golden[name + '_stream']
    info = imagefile.jpeg_info_any(stream)
    n = sum(info.blocks) * 64
    lib = _lib.load()
    guard = 64
    coef = np.zeros(n + 2 * guard, dtype=np.int16)
    qtab = np.zeros(192 + 2 * guard, dtype=np.uint16)
    raw = np.zeros(8, dtype=np.int32)

    def run(data):
        coef[:guard] = coef[-guard:] = 0x1234
        qtab[:guard] = qtab[-guard:] = 0x4321
        rc = lib.gx_jpeg_entropy_decode_any(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.c_void_p(coef[guard:].ctypes.data), n,
                                            ctypes.c_void_p(qtab[guard:].ctypes.data), ctypes.c_void_p(raw.ctypes.data))
        assert (coef[:guard] == 0x1234).all() and (coef[-guard:] == 0x1234).all()
        assert (qtab[:guard] == 0x4321).all() and (qtab[-guard:] == 0x4321).all()
        rc2 = lib.gx_jpeg_info_any(ctypes.c_void_p(data.ctypes.data), data.size, ctypes.c_void_p(raw.ctypes.data))
        assert rc2 in (GX_OK, GX_EDATA)
        return rc

    assert run(np.ascontiguousarray(stream)) == GX_OK
    failures = 0
    for length in range(len(stream)):
        cut = np.ascontiguousarray(stream[:length]).copy()      # its own allocation: an over-read leaves the array
        rc = run(cut)
        assert rc in (GX_OK, GX_EDATA)
        failures += rc != GX_OK
    assert failures >= len(stream) - 4                  # all but the cuts inside the final EOI marker / padding
    start = bytes(stream).find(b'\xff\xda')
    start += 2 + ((int(stream[start + 2]) << 8) | int(stream[start + 3]))
    rng = np.random.RandomState(5)
    outcomes = set()
    for _ in range(1500):                               # inside the entropy-coded segment: the geometry stays
        bad = stream.copy()
        bad[rng.randint(start, len(stream))] = rng.randint(256)
        outcomes.add(run(bad))
    assert outcomes <= {GX_OK, GX_EDATA} and GX_OK in outcomes
    for _ in range(1500):                               # anywhere, headers included: a frame that grew is refused for its size
        bad = stream.copy()
        bad[rng.randint(0, len(stream))] = rng.randint(256)
        assert run(bad) in (GX_OK, GX_EDATA, GX_EINVAL)
        if run(bad) == GX_EINVAL:
            assert 'the buffer holds' in _lib.last_error()


@pytest.mark.parametrize('name', MG.CASE_NAMES)
def test_transform_arithmetic_equals_pillow(golden, name):
    """The restated size, window and table rows, pushed through two numpy passes, equal Pillow's resize-then-crop."""
    for S in MG.SIZES:
        got = pil_two_pass(golden[name + '_u8'], S)
        assert np.array_equal(got, golden['%s_s%d' % (name, S)]), (name, S)


def test_a_pass_that_keeps_its_size_is_the_identity():
    b, w = imagefile.axis_tables(20, 20)
    assert (b[:, 1] <= 2).all() and (b[:, 0] == np.arange(20)).all() and (w[:, 0] == 1 << 22).all() and (w[:, 1:] == 0).all()
    assert imagefile.axis_tables(20, 20)[0] is b        # cached


def test_staging_arena_and_descriptor_tables(golden):
    """A mixed batch staged by several threads into an unpinned arena: every frame's bytes, read back through its descriptor
    and the restatements, are Pillow's; the tables say what the header says they say."""
    from concurrent.futures import ThreadPoolExecutor
    names = ['p7x9_rgba', 'j145x131_420_q75', 'p520x16_grey', 'j200x200_grey_q75', 'j7x9_422_q30', 'p145x131_rgb', 'j1x1_420_q75']
    S = 20
    arena = imagefile.Arena(len(names), sum(imagefile.frame_bound(520, S) for _ in names), pin=False)
    with ThreadPoolExecutor(4) as pool:
        frames = list(pool.map(lambda n: imagefile.stage_frame(arena, golden[n + '_stream'], S, 520), names))
    L = imagefile.lay_out(arena, frames, S)
    assert L.n == len(names) and [names[i][0] for i in L.jpeg] == ['j'] * 4 and [names[i][0] for i in L.png] == ['p'] * 3
    assert L.used == arena.used <= arena.nbytes
    spans = sorted((f.payload, f.tables[3] * 4 + 4 * S * f.kv) for f in frames)
    assert spans[0][0] >= arena.desc_bytes and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= L.used
    host = arena.host
    wg_idct = wg_pix = planes = 0
    for row, i in zip(L.jt, L.jpeg):
        f, want = frames[i], golden[names[i] + '_u8']
        H, W, nc, sampling, coef_at, qtab_at, planes_at, dst, w0, w1 = (int(v) for v in row)
        assert (H, W) == want.shape[:2] and nc == (1 if want.ndim == 2 else 3)
        assert coef_at % 8 == 0 and qtab_at % 8 == 0 and planes_at % 16 == 0 and planes_at == planes and (w0, w1) == (wg_idct, wg_pix)
        assert dst == L.dst[i]
        info = imagefile.jpeg_info_any(golden[names[i] + '_stream'])
        coef = host.view(np.int16)[coef_at:coef_at + f.blocks * 64]
        qtab = host.view(np.uint16)[qtab_at:qtab_at + 192]
        assert np.array_equal(decode_pixels_any(coef, qtab, info), want)
        planes += f.blocks * 64
        wg_idct += -(-f.blocks // imagefile.JPEGR_BLOCKS_PER_WG)
        wg_pix += -(-H // imagefile.JPEGR_TILE_H) * -(-W // imagefile.JPEGR_TILE_W)
    assert L.scratch_bytes == planes
    for row, i in zip(L.pt, L.png):
        H, W, C, src, dst = (int(v) for v in row)
        want = golden[names[i] + '_u8']
        assert (H, W) == want.shape[:2] and C == (1 if want.ndim == 2 else want.shape[2]) and dst == L.dst[i]
        got = PR.unfilter(host[src:src + H * (1 + W * C)], H, W, C)
        assert np.array_equal(got.reshape(want.shape), want)
    wg = 0
    tables = host.view(np.int32)
    for row, f, name in zip(L.rt, frames, names):
        Hs, Ws, C, src, H2, W2, hb, hw, kh, vb, vw, kv, Rr, wg0 = (int(v) for v in row)
        h2, w2, top, left = imagefile.resize_crop_geometry(Hs, Ws, S)
        assert (H2, W2) == (h2, w2) and wg0 == wg and 1 <= Rr <= 8
        wg += -(-S // Rr)
        whole_b, whole_w = imagefile.axis_tables(Ws, w2)
        assert kh == whole_w.shape[1] and np.array_equal(tables[hb:hb + 2 * S].reshape(S, 2), whole_b[left:left + S])
        assert np.array_equal(tables[hw:hw + kh * S].reshape(S, kh), whole_w[left:left + S])
        whole_b, whole_w = imagefile.axis_tables(Hs, h2)
        assert kv == whole_w.shape[1] and np.array_equal(tables[vb:vb + 2 * S].reshape(S, 2), whole_b[top:top + S])
        assert np.array_equal(tables[vw:vw + kv * S].reshape(S, kv), whole_w[top:top + S])
    offs = sorted(zip(L.dst, (f.H * f.W * f.C for f in frames)))
    assert all(a + n <= b for (a, n), (b, _) in zip(offs, offs[1:])) and offs[-1][0] + offs[-1][1] <= L.dst_bytes


def test_header_and_module_agree_on_the_descriptor_layout():
    header = open(osp.join(REPO, 'include', 'genesis_hip.h')).read()
    defines = {k: int(v) for k, v in re.findall(r'#define (GX_(?:JPEGR|PNGR|RSR)_\w+) (\d+)', header)}
    assert (defines['GX_JPEGR_DESC_WORDS'], defines['GX_PNGR_DESC_WORDS'], defines['GX_RSR_DESC_WORDS']) == \
        (imagefile.JPEGR_WORDS, imagefile.PNGR_WORDS, imagefile.RSR_WORDS)
    assert (defines['GX_JPEGR_BLOCKS_PER_WG'], defines['GX_JPEGR_TILE_H'], defines['GX_JPEGR_TILE_W']) == \
        (imagefile.JPEGR_BLOCKS_PER_WG, imagefile.JPEGR_TILE_H, imagefile.JPEGR_TILE_W)
    for prefix, words in (('GX_JPEGR_D_', 10), ('GX_PNGR_D_', 5), ('GX_RSR_D_', 14)):
        assert sorted(v for k, v in defines.items() if k.startswith(prefix)) == list(range(words))
    assert [defines['GX_RSR_D_' + k] for k in ('HS', 'WS', 'C', 'SRC', 'H2', 'W2', 'HB', 'HW', 'KH', 'VB', 'VW', 'KV', 'R', 'WG0')] == list(range(14))
    assert [defines['GX_JPEGR_D_' + k] for k in ('H', 'W', 'NCOMP', 'SAMPLING', 'COEF', 'QTAB', 'PLANES', 'DST', 'WG0_IDCT', 'WG0_PIX')] == list(range(10))
    common = open(osp.join(REPO, 'genesis_amd', 'csrc', 'gx_common.h')).read()
    assert 'constexpr int kGxImageMaxDim = kGxPngMaxDim;' in common and imagefile.MAX_DIM == png.MAX_DIM


def test_device_entry_points_check_their_tables_before_any_launch(golden):
    """A bad word in the host table is GX_EINVAL with a message that names the frame: nothing is launched (no GPU here)."""
    FAKE = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced: every case fails the checks
    S = 8
    arena = imagefile.Arena(2, 1 << 20, pin=False)
    frames = [imagefile.stage_frame(arena, golden[n + '_stream'], S, 4096) for n in ('j145x131_420_q75', 'p7x9_rgb')]
    L = imagefile.lay_out(arena, frames, S)

    def jpeg_call(table, **kw):
        _lib.call('gx_jpeg_decode_ragged', imagefile._ptr(table), FAKE, kw.get('n', 1), FAKE, kw.get('coef', L.used // 2), FAKE, L.used // 2,
                  FAKE, kw.get('scratch', L.scratch_bytes), FAKE, kw.get('dst', L.dst_bytes), None)

    def png_call(table, **kw):
        _lib.call('gx_png_unfilter_ragged', imagefile._ptr(table), FAKE, kw.get('n', 1), FAKE, kw.get('src', L.used), FAKE,
                  kw.get('dst', L.dst_bytes), None)

    def rsr_call(table, **kw):
        _lib.call('gx_u8_resample_ragged_f32chw', imagefile._ptr(table), FAKE, kw.get('n', 2), FAKE, kw.get('src', L.dst_bytes), FAKE,
                  kw.get('tables', L.used // 4), FAKE, kw.get('S', S), kw.get('S', S), None)

    with pytest.raises(GenesisHipError, match='n_frames = 0'):
        jpeg_call(L.jt.copy(), n=0)
    for word, value, what in ((0, 4097, 'outside'), (2, 2, 'components'), (3, 3, 'sampling'), (4, 4, 'COEF'), (4, -8, 'COEF'),
                              (5, L.used, 'QTAB'), (6, 8, 'PLANES'), (7, L.dst_bytes, 'DST'), (8, 1, 'WG0'), (9, 1, 'WG0')):
        t = L.jt.copy()
        t[0, word] = value
        with pytest.raises(GenesisHipError, match='frame 0.*%s' % what):
            jpeg_call(t)
    with pytest.raises(GenesisHipError, match='end outside the .* of coef'):
        jpeg_call(L.jt.copy(), coef=int(L.jt[0, 4]) + 64)
    with pytest.raises(GenesisHipError, match='of scratch'):
        jpeg_call(L.jt.copy(), scratch=L.scratch_bytes - 1)
    for word, value, what in ((1, 0, 'outside'), (2, 2, 'C = 2'), (3, L.used, 'SRC'), (3, -1, 'SRC'), (4, L.dst_bytes, 'DST')):
        t = L.pt.copy()
        t[0, word] = value
        with pytest.raises(GenesisHipError, match='frame 0.*%s' % what):
            png_call(t)
    for word, value, what in ((0, 0, 'outside'), (2, 5, 'C = 5'), (3, L.dst_bytes, 'SRC'), (4, S - 1, 'does not hold'), (8, 99, 'ksize'),
                              (6, L.used, 'table word 6'), (10, -4, 'table word 10'), (12, 3, 'gx_u8_resample_ragged_plan'),
                              (13, 7, 'gx_u8_resample_ragged_plan')):
        t = L.rt.copy()
        t[1, word] = value
        with pytest.raises(GenesisHipError, match='frame 1.*%s' % what):
            rsr_call(t)
    with pytest.raises(GenesisHipError, match='bad output size'):
        rsr_call(L.rt.copy(), S=0)
    with pytest.raises(GenesisHipError, match='null pointer'):
        _lib.call('gx_png_unfilter_ragged', None, FAKE, 1, FAKE, 1, FAKE, 1, None)


def test_batch_level_refusals_need_no_gpu(golden):
    import torch
    with pytest.raises(GenesisHipError, match='an empty batch'):
        imagefile.decode_image_batch([], 8)
    with pytest.raises(GenesisHipError, match='img_size must be an int'):
        imagefile.decode_image_batch([golden['p7x9_rgb_stream']], (8, 8))
    with pytest.raises(GenesisHipError, match='no CPU path'):
        imagefile.decode_image_batch([golden['p7x9_rgb_stream']], 8, device='cpu')
    with pytest.raises(GenesisHipError, match='out must be on the HIP device'):
        imagefile.decode_image_batch([golden['p7x9_rgb_stream']], 8, out=torch.empty(1, 3, 8, 8))
    with pytest.raises(GenesisHipError, match='max_side must be an int'):
        imagefile.ImageFileLoader(['a.png'], 2, 8, max_side=5000)
    with pytest.raises(GenesisHipError, match='shard'):
        imagefile.ImageFileLoader(['a.png'], 2, 8, shard=(2, 2))
    loader = imagefile.ImageFileLoader(['%d.png' % i for i in range(11)], 4, 8, shard=(1, 2))
    assert len(loader) == 2 and loader.files == ['1.png', '3.png', '5.png', '7.png', '9.png'] and loader.batch_size == 4
    assert imagefile.ImageFileLoader([], 4, 8, num_workers=40).workers == 16


def test_folder_config_flags_and_defaults():
    import importlib
    import genesis_amd.image_folder_config as F
    from forge import flags
    defaults = (('data_folder', 'data/images'), ('img_size', 64), ('num_workers', 4), ('K_steps', 7))
    saved = {name: flags.FLAGS.pop(name) for name, _ in defaults if name in flags.FLAGS}
    try:
        F = importlib.reload(F)
        for name, default in defaults:
            assert flags.FLAGS[name] == default
    finally:
        flags.FLAGS.update(saved)
    assert F.MODES == ('train', 'val', 'test')


def _write_tree(root, names, golden, rel):
    paths = []
    for i, (name, r) in enumerate(zip(names, rel)):
        path = osp.join(root, r)
        os.makedirs(osp.dirname(path), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(bytes(golden[name + '_stream']))
        paths.append(r)
    return paths


def test_folder_config_splits_and_list_files(tmp_path, golden):
    import genesis_amd.image_folder_config as F
    names = [MG.CASE_NAMES[i % len(MG.CASE_NAMES)] for i in range(23)]
    ext = lambda n, i: ('.PNG' if i % 2 else '.png') if n[0] == 'p' else ('.jpg', '.JPEG', '.jpeg', '.Jpg')[i % 4]   # noqa: E731
    # one flat-ish folder: the seeded split
    flat = str(tmp_path / 'flat')
    rel = [osp.join('sub%d' % (i % 3), 'f%02d%s' % (i, ext(n, i))) for i, n in enumerate(names)]
    _write_tree(flat, names, golden, rel)
    with open(osp.join(flat, 'notes.txt'), 'w') as f:
        f.write('not an image\n')
    want = sorted(rel)
    random.Random(0).shuffle(want)
    splits = {m: F.split_files(flat, m) for m in F.MODES}
    assert splits['val'] == sorted(want[:2]) and splits['test'] == sorted(want[2:4]) and splits['train'] == sorted(want[4:])
    for m in F.MODES:
        assert open(F.list_path(flat, m)).read().split() == splits[m]
    # the list file decides from then on
    with open(F.list_path(flat, 'val'), 'w') as f:
        f.write(splits['train'][0] + '\n')
    assert F.split_files(flat, 'val') == [splits['train'][0]] and F.split_files(flat, 'train') == splits['train']
    # split folders: each folder is a split, recursive, sorted
    tree = str(tmp_path / 'tree')
    rel = [osp.join(('train', 'train', 'val', 'test')[i % 4], 'd%d' % (i % 2), 'f%02d%s' % (i, ext(n, i))) for i, n in enumerate(names)]
    _write_tree(tree, names, golden, rel)
    for m in F.MODES:
        assert F.split_files(tree, m) == sorted(r for r in rel if r.startswith(m + os.sep))
        assert osp.exists(F.list_path(tree, m))
    with pytest.raises(ValueError):
        F.split_files(tree, 'valid')
    from genesis_amd.compat.attrdict import AttrDict
    with pytest.raises(GenesisHipError, match='does not exist'):
        F.load(AttrDict(data_folder=str(tmp_path / 'nowhere'), img_size=8, num_workers=2, batch_size=4))
    train, val, test = F.load(AttrDict(data_folder=tree, img_size=8, num_workers=2, batch_size=4, seed=3), shard=(1, 2))
    assert [len(l.files) for l in (train, val, test)] == [6, 3, 2] and len(train) == 2 and train.batch_size == 4
    assert train.files == [osp.join(tree, r) for r in F.split_files(tree, 'train')[1::2]]
