"""gx_igemm.hip off the beaten path: the generic implicit-GEMM conv (any k <= 5, stride, pad; forward, data gradient, weight gradient)
and the three stride-2 3 x 3 vector-ALU kernels at every plan their host code can pick, on the harness of
tests/test_conv_plans_gpu.py (whose tables stay as they are).  fwd_splits / wgrad_splits / fwd_small_ok / the `few` rule choose
grids, split counts, template instantiations and which of three forward paths runs; the workloads reach a few of those.  Every
row DECLARES the whole gx_conv_last_plan record it is meant to reach (family, grid, split, chunks per slab; lG = log2 CIB and
nq = UB for the stride-2 data gradient) and the tails it has.  Every case

  1. puts every operand in the middle of a larger device buffer whose remainder is NaN,
  2. puts every output between GUARD sentinel floats (the output itself starts as NaN) and a NaN-filled workspace, sized by the
     entry point's own query, between WS_GUARD bands, and calls the C entry point through _lib.call with explicit pointers,
  3. asserts that the recorded plan EQUALS the declared one, field for field (a case that lands elsewhere fails the table), and
     that the tails computed from record and shape equal the declared set; the weight gradients note nothing (the record must be
     the one from before) and their split count is read from gx_conv2d_direct_wgrad_ws_bytes / (4 M Ncols),
  4. compares with float64 F.conv2d autograd on the CPU at the bounds tests/test_kernels_gpu.py applies to the same entry point:
     forward 2e-5 / 2e-5, generic data gradient 1e-4 / 2e-5, generic weight gradient 1e-4 / 1e-4 (test_conv2d_direct), stride-2
     data gradient 1e-5 / 1e-5 (test_conv3x3_stride2_dgrad_on_the_vector_alus), stride-2 weight gradient rtol 1e-5 and
     atol 2e-6 max |dw| (test_conv3x3_stride2_wgrad_on_the_vector_alus).  No bound of this file is new,
  5. asserts finite values and bit-identical guard bands; launches with a split reduce run twice and must be bit-equal.

Every forward row with a split is also called with a NULL workspace and through gx_conv2d_direct_fwd: the record must show the
single-launch form (nsplit 1) and the values stay inside the same bound.

What each class would catch (one-line mistakes in the code it reaches; argued from the code, never run):

  igemm, grid_y = 2 / 3 (M = 70, 130), any mode         `m0` missing from the A row index or from the store (channels 64.. get the
                                                        first tile's values), the M tail stored without `m < M` (the next image)
  igemm K = 3 (fewer than one wave's four slots)        a contraction slot read without `kk < K` (NaN operand surround)
  igemm k = 1, 2, 4 (FastDiv d = 1, 4, 16: mul 0)       the d == 1 shortcut, a shift of -1, a power-of-two divisor's magic of 2^32
  igemm stride 3, (H + 2p - k) % s != 0                 MODE 1's `/ stride` branch; `oh * s == th` or `oh < Ho` missing after the
                                                        division (rows no window reaches must be EXACT zeros; dy's NaN surround)
  igemm pad 3 with k = 3                                `ih >= 0` / `ih < H` taken from the output grid, windows wholly in padding
  igemm dgrad grid_x = 12, 13                           the XCD tile map with a remainder (r = 4, 5): a tile computed twice and
                                                        another never (NaN output), n0 past Ncols
  igemm tiles straddling images                         `img` taken per tile instead of per column
  igemm forward split: uneven, empty slabs              c_end past nchunks, a slab the reduce reads but nobody wrote (NaN
                                                        workspace), the slab stride without the M tail, bias / act applied per slab
  igemm wgrad 10 / 17 / 25 slabs, grid_x = 5, 8         the slab stride, a reduce over nsplit where zs slabs were written
  s2 forward, Cout % 8 = 4 / 2, pixel tail, Cin = 64    `co0 + c < Cout` missing on the store (the next image), `q < N Ho Wo`,
                                                        the LDS weight block sized for another Cin
  s2 forward where the split predicate also holds       the order of the two dispatch rules (the record names the path)
  s2 dgrad CIB 4 / 2, UB 1 / 8, cin_n % CIB != 0        CIB tail channels stored past cin_n (NaN must survive in the channels
                                                        behind), dy channels co0 + u >= Cout read (the next image) or used
  s2 dgrad dx_channels = 1, 2, 4 with cin_n = 1         the image stride of dx taken from Cin or cin_n instead of dx_channels
  s2 dgrad 2 x 2 images, rectangular grids              `jr` / `ir` swapped, Wo used where Ho is meant
  s2 wgrad S = 1, 2, 5; Cout = 17, 9, 5                 the pixel chunk of the last split, COB tail rows written past Cout
  wrappers refuse a wrong Cin / kernel / grid / batch   a launch on trusted shapes (the record must stay the one from before)
  DirectConvActFn / sylvester.DirectConvFn / the        the branch conditions (even grid, powers of two, H < 4, out_pad), x and dy in
  BroadcastDecoder's wide head                          each other's roles for the transposed conv's weight gradient
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from genesis_amd import hip_ops
from tests import test_conv_plans_gpu as T
from tests.test_conv_plans_gpu import DEV, WS_GUARD, close, rnd

pytestmark = pytest.mark.gpu

FWD_TOL = (2e-5, 2e-5)          # rtol, atol: tests/test_kernels_gpu.py test_conv2d_direct 'fwd'
DG_TOL = (1e-4, 2e-5)           # ... 'dgrad'
WG_TOL = (1e-4, 1e-4)           # ... 'wgrad'
S2DG_TOL = (1e-5, 1e-5)         # test_conv3x3_stride2_dgrad_on_the_vector_alus
IGEMM_FAMILIES = ('igemm_fwd', 'igemm_dg', 's2_fwd', 's2_dg')


def cd(a, b):
    return -(-a // b)


# ===================================================================================================== declared records
def rec(family, **fields):
    """A whole gx_conv_last_plan record: form fp32, every field the row does not state is 0."""
    r = dict.fromkeys(hip_ops.PLAN_FIELDS, 0)
    r.update(family=family, form='fp32')
    r.update(fields)
    return r


def FW(grid_x, grid_y, nsplit, chunks):
    """igemm_kernel<0>: 128-column tiles, grid_z = the slabs of the split contraction, `chunks` 16-wide chunks per slab."""
    return rec('igemm_fwd', pixels=128, grid_x=grid_x, grid_y=grid_y, grid_z=nsplit, nsplit=nsplit, chunks_per_split=chunks)


def DG(grid_x, grid_y, chunks):
    return rec('igemm_dg', pixels=128, grid_x=grid_x, grid_y=grid_y, grid_z=1, nsplit=1, chunks_per_split=chunks)


def S2F(grid_x, grid_y):
    return rec('s2_fwd', pixels=256, grid_x=grid_x, grid_y=grid_y)


def S2D(cib, ub, grid_x, grid_y):
    return rec('s2_dg', pixels=256, lG={2: 1, 4: 2}[cib], nq=ub, grid_x=grid_x, grid_y=grid_y)


# ===================================================================================================== the case tables
def G(rid, dims, fwd, dg, wsplit, tails, act=None):
    """A generic row: dims (N, Cin, Cout, H, W, k, stride, pad); the forward and data-gradient records, the weight gradient's
    slab count, the tails of all three ('f.', 'd.', 'w.') and of the shape."""
    return dict(id=rid, dims=dims, fwd=fwd, dg=dg, wsplit=wsplit, tails=frozenset(tails), act=act)


GENERIC_CASES = [
    G('ig-k1-7x11-k3slots', (2, 3, 5, 7, 11, 1, 1, 0), FW(2, 1, 1, 1), DG(2, 1, 1), 10,
      {'k1', 'pad0', 'rect', 'f.m_tail', 'f.n_tail', 'f.n_tiles', 'f.k_tail', 'f.k_lt_wave', 'f.straddle', 'd.m_tail', 'd.n_tail',
       'd.n_tiles', 'd.k_tail', 'd.straddle', 'w.m_tail', 'w.n_tail', 'w.k_tail', 'w.splitk'}, act='relu'),
    G('ig-k2-s2-6x10', (2, 5, 3, 6, 10, 2, 2, 0), FW(1, 1, 1, 2), DG(1, 1, 1), 2,
      {'k2', 'pad0', 'rect', 'f.m_tail', 'f.n_tail', 'f.k_tail', 'f.straddle', 'd.m_tail', 'd.n_tail', 'd.k_tail', 'd.straddle',
       'w.m_tail', 'w.n_tail', 'w.k_tail', 'w.splitk'}),
    G('ig-k3-s3-9x13-zero-rows', (1, 4, 6, 9, 13, 3, 3, 1), FW(1, 1, 1, 3), DG(1, 1, 4), 1,
      {'k3', 's3', 'rect', 'f.m_tail', 'f.n_tail', 'f.k_tail', 'd.m_tail', 'd.n_tail', 'd.k_tail', 'd.zero_rows', 'w.m_tail',
       'w.n_tail', 'w.k_tail'}, act='elu'),
    G('ig-k4-s2-8x5', (2, 3, 4, 8, 5, 4, 2, 1), FW(1, 1, 1, 3), DG(1, 1, 4), 1,
      {'k4', 'rect', 'f.m_tail', 'f.n_tail', 'f.straddle', 'd.m_tail', 'd.n_tail', 'd.straddle', 'w.m_tail', 'w.n_tail'}),
    G('ig-k3-pad3-4x6', (1, 2, 3, 4, 6, 3, 1, 3), FW(1, 1, 1, 2), DG(1, 1, 2), 5,
      {'k3', 'rect', 'pad_window', 'f.m_tail', 'f.n_tail', 'f.k_tail', 'd.m_tail', 'd.n_tail', 'd.k_tail', 'w.m_tail', 'w.n_tail',
       'w.splitk'}, act='relu'),
    G('ig-k3-s2-pad0-n9-14x12-xcd12', (9, 2, 5, 14, 12, 3, 2, 0), FW(3, 1, 1, 2), DG(12, 1, 3), 17,
      {'k3', 'pad0', 'rect', 'f.m_tail', 'f.n_tail', 'f.n_tiles', 'f.k_tail', 'f.straddle', 'd.m_tail', 'd.n_tail', 'd.n_tiles',
       'd.k_tail', 'd.straddle', 'd.xcd_rem', 'd.zero_rows', 'w.m_tail', 'w.n_tail', 'w.k_tail', 'w.splitk'}),
    G('ig-k3-s2-n3-12x44-xcd13', (3, 4, 8, 12, 44, 3, 2, 1), FW(4, 1, 1, 3), DG(13, 1, 5), 25,
      {'k3', 'rect', 'f.m_tail', 'f.n_tail', 'f.n_tiles', 'f.k_tail', 'f.straddle', 'd.m_tail', 'd.n_tail', 'd.n_tiles', 'd.k_tail',
       'd.straddle', 'd.xcd_rem', 'w.m_tail', 'w.n_tail', 'w.k_tail', 'w.splitk'}, act='elu'),
    G('ig-m70-9x7', (2, 3, 70, 9, 7, 3, 2, 1), FW(1, 2, 1, 2), DG(1, 1, 40), 3,
      {'k3', 'rect', 'f.m_tail', 'f.m_tiles', 'f.n_tail', 'f.k_tail', 'f.straddle', 'd.m_tail', 'd.n_tail', 'd.k_tail', 'd.straddle',
       'w.m_tail', 'w.m_tiles', 'w.n_tail', 'w.k_tail', 'w.splitk'}, act='relu'),
    G('ig-cin70-6x6-split10x4', (1, 70, 3, 6, 6, 3, 1, 1), FW(1, 1, 10, 4), DG(1, 2, 2), 3,
      {'k3', 'f.m_tail', 'f.n_tail', 'f.k_tail', 'f.splitk', 'd.m_tail', 'd.m_tiles', 'd.n_tail', 'd.k_tail', 'w.m_tail', 'w.n_tail',
       'w.n_tiles', 'w.k_tail', 'w.splitk'}, act='elu'),
    G('ig-m130-6x10-split2-uneven', (1, 16, 130, 6, 10, 3, 1, 1), FW(1, 3, 2, 5), DG(1, 1, 74), 4,
      {'k3', 'rect', 'f.m_tail', 'f.m_tiles', 'f.n_tail', 'f.splitk', 'f.splitk_uneven', 'd.m_tail', 'd.n_tail', 'd.k_tail', 'w.m_tail',
       'w.m_tiles', 'w.n_tail', 'w.n_tiles', 'w.k_tail', 'w.splitk'}, act='relu'),
    G('ig-k5-cin21-6x6-split8-slab7-empty', (1, 21, 8, 6, 6, 5, 1, 2), FW(1, 1, 8, 5), DG(1, 1, 13), 3,
      {'k5', 'f.m_tail', 'f.n_tail', 'f.k_tail', 'f.splitk', 'f.splitk_uneven', 'f.slab_empty', 'd.m_tail', 'd.n_tail', 'd.k_tail',
       'w.m_tail', 'w.n_tail', 'w.n_tiles', 'w.k_tail', 'w.splitk'}),
    G('ig-k5-s2-cin40-4x4-split15-two-empty', (1, 40, 8, 4, 4, 5, 2, 2), FW(1, 1, 15, 5), DG(1, 1, 13), 1,
      {'k5', 'f.m_tail', 'f.n_tail', 'f.k_tail', 'f.splitk', 'f.splitk_uneven', 'f.slab_empty', 'd.m_tail', 'd.n_tail', 'd.k_tail',
       'w.m_tail', 'w.n_tail', 'w.n_tiles', 'w.k_tail'}, act='elu'),
]


def generic_shape(dims):
    """(Ho, Wo) and the GEMM (M, Ncols, K) of the three modes (ig_geom)."""
    N, Cin, Cout, H, W, k, s, p = dims
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return Ho, Wo, {'f': (Cout, N * Ho * Wo, Cin * k * k), 'd': (Cin, N * H * W, Cout * k * k), 'w': (Cout, Cin * k * k, N * Ho * Wo)}


def generic_tails(dims, fwd, dg, wsplit):
    """The tails launches with these records have on this shape -- every declared set is checked against it."""
    N, Cin, Cout, H, W, k, s, p = dims
    Ho, Wo, gemm = generic_shape(dims)
    t = {'k%d' % k}
    if s > 2:
        t.add('s%d' % s)
    if p == 0:
        t.add('pad0')
    if p >= k:
        t.add('pad_window')          # windows that lie wholly in the padding
    if H != W:
        t.add('rect')
    for m, plan, per_image in (('f', fwd, Ho * Wo), ('d', dg, H * W), ('w', None, 0)):
        M, Ncols, K = gemm[m]
        gx, gy = (plan['grid_x'], plan['grid_y']) if plan else (cd(Ncols, 128), cd(M, 64))
        if M % 64:
            t.add(m + '.m_tail')
        if gy > 1:
            t.add(m + '.m_tiles')
        if Ncols % 128:
            t.add(m + '.n_tail')
        if gx > 1:
            t.add(m + '.n_tiles')
        if K % 16:
            t.add(m + '.k_tail')
        if per_image and N > 1 and per_image % 128:
            t.add(m + '.straddle')   # a 128-column tile holds pixels of two images
        if plan and gx > 8 and gx % 8:
            t.add(m + '.xcd_rem')
    if gemm['f'][2] < 4:
        t.add('f.k_lt_wave')
    nchunks = cd(gemm['f'][2], 16)
    if fwd['nsplit'] > 1:
        t.add('f.splitk')
        if nchunks % fwd['chunks_per_split']:
            t.add('f.splitk_uneven')
        if (fwd['nsplit'] - 1) * fwd['chunks_per_split'] >= nchunks:
            t.add('f.slab_empty')
    if (Ho - 1) * s + k - 1 - p < H - 1 or (Wo - 1) * s + k - 1 - p < W - 1:
        t.add('d.zero_rows')         # input rows / columns no window reaches: their gradient is exactly zero
    if wsplit > 1:
        t.add('w.splitk')
    return t


# ---- the stride-2 3 x 3 kernels: dims (N, Cin, Cout, H, W)
def S(rid, dims, plan, tails, fallback=None, act='relu'):
    """fallback: the record of the same call with a NULL workspace (rows whose declared plan is the split)."""
    return dict(id=rid, dims=dims, plan=plan, tails=frozenset(tails), fallback=fallback, act=act)


S2_FWD_CASES = [
    S('s2f-256x256-cout60-512wg', (1, 3, 60, 256, 256), S2F(8, 64), {'co_tail', 'exact_512'}),
    S('s2f-n5-116x116-pixel-tail', (5, 3, 60, 116, 116), S2F(8, 66), {'co_tail', 'pix_tail', 'straddle'}, act='elu'),
    S('s2f-128x512-cout58', (1, 2, 58, 128, 512), S2F(8, 64), {'co_tail', 'rect', 'exact_512'}, act=None),
    S('s2f-cin64-256x256', (1, 64, 60, 256, 256), S2F(8, 64), {'co_tail', 'cin_max', 'exact_512'}),
    # 16 x 16 = 256 workgroups < 512: the small predicate does NOT hold here (the split alone does); the row after it is the one
    # where both hold (2 x 256 = 512 workgroups, 3 x 32 = 96 tiles) and the split, asked first, wins -- its NULL-workspace call
    # then takes the small kernel
    S('s2f-126x128-cout128-split2', (1, 16, 128, 126, 128), FW(32, 2, 2, 5), {'rect', 'pix_tail', 'splitk', 'splitk_uneven'},
      fallback=FW(32, 2, 1, 9)),
    S('s2f-32x40-cout2048-both-predicates', (1, 16, 2048, 32, 40), FW(3, 32, 2, 5),
      {'rect', 'pix_tail', 'splitk', 'splitk_uneven', 'split_over_small'}, fallback=S2F(256, 2), act='elu'),
]


def small_predicate(dims):
    """fwd_small_ok of a conv3x3 stride 2 pad 1 row."""
    N, Cin, Cout, H, W = dims
    q = cd(N * (H // 2) * (W // 2), 256)
    return H % 2 == 0 and W % 2 == 0 and Cin <= 64 and cd(Cout, 8) * q >= 512 and q <= 65535


def s2_fwd_tails(dims, plan):
    N, Cin, Cout, H, W = dims
    P = N * (H // 2) * (W // 2)
    t = set()
    if H != W:
        t.add('rect')
    if P % 256:
        t.add('pix_tail')
    if plan['family'] == 's2_fwd':
        if Cout % 8:
            t.add('co_tail')
        if N > 1 and (H // 2) * (W // 2) % 256:
            t.add('straddle')
        if Cin == 64:
            t.add('cin_max')
        if plan['grid_x'] * plan['grid_y'] == 512:
            t.add('exact_512')
    else:
        if plan['nsplit'] > 1:
            t.add('splitk')
            if cd(Cin * 9, 16) % plan['chunks_per_split']:
                t.add('splitk_uneven')
            if small_predicate(dims):
                t.add('split_over_small')
    return t


def D(rid, dims, cin_n, dxc, plan, tails, via='small'):
    """via: 'small' gx_conv3x3s2_dgrad_small (dx has Cin channels), 'ex' gx_conv3x3s2_dgrad_small_ex with dx_channels = dxc,
    'lead' hip_ops.conv3x3s2_dgrad_lead (the wrapper: a compact [N, cin_n, H, W])."""
    return dict(id=rid, dims=dims, cin_n=cin_n, dxc=dxc, plan=plan, tails=frozenset(tails), via=via)


S2_DG_CASES = [
    D('s2d-512x512-cin5-cib4-ub1', (1, 5, 3, 512, 512), 5, 5, S2D(4, 1, 2, 256), {'ci_tail'}),
    D('s2d-724x364-cin7-cib4-ub1', (1, 7, 3, 724, 364), 7, 7, S2D(4, 1, 2, 258), {'ci_tail', 'pix_tail', 'rect'}),
    D('s2d-1024x512-cin2-cib2-ub1', (1, 2, 3, 1024, 512), 2, 2, S2D(2, 1, 1, 512), {'rect'}),
    D('s2d-12x20-cin-n3-of-6', (2, 6, 10, 12, 20), 3, 6, S2D(4, 8, 1, 1), {'ci_tail', 'co_tail_ub', 'partial', 'pix_tail', 'rect', 'straddle'}),
    D('s2d-6x10-lead1', (3, 4, 5, 6, 10), 1, 1, S2D(2, 8, 1, 1), {'ci_tail', 'co_tail_ub', 'pix_tail', 'rect', 'straddle'}, via='lead'),
    D('s2d-6x10-ex-dxc1', (3, 4, 5, 6, 10), 1, 1, S2D(2, 8, 1, 1), {'ci_tail', 'co_tail_ub', 'pix_tail', 'rect', 'straddle'}, via='ex'),
    D('s2d-6x10-ex-dxc2', (3, 4, 5, 6, 10), 1, 2, S2D(2, 8, 1, 1), {'ci_tail', 'co_tail_ub', 'partial', 'pix_tail', 'rect', 'straddle'},
      via='ex'),
    D('s2d-6x10-ex-dxc4', (3, 4, 5, 6, 10), 1, 4, S2D(2, 8, 1, 1), {'ci_tail', 'co_tail_ub', 'partial', 'pix_tail', 'rect', 'straddle'},
      via='ex'),
    D('s2d-2x2-one-block-per-image', (2, 3, 4, 2, 2), 3, 3, S2D(4, 8, 1, 1), {'ci_tail', 'co_tail_ub', 'pix_tail', 'straddle', 'one_block'}),
]


def s2_dg_tails(row, plan):
    N, Cin, Cout, H, W = row['dims']
    cib, ub, npix = 1 << plan['lG'], plan['nq'], (H // 2) * (W // 2)
    t = set()
    if row['cin_n'] % cib:
        t.add('ci_tail')             # the last channel block computes channels nobody may store
    if Cout % ub:
        t.add('co_tail_ub')          # the last round of UB dy channels is ragged
    if row['cin_n'] < row['dxc']:
        t.add('partial')             # channels behind cin_n must stay as they were
    if N * npix % 256:
        t.add('pix_tail')
    if H != W:
        t.add('rect')
    if N > 1 and npix % 256:
        t.add('straddle')
    if npix == 1:
        t.add('one_block')
    return t


# ---- conv3x3s2_wgrad_small: (dims, S) -- S slabs of the pixel range (min(ceil(2048 / (Cin ceil(Cout / 8))), 64, ceil(P / 1024)));
#      the launch records nothing, tests/test_igemm_plans_cpu.py restates the rule
S2_WG_CASES = [('s2w-12x20', (2, 6, 10, 12, 20), 1), ('s2w-34x62-S2', (3, 3, 9, 34, 62), 2), ('s2w-66x62-S5', (5, 2, 17, 66, 62), 5),
               ('s2w-2x2', (1, 3, 5, 2, 2), 1)]

# ---- the autograd Functions: (id, kind, (N, Cin, Cout, H, W), stride, out_pad, family after forward, family after backward)
#      sylvester.DirectConvFn, k 5, pad 2.  A 'deconv' row's forward IS the conv's data gradient (igemm_kernel<1>) and its input
#      gradient the conv's forward.
SYLVESTER_CASES = [
    ('syl-conv-s2-6x10', 'conv', (2, 3, 6, 6, 10), 2, 0, 'igemm_fwd', 'igemm_dg'),
    ('syl-conv-s2-5x7', 'conv', (2, 3, 6, 5, 7), 2, 0, 'igemm_fwd', 'igemm_dg'),
    ('syl-deconv-s2-3x5-outpad1', 'deconv', (2, 6, 3, 3, 5), 2, 1, 'igemm_dg', 'igemm_fwd'),
    ('syl-conv-s1-3x6', 'conv', (2, 4, 6, 3, 6), 1, 0, 'igemm_fwd', 'igemm_dg'),
    ('syl-deconv-s1-3x6', 'deconv', (2, 6, 4, 3, 6), 1, 0, 'igemm_dg', 'igemm_fwd'),
    ('syl-conv-s2-8x8-power-of-two', 'conv', (2, 8, 16, 8, 8), 2, 0, None, None),       # None: any family but this file's four
]

# ---- what the Python wrappers refuse before any launch: (id, wrapper, argument shapes ..., piece of the message)
WRAPPER_REFUSALS = ['fwd-weight-cin', 'fwd-kernel-not-square', 'fwd-bias-length', 'dgrad-dy-grid', 'dgrad-dy-channels', 'wgrad-batch',
                    'wgrad-dy-grid', 's2-dgrad-dy-grid', 's2-dgrad-weight-5x5', 's2-lead-odd-h', 's2-lead-cin-n', 's2-wgrad-batch',
                    's2-wgrad-dy-grid']


# ===================================================================================================== guarded buffers
def _ws_guarded(nb):
    """A NaN-filled workspace of nb bytes between two WS_GUARD bands -> (buffer, pointer)."""
    buf = torch.full((nb + 2 * WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[:WS_GUARD] = 0xA5
    buf[WS_GUARD + nb:] = 0xA5
    return buf, ctypes.c_void_p(buf.data_ptr() + WS_GUARD)


def _ws_intact(buf, nb, what):
    band = torch.full((WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert torch.equal(buf[:WS_GUARD], band), '%s: the bytes in front of the workspace were written' % what
    assert torch.equal(buf[WS_GUARD + nb:], band), '%s: the bytes behind the workspace (%d bytes) were written' % (what, nb)


class guarded(object):
    """Operands in NaN surrounds, outputs between sentinel bands; check() asserts the bands and that no operand changed."""

    def __init__(self, what, **operands):
        self.what, self.cpu = what, operands
        self.ins = {k: T._guarded_in(v) for k, v in operands.items()}
        self.outs = {}

    def p(self, name):
        return ctypes.c_void_p(self.ins[name][1].data_ptr())

    def out(self, name, shape):
        self.outs[name] = T._guarded_out(shape)
        return ctypes.c_void_p(self.outs[name][1].data_ptr())

    def check(self):
        torch.cuda.synchronize()
        for name, (buf, view) in self.outs.items():
            T._bands_intact(buf, view.numel(), '%s %s' % (self.what, name))
        for k, (buf, view) in self.ins.items():
            assert torch.equal(view.cpu(), self.cpu[k]), '%s: operand %s was modified' % (self.what, k)
        return {k: v[1].cpu() for k, v in self.outs.items()}


def _act(v, act):
    return F.relu(v) if act == 'relu' else (F.elu(v) if act == 'elu' else v)


def _finite(t, what):
    assert bool(torch.isfinite(t).all()), '%s: non-finite values (an element nobody wrote, or a NaN surround was read)' % what


# ===================================================================================================== operands and references
_REF = {}


def conv_case(dims):
    """Seeded CPU operands of a conv (N, Cin, Cout, H, W, k, stride, pad) and its float64 autograd reference, made once:
    x, w, b, g (the gradient handed to dgrad / wgrad as dy), pre = conv2d(x, w, b), dx, dw."""
    if dims in _REF:
        return _REF[dims]
    N, Cin, Cout, H, W, k, s, p = dims
    o = dict(x=rnd(N, Cin, H, W, seed=11), w=rnd(Cout, Cin, k, k, seed=12, scale=1.0 / math.sqrt(Cin * k * k)), b=rnd(Cout, seed=13, scale=0.3))
    xr, wr = o['x'].double().requires_grad_(), o['w'].double().requires_grad_()
    pre = F.conv2d(xr, wr, None, s, p)
    o['g'] = rnd(*pre.shape, seed=14)
    pre.backward(o['g'].double())
    o['pre'] = pre.detach() + o['b'].double().view(1, -1, 1, 1)
    o['dx'], o['dw'] = xr.grad, wr.grad
    _REF[dims] = o
    return o


# ===================================================================================================== launches
def run_fwd(what, dims, act, entry='ws'):
    """gx_conv2d_direct_fwd_ws with the workspace its query asks for ('ws'), with a NULL workspace ('null'), or
    gx_conv2d_direct_fwd ('plain') -> (y on the CPU, the record)."""
    from genesis_amd import _lib
    N, Cin, Cout, H, W, k, s, p = dims
    o = conv_case(dims)
    gb = guarded(what, x=o['x'], w=o['w'], b=o['b'])
    y = gb.out('y', tuple(o['pre'].shape))
    a = hip_ops.ACTS[act]
    if entry == 'plain':
        _lib.call('gx_conv2d_direct_fwd', gb.p('x'), gb.p('w'), gb.p('b'), a, y, *dims, hip_ops._stream())
    elif entry == 'null':
        _lib.call('gx_conv2d_direct_fwd_ws', gb.p('x'), gb.p('w'), gb.p('b'), a, y, *dims, None, 0, hip_ops._stream())
    else:
        nb = _lib.query('gx_conv2d_direct_fwd_ws_bytes', *dims)
        wsbuf, ws = _ws_guarded(nb)
        _lib.call('gx_conv2d_direct_fwd_ws', gb.p('x'), gb.p('w'), gb.p('b'), a, y, *dims, ws, nb, hip_ops._stream())
    plan = hip_ops.conv_last_plan()
    res = gb.check()
    if entry == 'ws':
        _ws_intact(wsbuf, nb, what)
    return res['y'], plan


def check_fwd(what, dims, act, declared, fallback):
    """The forward of one row: the declared record, the bound, and for a split the repeat run and both single-launch calls."""
    from genesis_amd import _lib
    ref = _act(conv_case(dims)['pre'], act)
    y, plan = run_fwd(what, dims, act)
    assert plan == declared, 'the table is wrong about %s: declared %s, the launch recorded %s' % (what, declared, plan)
    ns = declared['nsplit'] if declared['family'] == 'igemm_fwd' else 1
    assert _lib.query('gx_conv2d_direct_fwd_ws_bytes', *dims) == (ns * ref.numel() * 4 if ns > 1 else 0)
    _finite(y, what)
    print('%-44s %s  max |err| %.3e (ref max %.3e)' % (what, {k: v for k, v in plan.items() if v}, float((y.double() - ref).abs().max()),
                                                        float(ref.abs().max())))
    close(y, ref, *FWD_TOL, msg=what + ' y')
    if ns > 1:
        again, _ = run_fwd(what, dims, act)
        assert torch.equal(y, again), '%s: the split forward is not bit-reproducible' % what
        for entry in ('null', 'plain'):
            y1, plan1 = run_fwd('%s (%s)' % (what, entry), dims, act, entry)
            assert plan1 == fallback, '%s without a workspace (%s): declared %s, recorded %s' % (what, entry, fallback, plan1)
            _finite(y1, what)
            close(y1, ref, *FWD_TOL, msg='%s y (%s)' % (what, entry))
    else:
        assert fallback is None


def _ids(rows):
    return [r['id'] for r in rows]


# ===================================================================================================== the generic kernel
@pytest.mark.parametrize('row', GENERIC_CASES, ids=_ids(GENERIC_CASES))
def test_igemm_forward(row):
    dims = row['dims']
    nchunks = cd(generic_shape(dims)[2]['f'][2], 16)
    fallback = FW(row['fwd']['grid_x'], row['fwd']['grid_y'], 1, nchunks) if row['fwd']['nsplit'] > 1 else None
    check_fwd(row['id'], dims, row['act'], row['fwd'], fallback)


@pytest.mark.parametrize('row', GENERIC_CASES, ids=_ids(GENERIC_CASES))
def test_igemm_data_gradient(row):
    from genesis_amd import _lib
    dims = row['dims']
    N, Cin, Cout, H, W, k, s, p = dims
    o = conv_case(dims)
    gb = guarded(row['id'], dy=o['g'], w=o['w'])
    _lib.call('gx_conv2d_direct_dgrad', gb.p('dy'), gb.p('w'), gb.out('dx', (N, Cin, H, W)), *dims, hip_ops._stream())
    plan = hip_ops.conv_last_plan()
    dx = gb.check()['dx']
    assert plan == row['dg'], 'the table is wrong about %s: declared %s, the launch recorded %s' % (row['id'], row['dg'], plan)
    assert generic_tails(dims, row['fwd'], plan, row['wsplit']) == set(row['tails']), sorted(generic_tails(dims, row['fwd'], plan, row['wsplit']))
    _finite(dx, row['id'])
    print('%-44s %s  max |err| %.3e (ref max %.3e)' % (row['id'], {k: v for k, v in plan.items() if v},
                                                        float((dx.double() - o['dx']).abs().max()), float(o['dx'].abs().max())))
    close(dx, o['dx'], *DG_TOL, msg=row['id'] + ' dx')
    if 'd.zero_rows' in row['tails']:       # rows / columns no window reaches: structural zeros, not small numbers
        Ho, Wo, _ = generic_shape(dims)
        rows_hit, cols_hit = (Ho - 1) * s + k - p, (Wo - 1) * s + k - p
        assert rows_hit < H or cols_hit < W
        assert float(dx[:, :, rows_hit:, :].abs().sum()) == 0.0 and float(dx[:, :, :, cols_hit:].abs().sum()) == 0.0
        assert float(o['dx'][:, :, rows_hit:, :].abs().sum()) == 0.0 and float(o['dx'][:, :, :, cols_hit:].abs().sum()) == 0.0


@pytest.mark.parametrize('row', GENERIC_CASES, ids=_ids(GENERIC_CASES))
def test_igemm_weight_gradient(row):
    """The record stays the one from before (weight gradients note nothing); the slab count is what the workspace query implies."""
    from genesis_amd import _lib
    dims = row['dims']
    N, Cin, Cout, H, W, k, s, p = dims
    o = conv_case(dims)
    nb = _lib.query('gx_conv2d_direct_wgrad_ws_bytes', *dims)
    assert nb == row['wsplit'] * 4 * Cout * Cin * k * k, (nb, row['wsplit'])
    before = hip_ops.conv_last_plan()
    got = []
    for _ in range(2):
        gb = guarded(row['id'], x=o['x'], dy=o['g'])
        wsbuf, ws = _ws_guarded(nb)
        _lib.call('gx_conv2d_direct_wgrad', gb.p('x'), gb.p('dy'), gb.out('dw', (Cout, Cin, k, k)), *dims, ws, nb, hip_ops._stream())
        got.append(gb.check()['dw'])
        _ws_intact(wsbuf, nb, row['id'])
    assert hip_ops.conv_last_plan() == before, 'a weight-gradient launch changed the forward / data-gradient record'
    dw = got[0]
    _finite(dw, row['id'])
    print('%-44s %d slabs  max |err| %.3e (ref max %.3e)' % (row['id'], row['wsplit'], float((dw.double() - o['dw']).abs().max()),
                                                              float(o['dw'].abs().max())))
    close(dw, o['dw'], *WG_TOL, msg=row['id'] + ' dw')
    assert torch.equal(got[0], got[1]), '%s: the weight gradient is not bit-reproducible' % row['id']


# ===================================================================================================== the stride-2 kernels
@pytest.mark.parametrize('row', S2_FWD_CASES, ids=_ids(S2_FWD_CASES))
def test_conv3x3s2_forward(row):
    dims = row['dims'] + (3, 2, 1)
    check_fwd(row['id'], dims, row['act'], row['plan'], row['fallback'])
    assert s2_fwd_tails(row['dims'], row['plan']) == set(row['tails']), sorted(s2_fwd_tails(row['dims'], row['plan']))


@pytest.mark.parametrize('row', S2_DG_CASES, ids=_ids(S2_DG_CASES))
def test_conv3x3s2_data_gradient(row):
    from genesis_amd import _lib
    N, Cin, Cout, H, W = row['dims']
    n, dxc = row['cin_n'], row['dxc']
    o = conv_case(row['dims'] + (3, 2, 1))
    if row['via'] == 'lead':
        dx = hip_ops.conv3x3s2_dgrad_lead(o['g'].to(DEV), o['w'].to(DEV), H, W, n)
        plan = hip_ops.conv_last_plan()
        assert tuple(dx.shape) == (N, n, H, W)
        dx = dx.cpu()
    else:
        gb = guarded(row['id'], dy=o['g'], w=o['w'])
        out = gb.out('dx', (N, dxc, H, W))
        if row['via'] == 'ex':
            _lib.call('gx_conv3x3s2_dgrad_small_ex', gb.p('dy'), gb.p('w'), out, N, Cin, Cout, H, W, n, dxc, hip_ops._stream())
        else:
            assert dxc == Cin
            _lib.call('gx_conv3x3s2_dgrad_small', gb.p('dy'), gb.p('w'), out, N, Cin, Cout, H, W, n, hip_ops._stream())
        plan = hip_ops.conv_last_plan()
        dx = gb.check()['dx']
    assert plan == row['plan'], 'the table is wrong about %s: declared %s, the launch recorded %s' % (row['id'], row['plan'], plan)
    assert s2_dg_tails(row, plan) == set(row['tails']), sorted(s2_dg_tails(row, plan))
    _finite(dx[:, :n], row['id'])
    print('%-44s %s  max |err| %.3e (ref max %.3e)' % (row['id'], {k: v for k, v in plan.items() if v},
                                                        float((dx[:, :n].double() - o['dx'][:, :n]).abs().max()), float(o['dx'][:, :n].abs().max())))
    close(dx[:, :n], o['dx'][:, :n], *S2DG_TOL, msg=row['id'] + ' dx')
    if n < dxc:
        assert bool(torch.isnan(dx[:, n:]).all()), '%s: channels behind cin_n were written' % row['id']


@pytest.mark.parametrize('rid,dims,S', S2_WG_CASES, ids=[c[0] for c in S2_WG_CASES])
def test_conv3x3s2_weight_gradient(rid, dims, S):
    from genesis_amd import _lib
    N, Cin, Cout, H, W = dims
    o = conv_case(dims + (3, 2, 1))
    nb = _lib.query('gx_conv3x3s2_wgrad_small_ws_bytes', *dims)
    assert nb == 64 * Cout * Cin * 9 * 4
    before = hip_ops.conv_last_plan()
    got = []
    for _ in range(2):
        gb = guarded(rid, x=o['x'], dy=o['g'])
        wsbuf, ws = _ws_guarded(nb)
        _lib.call('gx_conv3x3s2_wgrad_small', gb.p('x'), gb.p('dy'), gb.out('dw', (Cout, Cin, 3, 3)), *dims, ws, nb, hip_ops._stream())
        got.append(gb.check()['dw'])
        _ws_intact(wsbuf, nb, rid)
        # exactly S slabs were written: the reduce read no other (the values are finite) and the kernel wrote no other
        slabs = wsbuf[WS_GUARD:WS_GUARD + nb].view(torch.float32).view(64, -1)
        assert bool(torch.isfinite(slabs[:S]).all()) and bool(torch.isnan(slabs[S:]).all()), '%s: not %d slabs' % (rid, S)
    assert hip_ops.conv_last_plan() == before
    _finite(got[0], rid)
    scale = float(o['dw'].abs().max())
    print('%-44s S = %d  max |err| %.3e (ref max %.3e)' % (rid, S, float((got[0].double() - o['dw']).abs().max()), scale))
    close(got[0], o['dw'], 1e-5, 2e-6 * scale, msg=rid + ' dw')
    assert torch.equal(got[0], got[1]), '%s: the weight gradient is not bit-reproducible' % rid


# ===================================================================================================== the wrappers' refusals
def test_wrappers_refuse_wrong_shapes_before_any_launch():
    """Device tensors of shapes that disagree: GenesisHipError, and the record is still the one of the launch before."""
    from genesis_amd._lib import GenesisHipError
    z = lambda *s: torch.zeros(*s, device=DEV)
    hip_ops.conv2d_direct_fwd(z(2, 3, 8, 6), z(5, 3, 3, 3), z(5), None, 2, 1)           # a launch whose record must survive
    torch.cuda.synchronize()
    before = hip_ops.conv_last_plan()
    assert before == FW(1, 1, 1, 2)
    calls = {
        'fwd-weight-cin': lambda: hip_ops.conv2d_direct_fwd(z(2, 3, 8, 6), z(5, 4, 3, 3), None, None, 2, 1),
        'fwd-kernel-not-square': lambda: hip_ops.conv2d_direct_fwd(z(2, 3, 8, 6), z(5, 3, 3, 2), None, None, 2, 1),
        'fwd-bias-length': lambda: hip_ops.conv2d_direct_fwd(z(2, 3, 8, 6), z(5, 3, 3, 3), z(4), None, 2, 1),
        'dgrad-dy-grid': lambda: hip_ops.conv2d_direct_dgrad(z(2, 5, 4, 4), z(5, 3, 3, 3), 8, 6, 2, 1),       # 4 x 3 is right
        'dgrad-dy-channels': lambda: hip_ops.conv2d_direct_dgrad(z(2, 4, 4, 3), z(5, 3, 3, 3), 8, 6, 2, 1),
        'wgrad-batch': lambda: hip_ops.conv2d_direct_wgrad(z(2, 3, 8, 6), z(3, 5, 4, 3), 3, 2, 1),
        'wgrad-dy-grid': lambda: hip_ops.conv2d_direct_wgrad(z(2, 3, 8, 6), z(2, 5, 4, 4), 3, 2, 1),
        's2-dgrad-dy-grid': lambda: hip_ops.conv3x3s2_dgrad_small(z(2, 5, 4, 4), z(5, 3, 3, 3), 8, 6),
        's2-dgrad-weight-5x5': lambda: hip_ops.conv3x3s2_dgrad_small(z(2, 5, 4, 3), z(5, 3, 5, 5), 8, 6),
        's2-lead-odd-h': lambda: hip_ops.conv3x3s2_dgrad_lead(z(2, 5, 4, 3), z(5, 3, 3, 3), 7, 6, 1),
        's2-lead-cin-n': lambda: hip_ops.conv3x3s2_dgrad_lead(z(2, 5, 4, 3), z(5, 3, 3, 3), 8, 6, 4),
        's2-wgrad-batch': lambda: hip_ops.conv3x3s2_wgrad_small(z(2, 3, 8, 6), z(3, 5, 4, 3)),
        's2-wgrad-dy-grid': lambda: hip_ops.conv3x3s2_wgrad_small(z(2, 3, 8, 6), z(2, 5, 3, 3)),
    }
    assert sorted(calls) == sorted(WRAPPER_REFUSALS)
    for name in WRAPPER_REFUSALS:
        with pytest.raises(GenesisHipError):
            calls[name]()
        assert hip_ops.conv_last_plan() == before, name
    # ... and the right shapes of the same calls pass
    hip_ops.conv2d_direct_dgrad(z(2, 5, 4, 3), z(5, 3, 3, 3), 8, 6, 2, 1)
    assert hip_ops.conv_last_plan() == DG(1, 1, 3)
    hip_ops.conv3x3s2_wgrad_small(z(2, 3, 8, 6), z(2, 5, 4, 3))
    hip_ops.conv2d_direct_wgrad(z(2, 3, 8, 6), z(2, 5, 4, 3), 3, 2, 1)
    torch.cuda.synchronize()


# ===================================================================================================== autograd dispatch
class spy(object):
    """Notes the calls of hip_ops entry points while they go through unchanged, and the record each left -- read in the calling
    thread, right behind the call: autograd runs a backward on a thread of its own and the record is per thread."""

    def __init__(self, monkeypatch, *names):
        self.calls, self.plans = [], {}
        for name in names:
            monkeypatch.setattr(hip_ops, name, self._wrap(name, getattr(hip_ops, name)))

    def _wrap(self, name, f):
        def g(*a, **k):
            self.calls.append(name)
            out = f(*a, **k)
            self.plans[name] = hip_ops.conv_last_plan()
            return out
        return g


DIRECT = ('conv2d_direct_fwd', 'conv2d_direct_dgrad', 'conv2d_direct_wgrad', 'conv3x3s2_dgrad_small', 'conv3x3s2_dgrad_lead',
          'conv3x3s2_wgrad_small')


@pytest.mark.parametrize('H,dx_channels,want,last', [
    (12, None, ['conv2d_direct_fwd', 'conv3x3s2_wgrad_small', 'conv3x3s2_dgrad_small'], S2D(4, 8, 2, 1)),
    (11, None, ['conv2d_direct_fwd', 'conv2d_direct_wgrad', 'conv2d_direct_dgrad'], DG(4, 1, 6)),
    (12, 1, ['conv2d_direct_fwd', 'conv3x3s2_wgrad_small', 'conv3x3s2_dgrad_small'], S2D(2, 8, 1, 1))],
    ids=['12x20-s2-kernels', '11x20-odd-h-generic', '12x20-dx-channels-1'])
def test_direct_conv_act_fn_dispatch(monkeypatch, H, dx_channels, want, last):
    """functions.DirectConvActFn, conv3x3 stride 2 pad 1 + ELU on (2, 6, 10, H, 20): which kernels its backward takes, and values,
    dx, dw, db against float64 autograd at the bounds of the entry point that computed each."""
    from genesis_amd import functions as fn
    N, Cin, Cout, W = 2, 6, 10, 20
    x, w, b = rnd(N, Cin, H, W, seed=21), rnd(Cout, Cin, 3, 3, seed=22, scale=1.0 / math.sqrt(9 * Cin)), rnd(Cout, seed=23, scale=0.3)
    xr, wr, br = (t.double().requires_grad_() for t in (x, w, b))
    yr = F.elu(F.conv2d(xr, wr, br, 2, 1))
    g = rnd(*yr.shape, seed=24)
    yr.backward(g.double())
    xd, wd, bd = (t.to(DEV).requires_grad_() for t in (x, w, b))
    s = spy(monkeypatch, *DIRECT)
    y = fn.DirectConvActFn.apply(xd, wd, bd, 2, 1, 'elu', dx_channels)
    assert hip_ops.conv_last_plan() == FW(cd(N * yr.shape[2] * 10, 128), 1, 1, 4)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert s.calls == want, s.calls
    assert s.plans[want[-1]] == last, s.plans[want[-1]]
    s2 = 'conv3x3s2_dgrad_small' in want
    close(y, yr, *FWD_TOL, msg='y')
    n = Cin if dx_channels is None else dx_channels
    close(xd.grad[:, :n], xr.grad[:, :n], *(S2DG_TOL if s2 else DG_TOL), msg='dx')
    assert float(xd.grad[:, n:].abs().sum()) == 0.0
    if s2:
        close(wd.grad, wr.grad, 1e-5, 2e-6 * float(wr.grad.abs().max()), msg='dw')
    else:
        close(wd.grad, wr.grad, *WG_TOL, msg='dw')
    close(bd.grad, br.grad, 1e-4, 1e-4, msg='db')          # (test_conv2d_direct 'dbias')


@pytest.mark.parametrize('rid,kind,dims,stride,out_pad,fam_f,fam_b', SYLVESTER_CASES, ids=[c[0] for c in SYLVESTER_CASES])
def test_sylvester_direct_conv_fn_dispatch(monkeypatch, rid, kind, dims, stride, out_pad, fam_f, fam_b):
    """sylvester.DirectConvFn (bias-free 5 x 5, pad 2) on grids that are no power of two: the generic kernels in each other's roles."""
    from genesis_amd import sylvester
    N, Cin, Cout, H, W = dims
    x = rnd(N, Cin, H, W, seed=31)
    w = rnd(*((Cout, Cin, 5, 5) if kind == 'conv' else (Cin, Cout, 5, 5)), seed=32, scale=1.0 / math.sqrt(25 * Cin / stride ** 2))
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    yr = F.conv2d(xr, wr, None, stride, 2) if kind == 'conv' else F.conv_transpose2d(xr, wr, None, stride, 2, out_pad)
    g = rnd(*yr.shape, seed=33)
    yr.backward(g.double())
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    s = spy(monkeypatch, *DIRECT)
    y = sylvester.DirectConvFn.apply(xd, wd, kind, stride, 2, out_pad)
    after_f = hip_ops.conv_last_plan()['family']
    assert tuple(y.shape) == tuple(yr.shape)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    if fam_f is None:
        assert after_f not in IGEMM_FAMILIES and s.calls == [], (after_f, s.calls)
        close(y, yr, 2e-5, 2e-5, msg=rid + ' y')           # (tests/test_conv_plans_gpu.py's bound for the transposed conv's kernels)
        close(xd.grad, xr.grad, 2e-5, 2e-5, msg=rid + ' dx')
        return
    assert (after_f, s.plans[s.calls[-1]]['family']) == (fam_f, fam_b), (after_f, s.plans)
    if kind == 'conv':
        assert s.calls == ['conv2d_direct_fwd', 'conv2d_direct_wgrad', 'conv2d_direct_dgrad'], s.calls
        close(y, yr, *FWD_TOL, msg=rid + ' y')
        close(xd.grad, xr.grad, *DG_TOL, msg=rid + ' dx')
    else:
        assert s.calls == ['conv2d_direct_dgrad', 'conv2d_direct_wgrad', 'conv2d_direct_fwd'], s.calls
        close(y, yr, *DG_TOL, msg=rid + ' y')
        close(xd.grad, xr.grad, *FWD_TOL, msg=rid + ' dx')
    close(wd.grad, wr.grad, *WG_TOL, msg=rid + ' dw')


@pytest.mark.parametrize('out,out_act', [(12, None), (3, 'elu')], ids=['12-channels', '3-channels-elu'])
def test_broadcast_decoder_wide_head(monkeypatch, out, out_act):
    """functions.BroadcastDecoderFn with more than 8 output channels, or an output activation: the final 1 x 1 conv runs on the
    generic kernel (forward, weight gradient, data gradient).  A 10 x 10 image behind one 3 x 3 layer: the canvas is 12 x 12 (the
    broadcast layer's kernels take canvases whose side is a multiple of 4, so a 10 x 10 canvas never reaches the head)."""
    from genesis_amd import functions as fn
    from genesis_amd.genesisv2_config import pixel_coords
    N, L, hid, d = 3, 5, 16, 12
    z = rnd(N, L, seed=41)
    w0, b0 = rnd(hid, L + 2, 3, 3, seed=42, scale=1.0 / math.sqrt(9 * (L + 2))), rnd(hid, seed=43, scale=0.3)
    ow, ob = rnd(out, hid, seed=44, scale=1.0 / math.sqrt(hid)), rnd(out, seed=45, scale=0.3)
    coords = pixel_coords(d).contiguous()
    ref_in = [t.double().requires_grad_() for t in (z, w0, b0, ow, ob)]
    zr, w0r, b0r, owr, obr = ref_in
    h = torch.cat((zr.view(N, L, 1, 1).expand(-1, -1, d, d), coords.double().expand(N, -1, -1, -1)), 1)
    yr = _act(F.conv2d(F.relu(F.conv2d(h, w0r, b0r)), owr.view(out, hid, 1, 1), obr), out_act)
    g = rnd(*yr.shape, seed=46)
    yr.backward(g.double())
    dev_in = [t.to(DEV).requires_grad_() for t in (z, w0, b0, ow, ob)]
    s = spy(monkeypatch, *DIRECT)
    y = fn.BroadcastDecoderFn.apply(dev_in[0], coords.to(DEV), 'relu', out_act, *dev_in[1:])
    assert hip_ops.conv_last_plan() == FW(cd(N * d * d, 128), 1, 1, 1), hip_ops.conv_last_plan()
    assert tuple(y.shape) == (N, out, d - 2, d - 2)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    assert s.calls == ['conv2d_direct_fwd', 'conv2d_direct_wgrad', 'conv2d_direct_dgrad'], s.calls
    assert s.plans['conv2d_direct_dgrad'] == DG(cd(N * d * d, 128), 1, cd(out, 16)), s.plans
    close(y, yr, *FWD_TOL, msg='y')
    for name, got, want in zip(('dz', 'dw0', 'db0', 'dow', 'dob'), dev_in, ref_in):
        close(got.grad, want.grad, *WG_TOL, msg=name)
