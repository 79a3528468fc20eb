"""The forward and data-gradient convolutions off the beaten path: every tile plan their host planners can pick, reached by the
smallest shape that reaches it.  pick_tile / plan_tapconv / plan_c3 (gx_conv.hip), q_plan / q_plan_c3h / q_plan_c5h / q_split_tail
(gx_kq.hip) and wino_shape_ok (gx_wino.hip) choose template instantiations, LDS sizes and loops with tails from the shape; the
workloads' shapes reach a few of those plans.  One table of cases per entry point; every row DECLARES the plan class it is meant
to reach (family, operand form, lTH, lTW, lG, nq or NPOS, further record fields where they are the point, and the tails it has).
Every case

  1. sets the dispatch policies and precision switches of its row (restored in `finally`),
  2. puts every operand in the middle of a larger device buffer whose remainder is NaN,
  3. puts every output in the middle of a sentinel-filled buffer (GUARD floats on each side; the output itself starts as NaN) and
     the workspace -- sized by the entry point's *_ws_bytes query -- between two guard bands, through _lib.call with explicit pointers,
  4. reads gx_conv_last_plan and asserts that it equals the declared class: a case that reaches another plan fails the TABLE,
  5. compares with the same operation in float64 torch on the CPU at the rtol / atol tests/test_kernels_gpu.py applies to that
     output in that form (2e-5 / 2e-5: test_conv3x3, test_deconv5x5s2, test_conv3x3_winograd, test_conv5x5_stride1_on_the_tapconv_kernel,
     test_deconv_epilogue_groupnorm_statistics' mean / rstd bounds; 1e-5 / 1e-5 for the <= 32-channel 16-bit-pipe kernel:
     test_conv3x3_to_32_channels_on_the_bf16_pipe, test_conv3x3_data_gradient_with_the_previous_layers_activation_backward), and
     asserts finite values and bit-identical guard bands.

The one-bf16-piece form runs on the same rows against the yardsticks that exist: tests/test_matmul_precision_gpu.py's `check`
(operands rounded with bf(), modes 0 / 2 / 3) for the 16-bit-pipe families and Winograd, tests/test_tapconv_precision_gpu.py's
`judge` for the tap-conv kernels.  No bound of this file is new.

What each class would catch (one-line mistakes in the code it reaches; argued from the code, never run):

  kq C3 / DT / DG, G = 4 or 8 with N % G != 0           an image index `n0 + gi` used without `< N` on the load (the next tensor's
                                                        pixels: NaN here) or on the store (the guard band behind y)
  kq nq = 3 against nq = 4                              a staging loop that runs NQ - 1 rounds, LDS planes sized for the other nq
  kq 4 x 64, 64 x 4, 64 x 64                            lTH / lTW swapped in the halo copy, a row stride taken from TW
  kq M = 40, 72, 130; K = 8, 24                         the half-tile (M % 64 <= 32) epilogue storing 64 channels, `co <= M`, a chunk
                                                        loop that assumes two 8-channel chunks (K % 16 != 0 on the fp32 kernels)
  kq tail split on / off / refused                      blockIdx.x >= nfull mapped to the wrong tile or half (channels 32..63 of the
                                                        last tiles lost or written twice), a split of a tile whose upper half is empty
  kq DTH interleaved (grid.y = 1) or not                the row parity taken from blockIdx.z when the grid interleaves it along x
  kq DT / DTH statistics taken or declined              statistics written for a tile that spans images, or with M % 8 != 0
  kq DG / DGH with Cin_out < Cin                        the weight row stride taken from the masked channel count
  kq C3H whole-row tiles, ragged last tile              rows >= H of the last tile stored (the next channel's plane: value check) or
                                                        loaded without the zero padding
  kq C3H tile taller than the image (6 x 6)             rt_th used where H is meant
  kq C3H persistent loop, second partial round          `tile += gridDim.x` without `tile < nfull` (past the last image), a
                                                        prefetch of tile + gridDim.x that is not guarded
  kq C3H M = 7, 24; producer tap                        32-channel stores without `co < M`; partial maxima of masked lanes
  kq C5H 16 x 48 / 48 x 16, M = 24 / 72, N = 1 / 3      tiles_w and tiles_h swapped in the tile decode, the second channel tile's bias
  tap conv, ragged tiles both ways, TH = 1              gx_ceil_div tiles stored without `oh < Ho` / `ow < Wo`, lTH = 0 shifts
  tap conv NPOS low / high, 128-pixel tile              the halo staging loop bound taken from the other NPOS, MW = 2 wave map
  tap conv split-K: uneven, capped by nchunks, slabs    the last slab reading chunks past nchunks, the reduce summing a slab nobody
                                                        wrote (NaN workspace here), slab stride without the channel tail
  tap conv K = 3, 12, 66; M = 1, 65; 2 x 2; 1 x 4       K padding read from x without a mask, the upper MFMA tile skipped at M = 33..64
  Winograd 8 x 16, 8 x 256, 128 x 16, K = 17, M = 65    tiles_h / tiles_w swapped, the 16-channel chunk tail, the second channel tile
  small-Cin forward, Cout = 1 and SC_COB + 1            `co0 + co < Cout` missing on the store (the next image's plane / the guard)
  every eligibility boundary, one step outside          an `_eligible` that admits a shape its kernel cannot index (4 x 4: 2 CHS >
                                                        1024; H % 16 != 0; K % 16 != 0; M = 33; H % 8 != 0): the record must show the
                                                        fallback family and the values must still be right
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64 = torch.float64
GUARD = 4096              # floats on each side of every operand and output
WS_GUARD = 16384          # bytes on each side of the workspace
SENTINEL = 1.2345e30      # the output guard bands (finite, so that torch.equal can compare them)
PLAN_KEYS = ('family', 'form', 'lTH', 'lTW', 'lG', 'nq')      # what every row declares


# ===================================================================================================== the case tables
def P(family, form, lTH=0, lTW=0, lG=0, nq=0, **more):
    """A declared plan class: the six fields every row states, and any further record field that is the point of the row."""
    return dict(dict(family=family, form=form, lTH=lTH, lTW=lTW, lG=lG, nq=nq), **more)


def R(rid, op, dims, plan, tails=(), **opt):
    """One case.  dims: (N, Cin, Cout, H, W) of the layer ((N, K, M, H, W) for conv5x5s1; H, W: the transposed conv's INPUT grid).
    opt: kqp / winop (gx_kq_policy / gx_conv3x3_wino_policy; default 1), kq / wino / tapm (the precision switches; default: left
    alone), act, groups, cin_out, tap (arm gx_amax_tap), b1 (run the one-bf16-piece form on this row too)."""
    return dict(dict(id=rid, op=op, dims=dims, plan=plan, tails=frozenset(tails)), **opt)


def both(rid, op, dims, family, geom, tails=(), **opt):
    """A 16-bit-pipe row in both fp32-accurate forms: six bf16 piece products (gx_kq_precision(1)) and three fp16 piece products (2)."""
    return [R(rid + '-bf16x6', op, dims, P(family, 'bf16x6', **geom), tails, kq=1, b1=True, **opt),
            R(rid + '-fp16x3', op, dims, P(family, 'fp16x3', **geom), tails, kq=2, **opt)]


# ---- gx_conv3x3_fwd / _bias_act_fwd / _dgrad on kq_kernel<Q_C3> (fp32, 16-byte reads): gx_kq_policy(2), K % 8 == 0, power-of-two grids
KQ_C3_CASES = [
    R('kqc3-8x8-g4-n5', 'c3_fwd', (5, 8, 64, 8, 8), P('kq_c3', 'fp32', 3, 3, 2, 4), {'image_tail'}, kqp=2),
    R('kqc3-4x8-g8-n9', 'c3_fwd', (9, 8, 64, 4, 8), P('kq_c3', 'fp32', 2, 3, 3, 4), {'image_tail'}, kqp=2),
    R('kqc3-16x16-nq3-m40', 'c3_act', (3, 8, 40, 16, 16), P('kq_c3', 'fp32', 4, 4, 0, 3), {'m_tail'}, kqp=2, kq=0, act='relu'),
    R('kqc3-8x32-nq3', 'c3_dgrad', (2, 64, 8, 8, 32), P('kq_c3', 'fp32', 3, 5, 0, 3), (), kqp=2),
    R('kqc3-4x64-k24-m72', 'c3_fwd', (2, 24, 72, 4, 64), P('kq_c3', 'fp32', 2, 6, 0, 4, grid_y=2), {'m_tail'}, kqp=2),
    R('kqc3-64x4-k24-m130', 'c3_dgrad', (2, 130, 24, 64, 4), P('kq_c3', 'fp32', 6, 2, 0, 4, grid_y=3), {'m_tail'}, kqp=2),
    R('kqc3-64x64', 'c3_act', (1, 8, 64, 64, 64), P('kq_c3', 'fp32', 2, 6, 0, 4, tiles_h=16), (), kqp=2, act='elu'),
    R('kqc3-split-on-r1', 'c3_fwd', (1028, 8, 40, 8, 8), P('kq_c3', 'fp32', 3, 3, 2, 4, nfull=256, grid_x=258),
      {'split_tail', 'm_tail'}, kqp=2),
    R('kqc3-split-off-r129', 'c3_fwd', (1540, 8, 40, 8, 8), P('kq_c3', 'fp32', 3, 3, 2, 4, nfull=385, grid_x=385), {'m_tail'}, kqp=2),
    R('kqc3-split-refused-m24', 'c3_fwd', (1028, 8, 24, 8, 8), P('kq_c3', 'fp32', 3, 3, 2, 4, nfull=257, grid_x=257),
      {'split_refused', 'm_tail'}, kqp=2, kq=0),
    # one step outside q_plan: 4 x 4 (2 CHS = 1152 > 1024), K % 8 != 0 -- the tap conv takes them
    R('kqc3-out-4x4', 'c3_fwd', (2, 8, 64, 4, 4), P('tap_c3', 'fp32', 2, 2, 4, 4, pixels=256), {'image_tail'}, kqp=2),
    R('kqc3-out-k12', 'c3_fwd', (5, 12, 64, 8, 8), P('tap_c3', 'fp32', 3, 3, 1, 2, pixels=128, nsplit=2),
      {'image_tail', 'k_pad', 'splitk', 'splitk_capped', 'px128'}, kqp=2),
]

# ---- gx_deconv5x5s2_fwd / _gn_stats_fwd / _dgrad on kq_dt_kernel / kq_kernel<Q_DG> (fp32) and kq_dth_kernel / kq_dgh_kernel
G88 = dict(lTH=3, lTW=3, lG=2, nq=4)
G1616 = dict(lTH=4, lTW=4, lG=0, nq=3)
G3232 = dict(lTH=3, lTW=5, lG=0, nq=3)
KQ_DECONV_CASES = [
    # the fp32 kernels: the 16-bit pipe off, K % 16 != 0, or a tile the 16-bit kernels' LDS budget does not hold (4 x 16, 16 x 4)
    R('kqdt-8x8-n5-pipe-off', 'dt_fwd', (5, 16, 64, 8, 8), P('kq_dt', 'fp32', grid_z=2, **G88), {'image_tail'}, kqp=2, kq=0),
    R('kqdt-8x8-n7-k24-stats-declined', 'dt_stats', (7, 24, 64, 8, 8), P('kq_dt', 'fp32', stats=0, **G88), {'image_tail'}, kqp=2,
      groups=8),
    R('kqdt-4x16', 'dt_fwd', (3, 16, 64, 4, 16), P('kq_dt', 'fp32', 2, 4, 2, 4), {'image_tail'}, kqp=2),
    R('kqdg-16x4', 'dt_dgrad', (3, 64, 16, 16, 4), P('kq_dg', 'fp32', 4, 2, 2, 4), {'image_tail'}, kqp=2),
    R('kqdt-16x16-k24-stats', 'dt_stats', (2, 24, 64, 16, 16), P('kq_dt', 'fp32', stats=1, **G1616), {'stats'}, kqp=2, groups=8),
    R('kqdg-16x16-k24', 'dt_dgrad', (2, 64, 24, 16, 16), P('kq_dg', 'fp32', **G1616), (), kqp=2),
    R('kqdg-split-on', 'dt_dgrad', (1028, 40, 8, 8, 8), P('kq_dg', 'fp32', nfull=256, grid_x=258, **G88), {'split_tail', 'm_tail'},
      kqp=2),
    R('kqdt-split-on', 'dt_fwd', (1028, 8, 40, 8, 8), P('kq_dt', 'fp32', nfull=256, grid_x=258, grid_z=2, **G88),
      {'split_tail', 'm_tail'}, kqp=2),
    # one step outside: 4 x 4 base grid -- tapconv_dt_kernel / tapconv_kernel<M_DG> take it
    R('kqdt-out-4x4', 'dt_fwd', (2, 16, 64, 4, 4), P('tap_dt', 'fp32', 2, 2, 3, 2, pixels=128, nsplit=4),
      {'image_tail', 'splitk', 'splitk_capped', 'px128'}, kqp=2),
    R('kqdg-out-4x4', 'dt_dgrad', (2, 64, 16, 4, 4), P('tap_dg', 'fp32', 2, 2, 3, 8, pixels=128, nsplit=8),
      {'image_tail', 'splitk', 'splitk_capped', 'px128'}, kqp=2),
]
KQ_DECONV_CASES += (
    both('kqdth-8x8-n5', 'dt_fwd', (5, 16, 64, 8, 8), 'kq_dth', dict(G88, grid_z=1, grid_x=4), {'image_tail', 'ilv'}, kqp=2)
    + both('kqdth-16x16-k48-stats', 'dt_stats', (2, 48, 64, 16, 16), 'kq_dth', dict(G1616, stats=1), {'stats', 'ilv'}, kqp=2, groups=8)
    + both('kqdth-16x16-m20-stats-declined', 'dt_stats', (2, 16, 20, 16, 16), 'kq_dth', dict(G1616, stats=0), {'m_tail', 'ilv'}, kqp=2,
           groups=4)
    + both('kqdth-32x32-m72', 'dt_fwd', (1, 16, 72, 32, 32), 'kq_dth', dict(G3232, grid_y=2, grid_z=2, tiles_h=4), {'m_tail'}, kqp=2)
    + both('kqdgh-8x8-n7', 'dt_dgrad', (7, 64, 16, 8, 8), 'kq_dgh', G88, {'image_tail'}, kqp=2)
    + both('kqdgh-16x16-k48-masked-cin', 'dt_dgrad', (2, 66, 48, 16, 16), 'kq_dgh', dict(G1616, grid_y=1), (), kqp=2, cin_out=64)
    + both('kqdgh-32x32', 'dt_dgrad', (1, 64, 16, 32, 32), 'kq_dgh', dict(G3232, tiles_h=4), (), kqp=2)
    # (257 tiles: 256 whole + one split in two, both row parities interleaved along x -- 2 * 258 workgroups)
    + both('kqdth-split-on', 'dt_fwd', (1028, 16, 40, 8, 8), 'kq_dth', dict(G88, nfull=256, grid_x=516, grid_z=1),
           {'split_tail', 'm_tail', 'ilv'}, kqp=2)
    + both('kqdgh-split-on', 'dt_dgrad', (1028, 40, 16, 8, 8), 'kq_dgh', dict(G88, nfull=256, grid_x=258), {'split_tail', 'm_tail'},
           kqp=2)
)

# ---- gx_conv3x3_fwd / _bias_act_fwd / _dgrad / _dgrad_act on kq_c3h_kernel (<= 32 output channels, K % 16 == 0, any grid)
KQ_C3H_CASES = (
    both('c3h-8x8-g4-n5', 'c3_act', (5, 16, 32, 8, 8), 'kq_c3h', G88, {'image_tail'}, kqp=2, act='elu')
    + both('c3h-16x24-rows10-ragged-m24', 'c3_dgrad', (2, 24, 16, 16, 24), 'kq_c3h',
           dict(lTH=4, lTW=5, lG=0, nq=3, rt_th=10, rt_tw=24, tiles_h=2), {'ragged_h', 'm_tail'}, kqp=2)
    + both('c3h-8x72-rows3-ragged-m7-k48', 'c3_dgrad_act', (2, 7, 48, 8, 72), 'kq_c3h',
           dict(lTH=2, lTW=7, lG=0, nq=3, rt_th=3, rt_tw=72, tiles_h=3), {'ragged_h', 'm_tail'}, kqp=2, act='relu')
    + both('c3h-6x6-tile-taller', 'c3_act', (3, 16, 32, 6, 6), 'kq_c3h', dict(lTH=6, lTW=3, lG=0, nq=3, rt_th=42, rt_tw=6, tiles_h=1),
           {'tile_taller'}, kqp=2, act='relu')
    + both('c3h-4x128', 'c3_fwd', (1, 16, 32, 4, 128), 'kq_c3h', dict(lTH=2, lTW=6, lG=0, nq=4, tiles_w=2), (), kqp=2)
    + both('c3h-40x24-n200-second-round', 'c3_act', (200, 16, 32, 40, 24), 'kq_c3h',
           dict(lTH=4, lTW=5, lG=0, nq=3, rt_th=10, rt_tw=24, tiles_h=4, nfull=800, grid_x=768), {'second_round'}, kqp=2, act='elu')
    + both('c3h-dgrad-act-elu-8x8', 'c3_dgrad_act', (5, 32, 16, 8, 8), 'kq_c3h', G88, {'image_tail'}, kqp=2, act='elu')
    + [R('c3h-16x16-producer-tap-fp16x3', 'c3_act', (3, 16, 32, 16, 16), P('kq_c3h', 'fp16x3', **G1616), (), kqp=2, kq=2, act='elu',
         tap=True),
       # one step outside: M = 33 (the fp32 16-byte-read kernel), K % 16 != 0 on a grid that is no power of two, 4 x 4 and 2 x 2
       # (2 CHS > 1024 in q_plan_c3h and q_plan: the tap conv)
       R('c3h-out-m33', 'c3_act', (5, 16, 33, 8, 8), P('kq_c3', 'fp32', **G88), {'image_tail', 'm_tail'}, kqp=2, kq=1, act='elu'),
       R('c3h-out-k24', 'c3_act', (2, 24, 32, 16, 24), P('tap_c3', 'fp32', 4, 3, 0, 2, pixels=128, nsplit=3),
         {'m_tail', 'm_low', 'splitk', 'splitk_capped', 'px128'}, kqp=2, kq=1, act='elu'),
       R('c3h-out-4x4', 'c3_dgrad', (2, 32, 16, 4, 4), P('tap_c3', 'fp32', 2, 2, 3, 2, pixels=128, nsplit=2),
         {'image_tail', 'm_tail', 'm_low', 'splitk', 'splitk_capped', 'px128'}, kqp=2, kq=1),
       R('c3h-out-2x2', 'c3_act', (2, 16, 32, 2, 2), P('tap_c3', 'fp32', 1, 1, 5, 2, pixels=128, nsplit=2),
         {'image_tail', 'm_tail', 'm_low', 'splitk', 'splitk_capped', 'px128'}, kqp=2, kq=1, act='relu')]
)

# ---- gx_conv5x5s1 (both flips) on kq_c5h_kernel (K % 16 == 0, H % 16 == 0, W % 16 == 0)
GC5 = dict(lTH=4, lTW=4, lG=0, nq=4)
KQ_C5H_CASES = (
    both('c5h-16x16-n1-m24', 'c5_0', (1, 16, 24, 16, 16), 'kq_c5h', dict(GC5, nfull=1), {'m_tail'}, kqp=2)
    + both('c5h-16x48-n3-k48-m64-flip', 'c5_1', (3, 48, 64, 16, 48), 'kq_c5h', dict(GC5, tiles_h=1, tiles_w=3, nfull=9), (), kqp=2)
    + both('c5h-48x16-m72', 'c5_0', (1, 16, 72, 48, 16), 'kq_c5h', dict(GC5, tiles_h=3, tiles_w=1, grid_y=2), {'m_tail'}, kqp=2)
    # one step outside: H % 16 != 0, K % 16 != 0 -- refused by the 16-bit branch, run by tapconv_kernel<M_C5>
    + [R('c5h-out-24x16', 'c5_1', (2, 16, 64, 24, 16), P('tap_c5', 'fp32', 3, 4, 1, 2, pixels=256, nsplit=4), {'splitk', 'splitk_capped'}, kqp=2, kq=1),
       R('c5h-out-k24', 'c5_0', (2, 24, 64, 16, 16), P('tap_c5', 'fp32', 4, 4, 0, 2, pixels=256, nsplit=6), {'splitk', 'splitk_capped'}, kqp=2, kq=1)]
)

# ---- the tap-conv kernels (gx_kq_policy(0), gx_conv3x3_wino_policy(0)): tapconv_kernel<M_C3 | M_C5 | M_DG>, tapconv_dt_kernel
T = dict(kqp=0, winop=0, b1=True)
TAP_CASES = [
    # conv3x3
    R('tap-c3-72x72-k3-m1', 'c3_fwd', (2, 3, 1, 72, 72), P('tap_c3', 'fp32', 3, 3, 2, 2, pixels=256, tiles_h=9, tiles_w=9),
      {'image_tail', 'k_pad', 'm_tail', 'm_low'}, **T),
    R('tap-c3-12x20-k12-m65', 'c3_fwd', (2, 12, 65, 12, 20), P('tap_c3', 'fp32', 2, 2, 3, 2, pixels=128, nsplit=2, grid_y=2),
      {'image_tail', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-c3-9x12-rows-of-one', 'c3_act', (2, 12, 65, 9, 12), P('tap_c3', 'fp32', 0, 2, 5, 4, pixels=128, tiles_h=9, tiles_w=3),
      {'image_tail', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, act='relu', **T),
    R('tap-c3-10x18-2x2-tiles', 'c3_dgrad', (3, 16, 66, 10, 18), P('tap_c3', 'fp32', 1, 1, 5, 2, pixels=128, tiles_h=5, tiles_w=9),
      {'image_tail', 'k_pad', 'm_tail', 'm_low', 'splitk', 'splitk_capped', 'px128'}, **T),
    # (pick_tile finds an exact tiling of every grid at 128 pixels, and at 256 pixels unless H is odd and W % 8 == 4, or the
    #  other way round: these are the ragged last tiles of gx_ceil_div, one direction each -- the 3 x 3 kernels have no both-ways case)
    R('tap-c3-9x12-256-ragged-h', 'c3_fwd', (3, 8, 65, 9, 12), P('tap_c3', 'fp32', 1, 2, 5, 4, pixels=256, tiles_h=5, tiles_w=3),
      {'image_tail', 'ragged_h', 'm_tail'}, **T),
    R('tap-c3-12x9-256-ragged-w', 'c3_dgrad', (3, 12, 8, 12, 9), P('tap_c3', 'fp32', 2, 1, 5, 4, pixels=256, tiles_h=3, tiles_w=5),
      {'image_tail', 'ragged_w', 'm_tail', 'm_low'}, **T),
    R('tap-c3-2x2-k66-capped', 'c3_fwd', (2, 66, 64, 2, 2), P('tap_c3', 'fp32', 1, 1, 5, 2, pixels=128, nsplit=9, chunks_per_split=1),
      {'image_tail', 'k_pad', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-c3-1x4', 'c3_act', (3, 8, 8, 1, 4), P('tap_c3', 'fp32', 0, 2, 5, 4, pixels=128), {'image_tail', 'm_tail', 'm_low', 'px128'},
      act='elu', **T),
    R('tap-c3-4x4-npos4', 'c3_fwd', (20, 8, 8, 4, 4), P('tap_c3', 'fp32', 2, 2, 4, 4, pixels=256), {'image_tail', 'm_tail', 'm_low'}, **T),
    R('tap-c3-uneven-splitk-parts', 'c3_fwd_parts', (64, 40, 64, 16, 16),
      P('tap_c3', 'fp32', 3, 4, 0, 2, pixels=128, nsplit=3, chunks_per_split=2), {'splitk', 'splitk_uneven', 'px128'}, **T),
    R('tap-c3-uneven-splitk-dgrad-parts', 'c3_dgrad_parts', (64, 24, 40, 16, 16),
      P('tap_c3', 'fp32', 3, 4, 0, 2, pixels=128, nsplit=3, chunks_per_split=2), {'m_tail', 'm_low', 'splitk', 'splitk_uneven', 'px128'},
      **T),
    R('tap-c3-uneven-splitk-reduced', 'c3_act', (64, 40, 64, 16, 16),
      P('tap_c3', 'fp32', 3, 4, 0, 2, pixels=128, nsplit=3, chunks_per_split=2), {'splitk', 'splitk_uneven', 'px128'}, act='relu', **T),
    # conv5x5s1
    R('tap-c5-9x12-k12-m65', 'c5_0', (2, 12, 65, 9, 12), P('tap_c5', 'fp32', 2, 2, 4, 4, pixels=256, nsplit=4),
      {'image_tail', 'ragged_h', 'k_pad', 'm_tail', 'splitk', 'splitk_capped'}, **T),
    R('tap-c5-40x5-ragged-both', 'c5_1', (2, 12, 24, 40, 5), P('tap_c5', 'fp32', 4, 1, 3, 4, pixels=256, tiles_h=3, tiles_w=3),
      {'image_tail', 'ragged_h', 'ragged_w', 'k_pad', 'm_tail', 'm_low', 'splitk', 'splitk_capped'}, **T),
    R('tap-c5-72x72-k3-m1-flip', 'c5_1', (1, 3, 1, 72, 72), P('tap_c5', 'fp32', 3, 3, 2, 4, pixels=256, nsplit=2),
      {'image_tail', 'k_pad', 'm_tail', 'm_low', 'splitk', 'splitk_capped'}, **T),
    R('tap-c5-4x4-k66-capped', 'c5_1', (2, 66, 24, 4, 4), P('tap_c5', 'fp32', 2, 2, 4, 4, pixels=256, nsplit=18, chunks_per_split=1),
      {'image_tail', 'k_pad', 'm_tail', 'm_low', 'splitk', 'splitk_capped'}, **T),
    R('tap-c5-16x16-npos2', 'c5_0', (3, 8, 8, 16, 16), P('tap_c5', 'fp32', 4, 4, 0, 2, pixels=256, nsplit=2),
      {'m_tail', 'm_low', 'splitk', 'splitk_capped'}, **T),
    # transposed conv forward
    R('tap-dt-9x12-k12-m65', 'dt_fwd', (2, 12, 65, 9, 12), P('tap_dt', 'fp32', 0, 2, 5, 4, pixels=128, nsplit=4, grid_y=4),
      {'image_tail', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-dt-72x72-k3-m1-parts', 'dt_parts', (1, 3, 1, 72, 72), P('tap_dt', 'fp32', 3, 3, 1, 2, pixels=128, nsplit=2),
      {'image_tail', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-dt-2x2-k66-capped', 'dt_fwd', (2, 66, 64, 2, 2), P('tap_dt', 'fp32', 1, 1, 5, 2, pixels=128, nsplit=18, chunks_per_split=1),
      {'image_tail', 'k_pad', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-dt-1x4', 'dt_fwd', (3, 8, 8, 1, 4), P('tap_dt', 'fp32', 0, 2, 5, 4, pixels=128, nsplit=2),
      {'image_tail', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-dt-16x16-stats-taken', 'dt_stats', (200, 8, 8, 16, 16), P('tap_dt', 'fp32', 4, 4, 0, 2, pixels=256, nsplit=1, stats=1),
      {'m_tail', 'stats'}, groups=1, **T),
    R('tap-dt-16x16-stats-declined', 'dt_stats', (5, 16, 16, 16, 16), P('tap_dt', 'fp32', 3, 4, 0, 2, pixels=128, nsplit=4, stats=0),
      {'m_tail', 'splitk', 'splitk_capped', 'px128'}, groups=2, **T),
    R('tap-dt-9x12-256-ragged-h', 'dt_fwd', (416, 8, 8, 9, 12), P('tap_dt', 'fp32', 1, 2, 5, 4, pixels=256, nsplit=1, tiles_h=5),
      {'ragged_h', 'm_tail'}, **T),
    R('tap-dt-4x4-npos4', 'dt_fwd', (3072, 8, 8, 4, 4), P('tap_dt', 'fp32', 2, 2, 4, 4, pixels=256, nsplit=1), {'m_tail'}, **T),
    # transposed conv data gradient
    R('tap-dg-9x12-npos16', 'dt_dgrad', (2, 12, 65, 9, 12), P('tap_dg', 'fp32', 0, 2, 5, 16, pixels=128, nsplit=18, chunks_per_split=2),
      {'image_tail', 'k_pad', 'm_tail', 'splitk', 'px128'}, **T),
    R('tap-dg-72x72-k1-masked-cin', 'dt_dgrad', (1, 3, 1, 72, 72), P('tap_dg', 'fp32', 3, 3, 1, 8, pixels=128, nsplit=4),
      {'image_tail', 'k_pad', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, cin_out=2, **T),
    R('tap-dg-12x9-256-ragged-w', 'dt_dgrad', (832, 8, 8, 12, 9), P('tap_dg', 'fp32', 2, 1, 5, 16, pixels=256, nsplit=1, tiles_w=5),
      {'ragged_w', 'm_tail'}, **T),
    # (the one-bf16 form cannot hold this halo tile -- plan_b1 refuses and the layer keeps the fp32 plan: no b1 run of this row)
    R('tap-dg-1x4', 'dt_dgrad', (3, 8, 8, 1, 4), P('tap_dg', 'fp32', 0, 2, 5, 16, pixels=128, nsplit=4),
      {'image_tail', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, kqp=0, winop=0),
    R('tap-dg-2x2-m66', 'dt_dgrad', (2, 66, 64, 2, 2), P('tap_dg', 'fp32', 1, 1, 5, 8, pixels=128, nsplit=32, grid_y=2),
      {'image_tail', 'm_tail', 'splitk', 'splitk_capped', 'px128'}, **T),
    R('tap-dg-4x4-npos16-256', 'dt_dgrad', (6144, 8, 8, 4, 4), P('tap_dg', 'fp32', 2, 2, 4, 16, pixels=256, nsplit=1), {'m_tail'}, **T),
]

# ---- Winograd F(2x2, 3x3): gx_conv3x3_wino modes 0 / 1, and gx_conv3x3_fwd / _dgrad at gx_conv3x3_wino_policy(2)
W = dict(pixels=128)
WINO_CASES = [
    R('wino-8x16-min-f32', 'wino0', (2, 16, 16, 8, 16), P('wino', 'fp32', tiles_h=1, tiles_w=1, **W), {'m_tail'}, wino=0),
    R('wino-8x16-min', 'wino0', (2, 16, 16, 8, 16), P('wino', 'bf16x6', tiles_h=1, tiles_w=1, **W), {'m_tail'}, wino=1, b1=True),
    R('wino-8x256-m65', 'wino0', (1, 16, 65, 8, 256), P('wino', 'bf16x6', tiles_h=1, tiles_w=16, grid_y=2, **W), {'m_tail'}, wino=1,
      b1=True),
    R('wino-128x16-k17-dgrad-f32', 'wino1', (1, 16, 17, 128, 16), P('wino', 'fp32', tiles_h=16, tiles_w=1, **W), {'k_pad', 'm_tail'},
      wino=0),
    R('wino-128x16-k17-dgrad', 'wino1', (1, 16, 17, 128, 16), P('wino', 'bf16x6', tiles_h=16, tiles_w=1, **W), {'k_pad', 'm_tail'},
      wino=1, b1=True),
    R('wino-through-fwd-k17-m65', 'c3_fwd', (1, 17, 65, 16, 32), P('wino', 'bf16x6', tiles_h=2, tiles_w=2, grid_y=2, **W),
      {'k_pad', 'm_tail'}, kqp=0, winop=2, wino=1),
    R('wino-through-dgrad', 'c3_dgrad', (1, 64, 16, 8, 16), P('wino', 'fp32', tiles_h=1, tiles_w=1, **W), (), kqp=0, winop=2, wino=0),
    # just outside wino_shape_ok (H % 8 != 0, W % 16 != 0, K < 16): falls through to the tap conv
    R('wino-out-12x24-k8', 'c3_fwd', (2, 8, 64, 12, 24), P('tap_c3', 'fp32', 2, 3, 3, 2, pixels=256, nsplit=1), {'image_tail'}, kqp=0,
      winop=2, wino=1),
]

# ---- the input-layer kernel of gx_conv3x3_fwd (conv3x3_smallcin_fwd_kernel): Cin == 4, W % 4 == 0, H W >= 1024
S = dict(pixels=1024)
SMALLCIN_CASES = [
    R('smallcin-32x32-cout1', 'c3_act', (1, 4, 1, 32, 32), P('smallcin', 'fp32', grid_x=1, grid_y=1, **S), {'m_tail'}, act='elu'),
    R('smallcin-16x64-cout9-n3', 'c3_fwd', (3, 4, 9, 16, 64), P('smallcin', 'fp32', grid_x=3, grid_y=2, **S), {'m_tail'}),
    # the boundary's other side, one step each: Cin = 5, H W = 1008, W % 4 = 2
    R('smallcin-out-cin5', 'c3_act', (1, 5, 8, 32, 32), P('tap_c3', 'fp32', 3, 5, 0, 2, pixels=256), {'k_pad', 'm_tail', 'm_low'},
      act='elu', kqp=0, winop=0),
    R('smallcin-out-28x36', 'c3_fwd', (2, 4, 8, 28, 36), P('tap_c3', 'fp32', 2, 2, 4, 4, pixels=256),
      {'image_tail', 'k_pad', 'm_tail', 'm_low'}, kqp=0, winop=0),
    R('smallcin-out-32x34', 'c3_fwd', (1, 4, 8, 32, 34), P('tap_c3', 'fp32', 5, 1, 2, 4, pixels=256),
      {'image_tail', 'k_pad', 'm_tail', 'm_low'}, kqp=0, winop=0),
]

TABLES = {'kq_c3': KQ_C3_CASES, 'kq_deconv': KQ_DECONV_CASES, 'kq_c3h': KQ_C3H_CASES, 'kq_c5h': KQ_C5H_CASES, 'tap': TAP_CASES,
          'wino': WINO_CASES, 'smallcin': SMALLCIN_CASES}
ALL_CASES = [r for t in TABLES.values() for r in t]

# ---- refusals decided on the host before any launch.  REFUSALS: check_dims, the FIRST check of its entry point -- (entry point,
#      kind, dims, a piece of the message); tests/test_conv_plans_cpu.py calls each with NULL pointers (a refusal that stopped
#      refusing then meets the null-pointer check, never a launch) and expects GenesisHipError with that message, without a GPU.
#      UNSUPPORTED: what *_supported / wino_shape_ok decide (their entry points check the pointers first): the queries answer 0.
REFUSALS = [
    ('gx_conv3x3_fwd', 'c3', (2, 8, 8, 3, 3), 'a multiple of 4'),             # H W % 4 != 0
    ('gx_conv3x3_fwd', 'c3', (2, 8, 8, 4, 1), 'W in [2,4096]'),               # W < 2
    ('gx_conv3x3_dgrad', 'c3', (2, 8, 8, 1, 2), 'a multiple of 4'),           # H W = 2
    ('gx_conv3x3_dgrad', 'c3', (0, 8, 8, 4, 4), 'bad N/C'),                   # N = 0
    ('gx_conv3x3_dgrad_act', 'c3_dgrad_act', (2, 16, 16, 5, 5), 'a multiple of 4'),
    ('gx_deconv5x5s2_fwd', 'dt', (2, 8, 8, 3, 5), 'a multiple of 4'),         # H W % 4 != 0
    ('gx_deconv5x5s2_dgrad', 'dg', (2, 8, 8, 4, 4096 * 2), 'W in [2,4096]'),  # W > 4096
]
UNSUPPORTED = [                                             # (query, arguments): must answer 0
    ('gx_conv5x5s1_supported', (2, 16, 16, 3, 8)), ('gx_conv5x5s1_supported', (2, 16, 16, 8, 2)),
    ('gx_conv3x3_dgrad_act_supported', (2, 64, 16, 8, 8)),       # Cin = 64 > 32
    ('gx_conv3x3_dgrad_act_supported', (2, 32, 24, 8, 8)),       # Cout % 16 != 0
    ('gx_conv3x3_wino_supported', (2, 16, 16, 12, 16)),          # H % 8 != 0
    ('gx_conv3x3_wino_supported', (2, 16, 16, 8, 8)),            # W < 16
    ('gx_conv3x3_wino_supported', (2, 16, 16, 8, 24)),           # W % 16 != 0
    ('gx_conv3x3_wino_supported', (2, 8, 64, 16, 16)),           # K < 16
    ('gx_conv3x3_wino_supported', (2, 16, 15, 8, 16)),           # M < 16
]


# ===================================================================================================== geometry of a row
def geometry(row):
    """(N, K, M, Hb, Wb) as the planners see the row: reduction channels, output channels, base grid."""
    N, a, b, H, Wd = row['dims']
    op = row['op']
    if op in ('c5_0', 'c5_1'):
        return N, a, b, H, Wd
    if op in ('c3_dgrad', 'c3_dgrad_act', 'c3_dgrad_parts', 'wino1'):
        return N, b, a, H, Wd
    if op == 'dt_dgrad':
        return N, b, row.get('cin_out', a), H, Wd
    return N, a, b, H, Wd


def tails_of(row, plan):
    """The tails a launch with this record has on this row's shape -- every declared `tails` set is checked against it."""
    N, K, M, Hb, Wb = geometry(row)
    fam, t = plan['family'], set()
    if fam == 'wino':
        if K % (16 if plan['form'] != 'fp32' else 8):
            t.add('k_pad')
        if M % 64:
            t.add('m_tail')
        return t
    if fam == 'smallcin':
        if M % 8:
            t.add('m_tail')
        return t
    TH, TW, G = plan['rt_th'] or 1 << plan['lTH'], plan['rt_tw'] or 1 << plan['lTW'], 1 << plan['lG']
    if G > 1 and N % G:
        t.add('image_tail')
    if TH > Hb and plan['rt_th']:
        t.add('tile_taller')
    elif TH < Hb and Hb % TH:
        t.add('ragged_h')
    if TW < Wb and Wb % TW:
        t.add('ragged_w')
    if M % (32 if fam == 'kq_c3h' else 64):
        t.add('m_tail')
    if plan['stats']:
        t.add('stats')
    if fam.startswith('tap_'):
        kc = 8 if plan['form'] == 'bf16x1' else {'tap_c3': 8, 'tap_dt': 4, 'tap_dg': 2, 'tap_c5': 4}[fam]
        nchunks = (K + 7) // 8 * 8 // kc
        if K % 8:
            t.add('k_pad')
        if plan['nsplit'] > 1:
            t.add('splitk')
            if nchunks % plan['chunks_per_split']:
                t.add('splitk_uneven')
            if plan['nsplit'] == nchunks:
                t.add('splitk_capped')
        if plan['pixels'] == 128:
            t.add('px128')
        if fam in ('tap_c3', 'tap_c5') and M <= 32:
            t.add('m_low')
    elif fam == 'kq_c3h':
        if plan['nfull'] > plan['grid_x']:
            t.add('second_round')
    elif fam != 'kq_c5h':
        ptiles = plan['tiles_h'] * plan['tiles_w'] * ((N + G - 1) // G)
        if plan['nfull'] < ptiles:
            t.add('split_tail')
        elif ptiles > 256 and 0 < ptiles % 256 <= 128:
            t.add('split_refused')
        if fam == 'kq_dth' and plan['grid_z'] == 1:
            t.add('ilv')
    return t


# ===================================================================================================== operands and references
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def close(a, b, rtol, atol, msg=''):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, '%s max err %.3e (ref max %.3e)' % (msg, err, ref)


def ident(t):
    return t.double()


def _act(v, act):
    return F.relu(v) if act == 'relu' else (F.elu(v) if act == 'elu' else v)


_OPERANDS = {}


def _key(row):
    """What the operands and the fp64 reference depend on: rows that differ in form or policy alone share both."""
    return row['op'], row['dims'], row.get('act'), row.get('groups'), row.get('cin_out')


def operands(row):
    """The row's seeded CPU operands (made once per row, never modified)."""
    if _key(row) in _OPERANDS:
        return _OPERANDS[_key(row)]
    N, a, b, H, Wd = row['dims']
    op = row['op']
    o = {}
    if op.startswith('c3_') or op.startswith('wino'):
        Ci, Co = a, b
        o['w'] = rnd(Co, Ci, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * Ci))
        if op in ('c3_fwd', 'c3_act', 'c3_fwd_parts', 'wino0'):
            o['x'] = rnd(N, Ci, H, Wd, seed=1)
        else:
            o['x'] = rnd(N, Co, H, Wd, seed=4)               # dy
        if op == 'c3_act':
            o['bias'] = rnd(Co, seed=3, scale=0.3)
        if op == 'c3_dgrad_act':
            o['xout'] = _act(rnd(N, Ci, H, Wd, seed=5), row['act'])
    elif op.startswith('c5_'):
        K, M = a, b
        o['x'] = rnd(N, K, H, Wd, seed=1)
        o['w'] = rnd(*((K, M, 5, 5) if op == 'c5_1' else (M, K, 5, 5)), seed=2, scale=1.0 / math.sqrt(25 * K))
    else:
        Ci, Co = a, b
        o['w'] = rnd(Ci, Co, 5, 5, seed=5, scale=1.0 / math.sqrt(Ci * 6.25))
        if op == 'dt_dgrad':
            o['x'] = rnd(N, Co, 2 * H, 2 * Wd, seed=7)       # dy
        else:
            o['x'] = rnd(N, Ci, H, Wd, seed=4)
            if op != 'dt_parts':
                o['bias'] = rnd(Co, seed=6, scale=0.3)
    _OPERANDS[_key(row)] = o
    return o


def reference(row, rounder=ident, absolute=False):
    """float64 torch on the CPU of the row's operation on rounder(operands); absolute: the same sum over |a| |b| (+ |bias|), the
    scale tests/test_tapconv_precision_gpu.py's `judge` measures against.  -> {output name: tensor}."""
    o, op = operands(row), row['op']
    mag = (lambda t: t.abs()) if absolute else (lambda t: t)
    x, w = mag(rounder(o['x'])), mag(rounder(o['w']))
    bias = mag(o['bias'].double()) if 'bias' in o else None
    if op in ('c3_fwd', 'c3_fwd_parts', 'wino0'):
        return {'y': F.conv2d(x, w, None, 1, 1)}
    if op == 'c3_act':
        y = F.conv2d(x, w, bias, 1, 1)
        return {'y': y if absolute else _act(y, row['act'])}
    if op in ('c3_dgrad', 'c3_dgrad_parts', 'wino1'):
        return {'y': F.conv_transpose2d(x, w, None, 1, 1)}
    if op == 'c3_dgrad_act':
        xo = o['xout'].double()
        d = torch.where(xo > 0, torch.ones_like(xo), xo + 1.0 if row['act'] == 'elu' else torch.zeros_like(xo))
        y = F.conv_transpose2d(x, w, None, 1, 1) * d
        return {'y': y, 'dbias': y.sum((0, 2, 3))}
    if op == 'c5_0':
        return {'y': F.conv2d(x, w, None, 1, 2)}
    if op == 'c5_1':
        return {'y': F.conv_transpose2d(x, w, None, 1, 2)}
    if op in ('dt_fwd', 'dt_parts', 'dt_stats'):
        y = F.conv_transpose2d(x, w, bias, 2, 2, 1)
        out = {'y': y}
        if op == 'dt_stats' and not absolute:
            g = y.view(y.shape[0], row['groups'], -1)
            out['mean'], out['rstd'] = g.mean(2).flatten(), (g.var(2, unbiased=False) + 1e-5).rsqrt().flatten()
        return out
    assert op == 'dt_dgrad', op
    return {'y': F.conv2d(x, w, None, 2, 2)[:, :row.get('cin_out', row['dims'][1])]}


_REFS = {}


def fp64_reference(row):
    if _key(row) not in _REFS:
        _REFS[_key(row)] = reference(row)
    return _REFS[_key(row)]


# ===================================================================================================== the guarded launch
def _guarded_in(t):
    """t in the middle of a NaN buffer -> (the buffer, the view)."""
    buf = torch.full((t.numel() + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guarded_out(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + n] = float('nan')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _bands_intact(buf, n, what):
    s = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    assert torch.equal(buf[:GUARD], s), '%s: the guard band in FRONT of it was written' % what
    assert torch.equal(buf[GUARD + n:], s), '%s: the guard band BEHIND it was written' % what


class switches(object):
    """The row's dispatch policies and precision switches, the defaults restored on the way out."""

    def __init__(self, row, kq=None, wino=None, tapm=None):
        self.row = row
        self.kq = row.get('kq') if kq is None else kq
        self.wino = row.get('wino') if wino is None else wino
        self.tapm = row.get('tapm') if tapm is None else tapm

    def __enter__(self):
        from genesis_amd import _lib
        _lib.call('gx_kq_policy', self.row.get('kqp', 1))
        _lib.call('gx_conv3x3_wino_policy', self.row.get('winop', 1))
        if self.kq is not None:
            _lib.call('gx_kq_precision', self.kq)
        if self.wino is not None:
            _lib.call('gx_wino_precision', self.wino)
        if self.tapm is not None:
            assert int(_lib.load().gx_tapconv_precision(self.tapm)) >= 0

    def __exit__(self, *exc):
        from genesis_amd import _lib
        _lib.call('gx_kq_policy', 1)
        _lib.call('gx_conv3x3_wino_policy', 1)
        _lib.call('gx_kq_precision', -1)
        _lib.call('gx_wino_precision', -1)
        _lib.load().gx_tapconv_precision(-1)
        return False


def launch(row):
    """Runs the row's entry point on guarded buffers with the switches as they are.  -> ({output name: CPU tensor}, plan record,
    extras).  Asserts the guard bands of every output and of the workspace."""
    from genesis_amd import _lib, hip_ops as hip
    op = row['op']
    N, a, b, H, Wd = row['dims']
    o = operands(row)
    keep = {k: _guarded_in(v) for k, v in o.items()}
    p = {k: ctypes.c_void_p(v[1].data_ptr()) for k, v in keep.items()}
    dims = (N, a, b, H, Wd)
    act = hip.ACTS[row.get('act')]
    s = hip._stream()
    outs, extra = {}, {}

    def out(name, shape):
        outs[name] = _guarded_out(shape)
        return ctypes.c_void_p(outs[name][1].data_ptr())

    if op.startswith('c3_'):
        q = 'gx_conv3x3_dgrad_act_ws_bytes' if op == 'c3_dgrad_act' else 'gx_conv3x3_ws_bytes'
    elif op.startswith('wino'):
        q = 'gx_conv3x3_wino_ws_bytes'
    elif op.startswith('c5_'):
        q = 'gx_conv5x5s1_ws_bytes'
    else:
        q = 'gx_deconv5x5s2_gn_stats_ws_bytes' if op == 'dt_stats' else 'gx_deconv5x5s2_ws_bytes'
    nb = _lib.query(q, *dims)
    wsbuf = torch.full((nb + 2 * WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)        # (0xFF bytes read as floats: NaN)
    wsbuf[:WS_GUARD] = 0xA5
    wsbuf[WS_GUARD + nb:] = 0xA5
    ws = ctypes.c_void_p(wsbuf.data_ptr() + WS_GUARD)
    parts, nsplit, stride = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_size_t()
    tapbuf = None
    if row.get('tap'):
        tapbuf = _guarded_out((16384,))
        _lib.call('gx_amax_tap', ctypes.c_void_p(tapbuf[1].data_ptr()), 16384, N * b * H * Wd)

    if op == 'c3_fwd':
        _lib.call('gx_conv3x3_fwd', p['x'], p['w'], out('y', (N, b, H, Wd)), *dims, ws, nb, s)
    elif op == 'c3_act':
        _lib.call('gx_conv3x3_bias_act_fwd', p['x'], p['w'], p['bias'], act, out('y', (N, b, H, Wd)), *dims, ws, nb, s)
    elif op == 'c3_fwd_parts':
        _lib.call('gx_conv3x3_fwd_parts', p['x'], p['w'], out('y', (N, b, H, Wd)), *dims, ws, nb, ctypes.byref(parts),
                  ctypes.byref(nsplit), ctypes.byref(stride), s)
    elif op == 'c3_dgrad':
        _lib.call('gx_conv3x3_dgrad', p['x'], p['w'], out('y', (N, a, H, Wd)), *dims, ws, nb, s)
    elif op == 'c3_dgrad_parts':
        _lib.call('gx_conv3x3_dgrad_parts', p['x'], p['w'], out('y', (N, a, H, Wd)), *dims, ws, nb, ctypes.byref(parts),
                  ctypes.byref(nsplit), ctypes.byref(stride), s)
    elif op == 'c3_dgrad_act':
        _lib.call('gx_conv3x3_dgrad_act', p['x'], p['w'], p['xout'], act, out('y', (N, a, H, Wd)), out('dbias', (a,)), *dims, ws, nb, s)
    elif op in ('wino0', 'wino1'):
        mode = int(op[-1])
        _lib.call('gx_conv3x3_wino', p['x'], p['w'], out('y', (N, b if mode == 0 else a, H, Wd)), *dims, mode, ws, nb, s)
    elif op in ('c5_0', 'c5_1'):
        _lib.call('gx_conv5x5s1', p['x'], p['w'], out('y', (N, b, H, Wd)), *dims, int(op[-1]), ws, nb, s)
    elif op == 'dt_fwd':
        _lib.call('gx_deconv5x5s2_fwd', p['x'], p['w'], p['bias'], out('y', (N, b, 2 * H, 2 * Wd)), *dims, ws, nb, s)
    elif op == 'dt_parts':
        _lib.call('gx_deconv5x5s2_fwd_parts', p['x'], p['w'], out('y', (N, b, 2 * H, 2 * Wd)), *dims, ws, nb, ctypes.byref(parts),
                  ctypes.byref(nsplit), ctypes.byref(stride), s)
    elif op == 'dt_stats':
        fused, g = ctypes.c_int(-1), row['groups']
        _lib.call('gx_deconv5x5s2_gn_stats_fwd', p['x'], p['w'], p['bias'], out('y', (N, b, 2 * H, 2 * Wd)), *dims, g, 1e-5,
                  out('mean', (N * g,)), out('rstd', (N * g,)), ctypes.byref(fused), ws, nb, s)
        extra['fused'] = fused.value
    else:
        assert op == 'dt_dgrad', op
        co = row.get('cin_out', a)
        _lib.call('gx_deconv5x5s2_dgrad', p['x'], p['w'], out('y', (N, co, H, Wd)), N, a, co, b, H, Wd, ws, nb, s)
    plan = hip.conv_last_plan()
    torch.cuda.synchronize()

    for name, (buf, view) in outs.items():
        _bands_intact(buf, view.numel(), '%s %s' % (row['id'], name))
    band = torch.full((WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert torch.equal(wsbuf[:WS_GUARD], band), '%s: the bytes in front of the workspace were written' % row['id']
    assert torch.equal(wsbuf[WS_GUARD + nb:], band), '%s: the bytes behind the workspace (%d bytes from %s) were written' % (row['id'], nb, q)
    for k, (buf, view) in keep.items():
        assert torch.equal(view.cpu(), o[k]), '%s: operand %s was modified' % (row['id'], k)

    res = {k: v[1].cpu() for k, v in outs.items()}
    if op.endswith('_parts'):
        extra['nsplit'] = nsplit.value
        if nsplit.value == 1:
            assert parts.value == outs['y'][1].data_ptr()
        else:       # the slabs live in the caller's workspace: their sum, in slab order, is the layer's output
            off = parts.value - wsbuf.data_ptr()
            n = outs['y'][1].numel()
            assert stride.value == n and WS_GUARD <= off and off + 4 * n * nsplit.value <= WS_GUARD + nb, (off, nb, n, nsplit.value)
            slabs = wsbuf[off:off + 4 * n * nsplit.value].view(torch.float32).view(nsplit.value, *outs['y'][1].shape)
            res['y'] = slabs.double().sum(0).cpu()
    if tapbuf is not None:
        ntap = _lib.query('gx_amax_tap_result')
        _bands_intact(tapbuf[0], 16384, row['id'] + ' partial maxima')
        extra['tap_n'] = ntap
        extra['tap_max'] = float(tapbuf[1][:ntap].max()) if ntap > 0 else None
    return res, plan, extra


def check_plan(row, plan, declared=None):
    declared = row['plan'] if declared is None else declared
    got = {k: plan[k] for k in declared}
    assert got == declared, 'the table is wrong about %s: declared %s, the launch recorded %s' % (row['id'], declared, plan)
    assert tails_of(row, plan) == set(row['tails']), ('the table is wrong about the tails of %s: declared %s, the recorded plan has %s (%s)'
                                                      % (row['id'], sorted(row['tails']), sorted(tails_of(row, plan)), plan))


def bounds(plan):
    """rtol = atol of tests/test_kernels_gpu.py for the family that ran: 1e-5 on the <= 32-channel 16-bit-pipe kernel, else 2e-5."""
    return 1e-5 if plan['family'] == 'kq_c3h' else 2e-5


def _ids(rows):
    return [r['id'] for r in rows]


# ===================================================================================================== the tests
@pytest.mark.parametrize('row', ALL_CASES, ids=_ids(ALL_CASES))
def test_conv_plan_case(row):
    """Steps 1 - 5 of the module docstring in the row's declared form."""
    assert all(k in row['plan'] for k in PLAN_KEYS)
    ref = fp64_reference(row)
    with switches(row):
        res, plan, extra = launch(row)
    check_plan(row, plan)
    tol = bounds(plan)
    assert bool(torch.isfinite(res['y']).all()), '%s: non-finite output (an element nobody wrote, or a NaN operand guard read)' % row['id']
    print('%-44s %s  max |err| %.3e (ref max %.3e)' % (row['id'], {k: plan[k] for k in ('family', 'form', 'grid_x', 'grid_y', 'grid_z')},
                                                        float((res['y'].double() - ref['y']).abs().max()), float(ref['y'].abs().max())))
    close(res['y'], ref['y'], tol, tol, row['id'] + ' y')
    if row['op'] == 'c3_dgrad_act':     # (the bias gradient's bound: test_conv3x3_data_gradient_with_the_previous_layers_activation_backward)
        close(res['dbias'], ref['dbias'], 1e-5, 2e-6 * float(ref['dbias'].abs().max()) + 1e-5, row['id'] + ' dbias')
    if row['op'] == 'dt_stats':
        assert extra['fused'] == plan['stats'] == row['plan']['stats'], (extra, plan)
        if extra['fused']:              # (test_deconv_epilogue_groupnorm_statistics' bounds)
            m, r = res['mean'].double(), res['rstd'].double()
            assert bool(((m - ref['mean']).abs() <= 2e-6 + 2e-5 * ref['mean'].abs()).all()), row['id'] + ' mean'
            assert bool(((r - ref['rstd']).abs() <= 2e-5 * ref['rstd'].abs()).all()), row['id'] + ' rstd'
    if row['op'].endswith('_parts'):
        assert extra['nsplit'] == plan['nsplit'] == row['plan'].get('nsplit', plan['nsplit']), (extra, plan)
    if row.get('tap'):                  # one partial maximum per workgroup of the launch, together the output's largest magnitude
        assert extra['tap_n'] == plan['grid_x'] * plan['grid_y'], (extra, plan)
        assert extra['tap_max'] == float(res['y'].abs().max()), extra


B1_KQ = [r for r in ALL_CASES if r.get('b1') and r['plan']['family'].startswith('kq_')]
B1_WINO = [r for r in ALL_CASES if r.get('b1') and r['plan']['family'] == 'wino']
B1_TAP = [r for r in ALL_CASES if r.get('b1') and r['plan']['family'].startswith('tap_')]


def _b1_modes(row, which):
    """{0, 2, 3: outputs} of the row with gx_<which>_precision set; mode 3 must record the same family in the one-bf16 form."""
    got = {}
    # (gx_conv3x3_dgrad_act exists on the 16-bit pipe only: its fp32-accurate baseline in `check`'s slot 0 is the six-piece form)
    base = 1 if row['op'] == 'c3_dgrad_act' else 0
    for m in (base, 2, 3):
        with switches(row, **{which: m}):
            res, plan, _ = launch(row)
        got[0 if m == base else m] = res['y']
        if m == 3:
            assert (plan['family'], plan['form']) == (row['plan']['family'], 'bf16x1'), plan
            for k in ('lTH', 'lTW', 'lG', 'nq'):          # (the same tile: the form changes the LDS size per nq, not the plan)
                assert plan[k] == row['plan'][k], (k, plan)
    return got


@pytest.mark.parametrize('row', B1_KQ, ids=_ids(B1_KQ))
def test_conv_plan_case_on_one_bf16_piece_16_bit_pipe(row):
    """gx_kq_precision(3) on the rows of the 16-bit-pipe families: tests/test_matmul_precision_gpu.py's yardstick (fp64 on the
    bf16-rounded operands) and bars, its `check`."""
    from tests.test_matmul_precision_gpu import bf, check
    check(row['id'], _b1_modes(row, 'kq'), reference(row, bf)['y'], 1)


@pytest.mark.parametrize('row', B1_WINO, ids=_ids(B1_WINO))
def test_conv_plan_case_on_one_bf16_piece_winograd(row):
    """gx_wino_precision(3): tests/test_matmul_precision_gpu.py's Winograd-domain yardstick (wino_ref) and `check`."""
    from tests.test_matmul_precision_gpu import check, wino_ref
    o = operands(row)
    ref = wino_ref(o['x'], o['w']) if row['op'] == 'wino0' else wino_ref(o['x'], o['w'].flip(2, 3).transpose(0, 1))
    check(row['id'], _b1_modes(row, 'wino'), ref, 1)


@pytest.mark.parametrize('row', B1_TAP, ids=_ids(B1_TAP))
def test_conv_plan_case_on_one_bf16_piece_tap_conv(row):
    """gx_tapconv_precision(3) on the tap-conv rows: tests/test_tapconv_precision_gpu.py's yardstick and bars, its `judge`."""
    from genesis_amd import _lib
    from tests.test_tapconv_precision_gpu import bf, judge
    got = {}
    for m in (3, 0):
        with switches(row, tapm=m):
            res, plan, _ = launch(row)
            assert int(_lib.load().gx_tapconv_last_mode()) == m
        assert (plan['family'], plan['form']) == (row['plan']['family'], 'bf16x1' if m == 3 else 'fp32'), plan
        got[m] = res['y']
    judge(row['id'], got, reference(row, bf)['y'], reference(row, bf, absolute=True)['y'])
