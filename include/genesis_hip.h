/* libgenesis_hip.so -- C ABI of the MI355X-native GENESIS-V2 hot path.
 *
 * The reference (applied-ai-lab/genesis) is pure Python/PyTorch: it has NO native/FFI
 * boundary.  The drop-in boundary is therefore the reference's Python interface
 * (models/genesisv2_config.py:45-46 `load(cfg)`, :110-203 `forward(x)`), mirrored by
 * genesis_amd/genesisv2_config.py; this library sits UNDER that module and each entry
 * point replaces the ATen op group the reference executes at the cited file:line.
 *
 * Conventions:
 *   - arguments are raw device pointers + explicit sizes; tensors are contiguous NCHW fp32 (gx_vis_compose, which writes
 *     the TensorBoard image grids, takes its many sources through a device table of descriptors instead: see there);
 *   - the caller (PyTorch caching allocator) owns every buffer, including workspaces, whose
 *     required size is returned by the matching *_ws_bytes() query;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t); no allocation, no sync;
 *   - return 0 on success, negative GX_E* on error (gx_last_error() gives the message,
 *     thread-local); nothing throws across the boundary.
 */
#ifndef GENESIS_HIP_H
#define GENESIS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gx_stream_t; /* hipStream_t */

#define GX_OK 0
#define GX_EINVAL (-1)  /* bad argument / unsupported shape */
#define GX_ELAUNCH (-2) /* kernel launch failed */
#define GX_EDATA (-3)   /* malformed or corrupt input data (TFRecord reader) */

const char* gx_last_error(void);
int gx_version(void);

/* ---- conv3x3 stride 1 pad 1, no bias: modules/blocks.py:159-165 (ConvGNReLU[0]);
 *      UNet blocks modules/unet.py:53-56, seg_head/feat_head models/genesisv2_config.py:78-80.
 *      w is the nn.Conv2d weight [Cout,Cin,3,3]. fwd/dgrad repack w into `ws`. */
size_t gx_conv3x3_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv3x3_fwd(const float* x, const float* w, float* y, int N, int Cin, int Cout, int H, int W,
                   void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_conv3x3_dgrad(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int H, int W,
                     void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_conv3x3_dgrad_parts(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int H, int W, void* ws,
                           size_t ws_bytes, const float** parts, int* nsplit, size_t* split_stride, gx_stream_t stream);
size_t gx_conv3x3_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv3x3_wgrad(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int H, int W,
                     void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- the same 3x3 convolution by Winograd F(2x2,3x3) (2.25x fewer multiplies; fp32, ordinary rounding differences
 *      against the direct sum).  mode 0: forward y = conv(x, w); mode 1: data gradient dx from dy (same w [Cout,Cin,3,3]).
 *      Eligible shapes: gx_conv3x3_wino_supported (H % 8 == 0, W % 16 == 0, >= 16 channels). */
int gx_conv3x3_wino_supported(int N, int Cin, int Cout, int H, int W);
/*      which layers gx_conv3x3_fwd / _dgrad send to it: 0 none, 1 those whose grid fills the chip (default),
 *      2 every supported shape. */
int gx_conv3x3_wino_policy(int mode);
/*      which matrix pipe the Winograd layers' products run on (3: one bf16 piece per operand, gx_matmul_precision(2)): 1 (default; GENESIS_WINO_BF16X6=0/1 in the environment) = the
 *      bf16 pipe, every fp32 product U * V from six bf16 piece products accumulated in fp32 (hi + mid + lo pieces hold all 24
 *      mantissa bits: fp32 accuracy, tests/test_kernels_gpu.py::test_conv3x3_winograd); 0 = v_mfma_f32_32x32x2_f32.  Packed
 *      operands are laid out for the pipe in force when they were packed: switch between iterations, not inside one. */
int gx_wino_precision(int mode);
/*      k-quad tap-conv kernels (gx_kq.hip: 16-byte k-contiguous MFMA operand reads) behind gx_conv3x3_fwd / _dgrad and
 *      gx_deconv5x5s2_fwd / _dgrad: 0 never, 1 layers whose grid fills the chip (default),
 *      2 every eligible shape (power-of-two grids, reduction channels a multiple of 8). */
int gx_kq_policy(int mode);
/*      weight gradients of layers of width >= 8 (gx_wgq.hip): 1 (default) =
 *      LDS-DMA staged kernels, every queued layer in ONE stream-K launch at gx_defer_flush; 2 = the same kernels, one
 *      launch per (tap class, tile width); 0 = the round-1 kernels everywhere. */
int gx_wgq_policy(int mode);
/*      Which matrix pipe the LDS-DMA weight-gradient kernels multiply on.  1 (default): the bf16 pipe -- every fp32
 *      operand is split into three bf16 pieces (hi + mid + lo = all 24 mantissa bits) and a product is the six piece
 *      products of order <= 2, accumulated in fp32 (v_mfma_f32_32x32x16_bf16): the error against fp64 is that of the
 *      fp32 pipe (tools/bf16x6_probe.hip: 4.8e-7 vs 5.8e-7 relative L2; tests/test_kernels_gpu.py compares both pipes
 *      with fp64), at 6 x 32 instead of 8 x 64 matrix-pipe cycles per 16 contraction steps.  0: the fp32 pipe
 *      (v_mfma_f32_32x32x2_f32).  Environment: GENESIS_WGQ_BF16X6=0.  3: one bf16 piece per operand on the row-ring and LDS-DMA
 *      tiles of the stream-K launch (gx_matmul_precision(2)); gx_wgq_last_f16_share counts fp16-piece flops only. */
int gx_wgq_precision(int mode);
/*      Tile shape of the bf16-pipe weight gradients for layers whose base rows are 32 or 64 pixels wide (conv3x3 at
 *      32 / 64, transposed conv from 32 x 32): 1 (default) row-ring tiles -- a tile is one full-width base row, the x rows
 *      roll through a four-slot LDS ring, every operand value is split into its bf16 planes once on its way into LDS and
 *      the taps' column shifts are funnel shifts of the dy operand -- 0 the 64-pixel LDS-DMA tiles whose lanes split
 *      what they read (the A/B reference).  Replaces the same reference ops as
 *      gx_conv3x3_wgrad / gx_deconv5x5s2_wgrad (modules/blocks.py:159-165, models/genesisv2_config.py:89-99). */
/*      Mode 2 of gx_wgq_precision (the default since round 6; GENESIS_WGQ_F16X3=0: mode 1): the row-ring tiles form every fp32
 *      product from THREE fp16 piece products (x * 2^e = hi + lo, one power-of-two scale per operand TENSOR) instead of six
 *      bf16 ones -- for the layers whose operands' largest magnitudes are known without a pass over them.
 *      gx_wgq_operand_amax(...) is the one-shot, per-thread hint the NEXT gx_conv3x3_wgrad / gx_deconv5x5s2_wgrad call takes:
 *      partial maxima of dy in a0[0..na0) (+ a1[0..na1)), of x in b0[0..nb0) (+ b1[0..nb1): a concat buffer written by two
 *      producers), as left by gx_amax_tap / gx_amax_parts, and out2 -- two floats that receive {max |dy|, max |x|} in a small
 *      launch ahead of the stream-K launch.  All of them stay alive until the queued launch has run.  Layers without the hint
 *      (or with partial maxima of only one operand) run on bf16 pieces.  Range: a value below max|tensor| * 2^-18 keeps fewer
 *      than 22 bits (its low piece is an fp16 subnormal), below max|tensor| * 2^-40 it is flushed -- absolute accuracy
 *      2^-40 max|tensor|; tests/test_kernels_gpu.py *fp16x3* bound the error per output channel against fp64. */
int gx_wgq_operand_amax(const float* a0, int na0, const float* a1, int na1, const float* b0, int nb0, const float* b1,
                        int nb1, float* out2);
/*      Measurement: the share of the LAST stream-K launch's algorithmic flops that ran on three fp16 piece products (the rest:
 *      six bf16 ones) -- what bench.py prices the launch's matrix-pipe ceiling with. */
double gx_wgq_last_f16_share(void);
int gx_wgq_ring(int on);
/*      The same choice for the chip-filling transposed-conv forward / data-gradient layers (gx_kq.hip): 1
 *      bf16 pipe -- the staging splits the input tile into its three bf16 planes, the pack kernel the weights; needs a
 *      multiple of 16 reduction channels and a tile of <= 384 halo positions, other layers stay on the fp32 pipe --
 *      0 fp32 pipe.  Environment: GENESIS_KQ_BF16X6=0.  2: as 1, the transposed-conv forward / data gradient from THREE fp16
 *      piece products instead (x * 2^sx = hi + lo, 22 significant bits; hi*hi + hi*lo + lo*hi), one power-of-two scale per
 *      tensor from its largest magnitude -- the input's by one small launch ahead of the conv (partial maxima at the end of the
 *      conv's workspace), the weights' at pack time; error against fp64 at or below the bf16 form's on every operand set of the
 *      tests, two thirds of its matrix-pipe time: the DEFAULT since round 5 (GENESIS_KQ_F16X3=0: mode 1).  -1: back to the
 *      environment's default.
 *      RANGE of mode 2 (the same holds for gx_wgq_precision(2) and gx_wino_precision(2)): the scale is ONE power of two per tensor,
 *      max |x| * 2^e in [2^14, 2^15).  A value keeps its 22 significant bits down to max |x| * 2^-18; below that its low piece is
 *      an fp16 subnormal and bits drop off one by one; below max |x| * 2^-28 the high piece is subnormal too and below 2^-40 the
 *      value is flushed -- i.e. the representation error is max(2^-23 |x|, 2^-40 max |x|): absolute, not relative, accuracy for the
 *      smallest values of a tensor with one extreme outlier (an element 1e9 times the rest: tests/test_kernels_gpu.py
 *      ::test_fp16x3_transposed_conv_scales_follow_the_tensors[one_huge] pins exactly that bound).  Mode 1 has fp32's range.
 *      3 (the same for gx_wgq_precision(3) and gx_wino_precision(3)): the same layers from ONE bf16 piece per operand -- see
 *      gx_matmul_precision below. */
int gx_kq_precision(int mode);
/*      ONE switch for the three families above (gx_kq.hip, gx_wino.hip, gx_wgq.hip: the layers that multiply on the 16-bit matrix
 *      pipe), in torch.set_float32_matmul_precision's vocabulary:
 *        0 highest -- mode 0 of all three: every product on the fp32 pipe (v_mfma_f32_32x32x2_f32);
 *        1 high    -- mode 2 of all three (the defaults): fp32-equivalent products from three fp16 / six bf16 piece products;
 *        2 medium  -- mode 3 of all three: every operand of those layers rounded ONCE to bf16 (round to nearest even), one
 *                     v_mfma_f32_32x32x16_bf16 per k-step, fp32 accumulation, fp32 tensors.  Error statement: each product carries
 *                     the relative error of one bf16 product -- two roundings of 2^-9 each, about 2^-8 per product -- and fp32's
 *                     exponent range (no per-tensor scale: the partial-maxima hints of gx_amax_tap / gx_kq_amax_link /
 *                     gx_conv_input_amax / gx_wgq_operand_amax are not needed and are ignored when present); sums of many such
 *                     products are accumulated in fp32.  The small-level tap convs and gx_wstrip are NOT switched by this level:
 *                     gx_tapconv_precision below is their own opt-in.  Layers on the fp32 pipe in every mode stay there: gx_igemm,
 *                     the broadcast convs, dense layers, the LSTM.
 *        -1         -- every family back to its environment default.
 *      Returns the level in force BEFORE the call, or GX_MATMUL_MIXED when the three families' modes are not one level (set one by
 *      one, or by the per-family environment variables); negative: error.  gx_matmul_precision_get() returns the current level
 *      the same way.  Environment: GENESIS_MATMUL_PRECISION=highest|high|medium, when set, decides all three families' defaults
 *      ahead of the per-family variables (GENESIS_KQ_BF16X6 / GENESIS_KQ_F16X3 and their WGQ / WINO likes); unset, nothing changes.  Packed operands are laid out per mode:
 *      switch between iterations, not inside one.  Several ranks: every rank must set the same level (not checked). */
#define GX_MATMUL_MIXED 3
int gx_matmul_precision(int level);
int gx_matmul_precision_get(void);
/*      The arithmetic of the tap-conv kernels (gx_conv.hip: tapconv_kernel in every mode and tapconv_dt_kernel -- the layers of
 *      gx_conv3x3_fwd / _bias_act_fwd / _dgrad, gx_deconv5x5s2_fwd / _gn_stats_fwd / _dgrad and gx_conv5x5s1 that the 16-bit-pipe
 *      families do not take) and of the strip weight gradient (gx_wstrip.hip: gx_conv3x3_wgrad_quad / _bias on grids that are no
 *      power of two), a switch of its own beside gx_matmul_precision:
 *        0  -- the default: the tap-conv kernels multiply on the fp32 pipe (v_mfma_f32_32x32x2_f32), the strips from six bf16 piece
 *              products (fp32 accuracy);
 *        3  -- medium: every operand rounded ONCE to bf16 (round to nearest even) -- the packed weights one bf16 plane (the
 *              tap-conv one-bf16 pack form), the input halo tile converted on its way into LDS, one v_mfma_f32_32x32x16_bf16 per k-step (two taps x 8
 *              channels), fp32 accumulation; the strips split every window row and dy value into one piece and issue one MFMA per
 *              tap.  About 2^-8 relative error per product, fp32's exponent range.  Split-K partials, their reduce launches and the
 *              strips' two fixed-order reduce launches are unchanged: results stay bit-reproducible.  The input is staged through
 *              registers in this mode (LDS-DMA cannot convert).  A transposed conv's data gradient whose halo tile the bf16 stage
 *              cannot hold (1-pixel grids) runs mode 0, and gx_tapconv_last_mode() says so.
 *        -1 -- back to the environment's default (GENESIS_TAPCONV_PRECISION=default|medium; unset: 0).
 *      Returns the mode in force BEFORE the call; negative: error.  Independent of gx_matmul_precision: neither reads nor writes
 *      the other.  Out of scope (unchanged in every mode): wgrad_fast_kernel, conv3x3s2_wgrad_small_kernel, gx_igemm, the dense /
 *      LSTM kernels and the broadcast convs.  Packed weights are laid out per mode (a weight cache recorded in one mode never
 *      serves the other): switch between iterations, not inside one.
 *      gx_tapconv_last_mode(): the mode (0 or 3) of this thread's most recent tap-conv or strip launch, -1 if there was none. */
int gx_tapconv_precision(int mode);
int gx_tapconv_precision_get(void);
int gx_tapconv_last_mode(void);
/*      gx_conv_last_plan(out, n): the tile plan of this thread's most recent forward / data-gradient conv launch (the tap-conv
 *      kernels, the input-layer kernel of gx_conv3x3_fwd, every gx_kq.hip conv kernel, Winograd, the generic strided conv and the
 *      stride-2 vector-ALU kernels of gx_igemm.hip), written by the launcher on the
 *      host just before it launches, every field copied from the values the launch itself uses.  Fills out[0 .. min(n,
 *      GX_PLAN_FIELDS)) in the order of the GX_PLAN_* indices below and returns GX_PLAN_FIELDS; before any such launch the family
 *      is GX_PLAN_NONE and every other field 0.  A field the family does not have is 0.  Helper launches (weight packing, amax
 *      passes, split-K reduces) leave the record alone.  For tests and diagnosis: no synchronisation, no device work. */
#define GX_PLAN_FIELDS 18
/*      out[] indices */
#define GX_PLAN_FAMILY 0          /* GX_PLAN_NONE ... GX_PLAN_S2_DG */
#define GX_PLAN_FORM 1            /* operands: 0 fp32, 1 bf16 x 6, 2 fp16 x 3, 3 bf16 x 1 */
#define GX_PLAN_LTH 2             /* log2 of the tile's height, width and images per tile */
#define GX_PLAN_LTW 3
#define GX_PLAN_LG 4
#define GX_PLAN_NQ 5              /* gx_kq.hip: staging rounds nq (3 / 4); tap conv: the template's NPOS */
#define GX_PLAN_PIXELS 6          /* pixels per tile */
#define GX_PLAN_RT_TH 7           /* whole-row tiles (kq C3H), else 0 */
#define GX_PLAN_RT_TW 8
#define GX_PLAN_TILES_H 9
#define GX_PLAN_TILES_W 10
#define GX_PLAN_GRID_X 11
#define GX_PLAN_GRID_Y 12
#define GX_PLAN_GRID_Z 13
#define GX_PLAN_NSPLIT 14         /* split-K slabs (1: none) and 8- / 16-channel chunks per slab */
#define GX_PLAN_CHUNKS 15
#define GX_PLAN_NFULL 16          /* gx_kq.hip: whole-tile workgroups (q_split_tail) / tiles of the persistent loop */
#define GX_PLAN_STATS 17          /* 1: the GroupNorm statistics epilogue ran */
/*      families */
#define GX_PLAN_NONE 0
#define GX_PLAN_TAP_C3 1          /* tapconv_kernel<M_C3> */
#define GX_PLAN_TAP_DT 2          /* tapconv_dt_kernel (both row parities of the transposed conv) */
#define GX_PLAN_TAP_DG 3          /* tapconv_kernel<M_DG> */
#define GX_PLAN_TAP_C5 4          /* tapconv_kernel<M_C5> */
#define GX_PLAN_KQ_C3 5           /* kq_kernel<Q_C3> */
#define GX_PLAN_KQ_DT 6           /* kq_dt_kernel */
#define GX_PLAN_KQ_DG 7           /* kq_kernel<Q_DG> */
#define GX_PLAN_KQ_C3H 8          /* kq_c3h_kernel */
#define GX_PLAN_KQ_DTH 9          /* kq_dth_kernel */
#define GX_PLAN_KQ_DGH 10         /* kq_dgh_kernel */
#define GX_PLAN_KQ_C5H 11         /* kq_c5h_kernel */
#define GX_PLAN_WINO 12           /* wino_conv_kernel / wino_conv_h_kernel */
#define GX_PLAN_SMALLCIN 13       /* conv3x3_smallcin_fwd_kernel */
/*      gx_igemm.hip (form fp32): the implicit-GEMM families record pixels = 128 (the tile's columns), the grid, nsplit (1: the single-
 *      launch form) and the 16-wide contraction chunks per slab; the stride-2 vector-ALU kernels pixels = 256 (threads) and
 *      grid_x / grid_y, the data gradient also lG = log2 CIB (input channels per thread) and nq = UB (dy channels loaded ahead).  The
 *      weight gradients and the reduce launches note nothing. */
#define GX_PLAN_IGEMM_FWD 14      /* igemm_kernel<0>: gx_conv2d_direct_fwd / _fwd_ws */
#define GX_PLAN_IGEMM_DG 15       /* igemm_kernel<1>: gx_conv2d_direct_dgrad */
#define GX_PLAN_S2_FWD 16         /* conv3x3s2_fwd_small_kernel */
#define GX_PLAN_S2_DG 17          /* conv3x3s2_dgrad_small_kernel */
int gx_conv_last_plan(int* out, int n);
/*      Mode 2's per-tensor maximum without a second pass over the tensor: gx_kq_amax_link(parts, capacity, numel) arms a one-shot,
 *      per-thread hand-over -- the next producer that supports it (the register-resident GroupNorm + ReLU kernels behind gx_gn_relu_fwd_parts /
 *      gx_gn_relu_bwd_parts and the decoder head's backward behind gx_gn_relu_bwd_proj: models/genesisv2_config.py:90-99) writes one partial maximum of the gradient it stores
 *      per workgroup into `parts` (<= capacity floats) -- only a launch that covers all `numel` elements of the tensor: a chunked
 *      producer leaves the link alone -- and remembers that tensor's address; the next mode-2 conv call whose input IS
 *      that address and size (gx_deconv5x5s2_fwd* / gx_deconv5x5s2_dgrad / gx_conv5x5s1) reduces those partials instead of launching its own
 *      pass (more than 1024 of them: one small launch folds them first).  Producers: the GroupNorm + ReLU kernels (every form since
 *      round 6, the chunked decoder-head backward's apply kernel included) and the gated units' apply kernels (gx_gated_norm_fwd: out;
 *      gx_gated_norm_bwd: dy).  Any mode-2 conv call clears
 *      the link; results are bit-identical with and without it.  gx_kq_amax_link_hits(): hand-overs taken so far (this thread). */
int gx_kq_amax_link(float* parts, int capacity, size_t numel);
int gx_kq_amax_link_hits(void);
/*      The same partial maxima for a LATER reader (the weight gradients' stream-K launch at the end of the backward pass,
 *      gx_wgq_operand_amax below): gx_amax_tap(parts, capacity, numel) arms a one-shot, per-thread request -- the next producer launch
 *      that supports it (the GroupNorm + ReLU kernels, forward and backward; the gated units' apply kernels; the BroadcastDecoder
 *      chain's producers -- gx_bcast_conv3x3_fwd, the <= 32-output-channel conv3x3 of gx_conv3x3_bias_act_fwd / gx_conv3x3_dgrad_act /
 *      gx_conv3x3_dgrad in mode 2 of gx_kq_precision, gx_conv1x1_bwd_act's data gradient) writes one partial maximum of the
 *      values it stores per workgroup into parts[0 .. n) -- provided it stores exactly `numel` values: a chunked producer does not
 *      serve -- whatever its destination views are (the channel slice of a concat
 *      buffer and a resampled second copy hold the same values); gx_amax_tap_result() returns n (0: that launch could not
 *      serve, the request is void) and disarms.  The caller keeps `parts` alive until its reader has RUN.
 *      gx_amax_parts(x, n, parts, stream): the partial maxima of any tensor by a pass of its own -- 256 floats. */
int gx_amax_tap(float* parts, int capacity, size_t numel);
/*      The consumer side for the Winograd conv3x3 layers (gx_wino.hip; modules/blocks.py:159-165 forward and data gradient):
 *      gx_conv_input_amax(p0, n0, p1, n1) is the one-shot, per-thread hint that the INPUT tensor of the next gx_conv3x3_fwd* /
 *      gx_conv3x3_dgrad* / gx_conv3x3_pair_* / gx_conv3x3_wino call has its partial maxima in p0[0 .. n0) (+ p1[0 .. n1): a
 *      concat buffer written by two producers, or the pair data gradient's second tensor).  With it -- and gx_wino_precision(2),
 *      the default; GENESIS_WINO_F16X3=0: mode 1 -- a layer that takes the Winograd kernel forms every fp32 product from THREE
 *      fp16 piece products (U * 2^eU packed as two pieces, eU from max |w|; V * 2^eV split in registers, eV from 4 max |x|)
 *      instead of six bf16 ones -- up to 1536 partial maxima (every workgroup of that kernel reduces them itself; more: six bf16
 *      pieces).  A layer with <= 32 output channels (gx_kq.hip, mode 2 of gx_kq_precision) reads its input's scale from the same
 *      hint instead of making its own amax pass, any count.  Layers on other kernels ignore it.  NULL / 0 clears.  Same range note
 *      as gx_wgq_operand_amax. */
int gx_conv_input_amax(const float* p0, int n0, const float* p1, int n1);
/*      Measurement: the share of the bf16-pipe Winograd launches' algorithmic flops (since the process started) on fp16 pieces. */
double gx_wino_f16_share(void);
int gx_amax_tap_result(void);
int gx_amax_parts(const float* x, size_t n, float* parts, gx_stream_t stream);
size_t gx_conv3x3_wino_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv3x3_wino(const float* x, const float* w, float* y, int N, int Cin, int Cout, int H, int W, int mode,
                    void* ws, size_t ws_bytes, gx_stream_t stream);
/*      Two conv3x3 layers on ONE input as one layer (seg_head and feat_head[0] on the encoder features,
 *      models/genesisv2_config.py:70-73, :110-149): forward = one launch that writes y1 [N,Co1,H,W] = conv3x3(x, w1)
 *      and y2 [N,Co2,H,W] = conv3x3(x, w2); data gradient = one launch dx = dgrad(dy1, w1) + dgrad(dy2, w2) (the sum of
 *      the two consumers' input gradients forms in the accumulators: no second dgrad, no accumulation pass).
 *      Winograd kernel only: gx_conv3x3_pair_supported (Co1 % 64 == 0, gx_conv3x3_wino's shape rules).
 *      ws keeps the packed weights of both directions; dgrad with pack = 0 reuses what the forward of the same
 *      iteration packed. */
int gx_conv3x3_pair_supported(int N, int Cin, int Co1, int Co2, int H, int W);
size_t gx_conv3x3_pair_ws_bytes(int N, int Cin, int Co1, int Co2, int H, int W);
int gx_conv3x3_pair_fwd(const float* x, const float* w1, const float* w2, float* y1, float* y2, int N, int Cin, int Co1,
                        int Co2, int H, int W, void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_conv3x3_pair_dgrad(const float* dy1, const float* dy2, const float* w1, const float* w2, float* dx, int N, int Cin,
                          int Co1, int Co2, int H, int W, int pack, void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- ConvTranspose2d(k=5, s=2, p=2, output_padding=1) + bias:
 *      models/genesisv2_config.py:90-98 (decoder_module.{1,4,7,10}).
 *      w is the nn.ConvTranspose2d weight [Cin,Cout,5,5]; x [N,Cin,Hin,Win]; y [N,Cout,2Hin,2Win].
 *      dgrad writes only the first Cin_out channels of dx ([N,Cin_out,Hin,Win]). */
size_t gx_deconv5x5s2_ws_bytes(int N, int Cin, int Cout, int Hin, int Win);
int gx_deconv5x5s2_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout,
                       int Hin, int Win, void* ws, size_t ws_bytes, gx_stream_t stream);
/*      Forward + the GroupNorm statistics of its output (mean, rstd [N*groups], as gx_gn_relu_fwd with dst0 == NULL
 *      would compute them) without a pass over y: the conv epilogue sums every 8-channel block per workgroup, a tiny
 *      kernel finishes in fp64.  *fused = 0 (shape not eligible: channel split, several images per tile, groups not
 *      multiples of 8 channels): y is written, mean / rstd are NOT -- run gx_gn_relu_fwd(dst0 = NULL). */
size_t gx_deconv5x5s2_gn_stats_ws_bytes(int N, int Cin, int Cout, int Hin, int Win);
int gx_deconv5x5s2_gn_stats_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Cout,
                                int Hin, int Win, int groups, float eps, float* mean, float* rstd, int* fused,
                                void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_deconv5x5s2_dgrad(const float* dy, const float* w, float* dx, int N, int Cin, int Cin_out, int Cout,
                         int Hin, int Win, void* ws, size_t ws_bytes, gx_stream_t stream);
size_t gx_deconv5x5s2_wgrad_ws_bytes(int N, int Cin, int Cout, int Hin, int Win);
int gx_deconv5x5s2_wgrad(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int Hin, int Win,
                         void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- GroupNorm(groups, eps, affine) + ReLU: modules/blocks.py:159-165, models/genesisv2_config.py:91-98;
 *      fused with the UNet's nearest resampling + torch.cat placement (modules/unet.py:78,86,89).
 *      A "view" (ptr, ctot, c0, mode) names channels [c0, c0+C) of a buffer [N, ctot, Hd, Wd]:
 *      mode 0 same size, 1 buffer is 2x up-sampled (nearest), 2 buffer is 2x down-sampled ([::2, ::2]).
 *      fwd writes relu(gn(y)) to dst0 (and dst1 if non-NULL), and mean/rstd [N*groups].
 *      bwd reads d(out) from g0 (+ g1 if non-NULL), writes dy [N,C,H,W], dgamma/dbeta [C] and, if
 *      dbias != NULL, sum_{n,hw} dy (the gradient of a per-channel bias added before the norm).
 *      fwd with dst0 == NULL computes the statistics only: the consumer (gx_conv1x1_gn_fwd) normalises on load.
 *      gx_gn_relu_bwd_proj is the matching backward: d(out) is not read from memory but formed on load as the data
 *      gradient of the following 1x1 conv, gate * sum_o w[o][c] g_out[n][o][h][w] (g_out [N,Cout,H,W], w [Cout,C],
 *      Cout <= 8, gate an optional device scalar):
 *      the [N,C,H,W] activation and its gradient never exist in memory (genesisv2_config.py:97-98, last decoder stage). */
int gx_gn_relu_fwd(const float* y, const float* gamma, const float* beta, int N, int C, int H, int W, int groups,
                   float eps, float* dst0, int dst0_ctot, int dst0_c0, int dst0_mode, float* dst1, int dst1_ctot,
                   int dst1_c0, int dst1_mode, float* mean, float* rstd, gx_stream_t stream);
size_t gx_gn_relu_bwd_ws_bytes(int N, int C);
int gx_gn_relu_bwd(const float* y, const float* gamma, const float* beta, const float* mean, const float* rstd,
                   int N, int C, int H, int W, int groups, const float* g0, int g0_ctot, int g0_c0, int g0_mode,
                   const float* g1, int g1_ctot, int g1_c0, int g1_mode, float* dy, float* dgamma, float* dbeta,
                   float* dbias, void* ws, size_t ws_bytes, gx_stream_t stream);
/*      ..._parts: a gradient source (modes 0-2) may still be the `nsplit` split-K partial slabs of the data gradient that
 *      produced it (gx_conv3x3_dgrad_parts), `split_stride` floats apart: summed on load in slab order -- the stand-alone
 *      reduce launch of the <= 16 x 16 layers is skipped. */
int gx_gn_relu_bwd_parts(const float* y, const float* gamma, const float* beta, const float* mean, const float* rstd,
                         int N, int C, int H, int W, int groups, const float* g0, int g0_ctot, int g0_c0, int g0_mode,
                         int g0_nsplit, size_t g0_split_stride, const float* g1, int g1_ctot, int g1_c0, int g1_mode,
                         int g1_nsplit, size_t g1_split_stride, float* dy, float* dgamma, float* dbeta, float* dbias, void* ws,
                         size_t ws_bytes, gx_stream_t stream);
int gx_gn_relu_bwd_proj(const float* y, const float* gamma, const float* beta, const float* mean, const float* rstd,
                        int N, int C, int H, int W, int groups, const float* g_out, int Cout, const float* w,
                        const float* gate, float* dy, float* dgamma, float* dbeta, float* dbias, float* wpart,
                        float* bpart, void* ws, size_t ws_bytes, gx_stream_t stream);
/*      wpart [N,Cout,C] / bpart [N,Cout] (both or neither; allowed when gx_gn_relu_bwd_proj_fuses_wgrad(...) != 0): the
 *      kernel also emits the per-image partials of the 1x1 conv's weight / bias gradient (its input exists only inside
 *      this kernel); gx_conv1x1_gn_wgrad_finish sums them over the images -- no separate weight-gradient pass over y. */
int gx_gn_relu_bwd_proj_fuses_wgrad(int C, int H, int W, int groups, int Cout);
/*      Test diagnostic: the number of elements of relu(gn(y)) that are > 0, evaluated with the expression the kernels above use
 *      for their ReLU decision ((y - mean) * rstd * gamma + beta > 0) -- the count the reference's nn.ReLU modules
 *      (modules/blocks.py:164, models/genesisv2_config.py:92-98) would report for (out > 0).sum().  *count: device uint64. */
int gx_gn_relu_active_count(const float* y, const float* gamma, const float* beta, const float* mean, const float* rstd, int N,
                            int C, int H, int W, int groups, unsigned long long* count, gx_stream_t stream);
/*      workspace of gx_gn_relu_bwd_proj (>= gx_gn_relu_bwd_ws_bytes): slabs too large for one workgroup (128 x 128 images) are
 *      processed in 4096-pixel chunks -- chunk sums, per-slab constants, chunked apply -- whose records live here */
size_t gx_gn_relu_bwd_proj_ws_bytes(int N, int C, int H, int W, int groups, int Cout);
/*      gx_gn_last_plan(out, n): the kernel and launch geometry of this thread's most recent gx_gn_relu_fwd* / gx_gn_relu_bwd* launch,
 *      written by the launcher on the host just before it launches, every field copied from the values the launch itself uses.
 *      Fills out[0 .. min(n, GX_GN_PLAN_FIELDS)) in the order of the GX_GN_PLAN_* indices below and returns GX_GN_PLAN_FIELDS;
 *      before any such launch the kernel is GX_GN_NONE and every other field 0.  A field the kernel does not have is 0.  The
 *      parameter-gradient reduce that ends a backward call leaves the record alone, and so does a call that is refused.  For
 *      tests and diagnosis: no synchronisation, no device work. */
#define GX_GN_PLAN_FIELDS 15
/*      out[] indices */
#define GX_GN_PLAN_KERNEL 0       /* GX_GN_NONE ... GX_GN_BWD_SPLIT */
#define GX_GN_PLAN_VEC 1          /* 1: 16-byte accesses along W; 0: the scalar two-pass kernels (W == 2) */
#define GX_GN_PLAN_F 2            /* register kernels: float4 per lane and unit, units per wave, parts per channel */
#define GX_GN_PLAN_UPW 3
#define GX_GN_PLAN_P 4
#define GX_GN_PLAN_THREADS 5      /* workgroup size */
#define GX_GN_PLAN_GRID 6         /* workgroups (the chunked path: of its sums and apply launches) */
#define GX_GN_PLAN_LDS 7          /* dynamic LDS bytes (the staged output gradient of the following 1x1 conv) */
#define GX_GN_PLAN_CT 8           /* the template's 1x1-conv output channels: 4 (stage kernel), 4 / 8 (chunked path) */
#define GX_GN_PLAN_KEEP 9         /* stage kernel: y stays in registers between the passes */
#define GX_GN_PLAN_WP 10          /* the launch also writes wpart / bpart */
#define GX_GN_PLAN_CHUNKS 11      /* chunked path: 4096-pixel chunks per slab */
#define GX_GN_PLAN_NSPLIT0 12     /* backward: split-K slabs of gradient source 0 and source 1 (0: no such source, or mode 3) */
#define GX_GN_PLAN_NSPLIT1 13
#define GX_GN_PLAN_NSPLIT_IN 14   /* forward: split-K slabs of the input */
/*      kernels */
#define GX_GN_NONE 0
#define GX_GN_FWD_REG 1           /* gn_relu_fwd_reg_kernel<F, UPW> */
#define GX_GN_FWD_SMALL 2         /* gn_relu_fwd_small_kernel */
#define GX_GN_FWD_TWOPASS 3       /* gn_relu_fwd_kernel<VEC> */
#define GX_GN_BWD_REG 4           /* gn_relu_bwd_reg_kernel<F, UPW, false> */
#define GX_GN_BWD_REG_STAGED 5    /* gn_relu_bwd_reg_kernel<F, UPW, true> */
#define GX_GN_BWD_STAGE 6         /* gn_relu_bwd_stage_kernel<F, 4, WP, KEEP> */
#define GX_GN_BWD_SMALL 7         /* gn_relu_bwd_small_kernel */
#define GX_GN_BWD_TWOPASS 8       /* gn_relu_bwd_kernel<VEC> */
#define GX_GN_BWD_SPLIT 9         /* gn_bwd_proj_split_sums_kernel<CT> / _combine_kernel / _apply_kernel<CT> */
int gx_gn_last_plan(int* out, int n);
/*      gx_gn_fwd_plan / gx_gn_bwd_plan: the same record, as the launch with these arguments WOULD note it -- the host dispatch asked
 *      directly, no launch, no GPU, the calling thread's gx_gn_last_plan record untouched.  nsplit_in / g0_nsplit / g1_nsplit are the
 *      slab counts the entry point would be given (gx_gn_relu_fwd: 1; gx_gn_relu_bwd: 1 per source; g1_nsplit 0: no second source).
 *      g0_mode 3, g0_ctot = Cout, g0_nsplit 0: gx_gn_relu_bwd_proj, want_wpart != 0 with wpart / bpart, ws_bytes its workspace.
 *      Kernel GX_GN_NONE, every field 0: the entry point refuses these arguments (N / C / groups / H / W, a workspace below
 *      gx_gn_relu_bwd_ws_bytes, wpart / bpart on a shape that cannot fuse them).  Same out / n / result as gx_gn_last_plan. */
int gx_gn_fwd_plan(int N, int C, int H, int W, int groups, int nsplit_in, int* out, int n);
int gx_gn_bwd_plan(int N, int C, int H, int W, int groups, int g0_mode, int g0_ctot, int g0_nsplit, int g1_nsplit, int want_wpart,
                   size_t ws_bytes, int* out, int n);

/* ---- Instance-Colouring stick-breaking attention: modules/attention.py:162-226.
 *      colour [B,C<=8,H,W]; log_sigma: device pointer to the fp64 0-dim parameter; rand_pixel [B,1,H,W];
 *      seed_idx_in: NULL (argmax of rand*scope, first max) or [K-1,B] int64 seeds to force.
 *      kernel_type 0 gaussian, 1 laplacian, 2 epanechnikov.
 *      Outputs: log_m [K,B,1,H,W], log_s [K,B,1,H,W], seeds [K-1,B,C], seed_idx_out [K-1,B] int64.
 *      bwd: g_log_m [K,B,1,H,W] -> dcolour [B,C,H,W] (fully written), dlog_sigma (fp64 scalar). */
int gx_icsbp_fwd(const float* colour, const double* log_sigma, const float* rand_pixel, const int64_t* seed_idx_in,
                 int B, int C, int H, int W, int K, int kernel_type, float* log_m, float* log_s, float* seeds,
                 int64_t* seed_idx_out, gx_stream_t stream);
size_t gx_icsbp_bwd_ws_bytes(int B, int H, int W, int K);
int gx_icsbp_bwd(const float* colour, const double* log_sigma, const float* seeds, const int64_t* seed_idx,
                 const float* g_log_m, int B, int C, int H, int W, int K, int kernel_type, float* dcolour,
                 double* dlog_sigma, void* ws, size_t ws_bytes, gx_stream_t stream);
/*      dynamic_K (modules/attention.py:218-219, models/genesisv2_config.py:118-137): an image stops at the first step
 *      whose mask mass sum_p exp(log_m) falls below min_mass (the reference: 20); nsteps[b] = steps it ran; its mask
 *      nsteps[b] is the remaining scope, later masks are -1e10 (the reference's padding), later seeds 0.  The backward
 *      takes nsteps and treats the masks accordingly. */
int gx_icsbp_fwd_dyn(const float* colour, const double* log_sigma, const float* rand_pixel, const int64_t* seed_idx_in,
                     int B, int C, int H, int W, int K, int kernel_type, float min_mass, float* log_m, float* log_s,
                     float* seeds, int64_t* seed_idx_out, int* nsteps, gx_stream_t stream);
int gx_icsbp_bwd_dyn(const float* colour, const double* log_sigma, const float* seeds, const int64_t* seed_idx,
                     const float* g_log_m, const int* nsteps, int B, int C, int H, int W, int K, int kernel_type,
                     float* dcolour, double* dlog_sigma, void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- masked slot pooling: models/genesisv2_config.py:146-152.
 *      S[b,k,c] = sum_hw exp(log_m[k,b]) * f[b,c];  msum[b,k] = sum_hw exp(log_m[k,b]).
 *      (feat_head's 1x1 conv commutes with the pooling and is applied to S by the caller.) */
int gx_maskpool_fwd(const float* f, const float* log_m, int B, int C, int H, int W, int K, float* S, float* msum,
                    gx_stream_t stream);
int gx_maskpool_bwd(const float* f, const float* log_m, const float* gS, const float* gmsum, int B, int C, int H,
                    int W, int K, float* df, float* dlog_m, gx_stream_t stream);

/* ---- mixture likelihood + reconstruction: models/genesisv2_config.py:212-223,
 *      models/monet_config.py:137-139, models/genesis_config.py:273-286.
 *      dec [K*B,4,H,W] (slot-major rows k*B+b; ch 0-2 RGB pre-activation, ch 3 mask logit), x [B,3,H,W].
 *      Outputs recon [B,3,H,W], x_r [K,B,3,H,W], log_m_r [K,B,1,H,W], err [B].
 *      bwd: g_err [B] -> ddec [K*B,4,H,W]. */
size_t gx_mixture_ws_bytes(int B, int H, int W);
int gx_mixture_fwd(const float* x, const float* dec, int B, int H, int W, int K, float pixel_std, int pixel_bound,
                   float* recon, float* x_r, float* log_m_r, float* err, void* ws, size_t ws_bytes,
                   gx_stream_t stream);
int gx_mixture_bwd(const float* x, const float* dec, const float* g_err, int B, int H, int W, int K,
                   float pixel_std, int pixel_bound, float* ddec, gx_stream_t stream);

/* ---- 1x1 convolution with Cout <= 8: y = gate * (W x + b) + addend.
 *      modules/blocks.py:175-178 (SemiConv: gate = ScalarGate parameter on device, addend = uv [Cout,H,W]),
 *      models/genesisv2_config.py:99 (decoder_module.13; gate = addend = NULL).
 *      bwd writes dx, dw [Cout,Cin], db [Cout] (if non-NULL) and dgate (iff gate given). */
int gx_conv1x1_fwd(const float* x, const float* w, const float* bias, const float* gate, const float* addend,
                   int N, int Cin, int Cout, int H, int W, float* y, gx_stream_t stream);
size_t gx_conv1x1_bwd_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv1x1_bwd(const float* x, const float* dy, const float* w, const float* bias, const float* gate, int N,
                   int Cin, int Cout, int H, int W, float* dx, float* dw, float* db, float* dgate, void* ws,
                   size_t ws_bytes, gx_stream_t stream);
/*      ..._ex with accumulate = 1: dw / db are ADDED to what the destinations hold (the MONet UNet's final_conv is used K-1
 *      times per iteration); plain conv only (gate == NULL). */
int gx_conv1x1_bwd_ex(const float* x, const float* dy, const float* w, const float* bias, const float* gate, int N,
                      int Cin, int Cout, int H, int W, float* dx, float* dw, float* db, float* dgate, int accumulate,
                      void* ws, size_t ws_bytes, gx_stream_t stream);
/*      ..._act: the conv's input x is the output of a bias + activation layer (modules/decoders.py:25-32: ..., ReLU,
 *      Conv2d(1x1)): dxa = dx * act'(x) (act 1 ReLU, 2 ELU) in the data-gradient kernel and dbx [Cin] (NULL to skip) = sum_{n,hw} dxa, that
 *      layer's bias gradient -- gx_conv1x1_bwd followed by gx_bias_act_bwd without the latter's pass. */
size_t gx_conv1x1_bwd_act_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv1x1_bwd_act(const float* x, const float* dy, const float* w, const float* bias, int N, int Cin, int Cout, int H,
                       int W, int act, float* dxa, float* dw, float* db, float* dbx, void* ws, size_t ws_bytes,
                       gx_stream_t stream);
/*      The same 1x1 conv reading the PRE-norm tensor y of the GroupNorm+ReLU layer in front of it (statistics from
 *      gx_gn_relu_fwd with dst0 == NULL): relu(gn(y)) is formed on load, forward and in the weight gradient; the data
 *      gradient is folded into gx_gn_relu_bwd_proj.  Cin <= 64 (wgrad), H*W % 256 == 0. */
int gx_conv1x1_gn_fwd(const float* y_pre, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, int groups, const float* w, const float* bias, const float* gate,
                      const float* addend, int N, int Cin, int Cout, int H, int W, float* out, gx_stream_t stream);
size_t gx_conv1x1_gn_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv1x1_gn_wgrad(const float* y_pre, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int groups, const float* g_out, const float* w, const float* bias,
                        const float* gate, int N, int Cin, int Cout, int H, int W, float* dw, float* db,
                        float* dgate, void* ws, size_t ws_bytes, gx_stream_t stream);
size_t gx_conv1x1_gn_wgrad_finish_ws_bytes(int Cin, int Cout);
int gx_conv1x1_gn_wgrad_finish(const float* wpart, const float* bpart, int N, int Cin, int Cout, const float* w,
                               const float* bias, const float* gate, float* dw, float* db, float* dgate, void* ws,
                               size_t ws_bytes, gx_stream_t stream);

/* ---- optimiser side of the training step.
 *      gx_adam_step: torch.optim.Adam update (train.py:174-175,263) on flat buffers p/g/m/v of n elements
 *      (fp32, or fp64 when is_f64 -- att_process.log_sigma is an fp64 parameter); `step` is a device int64
 *      holding t (>= 1, bump it with gx_step_increment first); the gradient is multiplied by grad_scale.
 *      gx_geco_update: utils/geco.py:39-49 on device; state = {beta, err_ema, initialised}; err = device
 *      scalar with the batch-mean reconstruction error; no host sync (the reference calls .item()). */
int gx_adam_step(void* p, const void* g, void* m, void* v, size_t n, int is_f64, int64_t* step, double lr,
                 double beta1, double beta2, double eps, float grad_scale, gx_stream_t stream);
int gx_step_increment(int64_t* step, gx_stream_t stream);
/*      the step's noise (torch.rand for the IC-SBP's rand_pixel, modules/attention.py:177-178; torch.randn for the latents'
 *      rsample, models/genesisv2_config.py:157) in one launch: Philox4x32-10 keyed by (seed, *step, position), nu uniform [0, 1)
 *      numbers into u and nz standard normals into z; a replayed HIP graph draws fresh numbers every step. */
int gx_philox_noise(float* u, long long nu, float* z, long long nz, unsigned long long seed, const int64_t* step,
                    gx_stream_t stream);
int gx_geco_update(float* state, const float* err, float goal, float step_size, float alpha, float speedup,
                   int use_speedup, float beta_min, float beta_max, gx_stream_t stream);
/*      The tail of a training step in two launches: gx_geco_update_step = gx_geco_update + gx_step_increment;
 *      gx_adam_step_pair = gx_adam_step on the fp32 group and on the fp64 group (n64 may be 0) and, with
 *      zero_grads != 0, zeroes the gradients as it consumes them (the next iteration's backward accumulates into a
 *      clean bucket without a separate fill launch). */
int gx_geco_update_step(float* state, const float* err, float goal, float step_size, float alpha, float speedup,
                        int use_speedup, float beta_min, float beta_max, int64_t* step, gx_stream_t stream);
int gx_adam_step_pair(float* p32, float* g32, float* m32, float* v32, size_t n32, double* p64, double* g64,
                      double* m64, double* v64, size_t n64, int64_t* step, double lr, double beta1, double beta2,
                      double eps, float grad_scale, int zero_grads, gx_stream_t stream);

/*      The other branches of train.py's objective / optimiser set-up.
 *      gx_optimiser_step_pair: kind 1 = torch.optim.RMSprop(params, lr) (alpha = hp = 0.99, eps 1e-8, no momentum;
 *      train.py:171-172), kind 2 = torch.optim.SGD(params, lr, momentum = hp = 0.9) (:175-176); one state buffer m per group
 *      (square average / momentum buffer, zero before the first step); fp32 + fp64 groups in one launch like
 *      gx_adam_step_pair.
 *      gx_beta_warmup: *out = clamp(beta * (*step) / warm_iters, 0, beta) -- the fixed-beta objective's linear warm-up over
 *      warm_iters = 0.2 * train_iter iterations (train.py:252-258); *step = the iteration index (the optimiser's step counter
 *      before this iteration's increment).
 *      gx_mse_rmse: out[0] = mean_b mean_{chw} (x - recon)^2, out[1] = mean_b sqrt(mean_{chw} (x - recon)^2)
 *      (train.py:244-246; x, recon [B, n]); ws: gx_mse_rmse_ws_bytes(B), its first 16 bytes zero before the first launch. */
int gx_optimiser_step_pair(int kind, float* p32, float* g32, float* m32, size_t n32, double* p64, double* g64, double* m64,
                           size_t n64, int64_t* step, double lr, double hp, double eps, float grad_scale, int zero_grads,
                           gx_stream_t stream);
int gx_beta_warmup(const int64_t* step, float beta, float warm_iters, float* out, gx_stream_t stream);
size_t gx_mse_rmse_ws_bytes(int B);
int gx_mse_rmse(const float* x, const float* recon, int B, int n, float* out, void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- gradient guard: clip by global norm and skip non-finite steps without a host read (genesis_amd/grad_guard.py,
 *      TrainStep(max_grad_norm=, skip_nonfinite=)).  gx_grad_guard: ONE call reduces n_segments gradient segments -- each a
 *      contiguous device array with its own length, fp32 or fp64 -- to a device record of GX_GUARD_RECORD_BYTES bytes.  The
 *      descriptor table follows gx_hist_multi's convention: GX_GUARD_DESC_WORDS int64 words per segment, held twice with the same
 *      contents (table_host is validated before anything is launched, table_dev, 8-byte aligned, is what the kernels read):
 *        SRC    device address, aligned to its element (4 bytes for fp32, 8 for fp64: a slice of a flat buffer or a lone .grad is
 *               a legal segment; 16-byte loads from the first 16-byte boundary on, element loads before it and at the end)
 *        N      elements, 1 <= N < 2^31;  DTYPE  GX_GUARD_FP32 or GX_GUARD_FP64
 *        WORK   first chunk of the segment = sum over the segments before it of ceil(N / GX_GUARD_CHUNK)
 *      Arithmetic.  S = sum over all elements of (double)g * (double)g, in fp64 (each product fused into its sum), in a fixed
 *      order: a grid of min(total chunks, GX_GUARD_MAX_GRID) workgroups walks the chunks with that stride, four accumulators per
 *      thread -> wave -> workgroup -> one partial per workgroup in ws; a second one-workgroup launch adds the partials in order.
 *      No floating-point atomic: two calls on the same input write the same bits; ws needs no clearing.
 *        norm  = (float)((double)gscale * sqrt(S))              gscale: the factor the optimiser launch receives (1 / world)
 *        coef  = (float)min(1, max_norm / ((double)gscale * sqrt(S) + 1e-6)) with max_norm > 0 (torch.nn.utils.clip_grad_norm_;
 *                a NaN norm gives a NaN coef, as torch.clamp does), else 1
 *        scale = gscale * coef, ONE fp32 multiply
 *        ok    = 1 if force_ok, or if S and every one of the n_check device floats at `check` (0 <= n_check <=
 *                GX_GUARD_MAX_CHECK; the step's err and kl) are finite; else 0
 *      The record, 8-byte aligned (byte offsets GX_GUARD_R_*): S fp64 at 0, norm fp32 at 8, coef fp32 at 12, scale fp32 at 16,
 *      ok int32 at 20, skipped int64 at 24.  gx_grad_guard writes all but `skipped`, a cumulative counter that the caller zeroes
 *      once and the guarded launches below advance.
 *      ws: gx_grad_guard_ws_bytes(total chunks) bytes, 8-byte aligned.
 *      GX_EINVAL before any launch: a null pointer, n_segments < 1, N < 1 or >= 2^31, an unknown DTYPE, a SRC that is null or
 *      not aligned to its element, WORK that disagrees with the prefix, a table shorter than its descriptors, a misaligned
 *      table_dev / record / ws, n_check out of range, a workspace that is too small.
 *      gx_scale_multi_guarded: every element of the segments of such a table times the record's coef, in the element's own type
 *      (fp64: times (double)coef), in place; coef == 1 returns without reading or writing a gradient.
 *      The guarded tail: the entry points above with the record's device address in place of the host's grad_scale.  Record ok:
 *      bit for bit what the unguarded entry point does when its grad_scale is the record's `scale` (and what
 *      gx_geco_update_step / gx_step_increment do).  Not ok: parameters, every optimiser state buffer, the step counter and the
 *      GECO state keep their bits; the gradients are still zeroed with zero_grads != 0; gx_geco_update_step_guarded /
 *      gx_step_increment_guarded -- one of them per step -- adds 1 to `skipped`. */
#define GX_GUARD_FP32 0
#define GX_GUARD_FP64 1
#define GX_GUARD_D_SRC 0
#define GX_GUARD_D_N 1
#define GX_GUARD_D_DTYPE 2
#define GX_GUARD_D_WORK 3
#define GX_GUARD_DESC_WORDS 4
#define GX_GUARD_CHUNK 8192
#define GX_GUARD_MAX_GRID 1024
#define GX_GUARD_MAX_CHECK 8
#define GX_GUARD_R_S 0
#define GX_GUARD_R_NORM 8
#define GX_GUARD_R_COEF 12
#define GX_GUARD_R_SCALE 16
#define GX_GUARD_R_OK 20
#define GX_GUARD_R_SKIPPED 24
#define GX_GUARD_RECORD_BYTES 32
size_t gx_grad_guard_ws_bytes(long long total_chunks);
int gx_grad_guard(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                  const float* check, int n_check, float gscale, double max_norm, int force_ok, void* record, void* ws,
                  size_t ws_bytes, gx_stream_t stream);
int gx_scale_multi_guarded(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                           const void* record, gx_stream_t stream);
int gx_step_increment_guarded(int64_t* step, void* record, gx_stream_t stream);
int gx_geco_update_step_guarded(float* state, const float* err, float goal, float step_size, float alpha, float speedup,
                                int use_speedup, float beta_min, float beta_max, int64_t* step, void* record,
                                gx_stream_t stream);
int gx_adam_step_pair_guarded(float* p32, float* g32, float* m32, float* v32, size_t n32, double* p64, double* g64,
                              double* m64, double* v64, size_t n64, int64_t* step, double lr, double beta1, double beta2,
                              double eps, const void* record, int zero_grads, gx_stream_t stream);
int gx_optimiser_step_pair_guarded(int kind, float* p32, float* g32, float* m32, size_t n32, double* p64, double* g64,
                                   double* m64, size_t n64, int64_t* step, double lr, double hp, double eps, const void* record,
                                   int zero_grads, gx_stream_t stream);

/* ---- learning-rate schedules and averaged weights in the optimiser launch (genesis_amd/schedule.py, genesis_amd/ema.py,
 *      TrainStep(lr_schedule=, ema_decay=, ema_warmup=)).  gx_adam_step_pair_ex / gx_optimiser_step_pair_ex: the grid, the
 *      fp32 + fp64 split, zero_grads and the arithmetic on p, m, v of gx_adam_step_pair / gx_optimiser_step_pair, with the
 *      learning rate computed ON THE DEVICE from the step counter, so a captured HIP graph follows a schedule without being
 *      captured again.  The plain entry points are untouched: a caller that does not opt in keeps its launches and its bits.
 *      record: NULL = the unguarded form (the gradient times grad_scale); else the gradient guard's record: ok = the gradient
 *        times the record's `scale` (grad_scale is ignored); not ok = ONLY the gradients are zeroed (with zero_grads): p, m, v, the
 *        EMA and the tail record keep their bits.
 *      sched: GX_SCHED_WORDS fp64 words in HOST memory, read during the call (constants of the launch: fine inside a graph).
 *        With t = *step after the increment (>= 1), k = t - 1, base = word BASE, W = WARMUP (0: none), s0 = START in (0, 1]:
 *          k < W:   lr = base (s0 + (1 - s0) k / W)
 *          else, j = k - W, by KIND:
 *            GX_SCHED_CONSTANT     lr = base
 *            GX_SCHED_COSINE       lr = eta_min + (base - eta_min)(1 + cos(pi j / T)) / 2 for j < T, eta_min from j = T on.
 *                                  The rate is HELD there; torch's CosineAnnealingLR is periodic and climbs again.
 *            GX_SCHED_EXPONENTIAL  lr = base gamma^j
 *            GX_SCHED_STEP         lr = base gamma^(number of milestones <= j); at most GX_SCHED_MAX_MILESTONES, ascending
 *            GX_SCHED_DEVICE       lr = *lr_dev, an fp64 device scalar the host may write between steps; no warm-up factor
 *        -- the closed forms of torch's SequentialLR([LinearLR(s0, 1, W), X], [W]) at last_epoch = k, evaluated in fp64 in every
 *        workgroup (cos / pow: a few ulp of fp64).
 *      ema32 / ema64: NULL (both) = no average; else buffers laid out like p32 / p64, updated after p' is formed as
 *        d = p' - e; e' = e + w d, each operation rounded in the parameter's own type (no fma), w = (T)(1 - decay_t) with
 *        decay_t = ema_decay, or min(ema_decay, (1 + t) / (10 + t)) with ema_warmup != 0, formed in fp64.  The average is kept in
 *        the parameter's type (as torch.optim.swa_utils.AveragedModel and timm keep it).
 *      tail: two fp64 device words, 8-byte aligned, written by one thread of a step that is not skipped: the lr used at byte
 *        GX_TAIL_LR and decay_t (0 without an EMA) at byte GX_TAIL_DECAY.
 *      gx_ema_multi: the same e + w (p - e) for an unchanged loop (torch's own optimiser): one launch over a host + device table
 *        of n_segments x GX_EMA_DESC_WORDS int64 words (SRC: the parameter, DST: its average, N elements, DTYPE GX_EMA_FP32 /
 *        GX_EMA_FP64, WORK: first chunk = sum over the segments before it of ceil(N / GX_EMA_CHUNK)), a grid of at most
 *        GX_EMA_MAX_GRID workgroups; t is read from the device counter `step` (bump it with gx_step_increment first);
 *        decay_used: NULL, or an fp64 device word that receives decay_t.
 *      GX_EINVAL before any launch: a null group with n > 0 (a null ema64 with n64 > 0 when ema32 is given), a null step, a null
 *      or misaligned tail, ema_decay outside [0, 1), an unknown KIND, W < 0, T <= 0 (cosine), gamma <= 0 (exponential, step), more
 *      than GX_SCHED_MAX_MILESTONES milestones or unsorted ones, s0 outside (0, 1], GX_SCHED_DEVICE with a null lr_dev, a base
 *      rate that is not finite; for the table what gx_grad_guard refuses, for SRC and DST alike. */
#define GX_SCHED_CONSTANT 0
#define GX_SCHED_COSINE 1
#define GX_SCHED_EXPONENTIAL 2
#define GX_SCHED_STEP 3
#define GX_SCHED_DEVICE 4
#define GX_SCHED_KIND 0
#define GX_SCHED_BASE 1
#define GX_SCHED_WARMUP 2
#define GX_SCHED_START 3
#define GX_SCHED_T 4
#define GX_SCHED_ETA_MIN 5
#define GX_SCHED_GAMMA 6
#define GX_SCHED_N_MILESTONES 7
#define GX_SCHED_MILESTONE0 8
#define GX_SCHED_MAX_MILESTONES 8
#define GX_SCHED_WORDS 16
#define GX_TAIL_LR 0
#define GX_TAIL_DECAY 8
#define GX_TAIL_BYTES 16
#define GX_EMA_FP32 0
#define GX_EMA_FP64 1
#define GX_EMA_D_SRC 0
#define GX_EMA_D_DST 1
#define GX_EMA_D_N 2
#define GX_EMA_D_DTYPE 3
#define GX_EMA_D_WORK 4
#define GX_EMA_DESC_WORDS 5
#define GX_EMA_CHUNK 8192
#define GX_EMA_MAX_GRID 1024
int gx_adam_step_pair_ex(float* p32, float* g32, float* m32, float* v32, size_t n32, double* p64, double* g64, double* m64,
                         double* v64, size_t n64, int64_t* step, const double* sched, const double* lr_dev, double beta1,
                         double beta2, double eps, float grad_scale, const void* record, float* ema32, double* ema64,
                         double ema_decay, int ema_warmup, double* tail, int zero_grads, gx_stream_t stream);
int gx_optimiser_step_pair_ex(int kind, float* p32, float* g32, float* m32, size_t n32, double* p64, double* g64, double* m64,
                              size_t n64, int64_t* step, const double* sched, const double* lr_dev, double hp, double eps,
                              float grad_scale, const void* record, float* ema32, double* ema64, double ema_decay,
                              int ema_warmup, double* tail, int zero_grads, gx_stream_t stream);
int gx_ema_multi(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                 const int64_t* step, double decay, int warmup, double* decay_used, gx_stream_t stream);

/* ---- live per-kernel profiling (bench.py's roofline leg): when enabled every kernel launch is bracketed
 *      by two HIP events on its launch stream and tagged with its ALGORITHMIC flops / bytes
 *      (DESIGN.md "kernels and rooflines"); gx_profile_collect accumulates per kernel symbol. */
int gx_profile_enable(int on);
int gx_profile_num_kernels(void);
const char* gx_profile_kernel_name(int kid);
int gx_profile_collect(double* total_ms, double* launches, double* flops, double* bytes);

/* ---- ComponentVAE / MONet path (modules/component_vae.py:45-93, modules/encoders.py:31-37,
 *      modules/decoders.py:25-32, models/monet_config.py:74-128).
 *      gx_conv3x3_bias_act_fwd: conv3x3 s1 p1 + bias + activation (act 0 none, 1 ReLU, 2 ELU) on any HxW grid.
 *      The BroadcastDecoder's VALID 3x3 convs run as this 'same' conv on the (img+2L)^2 broadcast canvas: the
 *      centre crop after L layers equals the valid-conv chain exactly (border pollution advances one pixel per
 *      layer and is cropped; its gradients are identically zero).
 *      gx_bias_act_bwd: dy = g * act'(out) (derivative from the OUTPUT) and dbias[c] = sum dy (NULL to skip).
 *      gx_conv2d_direct_*: generic k<=5 / stride / pad convolution (implicit GEMM on the fp32 matrix cores, operands
 *      gathered; split-K + fixed-order reduce for the weight gradient): the stride-2 encoder convs here and the
 *      sylvester 5x5 gated (de)convolutions below.
 *      gx_mixture_w_*: mixture likelihood with EXTERNAL mixing log-weights log_w [K,B,1,H,W] (MONet mixes with
 *      the attention masks, not with log_softmax(logits)) and a separate std for the first slot; dec has dec_ch
 *      channels per slot: 4 (RGB + logit, MONet) or 3 (RGB, GENESIS); bwd also returns dlog_w; the logit channel
 *      of ddec (if any) is zero. */
int gx_conv3x3_bias_act_fwd(const float* x, const float* w, const float* bias, int act, float* y, int N, int Cin,
                            int Cout, int H, int W, void* ws, size_t ws_bytes, gx_stream_t stream);
size_t gx_bias_act_bwd_ws_bytes(int N, int C);
int gx_bias_act_bwd(const float* out, const float* g, int N, int C, int H, int W, int act, float* dy, float* dbias,
                    void* ws, size_t ws_bytes, gx_stream_t stream);
/*      gx_conv3x3_dgrad_act: the data gradient of a conv3x3 whose input was such a layer's output xout [N,Cin,H,W]
 *      (modules/decoders.py:25-32: Conv2d, ReLU, Conv2d, ...): dxa = dgrad(dy, w) * act'(xout) and dbias [Cin] (NULL to
 *      skip) = sum_{n,hw} dxa -- gx_conv3x3_dgrad followed by gx_bias_act_bwd with the activation's backward in the conv
 *      kernel's epilogue.  Shapes of the bf16-pipe <= 32-channel kernel only: gx_conv3x3_dgrad_act_supported. */
int gx_conv3x3_dgrad_act_supported(int N, int Cin, int Cout, int H, int W);
size_t gx_conv3x3_dgrad_act_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv3x3_dgrad_act(const float* dy, const float* w, const float* xout, int act, float* dxa, float* dbias, int N,
                         int Cin, int Cout, int H, int W, void* ws, size_t ws_bytes, gx_stream_t stream);
/* ---- 5 x 5 stride-1 pad-2 weight gradient of the gated stacks (third_party/sylvester/VAE.py:18-33, layers.py:40-101) on
 *      the bf16-pipe row-ring tiles: dw [CA][CB][5][5] = sum_{n,p} a[n][CA][p] * b[n][CB][p + (kh - 2, kw - 2)].
 *      Conv2d: a = dy, b = x -> dw [Cout][Cin][5][5]; ConvTranspose2d stride 1: a = x, b = dy -> dw [Cin][Cout][5][5].
 *      Queued into the step's stream-K launch when deferral is on (gx_defer_*), else launched at once. */
/*      conv3x3 weight gradient of a layer with 32 channels on both sides (the BroadcastDecoder's canvas convs,
 *      modules/decoders.py:21-35) and N % 4 == 0 images: four images per workgroup, one per wave, so that every wave's
 *      32 x 32 block is a wanted one; x, dy [N,32,H,W] -> dw [32,32,3,3] (overwritten).  H x W any grid with W % 4 == 0. */
int gx_conv3x3_wgrad_quad_supported(int N, int C, int H, int W);
size_t gx_conv3x3_wgrad_quad_ws_bytes(int N, int C, int H, int W);
int gx_conv3x3_wgrad_quad(const float* x, const float* dy, float* dw, int N, int C, int H, int W, void* ws, size_t ws_bytes,
                          gx_stream_t stream);
/*      ..._bias: also dbias [C] = sum_{n,hw} dy -- the layer's bias gradient from the weight gradient's own read of dy (per-thread
 *      sums inside the bf16-pipe kernel, one small reduce; a plane-sum pass over dy where that kernel is not the one that runs). */
size_t gx_conv3x3_wgrad_quad_bias_ws_bytes(int N, int C, int H, int W);
int gx_conv3x3_wgrad_quad_bias(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int H, int W, void* ws,
                               size_t ws_bytes, gx_stream_t stream);
/*      the layers themselves on the tap-conv MFMA kernel: out [N,M,H,W] from in [N,K,H,W];
 *      flip 0: cross-correlation with w [M][K][5][5] (Conv2d forward; data gradient of a stride-1 ConvTranspose2d),
 *      flip 1: convolution with w [K][M][5][5] (Conv2d data gradient, in = dy; stride-1 ConvTranspose2d forward). */
int gx_conv5x5s1_supported(int N, int K, int M, int H, int W);
size_t gx_conv5x5s1_ws_bytes(int N, int K, int M, int H, int W);
int gx_conv5x5s1(const float* in, const float* w, float* out, int N, int K, int M, int H, int W, int flip, void* ws,
                 size_t ws_bytes, gx_stream_t stream);
int gx_conv5x5_wgrad_supported(int N, int CA, int CB, int H, int W);
size_t gx_conv5x5_wgrad_ws_bytes(int N, int CA, int CB, int H, int W);
int gx_conv5x5_wgrad(const float* a, const float* b, float* dw, int N, int CA, int CB, int H, int W, void* ws,
                     size_t ws_bytes, gx_stream_t stream);

/*      conv3x3 stride 2 pad 1 data gradient (the ComponentVAE encoder, modules/encoders.py:31-34) without the stride's
 *      structural zeros, on the vector ALUs: only the first cin_n channels of dx [N,Cin,H,W] are computed and written
 *      (the encoder's first layer needs the mask channel's gradient alone). */
int gx_conv3x3s2_dgrad_small(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int H, int W, int cin_n,
                             gx_stream_t stream);
/*      _ex: dx holds dx_channels >= cin_n channels per image (dx_channels = cin_n: the compact gradient of the mask channel). */
int gx_conv3x3s2_dgrad_small_ex(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int H, int W, int cin_n,
                                int dx_channels, gx_stream_t stream);
/*      the slot-major ComponentVAE input [log_m_k | x] (modules/component_vae.py:59-66: torch.cat((log_m_k, x), 1) per slot;
 *      models/monet_config.py / genesis_config.py batch the K slots): out [K*B, 1 + C, H, W] from mask [K,B,1,H,W] and
 *      x [B,C,H,W] in one pass -- no x.repeat(K), no torch.cat.  H W % 4 == 0. */
int gx_mask_image_stack(const float* mask, const float* x, float* out, int K, int B, int C, int H, int W, gx_stream_t stream);
/*      ... and its weight gradient dw [Cout,Cin,3,3] (lanes = output pixels, 9 taps x 8 output channels per thread, fixed-
 *      order split reduction; ws: gx_conv3x3s2_wgrad_small_ws_bytes). */
size_t gx_conv3x3s2_wgrad_small_ws_bytes(int N, int Cin, int Cout, int H, int W);
int gx_conv3x3s2_wgrad_small(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int H, int W, void* ws,
                             size_t ws_bytes, gx_stream_t stream);
int gx_conv2d_direct_fwd(const float* x, const float* w, const float* bias, int act, float* y, int N, int Cin,
                         int Cout, int H, int W, int k, int stride, int pad, gx_stream_t stream);
/*      ... with a workspace: layers whose output tiles leave most of the chip idle (the ComponentVAE encoder's last stride-2
 *      convs, modules/encoders.py:31-34) split the contraction over workgroups and finish in a fixed-order reduce + bias +
 *      activation launch; ws_bytes 0 (or a NULL ws) = the single-launch form above */
size_t gx_conv2d_direct_fwd_ws_bytes(int N, int Cin, int Cout, int H, int W, int k, int stride, int pad);
int gx_conv2d_direct_fwd_ws(const float* x, const float* w, const float* bias, int act, float* y, int N, int Cin,
                            int Cout, int H, int W, int k, int stride, int pad, void* ws, size_t ws_bytes,
                            gx_stream_t stream);
int gx_conv2d_direct_dgrad(const float* dy, const float* w, float* dx, int N, int Cin, int Cout, int H, int W, int k,
                           int stride, int pad, gx_stream_t stream);
size_t gx_conv2d_direct_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W, int k, int stride, int pad);
int gx_conv2d_direct_wgrad(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int H, int W, int k,
                           int stride, int pad, void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_mixture_w_fwd(const float* x, const float* dec, const float* log_w, int dec_ch, int B, int H, int W, int K,
                     float pixel_std1, float pixel_std2, int pixel_bound, float* recon, float* x_r, float* err,
                     void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_mixture_w_bwd(const float* x, const float* dec, const float* log_w, const float* g_err, int dec_ch, int B,
                     int H, int W, int K, float pixel_std1, float pixel_std2, int pixel_bound, float* ddec,
                     float* dlog_w, gx_stream_t stream);

/* ---- gated (de)convolution unit of the sylvester VAE (third_party/sylvester/layers.py:40-54,87-101):
 *      out = norm_h(h + b_h) * sigmoid(norm_g(g + b_g)), [h | g] = the two channel halves of y [N,2C,H,W];
 *      norm 0 none, 1 BatchNorm2d with training-mode batch statistics, 2 InstanceNorm2d(affine); `bias` [2C] is the
 *      (de)conv bias, folded in here.  stats: gx_gated_stats_floats() floats ({mean, rstd} per unit), kept for bwd
 *      (and for the caller's running-statistics update).  bwd returns dy [N,2C,H,W] and the affine / bias grads. */
size_t gx_gated_stats_floats(int norm, int N, int C);
int gx_gated_norm_fwd(const float* y, const float* bias, int norm, const float* gamma_h, const float* beta_h,
                      const float* gamma_g, const float* beta_g, int N, int C, int H, int W, float eps, float* out,
                      float* stats, gx_stream_t stream);
/*      nn.BatchNorm2d running statistics of a gated unit's two norms (momentum update with the unbiased variance,
 *      num_batches_tracked += 1) from the {mean, rstd} pairs gx_gated_norm_fwd left in `stats`; m = N H W. */
int gx_bn_running_update(const float* stats, int C, double m, float eps, float momentum, float* rm_h, float* rv_h, float* rm_g,
                         float* rv_g, long long* nbt_h, long long* nbt_g, gx_stream_t stream);
/*      ... or the same update without a launch of its own: gx_gated_bn_running arms a one-shot, per-thread request that the NEXT
 *      gx_gated_norm_fwd of this thread (norm 1) applies inside its apply kernel, whose workgroups also fold the statistics pass's
 *      partial sums themselves (two launches less per unit; GENESIS_GATED_FUSE=0: the stand-alone launches; rm_h NULL disarms).
 *      gx_gated_norm_bwd (norm 1) folds its sums and writes the affine gradients the same way. */
int gx_gated_bn_running(float* rm_h, float* rv_h, float* rm_g, float* rv_g, long long* nbt_h, long long* nbt_g, float momentum);
size_t gx_gated_norm_bwd_ws_bytes(int norm, int N, int C);
int gx_gated_norm_bwd(const float* y, const float* bias, int norm, const float* gamma_h, const float* beta_h,
                      const float* gamma_g, const float* beta_g, const float* stats, const float* dout, int N, int C,
                      int H, int W, float* dy, float* dgamma_h, float* dbeta_h, float* dgamma_g, float* dbeta_g,
                      float* dbias, void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- the gated unit's BatchNorm over the batches of SEVERAL ranks (cross-replica BatchNorm: the reference's single-device
 *      statistics at the global batch, models/genesis_config.py:39-40 -> third_party/sylvester/layers.py:26-27, when the batch is
 *      sharded over GPUs).  Forward: gx_gated_bn_local_sums leaves fp64 {sum, sum of squares} of (y + bias) per
 *      channel in sums [2C][2]; the caller adds them over the ranks; gx_gated_bn_apply forms {mean, rstd} from the summed pairs
 *      and the GLOBAL count m = sum over ranks of N H W (written to `stats` [2C][2], kept for bwd and gx_bn_running_update) and
 *      applies the unit.  Backward: gx_gated_bn_bwd_local_sums leaves the rank's {S1, S2} per channel (float [2C][2]) and
 *      writes the affine / bias gradients from them (the step's gradient all-reduce adds the ranks); the caller adds the sums
 *      over the ranks; gx_gated_bn_bwd_apply writes dy from the summed pairs and m.  ws: gx_gated_bn_sums_ws_bytes(). */
size_t gx_gated_bn_sums_ws_bytes(int N, int C);
int gx_gated_bn_local_sums(const float* y, const float* bias, int N, int C, int H, int W, double* sums, void* ws,
                           size_t ws_bytes, gx_stream_t stream);
int gx_gated_bn_apply(const float* y, const float* bias, const double* sums, double m, const float* gamma_h,
                      const float* beta_h, const float* gamma_g, const float* beta_g, int N, int C, int H, int W, float eps,
                      float* out, float* stats, gx_stream_t stream);
int gx_gated_bn_bwd_local_sums(const float* y, const float* bias, const float* gamma_h, const float* beta_h,
                               const float* gamma_g, const float* beta_g, const float* stats, const float* dout, int N, int C,
                               int H, int W, float* sums, float* dgamma_h, float* dbeta_h, float* dgamma_g, float* dbeta_g,
                               float* dbias, void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_gated_bn_bwd_apply(const float* y, const float* bias, const float* gamma_h, const float* beta_h, const float* gamma_g,
                          const float* beta_g, const float* stats, const float* dout, const float* sums, double m, int N, int C,
                          int H, int W, float* dy, gx_stream_t stream);

/* ---- stick-breaking mask recursion in log space (modules/attention.py:31-51 SimpleSBP, :118-124 LatentSBP):
 *      log_m[t] = s_t + logsigmoid(l_t), s_{t+1} = s_t + logsigmoid(-l_t), s_0 = log_s0 (NULL: 0); logits / log_m /
 *      log_s [T,P] (log_s[t] = the scope AFTER step t); last_scope: log_m[T-1] = s_{T-1}, the remaining scope
 *      (genesis_config.py:167-169).  bwd: g_log_m / g_log_s [T,P] (either may be NULL) -> g_logits [T,P],
 *      g_log_s0 [P] (may be NULL). */
int gx_sbp_scan_fwd(const float* logits, const float* log_s0, int T, size_t P, int last_scope, float* log_m,
                    float* log_s, gx_stream_t stream);
int gx_sbp_scan_bwd(const float* logits, const float* g_log_m, const float* g_log_s, int T, size_t P, int last_scope,
                    float* g_logits, float* g_log_s0, gx_stream_t stream);
/* ---- MONet.kl_m_loss (models/monet_config.py:157-170): per image, sum over pixels of KL(Cat(q) || Cat(p)) with
 *      q = max(exp(log_m), 1e-5), p = max(exp(log_m_r), 1e-5) renormalised over K; log_m / log_m_r [K,B,HW] slot-major,
 *      kl [B].  bwd: g_kl [B] -> g_log_m and, when g_log_m_r != NULL (detach_mr_in_klm = False,
 *      genesisv2_config.py:172-176), the gradient through the reconstructed masks. */
int gx_categorical_kl_fwd(const float* log_m, const float* log_m_r, int K, int B, int HW, float* kl,
                          gx_stream_t stream);
int gx_categorical_kl_bwd(const float* log_m, const float* log_m_r, const float* g_kl, int K, int B, int HW,
                          float* g_log_m, float* g_log_m_r, gx_stream_t stream);
/*      the reconstructed masks log_m_r [K,B,HW] = log_softmax over the K slots of the decoder output's last channel
 *      (MONet.get_mask_recon_stack, monet_config.py:137-139; dec [K*B, C, HW] slot-major), and their gradient back into
 *      the decoder output: g [K,B,HW] -> g_dec [K*B, C, HW] (channels < C-1 zero) */
int gx_logsoftmax_k_fwd(const float* dec, int K, int B, int HW, int C, float* log_m_r, gx_stream_t stream);
int gx_logsoftmax_k_bwd(const float* log_m_r, const float* g, int K, int B, int HW, int C, float* g_dec,
                        gx_stream_t stream);

/* ---- spatial broadcast + coordinate channels (modules/blocks.py:104-130 BroadcastLayer / PixelCoords).
 *      gx_broadcast_concat: out [N, D+2, d, d] = [ z[n] broadcast | coords[0] | coords[1] ], z [N,D], coords [2,d,d]
 *      (the GENESIS-V2 decoder input, models/genesisv2_config.py:89-90).
 *      gx_bcast_conv3x3_*: the BroadcastDecoder's first layer act(conv3x3(broadcast canvas, w) + b)
 *      (modules/decoders.py:25-28) WITHOUT the canvas: w [Co, L+2, 3, 3]; rowc / colc [d] = the row / column
 *      coordinate (coords[0][:, 0] / coords[1][0, :]: channel L is constant along x, channel L+1 along y);
 *      out / y / g [N, Co, d, d] on the d x d canvas, d a multiple of 4.  Inside the canvas the result equals the
 *      conv on the materialised canvas; the one-pixel border ring (outside the VALID conv's output) holds the
 *      interior formula and must not be consumed.  bwd: g = dL/dout; gradients are taken over the interior
 *      [1, d-2]^2 (the valid conv's outputs): dz [N,L], dw [Co,L+2,3,3], db [Co] (may be NULL); act 0 none, 1 ReLU,
 *      2 ELU. */
int gx_broadcast_concat(const float* z, const float* coords, float* out, int N, int D, int d, gx_stream_t stream);
/*      The GENESIS-V2 decoder's first layer, ConvTranspose2d(D+2, Cout, 5, 2, 2, 1) on that broadcast input
 *      (models/genesisv2_config.py:89-90), WITHOUT the canvas: the input is constant over the pixels, so
 *      out[n,co,oy,ox] = sum_ci z[n,ci] Wz[ci][co][oy][ox] + C[co][oy][ox] -- one [N,D] x [D, Cout (2d)^2] product
 *      (gx_linear_fwd / gx_linear_bwd on wz).  pack: w [D+2,Cout,5,5], b [Cout] (may be NULL), coords [2,d,d] ->
 *      wz [Cout (2d)^2, D] (the tap sums, nn.Linear weight layout) and bias [Cout (2d)^2] (b + the coordinate
 *      channels' contribution).  unpack: the gradients of wz and bias -> dw [D+2,Cout,5,5], db [Cout] (may be NULL). */
int gx_bcast_deconv5x5s2_pack(const float* w, const float* b, const float* coords, int D, int Cout, int d, float* wz,
                              float* bias, gx_stream_t stream);
int gx_bcast_deconv5x5s2_unpack(const float* dwz, const float* dbias, const float* coords, int D, int Cout, int d,
                                float* dw, float* db, gx_stream_t stream);
int gx_bcast_conv3x3_fwd(const float* z, const float* w, const float* bias, const float* rowc, const float* colc,
                         int act, float* out, int N, int L, int Co, int d, gx_stream_t stream);
size_t gx_bcast_conv3x3_bwd_ws_bytes(int N, int Co);
int gx_bcast_conv3x3_bwd(const float* y, const float* g, const float* z, const float* w, const float* rowc,
                         const float* colc, int act, int N, int L, int Co, int d, float* dz, float* dw, float* db,
                         void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- slot-latent head: reparameterised posterior sample + Monte-Carlo KL terms
 *      (models/genesisv2_config.py:154-160: mu, sigma_ps = z_head(obj).chunk(2); sigma = to_sigma(sigma_ps);
 *      z = Normal(mu, sigma).rsample(); modules/blocks.py:22-23 to_sigma = softplus(x + 0.5) + 1e-8, :28-36
 *      to_prior_sigma = sigmoid(x + 4) + 1e-4; models/genesis_config.py:288-343 mask_latent_loss:
 *      log_q = q_z_k.log_prob(z_k).sum(1), log_p under N(0,1) for the first slot and under
 *      N(tanh(lin[:D]), to_prior_sigma(lin[D:])) for later slots, lin = prior_linear(prior_lstm(z_{<k}))).
 *      zh [B,K,2D] = z_head output (mu | sigma_ps), eps [K,B,D] standard normal; z, mu, sigma [K,B,D] slot-major,
 *      log_q / log_p [K,B].  lin [K-1,B,2D], or NULL for the standard-normal prior on every slot.
 *      gx_latent_prior_logp_fwd writes out = log_p, or the KL sample log_q - log_p when log_q is given
 *      (kl_mode = 1 in bwd: g_out is then dL/d(log_q - log_p)).
 *      bwd: incoming gradients gz / gmu / gsigma [K,B,D], glogq [K,B] may each be NULL (= zero). */
int gx_latent_posterior_fwd(const float* zh, const float* eps, int B, int K, int D, float* z, float* mu,
                            float* sigma, float* log_q, gx_stream_t stream);
int gx_latent_posterior_bwd(const float* zh, const float* eps, const float* gz, const float* gmu,
                            const float* gsigma, const float* glogq, int B, int K, int D, float* dzh,
                            gx_stream_t stream);
/* _ex: the recurrent posterior of GENESIS' LatentSBP (modules/attention.py:103-118: the sampled z_{k-1} is concatenated to
 * the encoder features as the next LSTM input) without torch.cat -- fwd also writes z to z2 [K*B rows of ldz2 floats] (the
 * z columns of the next step's input rows; NULL: none); bwd adds a second incoming gz2 [K*B rows of ldgz2 floats] (the
 * input-projection gradient's z columns) to gz. */
int gx_latent_posterior_fwd_ex(const float* zh, const float* eps, int B, int K, int D, float* z, float* mu,
                               float* sigma, float* log_q, float* z2, int ldz2, gx_stream_t stream);
int gx_latent_posterior_bwd_ex(const float* zh, const float* eps, const float* gz, const float* gmu,
                               const float* gsigma, const float* glogq, const float* gz2, int ldgz2, int B, int K,
                               int D, float* dzh, gx_stream_t stream);
int gx_latent_prior_logp_fwd(const float* z, const float* lin, const float* log_q, int B, int K, int D,
                             float* out, gx_stream_t stream);
int gx_latent_prior_logp_bwd(const float* z, const float* lin, const float* g_out, int kl_mode, int B, int K,
                             int D, float* dz, float* dlin, gx_stream_t stream);
/*      ..._ex with all_slots = 1: every slot has a conditional prior, lin [K,B,2D] (Genesis' component prior,
 *      models/genesis_config.py:229-247: p(z_c | z_m) = N(tanh(mlp[:L]), to_prior_sigma(mlp[L:])) for all K slots) */
int gx_latent_prior_logp_fwd_ex(const float* z, const float* lin, const float* log_q, int B, int K, int D, int all_slots,
                                float* out, gx_stream_t stream);
int gx_latent_prior_logp_bwd_ex(const float* z, const float* lin, const float* g_out, int kl_mode, int B, int K,
                                int D, int all_slots, float* dz, float* dlin, gx_stream_t stream);
/*      one ancestral step of GenesisV2.sample (models/genesisv2_config.py:235-246): lin [B,2D] = prior_linear(lstm out),
 *      eps [B,D] standard normal -> z [B,D] = tanh(lin[:D]) + to_prior_sigma(lin[D:]) * eps */
int gx_latent_prior_sample(const float* lin, const float* eps, int B, int D, float* z, gx_stream_t stream);
/*      the same with the mean's tanh selectable: Genesis.sample's mask rollout (models/genesis_config.py:352-362) uses
 *      the RAW first half of prior_linear's output as the mean (tanh_mu = 0); its component prior
 *      (models/genesis_config.py:391-397: tanh(prior_mlp[:L]), to_prior_sigma(prior_mlp[L:])) is tanh_mu = 1 */
int gx_latent_prior_sample_ex(const float* lin, const float* eps, int B, int D, int tanh_mu, float* z,
                              gx_stream_t stream);

/* ---- loss aggregation of the training loop (train.py:226-242) with GECO's beta (utils/geco.py:47-49):
 *      err_mean = mean_b err[b]; kl_mean = sum_r mean_b kl[r][b] (kl [R,B], R = 0 / NULL: no KL term);
 *      out[5] = (loss = err_mean + beta kl_mean, err_mean + kl_mean, err_mean, kl_mean, beta); beta is read from
 *      device memory (GECO state); tail (NULL to skip) receives (err_mean, kl_mean) -- the gradient bucket's
 *      piggy-backed scalars; loss (NULL to skip) receives out[0] again (a separate one-element objective tensor).  bwd: d_err[b] = g/B, d_kl[r][b] = g beta / B for the scalar g = dL/d loss. */
int gx_elbo_fwd(const float* err, const float* kl, const float* beta, int B, int R, float* out, float* tail,
                float* loss, gx_stream_t stream);
/*      gx_elbo_fwd + the gradients gx_elbo_bwd returns for an upstream gradient of one, in one launch */
int gx_elbo_fwd_grads(const float* err, const float* kl, const float* beta, int B, int R, float* out, float* tail,
                      float* loss, float* d_err, float* d_kl, gx_stream_t stream);
int gx_elbo_bwd(const float* g_loss, const float* beta, int B, int R, float* d_err, float* d_kl,
                gx_stream_t stream);

/* ---- pooled slot features -> z_head[0] (models/genesisv2_config.py:146-154: obj_feat = feat_head(enc) * mask
 *      summed over pixels / (mask.sum + 1e-5); :76 nn.LayerNorm(2 feat_dim)).  lin [R,C] = pooled sums through
 *      feat_head[1]'s weight (gx_linear_fwd), msum [R] mask mass, fbias [C] feat_head[1].bias:
 *      obj = (lin + msum fbias) / (msum + 1e-5); y = LayerNorm(obj; gamma, beta, eps); stats [R,2] = (mean, rstd). */
int gx_pooled_head_fwd(const float* lin, const float* msum, const float* fbias, const float* gamma,
                       const float* beta, float eps, int R, int C, float* y, float* stats, gx_stream_t stream);
size_t gx_pooled_head_bwd_ws_bytes(int R, int C);
int gx_pooled_head_bwd(const float* lin, const float* msum, const float* fbias, const float* gamma,
                       const float* stats, const float* g, int R, int C, float* dlin, float* dmsum, float* dfbias,
                       float* dgamma, float* dbeta, void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- small dense layers (nn.Linear: modules/unet.py:58-62 bottleneck MLP, models/genesisv2_config.py:76-80
 *      z_head, :73 feat_head[1] on the pooled slot sums, models/genesis_config.py:106 prior_linear).
 *      y[M,N] = act(x[M,K] w[N,K]^T + b[N]), act 0 none / 1 ReLU / 2 ELU, b may be NULL.
 *      bwd: g = dL/dy; dpre = g * [y > 0] for act 1, g * (y > 0 ? 1 : y + 1) for act 2 (y = the layer OUTPUT, may be NULL for act 0);
 *      dx[M,K] = dpre w, dw[N,K] = dpre^T x, db[N] = column sums of dpre; each of dx / dw / db may be NULL to skip
 *      (db needs dw).  Row-major contiguous; fixed reduction order. */
int gx_linear_fwd(const float* x, const float* w, const float* b, int act, float* y, int M, int N, int K,
                  gx_stream_t stream);
int gx_linear_bwd(const float* x, const float* w, const float* y, const float* g, int act, float* dx, float* dw,
                  float* db, int M, int N, int K, gx_stream_t stream);
/*      Strided variants for operands that live inside larger buffers (the UNet bottleneck MLP writes its last
 *      layer straight into the first up-block's concat buffer, modules/unet.py:83-84, and reads that layer's
 *      gradient out of the concat buffer's gradient; the AR prior's LSTM input z[:-1] is the leading part of z):
 *      ldx / ldy / ldg / lddx = row strides in floats (>= the row length); y and g of the backward share ldg.
 *      dx_accumulate: bit 0: dx += dpre w (the second consumer of a tensor adds its gradient in place); bit 1: dw / db / db2
 *      += (a parameter used again in the same iteration: MONet's recurrent UNet);
 *      db2 (may be NULL): a second copy of db (nn.LSTM's b_ih and b_hh have the same gradient). */
int gx_linear_fwd_ld(const float* x, int ldx, const float* w, const float* b, int act, float* y, int ldy, int M,
                     int N, int K, gx_stream_t stream);
int gx_linear_bwd_ex(const float* x, int ldx, const float* w, const float* y, const float* g, int ldg, int act,
                     float* dx, int lddx, int dx_accumulate, float* dw, float* db, float* db2, int M, int N, int K,
                     gx_stream_t stream);

/* ---- plain matrix product with the weight in [K, N] layout: y[M,N] = x[M,K] w[K,N] -- the gated ConvTranspose2d 'fc' layer
 *      of the sylvester stacks applied to a 1 x 1 input (third_party/sylvester/VAE.py:27-33, layers.py:62-101: the weight
 *      [z, 2c, k, k] flattened to [z, 2c k k] IS w; no transposed copy).  K is small (the latent size), N large: an
 *      HBM-bound product on the vector ALUs (w is read once per 8 rows of x, coalesced; x rides in scalar registers).
 *      bwd: dw[K,N] = x^T g (dw may be NULL);  dx[M,K] = g w^T (dx may be NULL) summed over N in fixed-order partial
 *      slabs held in ws (gx_matmul_nn_bwd_ws_bytes).  Row-major contiguous, N % 4 == 0, 16-byte aligned. */
int gx_matmul_nn_fwd(const float* x, const float* w, float* y, int M, int N, int K, gx_stream_t stream);
size_t gx_matmul_nn_bwd_ws_bytes(int M, int N, int K);
int gx_matmul_nn_bwd(const float* x, const float* w, const float* g, float* dx, float* dw, int M, int N, int K,
                     void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- LSTM cell step (nn.LSTM, one layer, gate order i, f, g, o: models/genesis_config.py:105 prior_lstm, :297-307;
 *      modules/attention.py LatentSBP core).  The caller computes gx = x w_ih^T + b_ih for all steps with
 *      gx_linear_fwd and unrolls time:
 *      pre = gx[B,4H] + h_prev[B,H] w_hh[4H,H]^T + b_hh; act[B,4H] = (sigm i | sigm f | tanh g | sigm o);
 *      c = f c_prev + i g; h = o tanh(c).  h_prev = c_prev = NULL: zero initial state.
 *      bwd of one step: dh = g_h[B,H] (NULL = 0) + dgates_next[B,4H] w_hh (NULL at the last step);
 *      dc = dc_next (NULL = 0) + dh o (1 - tanh(c)^2); dgates[B,4H] = pre-activation gradients; dc_prev = dc f.
 *      Weight gradients follow from gx_linear_bwd on the stacked dgates.  H % 16 == 0. */
int gx_lstm_step_fwd(const float* gx, const float* h_prev, const float* c_prev, const float* w_hh,
                     const float* b_hh, int B, int H, float* act, float* c, float* h, gx_stream_t stream);
int gx_lstm_step_bwd(const float* g_h, const float* dgates_next, const float* w_hh, const float* act,
                     const float* c, const float* c_prev, const float* dc_next, int B, int H, float* dgates,
                     float* dc_prev, gx_stream_t stream);
/*      the whole sequence (zero initial state) in ONE launch each way -- the same per-step arithmetic in the same order, i.e. the
 *      results of the unrolled gx_lstm_step_* calls bit for bit; the steps are separated by grid-wide barriers inside the
 *      kernel, so the grid (H / 16 x ceil(B / 16) workgroups) has to be resident at once: gx_lstm_seq_max_steps(B, H) is
 *      the longest sequence one launch takes for these sizes (0: use the per-step calls).
 *      fwd: gx [T,B,4H] (input projection of all steps) -> act [T,B,4H], c [T,B,H], h [T,B,H].
 *      bwd: g_h [T,B,H] (dL/dh of every step), act, c of the forward -> dgates [T,B,4H]; dc2: two [B,H] planes of scratch.
 *      bar: gx_lstm_seq_ws_bytes() bytes of device memory, ZERO before the first launch that uses it; a launch leaves it
 *      zero again.  One `bar` must not be shared by launches that can run concurrently.
 *      (models/genesis_config.py:297-307 prior_lstm over z_{<k}) */
int gx_lstm_seq_max_steps(int B, int H);
size_t gx_lstm_seq_ws_bytes(void);
int gx_lstm_seq_fwd(const float* gx, const float* w_hh, const float* b_hh, int T, int B, int H, float* act, float* c,
                    float* h, void* bar, gx_stream_t stream);
int gx_lstm_seq_bwd(const float* g_h, const float* w_hh, const float* act, const float* c, int T, int B, int H,
                    float* dgates, float* dc2, void* bar, gx_stream_t stream);

/* ---- packed-weight cache.  The conv / deconv entry points above re-pack their weight tensor into the MFMA
 *      operand layout on every call; inside a training loop the weights change once per optimiser step, so:
 *      id = gx_weight_cache_create(); gx_weight_cache_record(id, 1); <one iteration>; gx_weight_cache_record(id, 0)
 *      registers every (weight pointer, layout) the iteration used (device buffers are allocated here -- do not
 *      record inside a stream capture).  From then on gx_weight_cache_refresh(id, stream) re-packs all of them in
 *      ONE launch and the entry points are served from the cache (matching weight pointer and shape) until
 *      gx_weight_cache_release().  The caller guarantees the weights do not change inside that window. */
int gx_weight_cache_create(void);
int gx_weight_cache_record(int id, int on);
int gx_weight_cache_size(int id);
int gx_weight_cache_refresh(int id, gx_stream_t stream);
int gx_weight_cache_release(void);
/*      gx_weight_cache_activate(id): serve the calls that follow from cache `id` as gx_weight_cache_refresh does, WITHOUT re-packing
 *      -- the weights have not changed since the last refresh (a backward pass issued separately from its forward pass). */
int gx_weight_cache_activate(int id);
int gx_weight_cache_destroy(int id);

/* ---- contexts.  Library state that outlives a call -- the deferred-reduction queues, queued weight-gradient jobs, the
 *      packed-weight cache a step records / is served from, per-kernel profiling records -- belongs to a context; a
 *      thread works in its current context (thread-local, context 0 by default).  One context per training loop makes
 *      the library re-entrant: loops in different threads, or interleaved in one thread, never share a queue.
 *      gx_ctx_create returns an id > 0 (negative: error). */
int gx_ctx_create(void);
int gx_ctx_make_current(int id);
int gx_ctx_current(void);
int gx_ctx_destroy(int id);

/* ---- deferred parameter-gradient reductions.  gx_conv3x3_wgrad, gx_deconv5x5s2_wgrad and gx_gn_relu_bwd each end
 *      in a small reduce launch whose result (dw / dgamma, dbeta) only the optimiser reads.  While
 *      gx_defer_enable(1) is in effect those calls queue that reduce instead (up to 48 of each kind; beyond that they
 *      reduce immediately) and gx_defer_flush(stream) finishes all queued ones in one launch per kind, ADDING each
 *      result to its destination (which the caller has zeroed: a gradient bucket).  Contract: the
 *      workspaces and output buffers handed to the queued calls stay valid and untouched until the flush.
 *      gx_defer_enable(-1) switches deferral off and discards the queue without running it (error recovery). */
int gx_defer_enable(int on);
int gx_defer_pending(void);
int gx_defer_flush(gx_stream_t stream);

/* ---- conv -> GroupNorm without the split-K reduce pass.  Layers that cannot fill the chip split the channel
 *      reduction into `nsplit` partial output slabs which a small reduce kernel normally sums.  The *_parts variants
 *      stop before that reduce and report where the slabs are (*parts: inside ws when *nsplit > 1, else = y, already
 *      complete; *split_stride floats apart; no bias applied); gx_gn_relu_fwd_parts sums them while it reads its
 *      input (same order as the reduce kernel: identical bits), adds the conv bias (may be NULL), writes the summed
 *      pre-norm tensor to y_sum (the backward pass needs it; may alias parts when nsplit == 1) and continues as
 *      gx_gn_relu_fwd.  ws must stay untouched until gx_gn_relu_fwd_parts has run. */
int gx_conv3x3_fwd_parts(const float* x, const float* w, float* y, int N, int Cin, int Cout, int H, int W, void* ws,
                         size_t ws_bytes, const float** parts, int* nsplit, size_t* split_stride, gx_stream_t stream);
int gx_deconv5x5s2_fwd_parts(const float* x, const float* w, float* y, int N, int Cin, int Cout, int Hin, int Win,
                             void* ws, size_t ws_bytes, const float** parts, int* nsplit, size_t* split_stride,
                             gx_stream_t stream);
int gx_gn_relu_fwd_parts(const float* parts, int nsplit, size_t split_stride, const float* conv_bias, float* y_sum,
                         const float* gamma, const float* beta, int N, int C, int H, int W, int groups, float eps,
                         float* dst0, int dst0_ctot, int dst0_c0, int dst0_mode, float* dst1, int dst1_ctot,
                         int dst1_c0, int dst1_mode, float* mean, float* rstd, gx_stream_t stream);

/* ---- segmentation metrics on the device (utils/misc.py:101-114 average_ari, :173-235 average_segcover):
 *      counts[b][i][j] = #{p : segA[b][p] == i and segB[b][p] == j}, int32 [B, KA, KB+1]; column KB collects segB labels
 *      outside [0,KB); pixels with segA outside [0,KA) (negative = ignore regions) are skipped.  Labels are int64
 *      [B, HW] as the reference's instance maps / argmax outputs are.  Bit-exact integer work. */
int gx_label_contingency(const long long* segA, const long long* segB, int B, int HW, int KA, int KB, int* counts,
                         gx_stream_t stream);
/*      gx_seg_metrics: one batch of the validation loop (train.py:534-559) in one launch, from the K log-mask planes read in
 *      place and the instance map to every score: prediction = argmax_k of the log-masks (ties: lowest k; a NaN ranks above every
 *      number and the first one wins, as torch.argmax), the table [max_labels, K] of (ground truth, prediction) in LDS, then per
 *      image b the row rows[b] = (ARI, foreground ARI, mean covering, mean covering without background, scaled covering, scaled
 *      covering without background, counted pixels, ground-truth labels present) in fp64 -- ARI from int64 pair counts with the
 *      final expression in fp64 (1.0 when the partitions agree or no pixel is counted), covering in float32 with the labels
 *      added in ascending order.  Ground-truth labels < 0 are ignore regions (skipped); labels >= max_labels are not counted
 *      and add one each to state[2].  The last workgroup to finish adds the batch means (fp64 for ARI, float32 for covering,
 *      image order) to acc[0..8) -- the covering sums themselves kept in float32, as the reference adds its batch means --,
 *      increments state[1], copies the rows to log[state[3] ..] while they fit into log_capacity rows (log may be NULL) and
 *      advances state[3].  Planes: either base != NULL, plane k of image b at base + k plane_stride + b image_stride floats
 *      (planes == NULL), or planes = a HOST array of K device pointers to image 0 of each plane (base == NULL, plane_stride
 *      ignored), image b image_stride floats further; every plane is HW contiguous floats.  16-byte loads when HW % 4 == 0
 *      and every plane of every image is 16-byte aligned, 4-byte loads otherwise.  1 <= K <= 32, max_labels * K * 4 bytes
 *      <= 64 KiB.  instances int64 [B, HW]; rows fp64 [B, 8] (scratch); acc fp64 [8] and state [4] = (arrival counter,
 *      batches, overflowed pixels, log cursor) zero before the first launch; launches on one stream may share them. */
int gx_seg_metrics(const float* base, long long plane_stride, long long image_stride, const float* const* planes,
                   const long long* instances, int B, int HW, int K, int max_labels, double* rows, double* acc,
                   unsigned long long* state, double* log, long long log_capacity, gx_stream_t stream);

/* ---- per-object tables of an unsupervised segmentation (genesis_amd/objects.py): what a consumer of a label map asks next --
 *      which slots are present, how large, where, how confident -- for data without ground truth.  ONE launch per batch; integer
 *      and fp64 work only.  Planes: the K log-mask planes addressed exactly as gx_seg_metrics addresses them -- either
 *      base != NULL, plane k of image b at base + k plane_stride + b image_stride floats (planes == NULL), or planes = a HOST
 *      array of K device pointers to image 0 of each plane (base == NULL, plane_stride ignored), image b image_stride floats
 *      further; every plane is H W contiguous floats.  x: an optional image, fp32 [B, C, H, W], image b at x + b x_image_stride
 *      floats, each image C H W contiguous floats, 1 <= C <= 4; NULL: no colour sums (C and x_image_stride are then ignored).
 *        labels  uint8 [B, H W]: argmax_k of the log-masks (ties: lowest k; a NaN ranks above every number and the first one wins,
 *                as gx_seg_metrics and torch.argmax).
 *        geom    int64 [B, K, 8], per slot k over the pixels labelled k (column px, row py): area, x_min, y_min, x_max, y_max, sum_x =
 *                sum px, sum_y = sum py, border = bit 0 if a pixel lies in column 0, bit 1 row 0, bit 2 column W - 1, bit 3 row
 *                H - 1.  A slot without pixels is (0, W, H, -1, -1, 0, 0, 0).  Bit-exact.
 *        soft    fp64 [B, K, 6], per slot k: mass = sum over ALL pixels of exp((double)log_m_k), inside = the same sum over the
 *                pixels labelled k, c0..c3 = sum over the pixels labelled k of (double)x[c] (0 for c >= C, or when x is NULL).
 *                Every operation after the fp32 load is fp64, each rounded on its own; exp(-inf) = 0, and so is exp(-1e10), the
 *                padding of dynamic_K.  A NaN log-mask makes its slot's mass NaN (and inside, where it wins the pixel).
 *      Plan: one workgroup of 256 threads per image and nothing shared between workgroups.  Thread t owns the pixel quads t,
 *      t + 256, ... (pixels 4q .. 4q + 3) in both passes: pass 1 takes the argmax and writes labels; pass 2 goes slot after slot,
 *      every thread adding its pixels in ascending order into private accumulators, then a shuffle butterfly over the 64 lanes
 *      of each wave, then one LDS row per wave, and after the last slot the four rows are added in wave order.  No atomics,
 *      floating-point or integer.  An image's rows are the same bits whatever batch and batch position it arrives in, and
 *      whichever load width is used: 16-byte loads of the planes (4-byte of labels) when H W % 4 == 0, every plane of every image
 *      is 16-byte aligned and labels is 4-byte aligned; 4-byte (1-byte) loads in the same pixel order otherwise.  x is read with
 *      4-byte loads, every element once.
 *      GX_EINVAL before any launch: both or neither of base / planes, a null plane, labels, geom or soft; K outside [1, 32];
 *      B, H or W < 1, H or W > 4096; a negative plane_stride; image_stride below H W; with x non-null, C outside [1, 4] or
 *      x_image_stride below C H W. */
int gx_object_table(const float* base, long long plane_stride, long long image_stride, const float* const* planes, const float* x,
                    long long x_image_stride, int C, int B, int H, int W, int K, unsigned char* labels, long long* geom,
                    double* soft, gx_stream_t stream);

/* ---- reconstruction quality on the device (genesis_amd/image_quality.py): per image b of pred / target (fp32 [B, C, H, W], image b
 *      at base + b image_stride floats, each image C H W contiguous floats) the row rows[b] = (mse, rmse, psnr, ssim) in fp64 --
 *      every operation from the load onwards is fp64, each rounded on its own (no contraction):
 *        mse  = (1 / (C H W)) sum (pred - target)^2 (train.py:244 in fp64),  rmse = sqrt(mse),
 *        psnr = 10 log10(data_range^2 / mse), +inf when mse == 0; NaN inputs give NaN,
 *        ssim = mean over channels and VALID window positions ((H - win + 1) x (W - win + 1), no padding) of
 *               ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)),  C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2,
 *               mx = g * x, my = g * y, sx2 = g * x^2 - mx^2, sy2 = g * y^2 - my^2, sxy = g * (x y) - mx my, g the outer product of
 *               `window` (a HOST array of `win` fp64 taps that sum to 1: genesis_amd.image_quality.gaussian_window) with itself.
 *      ONE launch.  Tile plan: a workgroup owns one 16 x 16 tile of valid positions of one image and loops over the channels; it
 *      stages the haloed (16 + win - 1)^2 patch of both tensors in LDS once per channel, runs the window as a row pass then a column
 *      pass over the five maps, and adds its tile's SSIM values and squared errors in a fixed order into the tile's slot of ws.
 *      Squared error: every pixel exactly once -- a tile owns the 16 x 16 pixels at its valid positions, and the last tile of a row
 *      (column) of tiles also owns the win - 1 trailing columns (rows), which lie inside its staged patch.  No floating-point
 *      atomics: the last workgroup to arrive (state[0], an integer counter that it puts back to 0) adds every image's slots in tile
 *      order, writes the rows, adds them to acc[0..4) in image order, adds B to state[1] and 1 to state[2], copies the rows to
 *      log[state[3] ..] while they fit into log_capacity rows (log may be NULL) and advances state[3].  An image's row is the same
 *      bits whatever batch it arrives in.  16-byte loads when W % 4 == 0, both bases are 16-byte aligned and both image strides are
 *      multiples of 4; 4-byte loads otherwise.  GX_EINVAL before any launch: a null pred, target, window, rows, acc, state or ws;
 *      win even or outside [3, 11]; B or C < 1; H or W below win or above 4096; data_range not positive and finite; an image
 *      stride below C H W; ws_bytes below gx_image_quality_ws_bytes (two doubles per tile; 0 for a shape that is refused).
 *      rows fp64 [B, 4] (scratch); acc fp64 [4] and state [4] = (arrival counter, images, batches, log cursor) zero before the
 *      first launch; launches on one stream may share them and ws. */
int gx_image_quality(const float* pred, long long pred_image_stride, const float* target, long long target_image_stride, int B,
                     int C, int H, int W, const double* window, int win, double data_range, double* rows, double* acc,
                     unsigned long long* state, double* log, long long log_capacity, void* ws, size_t ws_bytes,
                     gx_stream_t stream);
size_t gx_image_quality_ws_bytes(int B, int C, int H, int W, int win);

/* ---- TensorBoard image grids on the device (train.py:423-476 visualise_outputs, utils/misc.py:82-98 colour_seg_masks,
 *      torchvision.utils.make_grid; genesis_amd/visualise.py).  gx_vis_compose: ONE launch fills a whole atlas -- `atlas`, a flat
 *      device buffer of atlas_words 4-byte words holding any number of grids back to back, its LAST word an unsigned overflow
 *      counter (zero before the launch) -- from n_grids descriptors of GX_VIS_DESC_WORDS int64 words each.  The descriptors
 *      (and, behind them, the pointer tables of ARGMAX_COLOUR grids) form one table of table_words words that the caller holds
 *      twice with the same contents: table_host is validated here before anything is launched, table_dev is what the kernel
 *      reads.  Descriptor words (GX_VIS_D_*):
 *        SRC0, SRC1      device addresses; STRIDE0, STRIDE1 element strides (see the kinds); every source image is contiguous
 *        DST             first atlas word of the grid;  WORK  first work item of the grid = sum over the grids before it of
 *                        ITEMS + (OWN_PAD ? Hg Wg : 0);  ITEMS  n H W / 4 when VEC else n H W
 *        KIND, N, C, H, W, K, NROW, PADDING, PAD_VALUE (the bits of a float in the low half), MODE, VEC, PACKED
 *        CELL0, N_GEOM, OWN_PAD   the N images fill the cells CELL0 .. CELL0 + N - 1 of a grid laid out for N_GEOM images;
 *                        a make_grid call is one descriptor with CELL0 = 0, N_GEOM = N, OWN_PAD = 1.  Several descriptors with
 *                        one DST, geometry and MODE compose a sheet whose cells come from different sources: exactly one of
 *                        them has OWN_PAD = 1, and every cell below N_GEOM belongs to exactly one of them.
 *      Geometry (make_grid(nrow, padding, pad_value), normalize=False): xmaps = min(NROW, N_GEOM), ymaps = ceil(N_GEOM / xmaps),
 *      p = PADDING (0 when N_GEOM == 1: the bare image, as torchvision returns it), Hg = ymaps (H + p) + p, Wg = xmaps (W + p) + p;
 *      cell i has its first pixel at row (i / xmaps)(H + p) + p, column (i % xmaps)(W + p) + p; every pixel outside the cells
 *      0 .. N_GEOM - 1 is written with PAD_VALUE by the OWN_PAD descriptor (the kernel writes the padding itself).
 *      Kinds: GX_VIS_COPY fp32 [N, C, H, W] at SRC0, image stride STRIDE0, C = 1 (written to all three channels) or 3;
 *      GX_VIS_EXP expf (the accurate one: exp(-1e10) = exp(-inf) = 0 and exp(0) = 1 exactly) of an fp32 [N, 1, H, W] plane;
 *      GX_VIS_EXP_MUL x expf(m), x [N, 3, H, W] at SRC0 / STRIDE0, m [N, 1, H, W] at SRC1 / STRIDE1, one fp32 rounding each;
 *      GX_VIS_LABEL_COLOUR int64 [N, 1, H, W] labels -> palette[label], black for a negative label, black and one more in the
 *      overflow counter for a label >= P; GX_VIS_ARGMAX_COLOUR K fp32 planes [N, 1, H, W] read in place -> argmax (ties: lowest
 *      k; a NaN ranks above every number and the first one wins, as gx_seg_metrics and torch.argmax) -> palette colour, overflow
 *      as for labels; PACKED = 1: plane k at SRC0 + k STRIDE1 floats, else SRC1 = the WORD index in the table of K device
 *      addresses; image b STRIDE0 floats further either way; GX_VIS_FILL no source: the cells hold PAD_VALUE.
 *      palette: P <= 256 RGB byte triples on the device (may be NULL when no colour kind is present).
 *      Modes: GX_VIS_FP32_CHW fp32 [3, Hg, Wg] (3 Hg Wg words; colour bytes 0..255 are exact); GX_VIS_U8_HWC bytes [Hg, Wg, 3]
 *      (ceil(3 Hg Wg / 4) words): rint(clamp(v, 0, 1) 255), half to even; colour kinds write the palette byte itself.
 *      One thread per source vector or element (16-byte loads when VEC: H W % 4 == 0, every image base 16-byte aligned --
 *      checked here --, 4-byte loads otherwise; labels always 8-byte loads), 8-byte stores where two neighbouring pixels of a
 *      row land on an 8-byte boundary (the 2-pixel padding rules out more), and one thread per grid pixel for the padding.
 *      GX_EINVAL before any launch: K outside [1, 32], C not 1 or 3, NROW < 1, negative padding, a null source, a destination
 *      range beyond the atlas, an unknown kind or mode, WORK / ITEMS / VEC that disagree with the rest of the descriptor. */
#define GX_VIS_COPY 0
#define GX_VIS_EXP 1
#define GX_VIS_EXP_MUL 2
#define GX_VIS_LABEL_COLOUR 3
#define GX_VIS_ARGMAX_COLOUR 4
#define GX_VIS_FILL 5
#define GX_VIS_FP32_CHW 0
#define GX_VIS_U8_HWC 1
#define GX_VIS_D_SRC0 0
#define GX_VIS_D_SRC1 1
#define GX_VIS_D_STRIDE0 2
#define GX_VIS_D_STRIDE1 3
#define GX_VIS_D_DST 4
#define GX_VIS_D_WORK 5
#define GX_VIS_D_ITEMS 6
#define GX_VIS_D_KIND 7
#define GX_VIS_D_N 8
#define GX_VIS_D_C 9
#define GX_VIS_D_H 10
#define GX_VIS_D_W 11
#define GX_VIS_D_K 12
#define GX_VIS_D_NROW 13
#define GX_VIS_D_PADDING 14
#define GX_VIS_D_PAD_VALUE 15
#define GX_VIS_D_MODE 16
#define GX_VIS_D_VEC 17
#define GX_VIS_D_PACKED 18
#define GX_VIS_D_CELL0 19
#define GX_VIS_D_N_GEOM 20
#define GX_VIS_D_OWN_PAD 21
#define GX_VIS_DESC_WORDS 24
int gx_vis_compose(const long long* table_host, const long long* table_dev, long long table_words, int n_grids,
                   const unsigned char* palette, int P, float* atlas, long long atlas_words, gx_stream_t stream);

/* ---- TensorBoard histograms on the device (train.py:313-325 log_distributions, :340-345 log_grads_and_weights: tensorboardX's
 *      add_histogram = numpy.histogram over a table of edges plus min / max / sum / dot, per tensor on the host;
 *      genesis_amd/histogram.py).  gx_hist_multi: ONE call histograms n_segments independent segments -- each a contiguous
 *      device array with its own length and element type -- against one shared edge table.  The descriptors, GX_HIST_DESC_WORDS
 *      int64 words each, form one table of table_words words that the caller holds twice with the same contents: table_host is
 *      validated here before anything is launched, table_dev is what the kernels read.  Descriptor words (GX_HIST_D_*):
 *        SRC    device address, aligned to its element (4 bytes for fp32, 8 for fp64: a slice of a flat buffer is a legal segment;
 *               16-byte loads from the first 16-byte boundary on, element loads before it and for what is left at the end)
 *        N      elements, 1 <= N < 2^31;  DTYPE  GX_HIST_FP32 or GX_HIST_FP64
 *        WORK   first chunk of the segment = sum over the segments before it of ceil(N / GX_HIST_CHUNK); one workgroup per chunk
 *      edges: fp64 [n_edges] on the device, strictly increasing and finite (the caller's duty: the contents are not read here),
 *      2 <= n_edges <= GX_HIST_MAX_EDGES.  fp32 values are widened to fp64 and compared with these doubles; a value's bin is found
 *      by bisection over the table's own entries.  Bin rule (numpy.histogram with explicit edges): bin i holds
 *      edges[i] <= v < edges[i + 1], the last bin also v == edges[n_edges - 1]; values below the first edge, above the last edge
 *      and NaN fall in no bin; -0.0 is 0.0.
 *      Outputs, all written here (nothing needs to be zero beforehand; counts is cleared by a memset node ahead of the launches):
 *        counts  unsigned [n_segments, n_edges - 1]
 *        stats   fp64 [n_segments, 4] = (min, max, sum, sum of squares): min and max over the non-NaN values, +-inf included
 *                (+inf, -inf for a segment of NaNs only), the sums over all non-NaN values in fp64
 *        tally   uint64 [n_segments, 3] = (NaN count, values below edges[0], values above edges[n_edges - 1])
 *      ws: gx_hist_multi_ws_bytes(total chunks) bytes, 8-byte aligned: one partial per chunk, added per segment in chunk order by
 *      a second small launch.  Counts are integer atomics (LDS, then the non-zero bins to memory); the fp64 sums go thread -> wave
 *      -> workgroup -> segment in a fixed order and through no floating-point atomic, so two calls on the same input return the
 *      same bits.  When all active lanes of a wave agree on the bin (a zero-filled segment), one lane adds their number.
 *      GX_EINVAL before any launch: a null pointer, n_segments < 1, n_edges outside [2, GX_HIST_MAX_EDGES], N < 1 or >= 2^31, an
 *      unknown DTYPE, a SRC that is null or not aligned to its element, WORK that disagrees with the prefix, a table shorter
 *      than its descriptors, a workspace that is too small. */
#define GX_HIST_FP32 0
#define GX_HIST_FP64 1
#define GX_HIST_D_SRC 0
#define GX_HIST_D_N 1
#define GX_HIST_D_DTYPE 2
#define GX_HIST_D_WORK 3
#define GX_HIST_DESC_WORDS 4
#define GX_HIST_CHUNK 8192
#define GX_HIST_MAX_EDGES 4096
size_t gx_hist_multi_ws_bytes(long long total_chunks);
int gx_hist_multi(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                  const double* edges, int n_edges, unsigned int* counts, double* stats, unsigned long long* tally, void* ws,
                  size_t ws_bytes, gx_stream_t stream);

/* ---- the device side of the TensorBoard event-file writer (genesis_amd/tbwriter.py: the import replacement of the reference's
 *      `from tensorboardX import SummaryWriter`, train.py:28).
 *      gx_scalar_snapshot: tensorboardX's add_scalar reads a device scalar with one blocking copy per call.  This copies n <=
 *      GX_SCALAR_MAX_REFS one-element device values, in stream order, into ring[first_slot .. first_slot + n) as fp64, one thread per
 *      value, by ONE launch.  `refs` is a HOST structure: its (address, dtype) pairs travel by value in the kernel arguments, so
 *      nothing is uploaded and the call never waits for the device.  dtype: GX_SCALAR_FP32 / _FP64 / _I32 / _I64 (an int64 beyond
 *      2^53 is rounded to the nearest double).  ring: fp64 [ring_slots] on the device, 8-byte aligned.
 *      GX_EINVAL before the launch: a null pointer, n outside [1, GX_SCALAR_MAX_REFS], an unknown dtype, an address that is null or
 *      not aligned to its element, slots outside the ring.
 *      gx_png_pack: ONE launch turns n_pictures pictures into the byte streams that zlib deflates for their PNGs.  Per picture
 *      H (1 + W C) bytes at out + DST: per row the filter-type byte, then the W C filtered bytes.  The descriptors,
 *      GX_PNGPACK_DESC_WORDS int64 words each, form one table of table_words words that the caller holds twice with the same
 *      contents: table_host is validated here before anything is launched, table_dev is what the kernel reads.  Descriptor words
 *      (GX_PNGPACK_D_*):
 *        SRC         device address of element (0, 0, 0), aligned to its element
 *        KIND        GX_PNGPACK_FP32: byte = trunc(clamp(x, 0, 1) * 255.0f), the product in fp32, NaN -> 0 (for x in [0, 1] what
 *                    tensorboardX publishes: (x * 255.0).astype(uint8));  GX_PNGPACK_U8: the byte itself;  GX_PNGPACK_I64: the value
 *                    clamped to 0..255
 *        C, H, W     C = 1 (grey, colour type 0) or 3 (RGB, colour type 2); 1 <= H, W <= GX_PNGPACK_MAX_DIM
 *        PIX_STRIDE, ROW_STRIDE, CH_STRIDE   in elements: pixel (y, x), channel c is element y ROW_STRIDE + x PIX_STRIDE +
 *                    c CH_STRIDE, so CHW (1, W, H W) and HWC (C, W C, 1) are read by the same kernel
 *        DST         byte offset of the picture's stream in out = sum over the pictures before it of H (1 + W C)
 *        ROW0        first global row of the picture = sum over the pictures before it of H
 *      The work item is one row, one wave per row.  The bytes of the row and of the row above are both derived from the source
 *      (row -1 and pixel -1 are zero), so rows are independent.  All five filters are computed (None, Sub with bpp = C, Up,
 *      Average = floor((a + b) / 2), Paeth with ties in the order a, b, c); the one with the smallest sum over the row of
 *      |filtered byte as a signed byte| is written, ties to the lowest filter number.
 *      GX_EINVAL before the launch: a null pointer, n_pictures < 1, a table shorter than its descriptors, an unknown KIND, C not 1
 *      or 3, H or W outside [1, GX_PNGPACK_MAX_DIM], a SRC that is null or not aligned, a stride below 1, DST or ROW0 that disagree
 *      with their prefixes, streams that do not fit out_bytes. */
#define GX_SCALAR_FP32 0
#define GX_SCALAR_FP64 1
#define GX_SCALAR_I32 2
#define GX_SCALAR_I64 3
#define GX_SCALAR_MAX_REFS 32
typedef struct {
    const void* ptr[GX_SCALAR_MAX_REFS];
    int dtype[GX_SCALAR_MAX_REFS];
} gx_scalar_refs;
int gx_scalar_snapshot(const gx_scalar_refs* refs, int n, double* ring, int ring_slots, int first_slot, gx_stream_t stream);
#define GX_PNGPACK_FP32 0
#define GX_PNGPACK_U8 1
#define GX_PNGPACK_I64 2
#define GX_PNGPACK_D_SRC 0
#define GX_PNGPACK_D_KIND 1
#define GX_PNGPACK_D_C 2
#define GX_PNGPACK_D_H 3
#define GX_PNGPACK_D_W 4
#define GX_PNGPACK_D_PIX_STRIDE 5
#define GX_PNGPACK_D_ROW_STRIDE 6
#define GX_PNGPACK_D_CH_STRIDE 7
#define GX_PNGPACK_D_DST 8
#define GX_PNGPACK_D_ROW0 9
#define GX_PNGPACK_DESC_WORDS 12
#define GX_PNGPACK_MAX_DIM 4096
int gx_png_pack(const long long* table_host, const long long* table_dev, long long table_words, int n_pictures, unsigned char* out,
                long long out_bytes, gx_stream_t stream);

/* ---- FID on the device (scripts/compute_fid.py + third_party/pytorch_fid; genesis_amd/fid.py): pytorch_fid's FID Inception
 *      (Inception-v3, BatchNorm folded into the conv weights by the caller) on NHWC fp32 activations, and the moments of its
 *      features.  Every output's reduction order is fixed by the layer shape alone (no split-K, no atomics), so an image's
 *      features are bit-identical whatever batch, batch size or position it is computed in.
 *      gx_fid_preprocess: fp32 images [B, 3, H, W] in [0, 1] -> the network input [B, 299, 299, 3] (NHWC): quantise != 0
 *      first restates the reference's PNG round trip per pixel, float32(uint8(clamp(255 x, 0, 255))) / 255 (the float32
 *      product, truncated); then torch's CPU bilinear resize to 299 x 299 (align_corners=False) and 2x - 1.
 *      gx_fid_conv_bias_relu: y = relu(conv(x, w) + bias) on the fp32 matrix pipe, x [B, H, W, Cin], any kh x kw, one
 *      stride, padding (ph, pw); Ho = (H + 2 ph - kh) / stride + 1.  The output channels are N = n0 + n1 + n2 (sibling
 *      convs of the same input stacked along N; n1 = n2 = 0 for one conv): channel n < n0 goes to channel d0_c0 + n of
 *      d0 [B, Ho, Wo, d0_ctot], the next n1 to d1 from d1_c0, the last n2 to d2 from d2_c0.  w is the packed weight
 *      [roundup(N, 64)][roundup(kh kw Cin, 16)], zero-padded, with k = (r kw + s) Cin + c; bias [N].
 *      gx_fid_pool: x [B, H, W, C] -> channels [y_c0, y_c0 + C) of y [B, Ho, Wo, y_ctot] by mode: GX_FID_MAXPOOL_S2
 *      (3 x 3, stride 2, no padding), GX_FID_MAXPOOL_S1P1 (3 x 3, stride 1, padding 1), GX_FID_AVGPOOL_S1P1 (3 x 3,
 *      stride 1, padding 1, count_include_pad=False), GX_FID_GLOBAL_AVGPOOL (Ho = Wo = 1).
 *      gx_fid_moments: adds sum_b f[b] into sum [D] and sum_b f[b] f[b]^T into sumsq [D, D] (fp64, images added one by one
 *      in order: bit-reproducible and independent of how the images are split into batches); feats fp32 [B, D]. */
#define GX_FID_MAXPOOL_S2 0
#define GX_FID_MAXPOOL_S1P1 1
#define GX_FID_AVGPOOL_S1P1 2
#define GX_FID_GLOBAL_AVGPOOL 3
int gx_fid_preprocess(const float* x, float* y, int B, int H, int W, int quantise, gx_stream_t stream);
int gx_fid_conv_bias_relu(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, int kh, int kw,
                          int stride, int ph, int pw, float* d0, int d0_ctot, int d0_c0, int n0, float* d1, int d1_ctot,
                          int d1_c0, int n1, float* d2, int d2_ctot, int d2_c0, int n2, gx_stream_t stream);
int gx_fid_pool(const float* x, int B, int H, int W, int C, int mode, float* y, int y_ctot, int y_c0, gx_stream_t stream);
int gx_fid_moments(const float* feats, int B, int D, double* sum, double* sumsq, gx_stream_t stream);

/* ---- sample quality beside FID (genesis_amd/sample_quality.py; gx_manifold.hip): the all-pairs work of improved precision /
 *      recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and KID (Binkowski et al. 2018) over fp32
 *      feature rows [rows, D], in fp64, with no rows x rows matrix in memory.  D is a multiple of 4 in [4, 8192]; feature
 *      pointers and workspaces are 16-byte aligned; at most 2^21 rows per operand.
 *      d2(a, b) = sum_d (a_d - b_d)^2: each feature converted to fp64, the difference formed first, the terms added by one
 *      fma chain over d = 0 .. D-1.  The order depends on D alone, so d2(a, b) has the same bits in every launch, at every
 *      tile position and in either argument order, and identical rows give exactly 0: exact ties compare as <=.
 *      gx_knn_radii: radii2[i] = the k-th smallest of {d2(x_i, x_j) : j != i} (self excluded by index, duplicates counted
 *      with multiplicity, no square root), X [N, D], 1 <= k <= 8, k <= N - 1; ws of gx_knn_radii_ws_bytes(N, k) bytes
 *      (ceil(N / 64) k N doubles: the k smallest of every 64-column tile, merged by a second launch).
 *      gx_manifold_counts: hits[j] = #{i : d2(q_j, r_i) <= radii2[i]} for Q [M, D] against R [N, D] with the radii of R's
 *      rows; covered[i] = 1 if any j satisfies that inequality for i, else 0.  Both outputs are written in full (cleared by
 *      the call; int32 atomics, whose result does not depend on order).  (Q = generated, R = real) gives precision
 *      (hits > 0), density (sum hits) and coverage (covered); (Q = real, R = generated) gives recall.
 *      gx_kid_sums: for each of S subsets s of m rows, x_a = X[ix[s m + a]] (X [NX, D]) and y_b = Y[iy[s m + b]] (Y [NY, D]),
 *      with kappa(x, y) = (x . y / D + 1)^3: sums[s] = (sum_{a != b} kappa(x_a, x_b), sum_{a != b} kappa(y_a, y_b),
 *      sum_{a, b} kappa(x_a, y_b)).  ix / iy are device int32 [S, m] that the caller has checked against [0, NX) / [0, NY)
 *      (the kernel clamps an index into the range instead of reading outside).  2 <= m <= 65536, 1 <= S <= 21845; ws of
 *      gx_kid_sums_ws_bytes(m, S) bytes.  Fixed summation order, no floating-point atomics: a repeat gives the same bits.
 *      The *_ws_bytes queries return 0 for arguments the calls refuse.  Non-finite features give unspecified values. */
size_t gx_knn_radii_ws_bytes(int N, int k);
int gx_knn_radii(const float* X, int N, int D, int k, double* radii2, void* ws, size_t ws_bytes, gx_stream_t stream);
int gx_manifold_counts(const float* Q, int M, const float* R, int N, int D, const double* radii2, int* hits, int* covered,
                       gx_stream_t stream);
size_t gx_kid_sums_ws_bytes(int m, int S);
int gx_kid_sums(const float* X, int NX, const int* ix, const float* Y, int NY, const int* iy, int m, int D, int S, double* sums,
                void* ws, size_t ws_bytes, gx_stream_t stream);

/* ---- input feeder (datasets/multid_config.py:131-135 ToTensor + F.interpolate(size), multi_object_config.py:176-186):
 *      uint8 frames [B, Hs, Ws, C] (HWC, as stored) -> fp32 [B, C, H, W] = value / 255, nearest-neighbour resampled to
 *      H x W when the stored size differs (F.interpolate's default mode).  Bit-exact against the torch ops. */
int gx_u8hwc_to_f32chw(const unsigned char* src, float* dst, int B, int Hs, int Ws, int C, int H, int W,
                       gx_stream_t stream);

/* ---- feeder transforms of the other datasets (datasets/shapestacks_config.py:126-130 CenterCrop + PIL Resize + ToTensor,
 *      :155-162 instance maps; datasets/multi_object_config.py:181-202 CLEVR centre crop + nearest F.interpolate):
 *      gx_u8hwc_resample_f32chw: uint8 [B, Hs, Ws, C] -> fp32 [B, C, H, W] = value / 255 of the crop window (top, left, Hc, Wc)
 *      resampled to H x W; the resample sees the window as the whole image.  mode GX_RESAMPLE_NEAREST: F.interpolate's
 *      nearest rule (the full-frame window computes what gx_u8hwc_to_f32chw does; the tables may be null).
 *      GX_RESAMPLE_PIL_BILINEAR: Pillow's 8-bit two-pass BILINEAR resampler (what torchvision's Resize does to a PIL image),
 *      bit-exact; {h,v}bounds / {h,v}weights are DEVICE copies of gx_pil_bilinear_coeffs(Wc, W, ...) / (Hc, H, ...), with
 *      ksize gx_pil_bilinear_ksize of the same sizes.  Any width and height; the downscale ratio r and channel count C are
 *      bounded by the kernel's fixed LDS band buffers (16 KB intermediate + 32 KB staged source rows): about
 *      (2r + 2)^2 x C source bytes must fit 32 KB, so up to r = 84 / 49 / 43 / 16 for C = 1 / 3 / 4 / 27 (at r = 16, at
 *      most 27 channels); beyond that the call fails with GX_EINVAL ("exceeds the kernel's band buffers").  Bit-exact
 *      against Pillow for 'L' (C = 1) and 'RGB' (C = 3) images and for opaque 'RGBA' (C = 4, alpha 255): Pillow
 *      premultiplies RGBA by alpha around the resample, which this kernel does not do.
 *      gx_pil_bilinear_ksize / gx_pil_bilinear_coeffs (host only, no GPU): Pillow's coefficient tables of one axis, computed in
 *      double: bounds int32 [out][2] = (first source index, tap count), weights int32 [out][ksize] with 22 fractional bits.
 *      gx_pil_bilinear_ksize returns 0 for a non-positive size.
 *      gx_labels_crop_nearest: integer label maps [B, Hs, Ws] (dtype GX_LABEL_U8 / _I32 / _I64) -> int64 [B, 1, H, W],
 *      nearest inside the crop window; equals the reference's F.interpolate(cropped.float()[:, None], size).long() for
 *      every label an fp32 holds exactly (negative ignore labels included). */
#define GX_RESAMPLE_NEAREST 0
#define GX_RESAMPLE_PIL_BILINEAR 1
#define GX_LABEL_U8 0
#define GX_LABEL_I32 1
#define GX_LABEL_I64 2
int gx_pil_bilinear_ksize(int in, int out);
int gx_pil_bilinear_coeffs(int in, int out, int ksize, int* bounds, int* weights);
int gx_u8hwc_resample_f32chw(const unsigned char* src, float* dst, int B, int Hs, int Ws, int C, int top, int left, int Hc,
                             int Wc, int H, int W, int mode, const int* hbounds, const int* hweights, int hksize,
                             const int* vbounds, const int* vweights, int vksize, gx_stream_t stream);
int gx_labels_crop_nearest(const void* src, int dtype, long long* dst, int B, int Hs, int Ws, int top, int left, int Hc, int Wc,
                           int H, int W, gx_stream_t stream);

/* ---- Multi-dSprites on the device (datasets/multid_config.py:113-143 dSpritesDataset; scripts/generate_multid.py:37-76).
 *      The stored split ([N, 64, 64, 3] float32 already / 255, or uint8; label maps [N, 64, 64] in any of five dtypes) is
 *      resident in device memory; a batch is a gather of B of its rows, the rows idx[first .. first + B) of a DEVICE index
 *      vector of idx_len int64 entries (an epoch's permutation), or, with idx NULL, the rows first .. first + B themselves
 *      (a staged batch).  N is the row count of src.  first + B must not pass idx_len (without idx: N); the VALUES of idx
 *      are not looked at by the library: the caller checks them against [0, N) before it uploads them.
 *      gx_rows_gather_f32chw: src [N, Hs, Ws, C] (dtype GX_ROWS_U8: value / 255, a true fp32 division as in
 *      gx_u8hwc_to_f32chw; GX_ROWS_F32: copied unchanged) -> dst fp32 [B, C, H, W], resampled nearest with
 *      gx_u8hwc_to_f32chw's index rule when (H, W) != (Hs, Ws): ToTensor + F.interpolate(size) (multid_config.py:131-135).
 *      gx_rows_gather_labels: src [N, Hs, Ws] (GX_LABEL_U8 / _I32 / _I64 / _F32 / _F64) -> dst int64 [B, 1, H, W], the same
 *      nearest rule and a truncating conversion: what ToTensor + F.interpolate + .type(LongTensor) leave
 *      (multid_config.py:137-143) for every label a float holds exactly.
 *      gx_sprites_compose: the loop body of generate_multid.py:47-73 for n images.  sprites uint8 [S, 64, 64] (non-zero =
 *      set, as np.array(..., dtype=bool)); image i pastes the count[i] (0..4) consecutive sprites from first[i], in that
 *      order; colours uint8 [n, 5, 3] = background, then the objects.  img fp32 [n, 64, 64, 3] = byte / 255 and mask uint8
 *      [n, 64, 64]: a pixel takes the colour and the label o + 1 of the LAST sprite o that covers it, else the background
 *      colour and 0.  first / count / colours are device arrays; the caller checks first[i] + count[i] <= S. */
#define GX_ROWS_U8 0
#define GX_ROWS_F32 1
#define GX_LABEL_F32 3
#define GX_LABEL_F64 4
int gx_rows_gather_f32chw(const void* src, int dtype, long long N, const long long* idx, long long idx_len, long long first,
                          float* dst, int B, int Hs, int Ws, int C, int H, int W, gx_stream_t stream);
int gx_rows_gather_labels(const void* src, int dtype, long long N, const long long* idx, long long idx_len, long long first,
                          long long* dst, int B, int Hs, int Ws, int H, int W, gx_stream_t stream);
int gx_sprites_compose(const unsigned char* sprites, int S, const int* first, const int* count, const unsigned char* colours,
                       float* img, unsigned char* mask, int n, gx_stream_t stream);

/* ---- the multi-object TFRecord datasets without TensorFlow (datasets/multi_object_config.py, third_party/multi_object_datasets:
 *      ObjectsRoom, CLEVR with masks, Tetrominoes, Multi-dSprites).  The first four are host only (no GPU, no stream):
 *      gx_crc32c: CRC-32C (Castagnoli) of n bytes; gx_crc32c_masked: TFRecord's masked form ((c >> 15) | (c << 17)) + 0xa282ead8.
 *      gx_tfrecord_scan: the complete records in buf[0..n) of a stream framed as u64 length | u32 masked crc of the length |
 *      data | u32 masked crc of the data: offsets[k] / lengths[k] of the data of up to max_records records, *num_records of
 *      them, and *consumed = the bytes they occupy from the start of buf.  A trailing partial record is not an error: the
 *      caller appends more of the stream and scans again.  Both checksums are verified unless verify_crc is 0; a mismatch
 *      returns GX_EDATA and the message names the record as first_index + k.
 *      gx_tfexample_find_bytes_list: walks one tf.Example (features(1) -> map entries (key 1, value 2) -> bytes_list(1)) and
 *      returns the span of the BytesList payload of feature `name` inside rec[0..n); every other field is skipped by wire
 *      type (float_list, packed or not, int64_list, unknown fields).  GX_EDATA: no such feature, not a bytes_list, or a
 *      varint / length that runs past the record (never an over-read).
 *      gx_bytes_list_unpack: the concatenated values of a BytesList payload into dst[0..expected); a list of one-byte values
 *      (a strict 0A 01 vv stride) takes a fast path.  GX_EDATA unless the values total exactly `expected` bytes.
 *      gx_entity_masks_to_labels: a uint8 entity-mask stack of B frames -> int64 instance maps [B, 1, H, W]:
 *      label(p) = max{ o + 1 : o >= background_entities, mask[o, p] == 255 }, 0 if there is none -- what the reference's
 *      overwrite loop over entities leaves (multi_object_config.py:188-203) -- of the crop window (top, left, Hc, Wc) resampled
 *      nearest to H x W with gx_labels_crop_nearest's index rule.  mask[b, o, y, x] is the byte at
 *      b * E * Hs * Ws + o * entity_stride + (y * Ws + x) * pixel_stride, so both stored layouts are read in place:
 *      [E, Hs, Ws] (entity_stride Hs * Ws, pixel_stride 1) and [Hs, Ws, E] (entity_stride 1, pixel_stride E); every offset
 *      must stay inside a frame's E * Hs * Ws bytes. */
unsigned int gx_crc32c(const void* data, size_t n);
unsigned int gx_crc32c_masked(const void* data, size_t n);
int gx_tfrecord_scan(const unsigned char* buf, size_t n, int verify_crc, long long first_index, int max_records,
                     long long* offsets, long long* lengths, int* num_records, size_t* consumed);
int gx_tfexample_find_bytes_list(const unsigned char* rec, size_t n, const char* name, long long* offset, long long* length);
int gx_bytes_list_unpack(const unsigned char* payload, size_t n, unsigned char* dst, size_t expected);
int gx_entity_masks_to_labels(const unsigned char* masks, long long* dst, int B, int E, int Hs, int Ws, long long entity_stride,
                              long long pixel_stride, int background_entities, int top, int left, int Hc, int Wc, int H, int W,
                              gx_stream_t stream);

/* ---- GQN's JPEG frames without TensorFlow (datasets/gqn_config.py, third_party/tf_gqn/gqn_tfr_provider.py:141-143:
 *      tf.image.decode_jpeg + convert_image_dtype).  Baseline JPEG split in two: the serial part (markers, Huffman codes) on
 *      the host, everything that touches a pixel in one kernel.  The first three are host only (no GPU, no stream).
 *      gx_bytes_list_index: offsets[k] / lengths[k] of every value of a BytesList payload (GQN's `frames`: ten JPEG strings of
 *      different lengths), *count of them; GX_EDATA when the list holds more than max_values or a length runs past the payload.
 *      gx_jpeg_info: the geometry of one stream, info[8] = width, height, components (3), sampling class (0 = 4:4:4,
 *      1 = 4:2:2 / chroma h2v1, 2 = 4:2:0 / chroma h2v2), blocks of the Y, Cb and Cr planes, restart interval.  A plane is
 *      padded to whole MCUs.
 *      gx_jpeg_entropy_decode: the same info, plus coef = per component the blocks of its padded plane in raster order (Y, then
 *      Cb, then Cr), each 64 QUANTISED int16 coefficients in natural (row-major) order with the DC prediction undone
 *      (coef_capacity counts int16 values), and qtab = three 64-entry tables, one per component, natural order.
 *      Accepted: SOF0, 8-bit samples, three components in one interleaved scan, luma 1x1 / 2x1 / 2x2 with chroma 1x1, 8-bit
 *      quantisation tables, any Huffman tables, DRI / RSTn, byte stuffing; APPn and COM are skipped.  GX_EDATA, with a message
 *      that names the case, for: progressive / extended SOF, arithmetic coding, one or four components, other sampling
 *      factors, 16-bit tables, frames above 128 x 128, a code that is not in its table, a coefficient index past 63, a
 *      stream that ends early.  No input makes them read or write out of bounds.
 *      gx_jpeg_decode_f32chw: B frames of one size H x W (<= 128 x 128) and one sampling class, coef [B][blocks][64] and qtab
 *      [B][3][64] on the device (16-byte aligned) -> dst_f32 [B, 3, S_h, S_w] = u8 * (1.0f / 255.0f) (TensorFlow's
 *      convert_image_dtype), resampled with F.interpolate's nearest index when (S_h, S_w) != (H, W), and / or dst_u8
 *      [B, H, W, 3] at the stored size; either may be NULL.  One launch, one workgroup per frame: dequantisation, the 13-bit
 *      fixed-point inverse DCT (columns, then rows), triangle-filter chroma upsampling and the 16-bit fixed-point YCbCr -> RGB
 *      conversion of libjpeg's default decoding path, bit for bit. */
int gx_bytes_list_index(const unsigned char* payload, size_t n, int max_values, long long* offsets, long long* lengths, int* count);
int gx_jpeg_info(const unsigned char* data, size_t len, int* info);
int gx_jpeg_entropy_decode(const unsigned char* data, size_t len, short* coef, size_t coef_capacity, unsigned short* qtab,
                           int* info);
int gx_jpeg_decode_f32chw(const short* coef, const unsigned short* qtab, float* dst_f32, unsigned char* dst_u8, int B, int H, int W,
                          int sampling, int S_h, int S_w, gx_stream_t stream);

/* ---- PNG frames without Pillow (datasets/shapestacks_config.py:141, datasets/sketchy_config.py:91: Image.open; ShapeStacks'
 *      .map files are PNGs too).  Split like the JPEG path: the serial part (chunk walk, CRC-32, zlib inflate) on the host,
 *      everything that touches a pixel on the device.  The first two are host only (no GPU, no stream); inflate and CRC-32 are
 *      zlib's, resolved from libz.so.1 at first use (GX_EINVAL with a message that says so when it is missing).
 *      gx_png_info: the geometry of one stream from its signature and IHDR, info[8] = width, height, channels C, bytes per
 *      pixel (= C), colour type, bit depth, interlace flag, inflated size H * (1 + W * C).
 *      gx_png_inflate: the same info, and dst[0 .. H * (1 + W * C)) = the inflated IDAT data, STILL FILTERED: per row one filter
 *      byte and W * C bytes.  Checks the signature, walks the chunks, verifies every chunk's CRC-32, concatenates the IDAT
 *      payloads, requires the inflated size to be exact and every filter byte to be at most 4.  dst_capacity counts bytes.
 *      Accepted: 8-bit samples, not interlaced, colour type 0 (grey, C = 1), 2 (RGB, C = 3) or 6 (RGBA, C = 4); ancillary
 *      chunks and a suggested palette are skipped.  GX_EDATA, with a message that names the case, for: 16-bit samples, samples
 *      under 8 bits, palette, grey+alpha, Adam7 interlacing, a CRC mismatch (the message names the chunk), a missing IHDR,
 *      IDAT or IEND, IDAT chunks that are not consecutive, a stream that ends early, an unknown critical chunk, an inflated size other than the expected one, a
 *      filter byte above 4, frames above 4096 x 4096 (the kernel's bound).  No input makes them read or write out of bounds.
 *      gx_png_unfilter: B frames of one geometry, filtered [B][H * (1 + W * C)] on the device as gx_png_inflate leaves them ->
 *      dst_u8 [B, H, W, C], the bytes reconstructed from the five filters (None, Sub, Up, Average = floor((a + b) / 2) on
 *      9-bit sums, Paeth with ties in the order a, b, c; per byte, the left neighbour C bytes back, 0 outside the frame),
 *      and / or dst_plane0 [B, H, W] = channel 0 of every pixel after plane_rule: GX_PNG_PLANE_BYTE the byte itself,
 *      GX_PNG_PLANE_SHAPESTACKS_REF what the reference makes of a ShapeStacks map ((byte / 255.0f) / 32 truncated
 *      (third_party/shapestacks/segmentation_utils.py:38-41 and .long()): 0 for every byte), GX_PNG_PLANE_INDEX byte >> 5.
 *      Either may be NULL.  One launch, one workgroup per frame: a skewed wavefront over bands of 1024 / C rows, thread =
 *      (row, channel byte), neighbouring rows handing values over by cross-lane moves and, between waves, through LDS; the
 *      frame stays in global memory.  H and W at most 4096, C = 1, 3 or 4. */
#define GX_PNG_PLANE_BYTE 0
#define GX_PNG_PLANE_SHAPESTACKS_REF 1
#define GX_PNG_PLANE_INDEX 2
int gx_png_info(const unsigned char* data, size_t len, int* info);
int gx_png_inflate(const unsigned char* data, size_t len, unsigned char* dst, size_t dst_capacity, int* info);
int gx_png_unfilter(const unsigned char* filtered, unsigned char* dst_u8, unsigned char* dst_plane0, int plane_rule, int B, int H,
                    int W, int C, gx_stream_t stream);

/* ---- loose image files: JPEG and PNG frames of ANY size, mixed within one batch (genesis_amd/imagefile.py; the reference's users
 *      point torchvision's ImageFolder-style loaders at a directory, datasets/apc_config.py:144-147: Resize, CenterCrop).
 *      Host half (no GPU, no stream), sharing the marker walk and the Huffman code of the two entry points above:
 *      gx_jpeg_info_any / gx_jpeg_entropy_decode_any: as gx_jpeg_info / gx_jpeg_entropy_decode, with two limits moved: frames up
 *      to 4096 x 4096 (the PNG bound), and ONE-component (greyscale) streams beside three-component ones.  info[2] is the
 *      component count, 1 or 3; a grey frame has one plane, padded to whole 8 x 8 blocks whatever its sampling factors say
 *      (info[3] = 0, info[5] = info[6] = 0), and qtab receives its one table three times: 192 values are always written.
 *      Accepted: SOF0, 8-bit samples, one component, or three in one interleaved scan with luma 1x1 / 2x1 / 2x2 and chroma
 *      1x1, 8-bit quantisation tables, any Huffman tables, DRI / RSTn, byte stuffing; APPn and COM are skipped.  GX_EDATA, with
 *      a message that names the case, for: progressive / extended SOF, arithmetic coding, four components (CMYK / YCCK), two
 *      components, other sampling factors (4:4:0, 4:1:1 among them), 16-bit tables, a three-component frame whose scan is not
 *      interleaved, frames above 4096 x 4096, a code that is not in its table, a coefficient index past 63, a stream that ends
 *      early.  No input makes them read or write out of bounds; coef is written only below coef_capacity.
 *      Device half: every entry point takes a per-frame descriptor table of n_frames * WORDS 64-bit words twice, the way
 *      gx_png_pack does: table_host is checked word by word before anything is launched (a bad word: GX_EINVAL, nothing
 *      launched), table_dev is the device copy the kernels read.  Offsets count elements of the array they index.
 *      gx_jpeg_decode_ragged: coefficients as the host half leaves them -> dst_u8, per frame a region [H, W, 3] (RGB) or
 *      [H, W] (grey).  Descriptor (GX_JPEGR_DESC_WORDS): H, W, NCOMP (1 or 3), SAMPLING (class; 0 for grey), COEF (index of the
 *      frame's first int16 in coef, a multiple of 8), QTAB (index of its 192 uint16 in qtab, a multiple of 8), PLANES (byte
 *      offset of its padded uint8 planes in scratch, a multiple of 16: 64 bytes per block), DST (byte offset in dst_u8),
 *      WG0_IDCT / WG0_PIX (its first workgroup in the two launches: the running sums of ceil(blocks / GX_JPEGR_BLOCKS_PER_WG)
 *      and of ceil(H / GX_JPEGR_TILE_H) * ceil(W / GX_JPEGR_TILE_W)).  coef, qtab and scratch are 16-byte aligned.  Two
 *      launches: blocks -> planes in scratch, planes -> pixels; the arithmetic is gx_jpeg_decode_f32chw's (one shared
 *      definition), at a frame's real edge the chroma neighbour is the edge sample.  No frame-sized LDS.
 *      gx_png_unfilter_ragged: frames as gx_png_inflate leaves them -> dst_u8 regions [H, W, C]; gx_png_unfilter's kernel, one
 *      workgroup per frame.  Descriptor (GX_PNGR_DESC_WORDS): H, W, C (1, 3 or 4), SRC (byte offset in filtered), DST (byte
 *      offset in dst_u8).  H and W at most 4096.
 *      gx_u8_resample_ragged_f32chw: per frame the uint8 [HS, WS, C] region at SRC of src is resized WHOLE to H2 x W2 with
 *      Pillow's two-pass 8-bit BILINEAR (horizontal pass first, into a uint8 intermediate) and the window of S_h x S_w pixels
 *      at (top', left') of that resized frame is written: dst [n_frames, 3, S_h, S_w] fp32 = byte / 255.  Only the window's
 *      rows and columns are computed: HB / HW / VB / VW are indices into `tables` (int32) of the rows of
 *      gx_pil_bilinear_coeffs(WS, W2) from left' on (S_w rows: bounds [S_w, 2], weights [S_w, KH]) and of
 *      gx_pil_bilinear_coeffs(HS, H2) from top' on (S_h rows), KH / KV their ksize.  C = 1 is replicated to three planes, the
 *      alpha of C = 4 is dropped (Pillow's convert('RGB')).  A pass whose size does not change copies (Pillow's table is then
 *      the identity).  S_h and S_w are at most 1024.  R and WG0 (rows of a band of the frame, its first workgroup) are
 *      written into the HOST table by gx_u8_resample_ragged_plan (host only), which must run before the table is copied to
 *      the device; the launch checks them.  Descriptor (GX_RSR_DESC_WORDS): HS, WS, C, SRC, H2, W2, HB, HW, KH, VB, VW, KV, R,
 *      WG0. */
#define GX_JPEGR_DESC_WORDS 10
#define GX_JPEGR_D_H 0
#define GX_JPEGR_D_W 1
#define GX_JPEGR_D_NCOMP 2
#define GX_JPEGR_D_SAMPLING 3
#define GX_JPEGR_D_COEF 4
#define GX_JPEGR_D_QTAB 5
#define GX_JPEGR_D_PLANES 6
#define GX_JPEGR_D_DST 7
#define GX_JPEGR_D_WG0_IDCT 8
#define GX_JPEGR_D_WG0_PIX 9
#define GX_JPEGR_BLOCKS_PER_WG 128
#define GX_JPEGR_TILE_H 16
#define GX_JPEGR_TILE_W 64
#define GX_PNGR_DESC_WORDS 5
#define GX_PNGR_D_H 0
#define GX_PNGR_D_W 1
#define GX_PNGR_D_C 2
#define GX_PNGR_D_SRC 3
#define GX_PNGR_D_DST 4
#define GX_RSR_DESC_WORDS 14
#define GX_RSR_D_HS 0
#define GX_RSR_D_WS 1
#define GX_RSR_D_C 2
#define GX_RSR_D_SRC 3
#define GX_RSR_D_H2 4
#define GX_RSR_D_W2 5
#define GX_RSR_D_HB 6
#define GX_RSR_D_HW 7
#define GX_RSR_D_KH 8
#define GX_RSR_D_VB 9
#define GX_RSR_D_VW 10
#define GX_RSR_D_KV 11
#define GX_RSR_D_R 12
#define GX_RSR_D_WG0 13
int gx_jpeg_info_any(const unsigned char* data, size_t len, int* info);
int gx_jpeg_entropy_decode_any(const unsigned char* data, size_t len, short* coef, size_t coef_capacity, unsigned short* qtab,
                               int* info);
int gx_jpeg_decode_ragged(const long long* table_host, const long long* table_dev, int n_frames, const short* coef, long long coef_values,
                          const unsigned short* qtab, long long qtab_values, unsigned char* scratch, long long scratch_bytes,
                          unsigned char* dst_u8, long long dst_bytes, gx_stream_t stream);
int gx_png_unfilter_ragged(const long long* table_host, const long long* table_dev, int n_frames, const unsigned char* filtered,
                           long long filtered_bytes, unsigned char* dst_u8, long long dst_bytes, gx_stream_t stream);
int gx_u8_resample_ragged_plan(long long* table_host, int n_frames, int S_h, int S_w, long long* workgroups);
int gx_u8_resample_ragged_f32chw(const long long* table_host, const long long* table_dev, int n_frames, const unsigned char* src,
                                 long long src_bytes, const int* tables, long long tables_values, float* dst, int S_h, int S_w,
                                 gx_stream_t stream);

/* ---- a loader's decoded split kept on the device (genesis_amd/data_cache.py; gx_cache.hip).  The store is planar: frames
 *      uint8 [rows][C * H * W] in CHW order, labels int16 [rows][H * W]; row_stride is in BYTES, a multiple of 16 and at least
 *      a row, and the store is 16-byte aligned, so every row starts 16-byte aligned.  Pad bytes between a row's end and the
 *      next row are never written by a store and never read by a gather.  counters: three int64 device words (8-byte
 *      aligned) = div_miss, mul_miss, label_misfit; the kernels ADD to them (one atomic per block and non-zero counter), the
 *      caller zeroes them.
 *      gx_cache_store_u8: batch fp32 [B, C, H, W] -> rows first_row .. first_row + B (which must not pass capacity_rows) as
 *      q = clamp(rintf(v * 255.0f), 0, 255), NaN -> 0.  div_miss counts the values whose bits differ from (float)q / 255.0f,
 *      mul_miss those whose bits differ from (float)q * (1.0f / 255.0f); a NaN, a value outside [0, 1] and -0.0f count as both.
 *      gx_cache_store_labels_i16: labels int64 [B, 1, H, W] -> (int16)v; label_misfit counts the values outside
 *      -32768 .. 32767 (they are stored truncated: the count is what tells).  Negative labels survive.
 *      gx_cache_gather_f32: out fp32 [B, C, H, W] = the rows idx[first .. first + B) of a store of `rows` rows (idx: DEVICE
 *      vector of idx_len int64 entries; NULL: the rows first .. first + B themselves), each byte q as (float)q / 255.0f
 *      (GX_CACHE_DIV255) or (float)q * (1.0f / 255.0f) (GX_CACHE_MUL255).  first + B must not pass idx_len (without idx:
 *      rows); as with gx_rows_gather_f32chw the VALUES of idx are the caller's to check against [0, rows) on the host.
 *      gx_cache_gather_labels: the same rows of an int16 store -> out int64 [B, 1, H, W], sign-extended.
 *      B is at most 65535 and a row holds fewer than 2^31 values.  One launch each on `stream`, nothing else. */
#define GX_CACHE_DIV255 0
#define GX_CACHE_MUL255 1
int gx_cache_store_u8(const float* batch, unsigned char* store, long long row_stride, long long first_row,
                      long long capacity_rows, long long* counters, int B, int C, int H, int W, gx_stream_t stream);
int gx_cache_store_labels_i16(const long long* labels, short* store, long long row_stride, long long first_row,
                              long long capacity_rows, long long* counters, int B, int H, int W, gx_stream_t stream);
int gx_cache_gather_f32(const unsigned char* store, long long row_stride, long long rows, const long long* idx, long long idx_len,
                        long long first, int mode, float* out, int B, int C, int H, int W, gx_stream_t stream);
int gx_cache_gather_labels(const short* store, long long row_stride, long long rows, const long long* idx, long long idx_len,
                           long long first, long long* out, int B, int H, int W, gx_stream_t stream);

/* ---- augmented batches from the same stores in ONE launch (genesis_amd/augment.py; gx_cache.hip): out fp32 [B, C, H, W] and,
 *      when labels is not NULL, out_labels int64 [B, 1, H, W] = the rows idx[first .. first + B) of a frame store and of a label
 *      store of `rows` rows each (strides in bytes, as above), every frame flipped, cropped, resampled back to H x W and scaled
 *      by a gain, its label map moved by the same geometry.  What follows is the normative text of the transform, "augment v1";
 *      tests/augment_restatement.py restates it in numpy and the kernel is tested against that bit for bit.
 *
 *      Random words.  All of them come from Philox4x32-10 (gx_philox.h).  For the frame of cache row r (the VALUE idx[first + b],
 *      or first + b without idx: not the position in the batch) in resident epoch e with seed s:
 *        key = (s & 0xffffffff, s >> 32);  call A: counter (r & 0xffffffff, r >> 32, e & 0xffffffff, 0xA06) -> r0 r1 r2 r3;
 *        call B: the same counter with last word 0xA07 -> r4 r5 r6 r7.
 *      t(x) = x >> 8 is a word's 24-bit integer, u(x) = float(t(x)) * 2^-24 (exact) the number in [0, 1).
 *      Flip.  The frame is mirrored left to right iff t(r0) < flip_t; the host passes flip_t = round(p_flip * 2^24), 0 .. 2^24.
 *      Scale crop, aspect ratio kept, all in integers with 64-bit products; the host passes wmin = max(1, ceil(min_side * W)):
 *        w = wmin + ((t(r1) * (W - wmin + 1)) >> 24);       h = clamp((w * H + W / 2) / W, 1, H)   (integer division);
 *        x0 = (t(r2) * (W - w + 1)) >> 24;                  y0 = (t(r3) * (H - h + 1)) >> 24.
 *      Resample.  The window [y0, y0 + h) x [x0, x0 + w) is resampled to H x W with half-pixel centres.  For output column x,
 *      with x' = W - 1 - x when flipped and x' = x otherwise:
 *        s = (2 * x' + 1) * w - W;   i0 = floor(s / 2W);   rem = s - i0 * 2W;   fx = float(rem) / float(2W), ONE correctly
 *        rounded fp32 division;   i1 = i0 + 1;   i0 and i1 are then clamped to [0, w - 1].
 *      Rows likewise with h, H: j0, j1, fy.  With a.. the bytes at window positions (j0, i0), (j0, i1), (j1, i0), (j1, i1) of the
 *      channel's plane, converted to fp32:
 *        top = a00 + (a01 - a00) * fx;   bot = a10 + (a11 - a10) * fx;   v = top + (bot - top) * fy
 *      with EVERY operation rounded to fp32 on its own (no fused multiply-add).  Labels take the nearest value of the same
 *      window: window column ((2 * x' + 1) * w) / (2W), window row ((2 * y + 1) * h) / (2H), integer divisions.
 *      Gain.  With brightness b and colour c in [0, 1):  g = 1 + b * (2 * u(r4) - 1);  for channel ch < C (C <= 3):
 *        g_ch = g * (1 + c * (2 * u(r[5 + ch]) - 1)), that is r5, r6, r7 for channels 0, 1, 2;   v = min(v * g_ch, 255.0f),
 *      again every operation rounded on its own (2 * u - 1 is exact).  Labels take no gain.
 *      Conversion, last, by the store's mode exactly as gx_cache_gather_f32: v / 255.0f (GX_CACHE_DIV255) or
 *      v * (1.0f / 255.0f) (GX_CACHE_MUL255).
 *      Identities this form gives (the tests lean on them): w == W gives fx == 0 and i0 == x', hence the byte itself; equal taps
 *      give the tap; g_ch == 1 changes nothing; so flip_t = 0, wmin = W, b = c = 0 reproduce gx_cache_gather_f32 and
 *      gx_cache_gather_labels bit for bit, and flip_t = 2^24 their mirror images.
 *
 *      params_out (may be NULL): int32 [B][8] = (flip, x0, y0, w, h, bits of g_0, bits of g_1, bits of g_2) of every frame of the
 *      batch, unused gains as the bits of 1.0f.  Refused besides what gx_cache_gather_f32 refuses (same messages; the label store
 *      is checked like the frame store): labels and out_labels not both NULL or both given, C > 3, H or W above 32767 (the tap
 *      arithmetic is 32-bit), a negative epoch (only its low 32 bits enter the counter), flip_t outside [0, 2^24], wmin outside
 *      [1, W], brightness or colour outside [0, 1) or NaN.  As with the plain gathers the VALUES of idx are the caller's to check.
 *      One launch on `stream`, nothing else: grid (blocks over the plane's quads of four columns, B), the frame's parameters
 *      computed once per block and shared through LDS. */
int gx_cache_gather_aug(const unsigned char* frames, long long frame_stride, const short* labels, long long label_stride,
                        long long rows, const long long* idx, long long idx_len, long long first, int mode,
                        unsigned long long seed, long long epoch, int flip_t, int wmin, float brightness, float colour, float* out,
                        long long* out_labels, int* params_out, int B, int C, int H, int W, gx_stream_t stream);

/* ---- the step's one collective without PyTorch (the reference's only multi-GPU mode is nn.DataParallel,
 *      train.py:153-155: replicas gathered on GPU 0 every iteration).  One process per GPU; each rank's flat fp32 gradient
 *      bucket (parameters' gradients + the err / kl tail, genesis_amd/dp.py) is summed IN PLACE over the ranks by one
 *      ncclAllReduce over RCCL / xGMI, enqueued on `stream` (capturable into the step's HIP graph).  RCCL is resolved at run
 *      time (a copy the process already holds, else librccl.so.1; GENESIS_RCCL_LIB overrides), so the library loads without it.
 *      Rank 0 calls gx_allreduce_unique_id and hands the gx_allreduce_unique_id_bytes() (= 128) bytes to every rank out of band
 *      (file, socket, MPI, a torch store); every rank then calls gx_allreduce_init on its device (collective: it returns when
 *      all `world` ranks have joined). */
size_t gx_allreduce_unique_id_bytes(void);
int gx_allreduce_unique_id(void* id, size_t id_bytes);
int gx_allreduce_init(const void* id, size_t id_bytes, int rank, int world, void** comm);
int gx_allreduce_run(void* comm, float* buf, size_t count, gx_stream_t stream);
int gx_allreduce_destroy(void* comm);

/* ---- measurement probe: `wgs` workgroups x 4 waves x 32 * iters v_mfma_f32_32x32x2_f32.  mode 0: register operands
 *      only (the fp32-MFMA ceiling); 1: B operand from LDS; 2: A and B from LDS (two ds_read_b32 per MFMA, the tap-conv
 *      pattern); 3: as 2 plus a workgroup barrier every 32 MFMAs; 4: A and B from LDS with one 16-byte read per four MFMAs;
 *      5: the gx_kq.hip inner loop (four 16-byte reads per 16 MFMAs, issued a step ahead); 6: the same on 2 x 4 tiles; 5 / 6
 *      store the shader clock they ran at (s_memtime ticks per 100 MHz tick) in scratch[1].  *flops = executed flops; time the stream around it
 *      (tools/mfma_peak.py). */
int gx_mfma_fp32_probe(int wgs, int iters, int mode, float* scratch, double* flops, gx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GENESIS_HIP_H */
