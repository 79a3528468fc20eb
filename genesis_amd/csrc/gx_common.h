// Shared internals of libgenesis_hip.so (not part of the public C ABI; see include/genesis_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/genesis_hip.h"
#include "gx_pack.h"

// ---- error plumbing: C ABI never throws; negative return + thread-local message ----
void gx_set_error(const char* fmt, ...);

#define GX_CHECK_ARG(cond, ...)                  \
    do {                                         \
        if (!(cond)) {                           \
            gx_set_error(__VA_ARGS__);           \
            return GX_EINVAL;                    \
        }                                        \
    } while (0)

#define GX_CHECK_LAUNCH(name)                                                   \
    do {                                                                        \
        hipError_t e__ = hipGetLastError();                                     \
        if (e__ != hipSuccess) {                                                \
            gx_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return GX_ELAUNCH;                                                  \
        }                                                                       \
    } while (0)

// ---- per-kernel live profiling (HIP events on the launch stream; off unless gx_profile_enable(1)) ----
enum GxKernelId {
    KID_TAPCONV_C3 = 0, KID_TAPCONV_DT0, KID_TAPCONV_DT1, KID_TAPCONV_DG, KID_PACK_WEIGHTS,
    KID_WGRAD_C3, KID_WGRAD_D00, KID_WGRAD_D01, KID_WGRAD_D10, KID_WGRAD_D11, KID_WGRAD_REDUCE,
    KID_GN_FWD, KID_GN_BWD, KID_GN_PARAM_REDUCE, KID_ICSBP_FWD, KID_ICSBP_BWD, KID_MASKPOOL_FWD,
    KID_MASKPOOL_BWD, KID_MIXTURE_FWD, KID_MIXTURE_BWD, KID_CONV1X1_FWD, KID_CONV1X1_DGRAD,
    KID_CONV1X1_WGRAD, KID_SMALL_REDUCE, KID_ADAM, KID_GECO, KID_SPLITK_REDUCE, KID_BIAS_ACT_BWD, KID_DCONV, KID_GATED, KID_LATENT, KID_DENSE, KID_WINO,
    KID_WGQ_STREAM, KID_KQ_DTH, KID_KQ_DGH, KID_KQ_C3H, KID_KQ_C5H, KID_COUNT
};
// ---- contexts: every piece of mutable library state that outlives a call (deferred-reduction queues, queued
// weight-gradient jobs, the packed-weight cache a step is recording / served from, the per-kernel profiling records)
// belongs to a context.  A thread works in its CURRENT context (thread-local; context 0 until gx_ctx_make_current), so
// two training loops -- in one thread one after the other, or in two threads -- never see each other's queues.
// What remains process-wide is one-time initialisation (zero pages, kernel attributes) and the dispatch policies.
constexpr int kGxMaxCtx = 32;
int gx_cur_ctx(void);
struct GxCtxFlags { bool prof_on, defer_on; int cache_recording, cache_active; };
GxCtxFlags& gx_ctx_flags(void);      // of the calling thread's current context
#define g_gx_prof_on (gx_ctx_flags().prof_on)
#define g_gx_defer_on (gx_ctx_flags().defer_on)
void gx_prof_begin(int kid, hipStream_t s, double flops, double bytes);
void gx_prof_end(hipStream_t s);
// RAII: brackets ONE kernel launch with two events when profiling is on; a flag test otherwise.
struct GxProf {
    hipStream_t s; bool on;
    GxProf(int kid, hipStream_t s_, double flops, double bytes) : s(s_), on(g_gx_prof_on) {
        if (on) gx_prof_begin(kid, s, flops, bytes);
    }
    ~GxProf() { if (on) gx_prof_end(s); }
};

// ---- the gradient guard's device record (gx_grad_guard writes it, the guarded tail launches read it; the byte layout is part
// of the ABI: include/genesis_hip.h, GX_GUARD_R_*) ----
struct GxGuardRecord { double S; float norm, coef, scale; int ok; long long skipped; };

// ---- deferred parameter-gradient reductions (gx_defer_*; gx_api.cpp owns the queue) ----
// ca0 / cb0 / CAf / CBf: the record covers the channel block (ca0.., cb0..) of a CAf x CBf weight (CAf == 0: the whole
// weight, CA x CB) -- the stream-K weight-gradient kernel keeps one slab region per 64 x 64 channel block
struct GxWgradRed { const float* partial; float* dw; int nsplit, Ttot, CA, CB, CApad, CBpad, layout, ns0, ns1, ns2, ns3,
                    ca0, cb0, CAf, CBf; };
struct GxGnRed { const float* part; float* dgamma; float* dbeta; float* dbias; int N, C; };
bool gx_defer_push_wgrad(const GxWgradRed& r);   // false: queue full (caller reduces immediately)
int gx_defer_wgrad_room();                      // free slots of the weight-gradient reduce queue of the current context
bool gx_defer_push_gn(const GxGnRed& r);
int gx_defer_flush_wgrad(const GxWgradRed* items, int n, hipStream_t s);   // gx_conv.hip
int gx_defer_flush_gn(const GxGnRed* items, int n, hipStream_t s);         // gx_norm.hip

// ---- PNG frames (gx_png.cpp, gx_png.hip): the largest width and height.  gx_png_unfilter hands the last row of a band to the
// next band through kGxPngMaxDim * C bytes of LDS (16 KB for RGBA); the host checks reject larger frames with this same constant.
constexpr int kGxPngMaxDim = 4096;
// ---- loose image files (gx_jpeg.cpp's _any entry points, gx_imagefile.hip): the largest width and height of a frame of either
// format, the PNG bound above
constexpr int kGxImageMaxDim = kGxPngMaxDim;
// Upper bound on the source rows (columns) that R consecutive output rows of Pillow's BILINEAR table of in -> out span (gx_feed.hip)
int gx_pil_band_rows(int in, int out, int R);

static inline int gx_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int gx_ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int gx_round_up(int a, int b) { return gx_ceil_div(a, b) * b; }

// XCD-aware block -> tile map (cdna_hip_programming.md T1).  The dispatcher is observed to place block b on XCD b % 8, each XCD with
// its own 4 MB L2: with tile = block id, spatially adjacent tiles (which share their halo rows / columns) sit on eight different
// L2s and every halo is fetched from HBM once per tile.  This bijection hands every XCD a CONTIGUOUS run of tiles (the blocks of an
// XCD are dispatched in increasing id, so neighbours in the run are neighbours in time).  Speed only: any placement is correct.
#ifdef __HIPCC__
__device__ __forceinline__ int gx_xcd_tile(int bid, int nwg) {
#ifdef GX_NO_XCD_SWIZZLE
    return bid;
#else
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
#endif
}
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// May planes of HW floats of these tensors be walked with 16-byte (f32x4) accesses?  HW % 4 == 0 puts every plane a multiple of
// 16 bytes behind its tensor's base, so the bases decide -- and a base need not be an allocation: a contiguous slice at an odd
// element offset of a larger buffer is a legal operand of every entry point.  One predicate for the statistics, apply and pooling
// kernels (null pointers count as aligned).
__host__ __device__ __forceinline__ bool gx_vec4_ok(int HW, const void* a, const void* b = nullptr, const void* c = nullptr,
                                                    const void* d = nullptr) {
    return (HW & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                              reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// 64-lane wavefront reductions (CDNA4: wave = 64).
__device__ __forceinline__ float gx_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double gx_wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float gx_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- Winograd F(2x2,3x3) conv3x3 (gx_wino.hip); the weight operand and its layouts: gx_pack.h ----
__host__ __device__ __forceinline__ size_t gx_wino_h_bytes(int Kpad16, int Mpad) {
    return (size_t)(Mpad >> 6) * (Kpad16 >> 4) * 16 * 6144;
}
bool gx_wino_h_on();     // Winograd layers on the bf16 pipe (default; gx_wino_precision(0) / GENESIS_WINO_BF16X6=0: fp32 pipe)
bool gx_conv_input_hint(const float** p0, int* n0, const float** p1, int* n1);      // the armed gx_conv_input_amax hint (gx_wino.hip), not cleared
bool gx_wino_f16_pending(void);   // ... and the NEXT launch of this thread on two fp16 pieces per operand (gx_conv_input_amax armed): the Winograd views in GX_FORM_F16X2
bool gx_wino_b1_on(void);         // ... on ONE bf16 piece per operand (gx_wino_precision(3)): the Winograd views in GX_FORM_BF16X1
// conv with an already packed U (16 * Kpad * Mpad floats; bf16 pipe: gx_wino_h_bytes): out[N,M,H,W] from in[N,K,H,W]
bool gx_wino_eligible(int N, int K, int M, int H, int W);
int gx_wino_launch(const float* in, const float* U, float* out, int N, int K, int M, int H, int W, hipStream_t s);


// ---- k-quad tap convolutions (gx_kq.hip): 16-byte k-contiguous MFMA operand reads for the chip-filling layers ----
// (packed-weight layouts: gx_pack.h)
bool gx_kq_c3_eligible(int N, int K, int M, int H, int W);
bool gx_kq_deconv_eligible(int N, int K, int M, int Hb, int Wb, int mult);   // mult: workgroups per (pixel, channel) tile
int gx_kq_c3_launch(const float* in, const float* wp, const float* bias, int act, float* out, int N, int K, int M, int H,
                    int W, hipStream_t s);
int gx_kq_deconv_fwd_launch(const float* in, const float* wp0, const float* wp1, const float* bias, float* out, int N,
                            int K, int M, int Hb, int Wb, float* stats, int* stats_parts, hipStream_t s);
int gx_kq_deconv_dgrad_launch(const float* dy, const float* wp, float* dx, int N, int K, int M, int Hb, int Wb,
                              hipStream_t s);
// ... on the bf16 matrix pipe: weights packed as GX_VIEW_DT_ROW0 / _ROW1 in GX_FORM_BF16X3 = [channel tile][16-channel chunk][tap][piece hi|mid|lo]
// [octet][64 output channels][8 channels] in bf16 (two per 32-bit word)
bool gx_kq_deconv_h_eligible(int N, int K, int M, int Hb, int Wb);
// ... or from THREE fp16 piece products (gx_kq_precision(2), DESIGN.md finding 40): x * 2^e = hi + lo (11 + 11 significant bits),
// hi*hi + hi*lo + lo*hi; e per TENSOR from its largest magnitude so that the pieces sit inside fp16's exponent range.  The weights
// are packed in GX_FORM_F16X2: two fp16 pieces of w * 2^e (two piece slots per tap), the weight tensor's amax in the packing's
// trailer (gx_pack.h).
bool gx_kq_f16_on();
// ... or from ONE bf16 piece per operand (gx_kq_precision(3)): the weights packed in GX_FORM_BF16X1
bool gx_kq_b1_on();
// GENESIS_MATMUL_PRECISION (gx_api.cpp): -1 unset, else the level 0 highest / 1 high / 2 medium -- read by every family's default
// ahead of its own variables; gx_matmul_level_mode: the family mode of a level (0 -> 0, 1 -> 2, 2 -> 3)
int gx_env_matmul_level(void);
inline int gx_matmul_level_mode(int level) { return level == 0 ? 0 : (level == 1 ? 2 : 3); }
int gx_kq_mode_now(void);         // the resolved mode of each family (gx_matmul_precision)
int gx_wgq_mode_now(void);
int gx_wino_mode_now(void);
// amax of a tensor (n floats) as kAmaxParts partial maxima in ws (gx_kq_amax_ws_floats() floats, 16-byte aligned): one launch; the
// conv kernels reduce the partials themselves
constexpr int kAmaxParts = 256;
__host__ __device__ __forceinline__ constexpr size_t gx_kq_amax_ws_floats() { return kAmaxParts; }
int gx_kq_amax_launch(const float* x, size_t n, float* ws, hipStream_t s);
// producer -> consumer hand-over of those partial maxima (gx_kq_amax_link, include/genesis_hip.h): armed by the caller with a scratch
// buffer; the next producer that can (the decoder head's GroupNorm backward) writes one partial maximum per workgroup of the tensor it
// stores -- only a launch that covers the WHOLE tensor (numel elements: a chunked producer does not qualify) -- and records the tensor's
// address; the next fp16 x 3 conv whose INPUT is that address (and size) reads them instead of making its own pass.
// One-shot, per thread; any fp16 x 3 conv call clears it.
struct GxAmaxLink { float* parts; int capacity; size_t numel; const float* tensor; int n; int hits; };      // numel: the WHOLE tensor's
GxAmaxLink& gx_amax_link(void);          // (gx_api.cpp)
// TAP (round 6): the same partial maxima for ANY later reader -- the weight-gradient stream-K launch at the end of the backward
// pass needs the scale of BOTH operands of every layer (gx_wgq_operand_amax).  gx_amax_tap(parts, capacity, numel) arms a one-shot,
// per-thread request: the next amax-capable producer launch (whatever its destination views: channel slices of concat buffers
// and resampled second copies hold the same values) writes one partial maximum of the values it stores per workgroup and
// records how many; gx_amax_tap_result() returns that count (0: the launch could not serve) and disarms.
struct GxAmaxTap { float* parts; int capacity; int n; size_t numel; };      // numel: the elements the producer launch must cover
GxAmaxTap& gx_amax_tap_state(void);      // (gx_api.cpp)
// producer side, both mechanisms: where the launch of `nwg` workgroups writes its partial maxima (NULL: nowhere).  link_ok: the
// destination qualifies for the armed link (a whole plain tensor of L.numel elements).
inline float* gx_amax_producer_out(const float* tensor, bool link_ok, unsigned nwg, size_t covered) {
    GxAmaxTap& T = gx_amax_tap_state();
    GxAmaxLink& L = gx_amax_link();
    float* p = nullptr;
    // (a launch that covers only part of the tensor -- the chunked callers -- must not serve: its maxima are not the tensor's)
    if (T.parts && (int)nwg <= T.capacity && covered == T.numel) { p = T.parts; T.n = (int)nwg; T.parts = nullptr; }
    if (link_ok && L.parts && !L.tensor && tensor && (p || (int)nwg <= L.capacity)) {
        if (p) L.parts = p; else p = L.parts;      // (one set of partials serves both readers)
        L.tensor = tensor; L.n = (int)nwg;
    }
    return p;
}
// consumer side: partials of `x` if the armed link holds them (then *n > 0), clearing the link either way
inline const float* gx_amax_link_take(const float* x, size_t numel, int* n) {
    GxAmaxLink& L = gx_amax_link();
    const float* p = nullptr;
    *n = 0;
    if (L.parts && x && L.tensor == x && L.numel == numel && L.n > 0) { p = L.parts; *n = L.n; ++L.hits; }
    L.parts = nullptr; L.capacity = 0; L.numel = 0; L.tensor = nullptr; L.n = 0;
    return p;
}
#ifdef __HIPCC__
// |.|-maximum of n floats by ONE workgroup of 1024 threads (a weight tensor: ~100 k floats; 16-byte loads, eight in flight per thread);
// the result is valid in thread 0
__device__ __forceinline__ float gx_wg1024_amax(const float* __restrict__ w, int n) {
    typedef float gx_amax_f4 __attribute__((ext_vector_type(4)));
    float m = 0.f;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(w) & 15) == 0) {
        const gx_amax_f4* w4 = reinterpret_cast<const gx_amax_f4*>(w);
        const int n4 = n >> 2;
#pragma unroll 8
        for (int i = threadIdx.x; i < n4; i += 1024) {
            const gx_amax_f4 v = w4[i];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(w[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float gx_amax_red[16];
    if ((threadIdx.x & 63) == 0) gx_amax_red[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = gx_amax_red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) r = fmaxf(r, gx_amax_red[i]);
    return r;
}
// producer-side tap (gx_amax_producer_out): the workgroup's largest stored magnitude -> parts[idx]; am >= 0, every thread calls
__device__ __forceinline__ void gx_block_amax_store(float am, float* __restrict__ parts, unsigned idx) {
    __shared__ float gx_bam_red[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
    if ((threadIdx.x & 63) == 0) gx_bam_red[threadIdx.x >> 6] = am;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = 0.f;
        for (int i = 0; i < (int)((blockDim.x + 63) >> 6); ++i) r = fmaxf(r, gx_bam_red[i]);
        parts[idx] = r;
    }
}
#endif
int gx_kq_weight_amax_launch(const float* w, int n, float* out, hipStream_t s);          // one workgroup (weights are small)
bool gx_kq_deconv_dgrad_h_eligible(int N, int K, int M, int Hb, int Wb);      // GX_VIEW_DT_DGRAD: all 25 taps, plane-major slots
int gx_kq_deconv_dgrad_h_launch(const float* dy, const float* wp, float* dx, int N, int K, int M, int Hb, int Wb,
                                hipStream_t s, float* amax_ws = nullptr, const float* w_amax = nullptr,
                                const float* x_parts = nullptr, int x_nparts = 0);     // x_parts: the input's partial maxima from its producer
int gx_kq_deconv_fwd_h_launch(const float* in, const float* wp0, const float* wp1, const float* bias, float* out, int N,
                              int K, int M, int Hb, int Wb, float* stats, int* stats_parts, hipStream_t s,
                              float* amax_ws = nullptr, const float* w_amax = nullptr,    // amax_ws != NULL: the fp16 x 3 form (GX_FORM_F16X2)
                              const float* x_parts = nullptr, int x_nparts = 0);
bool gx_kq_c3h_eligible(int N, int K, int M, int H, int W);
int gx_kq_c3h_launch(const float* in, const float* wp, const float* bias, int act, float* out, int N, int K, int M, int H,
                     int W, hipStream_t s, const float* mask = nullptr, int mask_act = 0, float* amax_ws = nullptr,
                     const float* w_amax = nullptr);         // amax_ws != NULL: the fp16 x 3 form (GX_FORM_F16X2)
// 5 x 5 stride-1 conv on the bf16 pipe (GX_VIEW_C5 / _C5_FLIP in the 16-bit-pipe forms; K a multiple of 16, H and W of 16)
bool gx_kq_c5h_eligible(int N, int K, int M, int H, int W);
int gx_chan_sums_launch(const float* x, int N, int C, int HW, float* part, float* out, hipStream_t s);   // gx_misc.hip
int gx_kq_c5h_launch(const float* in, const float* wp, float* out, int N, int K, int M, int H, int W, hipStream_t s,
                     float* amax_ws = nullptr, const float* w_amax = nullptr, const float* x_parts = nullptr,
                     int x_nparts = 0);      // (x_parts: the input's partial maxima, gx_kq_amax_link)

// ---- second-generation weight gradients (gx_wgq.hip): LDS-DMA staging of both operands, grouped launches -------------
bool gx_wgq_c3_eligible(int N, int Cin, int Cout, int H, int W);
bool gx_wgq_deconv_eligible(int N, int Cin, int Cout, int Hb, int Wb);
int gx_wgq_max_split(int CA, int CB);
// ws: room for ws_slabs split-K slabs of Ttot * CApad * CBpad floats.  With deferral on (gx_defer_enable) the job is only
// queued: gx_defer_flush launches all queued jobs in groups and then the batched slab reduce.
int gx_wgq_c3(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int H, int W, float* ws, int ws_slabs,
              hipStream_t s);
int gx_wgq_deconv(const float* x, const float* dy, float* dw, int N, int Cin, int Cout, int Hb, int Wb, float* ws,
                  int ws_slabs, hipStream_t s);
bool gx_wgq_c5_eligible(int N, int CA, int CB, int H, int W);
int gx_wgq_c5(const float* a, const float* b, float* dw, int N, int CA, int CB, int H, int W, float* ws, int ws_slabs,
              hipStream_t s);
// gx_wstrip.hip: the 32 -> 32 conv3x3 weight gradient as column strips (grids that are no power of two, W % 8 == 0)
bool gx_wstrip_supported(int N, int C, int H, int W);
// gx_tapconv_precision (gx_conv.hip): the tap-conv kernels and the strips on ONE bf16 piece per operand (mode 3), and the record of
// the mode the last such launch of this thread ran in (gx_tapconv_last_mode)
bool gx_tapconv_b1_on(void);
void gx_tapconv_note(int mode);
// gx_conv_last_plan (gx_conv.hip): the tile plan of this thread's last forward / data-gradient conv launch.  Every launcher fills
// one of these from the values it launches with (never from the shape again) and notes it on the host just before the launch;
// helper launches (packing, amax passes, reduces) note nothing.  The field order is the ABI's (GX_PLAN_* indices).
struct GxConvPlan {
    int family, form, lTH, lTW, lG, nq, pixels, rt_th, rt_tw, tiles_h, tiles_w, grid_x, grid_y, grid_z, nsplit, chunks_per_split,
        nfull, stats;
};
static_assert(sizeof(GxConvPlan) == GX_PLAN_FIELDS * sizeof(int), "GxConvPlan and GX_PLAN_FIELDS disagree");
void gx_conv_plan_note(const GxConvPlan& p);
size_t gx_wstrip_ws_floats(int N, int C, int H, int W);
int gx_wstrip_launch(const float* x, const float* dy, float* dw, float* dbias, int N, int C, int H, int W, void* ws, hipStream_t s);
bool gx_wgq_bf16_pipe(void);      // gx_wgq_precision / GENESIS_WGQ_BF16X6: weight gradients on the bf16 matrix pipe (six piece products)
int gx_wgq_pending(void);
void gx_wgq_discard(void);
int gx_wgq_flush(hipStream_t s);
// gx_conv.hip: conv3x3 weight gradients of layers too small for the stream-K launch (4 x 4 grids), queued while deferral is on
int gx_wf_flush(hipStream_t s);
int gx_wf_pending(void);
void gx_wf_discard(void);
int gx_wgrad_reduce_now(const GxWgradRed& r, hipStream_t s, int accumulate = 0);    // gx_conv.hip: dw (+)= sum of the slabs
