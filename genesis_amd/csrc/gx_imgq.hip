// Reconstruction quality of a validation batch (genesis_amd/image_quality.py): per image the mean squared error, its root, PSNR and
// the Gaussian-window SSIM of Wang et al. 2004, all in fp64 from the fp32 load onwards, one launch per batch (contract:
// include/genesis_hip.h).
//
// Tile plan.  A workgroup of 256 threads owns one IQ_T x IQ_T = 16 x 16 tile of VALID window positions of one image and loops over
// the channels.  Per channel it
//   1. stages the (16 + win - 1)^2 <= 26 x 26 haloed patch of pred and target in LDS as fp32 (exact; half the LDS traffic of fp64),
//      rows IQ_LDX = 48 floats apart: the row pass reads with 16 consecutive lanes per row and two rows per 32-lane group, and a
//      stride of 16 mod 32 dwords puts the two rows on disjoint banks;
//   2. row pass: for every staged row and each of the 16 output columns the win-tap sums of x, y, x^2, y^2, xy -> rb[5][26][16] fp64
//      (rows of 16 doubles = 32 dwords: the column pass reads two adjacent rows per 32-lane group = 64 consecutive dwords, every bank
//      once);
//   3. column pass: thread (ty, tx) sums win rows of each of the five maps and forms its position's SSIM value.
// The squared error is taken from the staged patch (after the barrier, so its order does not depend on the load width): a tile owns
// the 16 x 16 pixels under its valid positions, and the last tile of a row (column) of tiles also owns the win - 1 trailing columns
// (rows) that no further tile starts at -- every pixel exactly once.
// Each thread adds its values in a fixed order, the workgroup reduces by wave butterflies and then wave 0..3 in order, and thread 0
// writes the two sums to the tile's slot of ws.  No floating-point atomics: the last workgroup to arrive (integer counter) adds each
// image's slots in tile order -- one thread per image --, writes the rows, and one thread does the batch's bookkeeping in image
// order.  An image's row therefore does not depend on the batch it came in.
#include <math.h>

#include "gx_common.h"

namespace {

constexpr int IQ_T = 16, IQ_MAXWIN = 11, IQ_SH = IQ_T + IQ_MAXWIN - 1, IQ_LDX = 48, IQ_MAXDIM = 4096;
enum { IQ_COUNTER = 0, IQ_IMAGES = 1, IQ_BATCHES = 2, IQ_CURSOR = 3 };      // words of `state`
struct IqWindow { double g[IQ_MAXWIN]; };

__host__ __device__ __forceinline__ int iq_tiles(int extent, int win) { return (extent - win + 1 + IQ_T - 1) / IQ_T; }

template <bool VEC>
__global__ void __launch_bounds__(256)
image_quality_kernel(const float* __restrict__ pred, long long pred_stride, const float* __restrict__ target,
                     long long target_stride, int B, int C, int H, int W, IqWindow win, int n, double L, double* __restrict__ rows,
                     double* __restrict__ acc, unsigned long long* __restrict__ state, double* __restrict__ log,
                     long long log_capacity, double* __restrict__ slots) {
#pragma clang fp contract(off)
    __shared__ float sx[IQ_SH * IQ_LDX], sy[IQ_SH * IQ_LDX];
    __shared__ double rb[5][IQ_SH][IQ_T];
    __shared__ double red[4][2];
    __shared__ int s_last;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int tiles_h = iq_tiles(H, n), tiles_w = iq_tiles(W, n), tiles = tiles_h * tiles_w;
    const int b = blockIdx.x / tiles, t = blockIdx.x % tiles, ti = t / tiles_w, tj = t % tiles_w;
    const int vh = H - n + 1, vw = W - n + 1, r0 = ti * IQ_T, c0 = tj * IQ_T;
    const int sh = IQ_T + n - 1;                                     // staged rows and columns
    const int own_h = ti == tiles_h - 1 ? H - r0 : IQ_T;             // pixels whose squared error this tile counts (<= sh)
    const int own_w = tj == tiles_w - 1 ? W - c0 : IQ_T;
    const bool valid = r0 + ty < vh && c0 + tx < vw;
    const double C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    double ssim_sum = 0.0, se = 0.0;
    for (int c = 0; c < C; ++c) {
        const float* xp = pred + (size_t)b * (size_t)pred_stride + (size_t)c * H * W;
        const float* yp = target + (size_t)b * (size_t)target_stride + (size_t)c * H * W;
        if (VEC) {
            const int nv = (sh + 3) >> 2;                            // <= 7: 4 nv - 1 < IQ_LDX
            for (int i = tid; i < sh * nv; i += 256) {
                const int r = i / nv, v = i - r * nv, gr = r0 + r, gc = c0 + 4 * v;
                f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
                if (gr < H && gc < W) {                              // W % 4 == 0 and gc % 4 == 0: all four columns or none
                    a = *reinterpret_cast<const f32x4*>(xp + (size_t)gr * W + gc);
                    d = *reinterpret_cast<const f32x4*>(yp + (size_t)gr * W + gc);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sx[r * IQ_LDX + 4 * v + j] = a[j];
                    sy[r * IQ_LDX + 4 * v + j] = d[j];
                }
            }
        } else {
            for (int i = tid; i < sh * sh; i += 256) {
                const int r = i / sh, cc = i - r * sh, gr = r0 + r, gc = c0 + cc;
                float a = 0.f, d = 0.f;
                if (gr < H && gc < W) {
                    a = xp[(size_t)gr * W + gc];
                    d = yp[(size_t)gr * W + gc];
                }
                sx[r * IQ_LDX + cc] = a;
                sy[r * IQ_LDX + cc] = d;
            }
        }
        __syncthreads();
        for (int i = tid; i < own_h * own_w; i += 256) {             // squared error of the owned pixels, from the staged patch:
            const int r = i / own_w, cc = i - r * own_w;             // the same order whichever loads staged it
            const double e = (double)sx[r * IQ_LDX + cc] - (double)sy[r * IQ_LDX + cc];
            se += e * e;
        }
        for (int i = tid; i < sh * IQ_T; i += 256) {                 // row pass
            const int r = i >> 4, j = i & 15;
            double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
            for (int k = 0; k < n; ++k) {
                const double g = win.g[k], x = (double)sx[r * IQ_LDX + j + k], y = (double)sy[r * IQ_LDX + j + k];
                mx += g * x; my += g * y; mxx += g * (x * x); myy += g * (y * y); mxy += g * (x * y);
            }
            rb[0][r][j] = mx; rb[1][r][j] = my; rb[2][r][j] = mxx; rb[3][r][j] = myy; rb[4][r][j] = mxy;
        }
        __syncthreads();
        if (valid) {                                                 // column pass
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < n; ++k) {
                const double g = win.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] += g * rb[q][ty + k][tx];
            }
            const double mxmy = m[0] * m[1], mx2 = m[0] * m[0], my2 = m[1] * m[1];
            const double vx = m[2] - mx2, vy = m[3] - my2, cxy = m[4] - mxmy;
            ssim_sum += ((2.0 * mxmy + C1) * (2.0 * cxy + C2)) / ((mx2 + my2 + C1) * (vx + vy + C2));
        }
        // (the next channel's staging writes sx / sy only, which nobody reads after the barrier above; its row pass writes rb
        // after a barrier that every thread reaches with its column pass done)
    }
    ssim_sum = gx_wave_sum_d(ssim_sum);
    se = gx_wave_sum_d(se);
    if ((tid & 63) == 0) { red[tid >> 6][0] = ssim_sum; red[tid >> 6][1] = se; }
    __syncthreads();
    const unsigned long long total = (unsigned long long)B * (unsigned long long)tiles;
    if (tid == 0) {
        double* slot = slots + ((size_t)b * tiles + t) * 2;
        slot[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        slot[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        __threadfence();
        s_last = atomicAdd(state + IQ_COUNTER, 1ull) == total - 1ull;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup: every image's slots in tile order, then the batch step by one thread in image order
    __threadfence();
    const double count = (double)C * (double)vh * (double)vw, N = (double)C * (double)H * (double)W;
    for (int i = tid; i < B; i += 256) {
        const double* s = slots + (size_t)i * tiles * 2;
        double ss = 0.0, e = 0.0;
        for (int k = 0; k < tiles; ++k) {
            ss += __builtin_nontemporal_load(s + 2 * k);
            e += __builtin_nontemporal_load(s + 2 * k + 1);
        }
        const double mse = e / N;
        double* r = rows + (size_t)i * 4;
        r[0] = mse;
        r[1] = sqrt(mse);
        r[2] = mse == 0.0 ? (double)INFINITY : 10.0 * log10((L * L) / mse);
        r[3] = ss / count;
    }
    __threadfence();
    __syncthreads();
    if (tid != 0) return;
    double m[4] = {acc[0], acc[1], acc[2], acc[3]};
    for (int i = 0; i < B; ++i)
        for (int c = 0; c < 4; ++c) m[c] += __builtin_nontemporal_load(rows + (size_t)i * 4 + c);
    for (int c = 0; c < 4; ++c) acc[c] = m[c];
    state[IQ_IMAGES] += (unsigned long long)B;
    state[IQ_BATCHES] += 1ull;
    if (log) {
        const long long cur = (long long)state[IQ_CURSOR];
        const long long room = log_capacity - cur, take = room < B ? room : (long long)B;
        for (long long i = 0; i < take; ++i)
            for (int c = 0; c < 4; ++c) log[(cur + i) * 4 + c] = __builtin_nontemporal_load(rows + (size_t)i * 4 + c);
        if (take > 0) state[IQ_CURSOR] = (unsigned long long)(cur + take);
    }
    state[IQ_COUNTER] = 0ull;      // ready for the next launch (graph replay)
}

bool iq_shape_ok(int B, int C, int H, int W, int win) {
    return B >= 1 && C >= 1 && win >= 3 && win <= IQ_MAXWIN && (win & 1) && H >= win && W >= win && H <= IQ_MAXDIM && W <= IQ_MAXDIM;
}

}  // namespace

extern "C" {

size_t gx_image_quality_ws_bytes(int B, int C, int H, int W, int win) {
    if (!iq_shape_ok(B, C, H, W, win)) return 0;
    return (size_t)B * iq_tiles(H, win) * iq_tiles(W, win) * 2 * sizeof(double);
}

int gx_image_quality(const float* pred, long long pred_image_stride, const float* target, long long target_image_stride, int B,
                     int C, int H, int W, const double* window, int win, double data_range, double* rows, double* acc,
                     unsigned long long* state, double* log, long long log_capacity, void* ws, size_t ws_bytes,
                     gx_stream_t stream) {
    GX_CHECK_ARG(pred && target, "gx_image_quality: pred or target is a null pointer");
    GX_CHECK_ARG(window, "gx_image_quality: window is a null pointer");
    GX_CHECK_ARG(rows && acc && state, "gx_image_quality: rows, acc or state is a null pointer");
    GX_CHECK_ARG(ws, "gx_image_quality: ws is a null pointer");
    GX_CHECK_ARG(win >= 3 && win <= IQ_MAXWIN && (win & 1), "gx_image_quality: win = %d is not odd and in [3, %d]", win, IQ_MAXWIN);
    GX_CHECK_ARG(B >= 1, "gx_image_quality: B = %d below 1", B);
    GX_CHECK_ARG(C >= 1, "gx_image_quality: C = %d below 1", C);
    GX_CHECK_ARG(H >= win && H <= IQ_MAXDIM, "gx_image_quality: H = %d outside [win = %d, %d]", H, win, IQ_MAXDIM);
    GX_CHECK_ARG(W >= win && W <= IQ_MAXDIM, "gx_image_quality: W = %d outside [win = %d, %d]", W, win, IQ_MAXDIM);
    GX_CHECK_ARG(data_range > 0.0 && __builtin_isfinite(data_range), "gx_image_quality: data_range = %g is not positive and finite", data_range);
    const long long chw = (long long)C * H * W;
    GX_CHECK_ARG(pred_image_stride >= chw, "gx_image_quality: pred_image_stride %lld below C H W = %lld", pred_image_stride, chw);
    GX_CHECK_ARG(target_image_stride >= chw, "gx_image_quality: target_image_stride %lld below C H W = %lld", target_image_stride, chw);
    GX_CHECK_ARG(!log || log_capacity >= 0, "gx_image_quality: negative log_capacity");
    const long long tiles = (long long)iq_tiles(H, win) * iq_tiles(W, win);
    GX_CHECK_ARG((long long)B * tiles <= 0x7fffffffLL, "gx_image_quality: B = %d images of %lld tiles exceed one launch", B, tiles);
    const size_t need = gx_image_quality_ws_bytes(B, C, H, W, win);
    GX_CHECK_ARG(ws_bytes >= need, "gx_image_quality: ws_bytes %zu below the %zu needed", ws_bytes, need);
    GX_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "gx_image_quality: ws is not 8-byte aligned");
    IqWindow g;
    for (int k = 0; k < IQ_MAXWIN; ++k) g.g[k] = k < win ? window[k] : 0.0;
    // 16-byte loads: every row of every plane of every image of both tensors on a 16-byte boundary
    const bool vec = gx_vec4_ok(W, pred, target) && ((pred_image_stride | target_image_stride) & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)B * tiles));
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 8.0 * B * (double)chw);
        if (vec)
            hipLaunchKernelGGL(image_quality_kernel<true>, grid, dim3(256), 0, s, pred, pred_image_stride, target,
                               target_image_stride, B, C, H, W, g, win, data_range, rows, acc, state, log, log_capacity, (double*)ws);
        else
            hipLaunchKernelGGL(image_quality_kernel<false>, grid, dim3(256), 0, s, pred, pred_image_stride, target,
                               target_image_stride, B, C, H, W, g, win, data_range, rows, acc, state, log, log_capacity, (double*)ws);
    }
    GX_CHECK_LAUNCH("gx_image_quality");
    return GX_OK;
}

}  // extern "C"
