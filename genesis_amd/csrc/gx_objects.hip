// Per-object tables of an unsupervised segmentation (genesis_amd/objects.py): from the K log-mask planes of a batch, read in
// place as gx_seg_metrics reads them, the label map and per slot its geometry (integers) and its soft statistics (fp64).
// Contract: include/genesis_hip.h, gx_object_table.
//
// One workgroup of 256 threads per image, two passes over the image's planes (0.7 MB at 128 x 128, K = 11: the second pass is
// served by the L2):
//   1. argmax over the K planes -> labels;
//   2. slot after slot: every thread folds its pixels of plane k into private accumulators (mass over all of them; inside, the
//      geometry words and the colour sums over those labelled k), a wave folds its 64 lanes with shuffles and leaves the result in
//      its own LDS row, and after the last slot one thread per (slot, word) folds the four rows in wave order.
// There is no atomic of any kind and nothing crosses a workgroup, so an image's rows depend on its own pixels alone.  Both load
// widths give the pixels to the threads in the same way -- thread t owns the quads t, t + 256, ... (pixels 4q .. 4q + 3) and
// adds them in ascending order -- so the fp64 sums are the same bits whichever the alignment selects.
#include "gx_common.h"

namespace {

struct ObjPlanes { const float* p[32]; };      // plane k of image 0; image b lies image_stride floats further

constexpr int kObjThreads = 256, kObjWaves = kObjThreads / 64;
enum { OBJ_AREA = 0, OBJ_XMIN, OBJ_YMIN, OBJ_XMAX, OBJ_YMAX, OBJ_SUMX, OBJ_SUMY, OBJ_BORDER, OBJ_GEOM = 8 };
enum { OBJ_MASS = 0, OBJ_INSIDE, OBJ_C0, OBJ_SOFT = 6 };

// torch.argmax's order: a NaN ranks above every number and the first one wins; among equal numbers the lowest k wins
__device__ __forceinline__ void obj_take(float v, int k, float& best, int& bi) {
    if (best == best && (v > best || v != v)) { best = v; bi = k; }
}

__device__ __forceinline__ long long obj_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int obj_wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int obj_wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int obj_wave_or(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(kObjThreads)
object_table_kernel(ObjPlanes planes, long long image_stride, const float* __restrict__ x, long long x_image_stride, int C, int H,
                    int W, int K, unsigned char* __restrict__ labels, long long* __restrict__ geom, double* __restrict__ soft) {
#pragma clang fp contract(off)
    __shared__ long long s_geom[32][kObjWaves][OBJ_GEOM];
    __shared__ double s_soft[32][kObjWaves][OBJ_SOFT];
    const int b = blockIdx.x, HW = H * W, quads = (HW + 3) >> 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = (size_t)b * (size_t)image_stride;
    unsigned char* lab = labels + (size_t)b * HW;
    const float* xb = x ? x + (size_t)b * (size_t)x_image_stride : nullptr;

    // ---- pass 1: labels
    for (int q = threadIdx.x; q < quads; q += kObjThreads) {
        if (VEC) {
            const f32x4 v0 = reinterpret_cast<const f32x4*>(planes.p[0] + img)[q];
            float best[4] = {v0[0], v0[1], v0[2], v0[3]};
            int bi[4] = {0, 0, 0, 0};
#pragma unroll 4
            for (int k = 1; k < K; ++k) {
                const f32x4 v = reinterpret_cast<const f32x4*>(planes.p[k] + img)[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) obj_take(v[j], k, best[j], bi[j]);
            }
            reinterpret_cast<unsigned*>(lab)[q] = (unsigned)bi[0] | ((unsigned)bi[1] << 8) | ((unsigned)bi[2] << 16) | ((unsigned)bi[3] << 24);
        } else {
            const int n = HW - 4 * q < 4 ? HW - 4 * q : 4;
            for (int j = 0; j < n; ++j) {
                const int p = 4 * q + j;
                float best = planes.p[0][img + p];
                int bi = 0;
#pragma unroll 4
                for (int k = 1; k < K; ++k) obj_take(planes.p[k][img + p], k, best, bi);
                lab[p] = (unsigned char)bi;
            }
        }
    }
    __syncthreads();      // (a thread reads back only labels it wrote itself; the barrier keeps that from being a requirement)

    // ---- pass 2: slot after slot
    for (int k = 0; k < K; ++k) {
        const float* pk = planes.p[k] + img;
        double mass = 0.0, inside = 0.0, col[4] = {0.0, 0.0, 0.0, 0.0};
        long long sum_x = 0, sum_y = 0;
        int area = 0, x_min = W, y_min = H, x_max = -1, y_max = -1, border = 0;
        for (int q = threadIdx.x; q < quads; q += kObjThreads) {
            float v[4];
            unsigned l4;
            int n = 4;
            if (VEC) {
                const f32x4 t = reinterpret_cast<const f32x4*>(pk)[q];
                v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
                l4 = reinterpret_cast<const unsigned*>(lab)[q];
            } else {
                n = HW - 4 * q < 4 ? HW - 4 * q : 4;
                l4 = 0;
                for (int j = 0; j < 4; ++j) {
                    v[j] = j < n ? pk[4 * q + j] : 0.f;
                    l4 |= (j < n ? (unsigned)lab[4 * q + j] : 0xffu) << (8 * j);      // (0xff: no slot)
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= n) break;
                const double e = exp((double)v[j]);
                mass += e;
                if ((int)((l4 >> (8 * j)) & 0xffu) != k) continue;
                const int p = 4 * q + j, py = p / W, px = p - py * W;
                inside += e;
                ++area;
                x_min = px < x_min ? px : x_min; x_max = px > x_max ? px : x_max;
                y_min = py < y_min ? py : y_min; y_max = py > y_max ? py : y_max;
                sum_x += px; sum_y += py;
                border |= (px == 0 ? 1 : 0) | (py == 0 ? 2 : 0) | (px == W - 1 ? 4 : 0) | (py == H - 1 ? 8 : 0);
                if (xb) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < C) col[c] += (double)xb[(size_t)c * HW + p];
                }
            }
        }
        const long long g_area = obj_wave_sum(area), g_sx = obj_wave_sum(sum_x), g_sy = obj_wave_sum(sum_y);
        const int g_x0 = obj_wave_min(x_min), g_y0 = obj_wave_min(y_min), g_x1 = obj_wave_max(x_max), g_y1 = obj_wave_max(y_max);
        const int g_border = obj_wave_or(border);
        mass = gx_wave_sum_d(mass); inside = gx_wave_sum_d(inside);
#pragma unroll
        for (int c = 0; c < 4; ++c) col[c] = gx_wave_sum_d(col[c]);
        if (lane == 0) {
            long long* g = s_geom[k][wave];
            g[OBJ_AREA] = g_area; g[OBJ_XMIN] = g_x0; g[OBJ_YMIN] = g_y0; g[OBJ_XMAX] = g_x1; g[OBJ_YMAX] = g_y1;
            g[OBJ_SUMX] = g_sx; g[OBJ_SUMY] = g_sy; g[OBJ_BORDER] = g_border;
            double* s = s_soft[k][wave];
            s[OBJ_MASS] = mass; s[OBJ_INSIDE] = inside;
#pragma unroll
            for (int c = 0; c < 4; ++c) s[OBJ_C0 + c] = col[c];
        }
    }
    __syncthreads();

    // ---- the four wave rows of every (slot, word), in wave order
    for (int i = threadIdx.x; i < K * OBJ_GEOM; i += kObjThreads) {
        const int k = i / OBJ_GEOM, f = i % OBJ_GEOM;
        long long r = s_geom[k][0][f];
        for (int w = 1; w < kObjWaves; ++w) {
            const long long o = s_geom[k][w][f];
            if (f == OBJ_XMIN || f == OBJ_YMIN) r = o < r ? o : r;
            else if (f == OBJ_XMAX || f == OBJ_YMAX) r = o > r ? o : r;
            else if (f == OBJ_BORDER) r |= o;
            else r += o;
        }
        geom[((size_t)b * K + k) * OBJ_GEOM + f] = r;
    }
    for (int i = threadIdx.x; i < K * OBJ_SOFT; i += kObjThreads) {
        const int k = i / OBJ_SOFT, f = i % OBJ_SOFT;
        double r = s_soft[k][0][f];
        for (int w = 1; w < kObjWaves; ++w) r += s_soft[k][w][f];
        soft[((size_t)b * K + k) * OBJ_SOFT + f] = r;
    }
}

}  // namespace

extern "C" {

int gx_object_table(const float* base, long long plane_stride, long long image_stride, const float* const* planes, const float* x,
                    long long x_image_stride, int C, int B, int H, int W, int K, unsigned char* labels, long long* geom,
                    double* soft, gx_stream_t stream) {
    GX_CHECK_ARG(K >= 1 && K <= 32, "gx_object_table: K = %d outside [1, 32]", K);
    GX_CHECK_ARG((base != nullptr) != (planes != nullptr), "gx_object_table: give either base (packed planes) or planes (a table)");
    GX_CHECK_ARG(labels && geom && soft, "gx_object_table: labels, geom or soft is a null pointer");
    GX_CHECK_ARG(B >= 1, "gx_object_table: B = %d below 1", B);
    GX_CHECK_ARG(H >= 1 && H <= 4096 && W >= 1 && W <= 4096, "gx_object_table: H = %d or W = %d outside [1, 4096]", H, W);
    const long long HW = (long long)H * W;
    GX_CHECK_ARG(image_stride >= HW, "gx_object_table: image_stride %lld below H W = %lld", image_stride, HW);
    GX_CHECK_ARG(!base || plane_stride >= 0, "gx_object_table: negative plane_stride");
    if (x) {
        GX_CHECK_ARG(C >= 1 && C <= 4, "gx_object_table: C = %d outside [1, 4]", C);
        GX_CHECK_ARG(x_image_stride >= C * HW, "gx_object_table: x_image_stride %lld below C H W = %lld", x_image_stride, C * HW);
    }
    ObjPlanes T;
    uintptr_t bits = (uintptr_t)((unsigned long long)image_stride * sizeof(float));
    for (int k = 0; k < 32; ++k) {
        T.p[k] = k >= K ? nullptr : (base ? base + (size_t)k * (size_t)plane_stride : planes[k]);
        GX_CHECK_ARG(k >= K || T.p[k], "gx_object_table: plane %d is null", k);
        bits |= reinterpret_cast<uintptr_t>(T.p[k]);
    }
    // every plane of every image on a 16-byte boundary (and with H W % 4 == 0 every image's labels on a 4-byte one)
    const bool vec = (HW & 3) == 0 && (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(labels) & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (8.0 * K + 1.0 + K + (x ? 4.0 * C : 0.0)) * B * (double)HW);
        if (vec)
            hipLaunchKernelGGL(object_table_kernel<true>, dim3(B), dim3(kObjThreads), 0, s, T, image_stride, x, x_image_stride, C, H,
                               W, K, labels, geom, soft);
        else
            hipLaunchKernelGGL(object_table_kernel<false>, dim3(B), dim3(kObjThreads), 0, s, T, image_stride, x, x_image_stride, C,
                               H, W, K, labels, geom, soft);
    }
    GX_CHECK_LAUNCH("gx_object_table");
    return GX_OK;
}

}  // extern "C"
