// Multi-dSprites on the device (datasets/multid_config.py, scripts/generate_multid.py).  The dataset is 50 000 frames of
// 64 x 64 x 3, stored as float32 (already / 255) with float64 label maps: at most 2.4 GB, so a whole split lives in HBM and
// a batch is a gather of its rows by a permutation that is on the device too.  Reference: multid_config.py:131-143
// (ToTensor: HWC -> CHW, uint8 / 255 or float unchanged; F.interpolate(size), default mode 'nearest'; the label map through
// the same two and .type(LongTensor)) and generate_multid.py:47-73 (sprites pasted in order onto a background colour).
//
// All three kernels are pure memory kernels of one shape: one thread per output pixel, grid (pixel blocks, frames).  A lane
// reads its pixel's C interleaved values (3 or 12 contiguous bytes at C = 3; consecutive lanes read adjacent pixels when
// there is no resample) and writes one value into each of the C planes, so every store instruction of a wave covers 256
// contiguous bytes.  No LDS.
#include "gx_common.h"

#include <math.h>

namespace {

// s = min(floor(d * scale), in - 1) with scale = in / out in fp32: F.interpolate's nearest source index (gx_feed.hip)
__device__ __forceinline__ int nearest_src(int d, float scale, int in) {
    const int s = (int)floorf((float)d * scale);
    return s < in - 1 ? s : in - 1;
}

__device__ __forceinline__ float to_unit(unsigned char v) { return (float)v / 255.0f; }   // a true division, as ToTensor's
__device__ __forceinline__ float to_unit(float v) { return v; }

// dst[b][c][y][x] = unit(src[row(b)][sy][sx][c]), row(b) = idx ? idx[first + b] : first + b.  CT = C when known at compile
// time (the loads of a pixel unroll into one 12-byte read for fp32 at C = 3), 0 for any other channel count.
template <typename T, int CT>
__global__ void __launch_bounds__(256)
rows_gather_f32chw_kernel(const T* __restrict__ src, const long long* __restrict__ idx, long long first,
                          float* __restrict__ dst, int Hs, int Ws, int Crt, int H, int W) {
    const int C = CT ? CT : Crt;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int b = blockIdx.y;
    const long long row = idx ? idx[first + b] : first + b;
    const int y = p / W, x = p - y * W;
    const int sy = nearest_src(y, (float)Hs / (float)H, Hs), sx = nearest_src(x, (float)Ws / (float)W, Ws);
    const T* q = src + (((size_t)row * Hs + sy) * Ws + sx) * (size_t)C;
    float* d = dst + (size_t)b * C * H * W + p;
    if (CT) {
        T v[CT ? CT : 1];
#pragma unroll
        for (int c = 0; c < CT; ++c) v[c] = q[c];
#pragma unroll
        for (int c = 0; c < CT; ++c) d[(size_t)c * H * W] = to_unit(v[c]);
    } else {
        for (int c = 0; c < C; ++c) d[(size_t)c * H * W] = to_unit(q[c]);
    }
}

// The same gather for label maps [N, Hs, Ws] -> int64 [B, 1, H, W]; a float label is truncated towards zero, as
// .type(LongTensor) does.
template <typename T>
__global__ void __launch_bounds__(256)
rows_gather_labels_kernel(const T* __restrict__ src, const long long* __restrict__ idx, long long first,
                          long long* __restrict__ dst, int Hs, int Ws, int H, int W) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int b = blockIdx.y;
    const long long row = idx ? idx[first + b] : first + b;
    const int y = p / W, x = p - y * W;
    const int sy = nearest_src(y, (float)Hs / (float)H, Hs), sx = nearest_src(x, (float)Ws / (float)W, Ws);
    dst[(size_t)b * H * W + p] = (long long)src[((size_t)row * Hs + sy) * Ws + sx];
}

constexpr int kSprite = 64, kSpritePixels = kSprite * kSprite, kMaxObjects = 4;

// generate_multid.py:47-73 for one image a blockIdx.y: the sprites first[i] .. first[i] + count[i] - 1 of the stack are pasted
// in that order, so a pixel shows the LAST one that covers it; they are visited from the last down and a pixel stops at its
// first hit.  colours[i][0] is the background, colours[i][1 + o] object o.  img is HWC fp32 (12 contiguous bytes a lane),
// mask one byte a lane.  The host checks first / count against the stack; an entry that still points outside it is skipped
// here, so that no launch reads past the stack.
__global__ void __launch_bounds__(256)
sprites_compose_kernel(const unsigned char* __restrict__ sprites, int S, const int* __restrict__ first,
                       const int* __restrict__ count, const unsigned char* __restrict__ colours, float* __restrict__ img,
                       unsigned char* __restrict__ mask) {
    const int p = blockIdx.x * 256 + threadIdx.x;     // kSpritePixels is a multiple of 256: no tail
    const int i = blockIdx.y;
    const int f = first[i];
    int n = count[i];
    n = n < kMaxObjects ? n : kMaxObjects;
    int label = 0;
    for (int o = n - 1; o >= 0; --o) {
        const int s = f + o;
        if (s < 0 || s >= S) continue;
        if (sprites[(size_t)s * kSpritePixels + p] != 0) {
            label = o + 1;
            break;
        }
    }
    const unsigned char* col = colours + ((size_t)i * (kMaxObjects + 1) + label) * 3;
    float* d = img + ((size_t)i * kSpritePixels + p) * 3;
    const float r = to_unit(col[0]), g = to_unit(col[1]), bl = to_unit(col[2]);
    d[0] = r;
    d[1] = g;
    d[2] = bl;
    mask[(size_t)i * kSpritePixels + p] = (unsigned char)label;
}

template <typename T>
void launch_frames(const void* src, const long long* idx, long long first, float* dst, int B, int Hs, int Ws, int C, int H, int W,
                   hipStream_t s) {
    const dim3 grid((unsigned)gx_ceil_div(H * W, 256), (unsigned)B);
    if (C == 3)
        hipLaunchKernelGGL((rows_gather_f32chw_kernel<T, 3>), grid, dim3(256), 0, s, (const T*)src, idx, first, dst, Hs, Ws, C, H, W);
    else if (C == 1)
        hipLaunchKernelGGL((rows_gather_f32chw_kernel<T, 1>), grid, dim3(256), 0, s, (const T*)src, idx, first, dst, Hs, Ws, C, H, W);
    else
        hipLaunchKernelGGL((rows_gather_f32chw_kernel<T, 0>), grid, dim3(256), 0, s, (const T*)src, idx, first, dst, Hs, Ws, C, H, W);
}

template <typename T>
void launch_labels(const void* src, const long long* idx, long long first, long long* dst, int B, int Hs, int Ws, int H, int W,
                   hipStream_t s) {
    const dim3 grid((unsigned)gx_ceil_div(H * W, 256), (unsigned)B);
    hipLaunchKernelGGL(rows_gather_labels_kernel<T>, grid, dim3(256), 0, s, (const T*)src, idx, first, dst, Hs, Ws, H, W);
}

// what both gathers require of (first, B) and of the frame sizes; the values of idx are the caller's to check
const char* gather_args_error(const void* src, const void* dst, const long long* idx, long long idx_len, long long first,
                              long long N, int B, int Hs, int Ws, int H, int W) {
    if (!src || !dst) return "null pointer";
    if (!(B > 0 && B <= 65535 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && N > 0)) return "bad dims (B at most 65535)";
    if ((long long)H * W >= (1ll << 31) || (long long)Hs * Ws >= (1ll << 31)) return "frame too large";
    if (first < 0) return "negative first";
    if (idx ? first + B > idx_len : first + B > N) return "rows first .. first + B reach past the index vector (or, without one, past N)";
    return nullptr;
}

}  // namespace

extern "C" {

int gx_rows_gather_f32chw(const void* src, int dtype, long long N, const long long* idx, long long idx_len, long long first,
                          float* dst, int B, int Hs, int Ws, int C, int H, int W, gx_stream_t stream) {
    const char* err = gather_args_error(src, dst, idx, idx_len, first, N, B, Hs, Ws, H, W);
    GX_CHECK_ARG(!err, "gx_rows_gather_f32chw: %s", err ? err : "");
    GX_CHECK_ARG(C > 0 && C <= 64, "gx_rows_gather_f32chw: bad channel count %d", C);
    GX_CHECK_ARG(dtype == GX_ROWS_U8 || dtype == GX_ROWS_F32, "gx_rows_gather_f32chw: bad dtype %d", dtype);
    hipStream_t s = (hipStream_t)stream;
    {
        const double px = (double)B * H * W * C;
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, px * (dtype == GX_ROWS_U8 ? 1 : 4) + 4.0 * px);
        if (dtype == GX_ROWS_U8) launch_frames<unsigned char>(src, idx, first, dst, B, Hs, Ws, C, H, W, s);
        else launch_frames<float>(src, idx, first, dst, B, Hs, Ws, C, H, W, s);
    }
    GX_CHECK_LAUNCH("gx_rows_gather_f32chw");
    return GX_OK;
}

int gx_rows_gather_labels(const void* src, int dtype, long long N, const long long* idx, long long idx_len, long long first,
                          long long* dst, int B, int Hs, int Ws, int H, int W, gx_stream_t stream) {
    const char* err = gather_args_error(src, dst, idx, idx_len, first, N, B, Hs, Ws, H, W);
    GX_CHECK_ARG(!err, "gx_rows_gather_labels: %s", err ? err : "");
    GX_CHECK_ARG(dtype == GX_LABEL_U8 || dtype == GX_LABEL_I32 || dtype == GX_LABEL_I64 || dtype == GX_LABEL_F32 ||
                     dtype == GX_LABEL_F64, "gx_rows_gather_labels: bad dtype %d", dtype);
    hipStream_t s = (hipStream_t)stream;
    {
        const int esz = dtype == GX_LABEL_U8 ? 1 : ((dtype == GX_LABEL_I32 || dtype == GX_LABEL_F32) ? 4 : 8);
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * H * W * (esz + 8.0));
        switch (dtype) {
            case GX_LABEL_U8: launch_labels<unsigned char>(src, idx, first, dst, B, Hs, Ws, H, W, s); break;
            case GX_LABEL_I32: launch_labels<int>(src, idx, first, dst, B, Hs, Ws, H, W, s); break;
            case GX_LABEL_I64: launch_labels<long long>(src, idx, first, dst, B, Hs, Ws, H, W, s); break;
            case GX_LABEL_F32: launch_labels<float>(src, idx, first, dst, B, Hs, Ws, H, W, s); break;
            default: launch_labels<double>(src, idx, first, dst, B, Hs, Ws, H, W, s); break;
        }
    }
    GX_CHECK_LAUNCH("gx_rows_gather_labels");
    return GX_OK;
}

int gx_sprites_compose(const unsigned char* sprites, int S, const int* first, const int* count, const unsigned char* colours,
                       float* img, unsigned char* mask, int n, gx_stream_t stream) {
    GX_CHECK_ARG(sprites && first && count && colours && img && mask, "gx_sprites_compose: null pointer");
    GX_CHECK_ARG(S > 0 && n > 0 && n <= 65535, "gx_sprites_compose: bad dims (S %d, n %d; n at most 65535)", S, n);
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)n * kSpritePixels * (kMaxObjects + 13.0));
        hipLaunchKernelGGL(sprites_compose_kernel, dim3(kSpritePixels / 256, (unsigned)n), dim3(256), 0, s, sprites, S, first,
                           count, colours, img, mask);
    }
    GX_CHECK_LAUNCH("gx_sprites_compose");
    return GX_OK;
}

}  // extern "C"
