// A loader's decoded split kept on the device (genesis_amd/data_cache.py).  Every loader delivers fp32 [B, C, H, W] frames that
// were bytes a moment before (byte / 255, or byte * (1 / 255) from the JPEG path) and, some of them, int64 label maps whose
// values fit 16 bits.  The store kernels narrow a batch back to bytes / int16 while the first epoch runs and COUNT what does
// not survive the trip, so the host can decide with one read whether the cache may serve the later epochs; the gather kernels
// then deliver a batch from the store by an index vector, as gx_rows_gather_* do for Multi-dSprites.
//
// Layout: planar rows, frames uint8 [rows][C * H * W] in CHW order, labels int16 [rows][H * W]; the row stride is a multiple
// of 16 bytes, so every row starts 16-byte aligned.  All four kernels are 1-D copies of one shape: grid (chunk blocks, B), a
// lane moves one 16-byte chunk of the narrow side (16 frame values, 8 labels) with one 16-byte access and the 64 bytes of the
// wide side with four 16-byte accesses when the wide rows are 16-byte aligned too, with scalar accesses when they are not
// (row lengths that are no multiple of 4 floats / 2 labels).  The chunk that holds a row's tail goes value by value on both
// sides: pad bytes are never written by a store and never read by a gather.  No LDS besides the counters' block reduction.
// gx_cache_gather_aug is both gathers in one launch with the augmentation of genesis_amd/augment.py between the byte and the
// float: a 2-D grid of four-column quads instead, because a lane's source bytes depend on the frame's window.
#include "gx_common.h"
#include "gx_philox.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFrameChunk = 16, kLabelChunk = 8;          // values of a 16-byte chunk of the store

struct alignas(16) LL2 { long long x, y; };

// q = clamp(rint(v * 255), 0, 255), NaN -> 0; counts v against both ways back, as bits
__device__ __forceinline__ unsigned quantise(float v, int& div_miss, int& mul_miss) {
    const float r = rintf(v * 255.0f);
    const int q = r >= 0.0f ? (r <= 255.0f ? (int)r : 255) : 0;
    const unsigned bits = __float_as_uint(v);
    div_miss += bits != __float_as_uint((float)q / 255.0f);
    mul_miss += bits != __float_as_uint((float)q * (1.0f / 255.0f));
    return (unsigned)q;
}

template <int MODE>
__device__ __forceinline__ float to_unit(unsigned q) {
    return MODE ? (float)q * (1.0f / 255.0f) : (float)q / 255.0f;
}

// Adds every lane's N counts to counters[0 .. N): shuffles within the wave, LDS across the block's waves, then ONE atomic per
// non-zero counter and block.  Every thread of the block calls it.
template <int N>
__device__ __forceinline__ void block_counts_add(const int (&count)[N], unsigned long long* counters) {
    __shared__ int red[N][kWaves];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int v = count[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += red[threadIdx.x][w];
        if (total) atomicAdd(counters + threadIdx.x, (unsigned long long)total);
    }
}

// store[first_row + b][e] = quantise(batch[b][e]), e < n; counters[0] += div_miss, counters[1] += mul_miss
__global__ void __launch_bounds__(kThreads)
cache_store_u8_kernel(const float* __restrict__ batch, unsigned char* __restrict__ store, long long row_stride,
                      long long first_row, int n, int wide, unsigned long long* counters) {
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kFrameChunk;
    const int b = blockIdx.y;
    int count[2] = {0, 0};
    if (e0 < n) {
        const float* src = batch + (size_t)b * n + e0;
        unsigned char* dst = store + (size_t)(first_row + b) * row_stride + e0;
        if (e0 + kFrameChunk <= n) {
            float v[kFrameChunk];
            if (wide) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 f = reinterpret_cast<const float4*>(src)[i];
                    v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
                }
            } else {
#pragma unroll
                for (int i = 0; i < kFrameChunk; ++i) v[i] = src[i];
            }
            unsigned w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[i] |= quantise(v[4 * i + j], count[0], count[1]) << (8 * j);
            }
            *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            const int m = (int)(n - e0);
            for (int i = 0; i < m; ++i) dst[i] = (unsigned char)quantise(src[i], count[0], count[1]);
        }
    }
    block_counts_add<2>(count, counters);
}

// store[first_row + b][e] = (int16)labels[b][e]; counters[2] += the values outside -32768 .. 32767
__global__ void __launch_bounds__(kThreads)
cache_store_labels_i16_kernel(const long long* __restrict__ labels, short* __restrict__ store, long long row_stride,
                              long long first_row, int n, int wide, unsigned long long* counters) {
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kLabelChunk;
    const int b = blockIdx.y;
    int count[1] = {0};
    if (e0 < n) {
        const long long* src = labels + (size_t)b * n + e0;
        short* dst = reinterpret_cast<short*>(reinterpret_cast<unsigned char*>(store) + (size_t)(first_row + b) * row_stride) + e0;
        if (e0 + kLabelChunk <= n) {
            long long v[kLabelChunk];
            if (wide) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const LL2 p = reinterpret_cast<const LL2*>(src)[i];
                    v[2 * i] = p.x; v[2 * i + 1] = p.y;
                }
            } else {
#pragma unroll
                for (int i = 0; i < kLabelChunk; ++i) v[i] = src[i];
            }
            unsigned w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long lo = v[2 * i], hi = v[2 * i + 1];
                count[0] += (lo < -32768 || lo > 32767) + (hi < -32768 || hi > 32767);
                w[i] = ((unsigned)lo & 0xffffu) | (((unsigned)hi & 0xffffu) << 16);
            }
            *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            const int m = (int)(n - e0);
            for (int i = 0; i < m; ++i) {
                const long long l = src[i];
                count[0] += l < -32768 || l > 32767;
                dst[i] = (short)l;
            }
        }
    }
    block_counts_add<1>(count, counters + 2);
}

// out[b][e] = unit(store[row(b)][e]), row(b) = idx ? idx[first + b] : first + b
template <int MODE>
__global__ void __launch_bounds__(kThreads)
cache_gather_f32_kernel(const unsigned char* __restrict__ store, long long row_stride, const long long* __restrict__ idx,
                        long long first, float* __restrict__ out, int n, int wide) {
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kFrameChunk;
    if (e0 >= n) return;
    const int b = blockIdx.y;
    const long long row = idx ? idx[first + b] : first + b;
    const unsigned char* src = store + (size_t)row * row_stride + e0;
    float* dst = out + (size_t)b * n + e0;
    if (e0 + kFrameChunk <= n) {
        const uint4 p = *reinterpret_cast<const uint4*>(src);
        const unsigned w[4] = {p.x, p.y, p.z, p.w};
        float v[kFrameChunk];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * i + j] = to_unit<MODE>((w[i] >> (8 * j)) & 0xffu);
        if (wide) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                reinterpret_cast<float4*>(dst)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < kFrameChunk; ++i) dst[i] = v[i];
        }
    } else {
        const int m = (int)(n - e0);
        for (int i = 0; i < m; ++i) dst[i] = to_unit<MODE>(src[i]);
    }
}

// the same gather for the int16 label rows -> int64
__global__ void __launch_bounds__(kThreads)
cache_gather_labels_kernel(const short* __restrict__ store, long long row_stride, const long long* __restrict__ idx,
                           long long first, long long* __restrict__ out, int n, int wide) {
    const long long e0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kLabelChunk;
    if (e0 >= n) return;
    const int b = blockIdx.y;
    const long long row = idx ? idx[first + b] : first + b;
    const short* src = reinterpret_cast<const short*>(reinterpret_cast<const unsigned char*>(store) + (size_t)row * row_stride) + e0;
    long long* dst = out + (size_t)b * n + e0;
    if (e0 + kLabelChunk <= n) {
        const uint4 p = *reinterpret_cast<const uint4*>(src);
        const unsigned w[4] = {p.x, p.y, p.z, p.w};
        long long v[kLabelChunk];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = (long long)(short)(w[i] & 0xffffu);
            v[2 * i + 1] = (long long)(short)(w[i] >> 16);
        }
        if (wide) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                LL2 q;
                q.x = v[2 * i]; q.y = v[2 * i + 1];
                reinterpret_cast<LL2*>(dst)[i] = q;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kLabelChunk; ++i) dst[i] = v[i];
        }
    } else {
        const int m = (int)(n - e0);
        for (int i = 0; i < m; ++i) dst[i] = (long long)src[i];
    }
}

// ---- "augment v1": the two gathers above in one launch, with a left-right flip, a scale crop resampled back to H x W and a
//      brightness / colour gain per frame (the normative text: include/genesis_hip.h, gx_cache_gather_aug).  Every float
//      operation of the definition is rounded on its own, so the bodies below switch contraction off.
constexpr int kAugMaxDim = 32767;              // (2 x + 1) * w < 2 * kAugMaxDim^2 < 2^31: the tap arithmetic stays in int
struct AugParams { int flip, x0, y0, w, h; float g[3]; };

// 1 + amount * (2 * u(word) - 1); u and 2 * u - 1 are exact
__device__ __forceinline__ float aug_gain(float amount, unsigned word) {
#pragma clang fp contract(off)
    const float u = (float)(word >> 8) * 5.9604644775390625e-8f;
    return 1.0f + amount * (2.0f * u - 1.0f);
}

// The two taps (clamped to the window) and the fraction of output index o of `full`, over a window of `win` source values with
// half-pixel centres: s = (2 o + 1) win - full >= win - full > -2 full, so floor(s / (2 full)) is -1 for every negative s.
__device__ __forceinline__ void aug_taps(int o, int win, int full, int& i0, int& i1, float& f) {
#pragma clang fp contract(off)
    const int s = (2 * o + 1) * win - full, two = 2 * full;
    const int q = s >= 0 ? s / two : -1;
    f = (float)(s - q * two) / (float)two;
    i0 = max(q, 0);
    i1 = min(q + 1, win - 1);
}

// Grid (blocks over the H * ceil(W / 4) quads of a plane, B).  Wave 0 draws the frame's eight words (odd lanes call B, even
// lanes call A) and its lane 0 derives the parameters into LDS; after the barrier every lane reads them as broadcasts and
// produces four consecutive columns of one row: all C channels of the frame and the label.
template <int MODE>
__global__ void __launch_bounds__(kThreads)
cache_gather_aug_kernel(const unsigned char* __restrict__ frames, long long frame_stride, const short* __restrict__ labels,
                        long long label_stride, const long long* __restrict__ idx, long long first, unsigned long long seed,
                        unsigned epoch_lo, int flip_t, int wmin, float brightness, float colour, float* __restrict__ out,
                        long long* __restrict__ out_labels, int* __restrict__ params_out, int C, int H, int W, int wide) {
#pragma clang fp contract(off)
    __shared__ AugParams P;
    const int b = blockIdx.y;
    const long long row = idx ? idx[first + b] : first + b;
    if (threadIdx.x < 64) {
        unsigned r[4], rb[4];
        philox4x32_10((unsigned)row, (unsigned)((unsigned long long)row >> 32), epoch_lo, 0xA06u + (threadIdx.x & 1u),
                      (unsigned)seed, (unsigned)(seed >> 32), r);
#pragma unroll
        for (int k = 0; k < 4; ++k) rb[k] = (unsigned)__shfl((int)r[k], 1, 64);
        if (threadIdx.x == 0) {
            const int flip = (int)(r[0] >> 8) < flip_t;
            const int w = wmin + (int)(((unsigned long long)(r[1] >> 8) * (unsigned)(W - wmin + 1)) >> 24);
            const int h = min(max((w * H + W / 2) / W, 1), H);
            const int x0 = (int)(((unsigned long long)(r[2] >> 8) * (unsigned)(W - w + 1)) >> 24);
            const int y0 = (int)(((unsigned long long)(r[3] >> 8) * (unsigned)(H - h + 1)) >> 24);
            const float g = aug_gain(brightness, rb[0]);
            P.flip = flip; P.x0 = x0; P.y0 = y0; P.w = w; P.h = h;
#pragma unroll
            for (int c = 0; c < 3; ++c) P.g[c] = c < C ? g * aug_gain(colour, rb[1 + c]) : 1.0f;
            if (params_out && blockIdx.x == 0) {
                int* p = params_out + (size_t)b * 8;
                p[0] = flip; p[1] = x0; p[2] = y0; p[3] = w; p[4] = h;
#pragma unroll
                for (int c = 0; c < 3; ++c) p[5 + c] = __float_as_int(P.g[c]);
            }
        }
    }
    __syncthreads();
    const int Wq = (W + 3) >> 2;
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= H * Wq) return;
    const int y = q / Wq, x4 = (q - y * Wq) * 4;
    const int flip = P.flip, x0 = P.x0, y0 = P.y0, w = P.w, h = P.h;

    int j0, j1, i0[4], i1[4], lx[4];
    float fy, fx[4];
    aug_taps(y, h, H, j0, j1, fy);
    const int ly = ((2 * y + 1) * h) / (2 * H);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(x4 + k, W - 1);                    // (a quad's columns past the row's end repeat the last one: read, not stored)
        const int xs = flip ? W - 1 - x : x;
        aug_taps(xs, w, W, i0[k], i1[k], fx[k]);
        lx[k] = ((2 * xs + 1) * w) / (2 * W);
    }
    const int m = min(4, W - x4);                            // the quad's columns inside the row
    const int plane = H * W;
    const unsigned char* src = frames + (size_t)row * frame_stride + x0;
    const int top_row = (y0 + j0) * W, bot_row = (y0 + j1) * W;
    float* dst = out + (size_t)b * C * plane + (size_t)y * W + x4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < C) {
            const unsigned char* sp = src + (size_t)c * plane;
            const float gain = P.g[c];
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a00 = (float)sp[top_row + i0[k]], a01 = (float)sp[top_row + i1[k]];
                const float a10 = (float)sp[bot_row + i0[k]], a11 = (float)sp[bot_row + i1[k]];
                const float top = a00 + (a01 - a00) * fx[k];
                const float bot = a10 + (a11 - a10) * fx[k];
                const float t = fminf((top + (bot - top) * fy) * gain, 255.0f);
                v[k] = MODE ? t * (1.0f / 255.0f) : t / 255.0f;
            }
            float* d = dst + (size_t)c * plane;
            if (wide) {
                *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < m) d[k] = v[k];
            }
        }
    }
    if (labels) {
        const short* lp = reinterpret_cast<const short*>(reinterpret_cast<const unsigned char*>(labels) + (size_t)row * label_stride) +
                          (size_t)(y0 + ly) * W + x0;
        long long l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) l[k] = (long long)lp[lx[k]];
        long long* d = out_labels + (size_t)b * plane + (size_t)y * W + x4;
        if (wide) {
            LL2 p0, p1;
            p0.x = l[0]; p0.y = l[1]; p1.x = l[2]; p1.y = l[3];
            reinterpret_cast<LL2*>(d)[0] = p0;
            reinterpret_cast<LL2*>(d)[1] = p1;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < m) d[k] = l[k];
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

dim3 chunk_grid(long long n, int chunk, int B) {
    const long long chunks = (n + chunk - 1) / chunk;
    return dim3((unsigned)((chunks + kThreads - 1) / kThreads), (unsigned)B);
}

// what all four entry points require of the batch and of the store's geometry; n = values of a row, esz their size in the store
const char* common_args_error(const void* a, const void* b, int B, long long n, int esz, long long row_stride) {
    if (!a || !b) return "null pointer";
    if (!(B > 0 && B <= 65535 && n > 0)) return "bad dims (B at most 65535)";
    if (n >= (1ll << 31)) return "frame too large";
    if (row_stride <= 0 || row_stride % 16 != 0) return "the row stride must be a positive multiple of 16 bytes";
    if (row_stride < n * esz) return "the row stride is shorter than a row";
    return nullptr;
}

const char* store_args_error(const void* batch, const void* store, const void* counters, int B, long long n, int esz,
                             long long row_stride, long long first_row, long long capacity_rows) {
    if (!counters) return "null pointer";
    if (const char* err = common_args_error(batch, store, B, n, esz, row_stride)) return err;
    if (!aligned16(store)) return "the store must be 16-byte aligned";
    if (((uintptr_t)counters & 7) != 0) return "the counters must be 8-byte aligned";
    if (first_row < 0) return "negative first_row";
    if (capacity_rows <= 0 || first_row + B > capacity_rows) return "rows first_row .. first_row + B reach past the store's capacity";
    return nullptr;
}

// gather_args_error of gx_multid.hip, for a store of `rows` rows
const char* gather_args_error(const void* store, const void* out, const long long* idx, long long idx_len, long long first,
                              long long rows, int B, long long n, int esz, long long row_stride) {
    if (const char* err = common_args_error(store, out, B, n, esz, row_stride)) return err;
    if (rows <= 0) return "bad dims (B at most 65535)";
    if (!aligned16(store)) return "the store must be 16-byte aligned";
    if (first < 0) return "negative first";
    if (idx ? first + B > idx_len : first + B > rows) return "rows first .. first + B reach past the index vector (or, without one, past the store)";
    return nullptr;
}

long long row_values(int C, int H, int W) {
    return (C > 0 && H > 0 && W > 0) ? (long long)C * H * W : 0;       // 0: refused as bad dims
}

}  // namespace

extern "C" {

int gx_cache_store_u8(const float* batch, unsigned char* store, long long row_stride, long long first_row,
                      long long capacity_rows, long long* counters, int B, int C, int H, int W, gx_stream_t stream) {
    const long long n = row_values(C, H, W);
    const char* err = store_args_error(batch, store, counters, B, n, 1, row_stride, first_row, capacity_rows);
    GX_CHECK_ARG(!err, "gx_cache_store_u8: %s", err ? err : "");
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 5.0 * B * n);
        hipLaunchKernelGGL(cache_store_u8_kernel, chunk_grid(n, kFrameChunk, B), dim3(kThreads), 0, s, batch, store, row_stride,
                           first_row, (int)n, (int)(n % 4 == 0 && aligned16(batch)), (unsigned long long*)counters);
    }
    GX_CHECK_LAUNCH("gx_cache_store_u8");
    return GX_OK;
}

int gx_cache_store_labels_i16(const long long* labels, short* store, long long row_stride, long long first_row,
                              long long capacity_rows, long long* counters, int B, int H, int W, gx_stream_t stream) {
    const long long n = row_values(1, H, W);
    const char* err = store_args_error(labels, store, counters, B, n, 2, row_stride, first_row, capacity_rows);
    GX_CHECK_ARG(!err, "gx_cache_store_labels_i16: %s", err ? err : "");
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 10.0 * B * n);
        hipLaunchKernelGGL(cache_store_labels_i16_kernel, chunk_grid(n, kLabelChunk, B), dim3(kThreads), 0, s, labels, store,
                           row_stride, first_row, (int)n, (int)(n % 2 == 0 && aligned16(labels)), (unsigned long long*)counters);
    }
    GX_CHECK_LAUNCH("gx_cache_store_labels_i16");
    return GX_OK;
}

int gx_cache_gather_f32(const unsigned char* store, long long row_stride, long long rows, const long long* idx, long long idx_len,
                        long long first, int mode, float* out, int B, int C, int H, int W, gx_stream_t stream) {
    const long long n = row_values(C, H, W);
    const char* err = gather_args_error(store, out, idx, idx_len, first, rows, B, n, 1, row_stride);
    GX_CHECK_ARG(!err, "gx_cache_gather_f32: %s", err ? err : "");
    GX_CHECK_ARG(mode == GX_CACHE_DIV255 || mode == GX_CACHE_MUL255, "gx_cache_gather_f32: bad mode %d", mode);
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 5.0 * B * n);
        const dim3 grid = chunk_grid(n, kFrameChunk, B);
        const int wide = n % 4 == 0 && aligned16(out);
        if (mode == GX_CACHE_DIV255)
            hipLaunchKernelGGL(cache_gather_f32_kernel<0>, grid, dim3(kThreads), 0, s, store, row_stride, idx, first, out, (int)n, wide);
        else
            hipLaunchKernelGGL(cache_gather_f32_kernel<1>, grid, dim3(kThreads), 0, s, store, row_stride, idx, first, out, (int)n, wide);
    }
    GX_CHECK_LAUNCH("gx_cache_gather_f32");
    return GX_OK;
}

int gx_cache_gather_labels(const short* store, long long row_stride, long long rows, const long long* idx, long long idx_len,
                           long long first, long long* out, int B, int H, int W, gx_stream_t stream) {
    const long long n = row_values(1, H, W);
    const char* err = gather_args_error(store, out, idx, idx_len, first, rows, B, n, 2, row_stride);
    GX_CHECK_ARG(!err, "gx_cache_gather_labels: %s", err ? err : "");
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 10.0 * B * n);
        hipLaunchKernelGGL(cache_gather_labels_kernel, chunk_grid(n, kLabelChunk, B), dim3(kThreads), 0, s, store, row_stride, idx,
                           first, out, (int)n, (int)(n % 2 == 0 && aligned16(out)));
    }
    GX_CHECK_LAUNCH("gx_cache_gather_labels");
    return GX_OK;
}

int gx_cache_gather_aug(const unsigned char* frames, long long frame_stride, const short* labels, long long label_stride,
                        long long rows, const long long* idx, long long idx_len, long long first, int mode,
                        unsigned long long seed, long long epoch, int flip_t, int wmin, float brightness, float colour, float* out,
                        long long* out_labels, int* params_out, int B, int C, int H, int W, gx_stream_t stream) {
    const long long n = row_values(C, H, W);
    const char* err = gather_args_error(frames, out, idx, idx_len, first, rows, B, n, 1, frame_stride);
    GX_CHECK_ARG(!err, "gx_cache_gather_aug: %s", err ? err : "");
    GX_CHECK_ARG(mode == GX_CACHE_DIV255 || mode == GX_CACHE_MUL255, "gx_cache_gather_aug: bad mode %d", mode);
    GX_CHECK_ARG(C <= 3, "gx_cache_gather_aug: at most 3 channels (one colour gain each), not %d", C);
    GX_CHECK_ARG(H <= kAugMaxDim && W <= kAugMaxDim, "gx_cache_gather_aug: frame too large (H and W at most %d)", kAugMaxDim);
    GX_CHECK_ARG((labels != nullptr) == (out_labels != nullptr),
                 "gx_cache_gather_aug: labels and out_labels go together: both or neither");
    if (labels) {
        err = gather_args_error(labels, out_labels, idx, idx_len, first, rows, B, (long long)H * W, 2, label_stride);
        GX_CHECK_ARG(!err, "gx_cache_gather_aug: labels: %s", err ? err : "");
    }
    GX_CHECK_ARG(epoch >= 0, "gx_cache_gather_aug: negative epoch");
    GX_CHECK_ARG(flip_t >= 0 && flip_t <= (1 << 24), "gx_cache_gather_aug: flip_t %d outside [0, 2^24]", flip_t);
    GX_CHECK_ARG(wmin >= 1 && wmin <= W, "gx_cache_gather_aug: wmin %d outside [1, W = %d]", wmin, W);
    GX_CHECK_ARG(brightness >= 0.0f && brightness < 1.0f, "gx_cache_gather_aug: brightness %g outside [0, 1)", (double)brightness);
    GX_CHECK_ARG(colour >= 0.0f && colour < 1.0f, "gx_cache_gather_aug: colour %g outside [0, 1)", (double)colour);
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (labels ? 15.0 : 5.0) * B * n);
        const long long quads = (long long)H * ((W + 3) / 4);
        const dim3 grid((unsigned)((quads + kThreads - 1) / kThreads), (unsigned)B);
        const int wide = W % 4 == 0 && aligned16(out) && aligned16(out_labels);
        if (mode == GX_CACHE_DIV255)
            hipLaunchKernelGGL(cache_gather_aug_kernel<0>, grid, dim3(kThreads), 0, s, frames, frame_stride, labels, label_stride, idx,
                               first, seed, (unsigned)epoch, flip_t, wmin, brightness, colour, out, out_labels, params_out, C, H, W, wide);
        else
            hipLaunchKernelGGL(cache_gather_aug_kernel<1>, grid, dim3(kThreads), 0, s, frames, frame_stride, labels, label_stride, idx,
                               first, seed, (unsigned)epoch, flip_t, wmin, brightness, colour, out, out_labels, params_out, C, H, W, wide);
    }
    GX_CHECK_LAUNCH("gx_cache_gather_aug");
    return GX_OK;
}

}  // extern "C"
