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
#include "gx_common.h"

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

}  // extern "C"
