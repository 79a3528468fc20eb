// The device side of the TensorBoard event-file writer (genesis_amd/tbwriter.py; contract: include/genesis_hip.h, gx_scalar_snapshot
// and gx_png_pack).
// gx_scalar_snapshot: tensorboardX's add_scalar reads a device scalar with one blocking copy per call.  Here up to 32 scalars are
// copied, in stream order, into fp64 slots of a device ring by ONE small launch whose (address, dtype) pairs travel by value in the
// kernel arguments: nothing is uploaded and nothing is read back until the writer flushes.
// gx_png_pack: ONE launch turns every picture of a logging event into the byte stream zlib deflates for a PNG: per row the
// filter-type byte and the filtered bytes.  A wave owns one row: it derives the bytes of its row and of the row above from the
// source (fp32 through trunc(clamp(x, 0, 1) * 255), NaN -> 0; uint8 as it is; int64 clamped to 0..255) into LDS, sums |signed byte|
// of the five PNG filters over the row, folds the sums across the wave, and writes the filter with the smallest sum (ties: the lowest
// number).  Rows depend on nothing but the source, so there is no hand-over between waves or workgroups.
#include "gx_common.h"

static_assert(GX_PNGPACK_MAX_DIM == kGxPngMaxDim, "GX_PNGPACK_MAX_DIM and kGxPngMaxDim disagree");

namespace {

// ---- scalars ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
scalar_snapshot_kernel(gx_scalar_refs refs, int n, double* __restrict__ ring) {
    const int i = threadIdx.x;
    if (i >= n) return;
    const void* p = refs.ptr[i];
    double v;
    switch (refs.dtype[i]) {
        case GX_SCALAR_FP32: v = (double)*reinterpret_cast<const float*>(p); break;
        case GX_SCALAR_FP64: v = *reinterpret_cast<const double*>(p); break;
        case GX_SCALAR_I32: v = (double)*reinterpret_cast<const int*>(p); break;
        default: v = (double)*reinterpret_cast<const long long*>(p); break;
    }
    ring[i] = v;
}

// ---- pictures --------------------------------------------------------------------------------------------------------------------
constexpr int kPackWavesWide = 4;       // rows per workgroup while the rows are short ...
constexpr int kPackWideBytes = 4096;    // ... up to this many bytes; one row per workgroup beyond (2 x 12 KB of LDS per row at most)

// the byte of one source element (the writer's byte rule)
__device__ __forceinline__ unsigned pack_byte(const unsigned char* __restrict__ src, long long e, int kind) {
    if (kind == GX_PNGPACK_FP32) {
        const float x = reinterpret_cast<const float*>(src)[e];
        if (x != x) return 0u;
        return (unsigned)(int)(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f);      // (fp32 product, truncated)
    }
    if (kind == GX_PNGPACK_U8) return src[e];
    const long long v = reinterpret_cast<const long long*>(src)[e];
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ unsigned pack_abs(unsigned v) {      // |v as a signed byte|, v already mod 256
    return v < 128u ? v : 256u - v;
}

// the five filtered bytes of x with left a, above b, above-left c (PNG specification, section 9; all mod 256)
__device__ __forceinline__ void pack_filters(unsigned x, unsigned a, unsigned b, unsigned c, unsigned (&f)[5]) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    const unsigned pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    f[0] = x;
    f[1] = (x - a) & 255u;
    f[2] = (x - b) & 255u;
    f[3] = (x - ((a + b) >> 1)) & 255u;
    f[4] = (x - pred) & 255u;
}

__global__ void __launch_bounds__(64 * kPackWavesWide)
png_pack_kernel(const long long* __restrict__ table, int P, long long total_rows, int row_lds, unsigned char* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_rows[];      // per wave: the row, then the row above
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    const bool live = r < total_rows;      // (a wave past the last row still meets the barrier)
    unsigned char* cur = s_rows + (size_t)wave * 2 * row_lds;
    unsigned char* prev = cur + row_lds;
    const long long* d = table;
    int C = 1, W = 0, y = 0, n = 0;
    if (live) {
        int lo = 0, hi = P - 1;      // the last picture whose first row is <= r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[(size_t)mid * GX_PNGPACK_DESC_WORDS + GX_PNGPACK_D_ROW0] <= r) lo = mid; else hi = mid - 1;
        }
        d = table + (size_t)lo * GX_PNGPACK_DESC_WORDS;
        C = (int)d[GX_PNGPACK_D_C]; W = (int)d[GX_PNGPACK_D_W];
        y = (int)(r - d[GX_PNGPACK_D_ROW0]);
        n = W * C;
        const unsigned char* src = reinterpret_cast<const unsigned char*>(d[GX_PNGPACK_D_SRC]);
        const int kind = (int)d[GX_PNGPACK_D_KIND];
        const long long ps = d[GX_PNGPACK_D_PIX_STRIDE], rs = d[GX_PNGPACK_D_ROW_STRIDE], cs = d[GX_PNGPACK_D_CH_STRIDE];
        for (int j = lane; j < n; j += 64) {
            const int x = C == 1 ? j : j / 3, c = j - x * C;
            const long long e = x * ps + c * cs + y * rs;
            cur[j] = (unsigned char)pack_byte(src, e, kind);
            prev[j] = y > 0 ? (unsigned char)pack_byte(src, e - rs, kind) : (unsigned char)0;
        }
    }
    __syncthreads();
    if (!live) return;
    unsigned sum[5] = {0u, 0u, 0u, 0u, 0u};
    for (int j = lane; j < n; j += 64) {
        const unsigned a = j >= C ? cur[j - C] : 0u, c = j >= C ? prev[j - C] : 0u;
        unsigned f[5];
        pack_filters(cur[j], a, prev[j], c, f);
#pragma unroll
        for (int k = 0; k < 5; ++k) sum[k] += pack_abs(f[k]);
    }
    int best = 0;
    unsigned best_sum = 0u;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum[k] += __shfl_xor(sum[k], off, 64);
        if (k == 0 || sum[k] < best_sum) { best = k; best_sum = sum[k]; }
    }
    unsigned char* dst = out + d[GX_PNGPACK_D_DST] + (long long)y * (1 + n);
    if (lane == 0) dst[0] = (unsigned char)best;
    for (int j = lane; j < n; j += 64) {
        const unsigned a = j >= C ? cur[j - C] : 0u, c = j >= C ? prev[j - C] : 0u;
        unsigned f[5];
        pack_filters(cur[j], a, prev[j], c, f);
        dst[1 + j] = (unsigned char)f[best];
    }
}

}  // namespace

extern "C" {

int gx_scalar_snapshot(const gx_scalar_refs* refs, int n, double* ring, int ring_slots, int first_slot, gx_stream_t stream) {
    GX_CHECK_ARG(refs && ring, "gx_scalar_snapshot: null pointer");
    GX_CHECK_ARG(n >= 1 && n <= GX_SCALAR_MAX_REFS, "gx_scalar_snapshot: n = %d outside [1, %d]", n, GX_SCALAR_MAX_REFS);
    GX_CHECK_ARG((reinterpret_cast<uintptr_t>(ring) & 7) == 0, "gx_scalar_snapshot: ring must be 8-byte aligned");
    GX_CHECK_ARG(ring_slots >= 1 && first_slot >= 0 && (long long)first_slot + n <= ring_slots,
                 "gx_scalar_snapshot: slots %d .. %lld lie outside a ring of %d", first_slot, (long long)first_slot + n - 1, ring_slots);
    for (int i = 0; i < n; ++i) {
        const int dtype = refs->dtype[i];
        const uintptr_t p = reinterpret_cast<uintptr_t>(refs->ptr[i]);
        GX_CHECK_ARG(dtype == GX_SCALAR_FP32 || dtype == GX_SCALAR_FP64 || dtype == GX_SCALAR_I32 || dtype == GX_SCALAR_I64,
                     "gx_scalar_snapshot: value %d: unknown dtype %d", i, dtype);
        GX_CHECK_ARG(p, "gx_scalar_snapshot: value %d: null address", i);
        const int size = (dtype == GX_SCALAR_FP32 || dtype == GX_SCALAR_I32) ? 4 : 8;
        GX_CHECK_ARG((p & (size - 1)) == 0, "gx_scalar_snapshot: value %d: address %#llx is not aligned to its %d-byte element", i,
                     (unsigned long long)p, size);
    }
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 16.0 * n);
        hipLaunchKernelGGL(scalar_snapshot_kernel, dim3(1), dim3(64), 0, s, *refs, n, ring + first_slot);
    }
    GX_CHECK_LAUNCH("gx_scalar_snapshot");
    return GX_OK;
}

int gx_png_pack(const long long* table_host, const long long* table_dev, long long table_words, int n_pictures, unsigned char* out,
                long long out_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(table_host && table_dev && out, "gx_png_pack: null pointer");
    GX_CHECK_ARG(n_pictures >= 1, "gx_png_pack: n_pictures = %d below 1", n_pictures);
    GX_CHECK_ARG(table_words >= (long long)n_pictures * GX_PNGPACK_DESC_WORDS, "gx_png_pack: %d pictures do not fit a table of %lld words",
                 n_pictures, table_words);
    long long rows = 0, bytes = 0;
    int widest = 0;
    double read = 0.0;
    for (int i = 0; i < n_pictures; ++i) {
        const long long* d = table_host + (size_t)i * GX_PNGPACK_DESC_WORDS;
        const long long kind = d[GX_PNGPACK_D_KIND], C = d[GX_PNGPACK_D_C], H = d[GX_PNGPACK_D_H], W = d[GX_PNGPACK_D_W];
        const uintptr_t src = (uintptr_t)d[GX_PNGPACK_D_SRC];
        GX_CHECK_ARG(kind == GX_PNGPACK_FP32 || kind == GX_PNGPACK_U8 || kind == GX_PNGPACK_I64, "gx_png_pack: picture %d: unknown kind %lld",
                     i, kind);
        GX_CHECK_ARG(C == 1 || C == 3, "gx_png_pack: picture %d: C = %lld is neither 1 nor 3", i, C);
        GX_CHECK_ARG(H >= 1 && H <= GX_PNGPACK_MAX_DIM && W >= 1 && W <= GX_PNGPACK_MAX_DIM,
                     "gx_png_pack: picture %d: H = %lld, W = %lld outside [1, %d]", i, H, W, GX_PNGPACK_MAX_DIM);
        GX_CHECK_ARG(src, "gx_png_pack: picture %d: null source", i);
        const int size = kind == GX_PNGPACK_FP32 ? 4 : (kind == GX_PNGPACK_U8 ? 1 : 8);
        GX_CHECK_ARG((src & (size - 1)) == 0, "gx_png_pack: picture %d: source %#llx is not aligned to its %d-byte elements", i,
                     (unsigned long long)src, size);
        GX_CHECK_ARG(d[GX_PNGPACK_D_PIX_STRIDE] >= 1 && d[GX_PNGPACK_D_ROW_STRIDE] >= 1 && d[GX_PNGPACK_D_CH_STRIDE] >= (C == 3 ? 1 : 0),
                     "gx_png_pack: picture %d: strides (%lld, %lld, %lld) must be positive", i, d[GX_PNGPACK_D_PIX_STRIDE],
                     d[GX_PNGPACK_D_ROW_STRIDE], d[GX_PNGPACK_D_CH_STRIDE]);
        GX_CHECK_ARG(d[GX_PNGPACK_D_DST] == bytes, "gx_png_pack: picture %d: DST = %lld, the prefix is %lld", i, d[GX_PNGPACK_D_DST], bytes);
        GX_CHECK_ARG(d[GX_PNGPACK_D_ROW0] == rows, "gx_png_pack: picture %d: ROW0 = %lld, the prefix is %lld", i, d[GX_PNGPACK_D_ROW0], rows);
        rows += H;
        bytes += H * (1 + W * C);
        read += (double)H * W * C * size;
        if ((int)(W * C) > widest) widest = (int)(W * C);
    }
    GX_CHECK_ARG(bytes <= out_bytes, "gx_png_pack: the streams take %lld bytes, out holds %lld", bytes, out_bytes);
    const int row_lds = gx_round_up(widest, 16);
    const int waves = widest <= kPackWideBytes ? kPackWavesWide : 1;
    const long long blocks = (rows + waves - 1) / waves;
    GX_CHECK_ARG(blocks < (1LL << 31), "gx_png_pack: %lld rows are too many for one launch", rows);
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 2.0 * read + (double)bytes);
        hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)blocks), dim3(64 * waves), (size_t)waves * 2 * row_lds, s, table_dev, n_pictures,
                           rows, row_lds, out);
    }
    GX_CHECK_LAUNCH("gx_png_pack");
    return GX_OK;
}

}  // extern "C"
