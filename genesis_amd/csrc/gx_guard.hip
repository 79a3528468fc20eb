// Gradient guard of the training step (contract: include/genesis_hip.h, gx_grad_guard): the global L2 norm of any number of
// gradient segments, the clip_grad_norm_ coefficient and the "every value is finite" flag as one small device record that the
// guarded tail launches of gx_optim.hip (and gx_scale_multi_guarded below) read -- no host read, no branch on the host.
// torch.nn.utils.clip_grad_norm_ is a norm launch per parameter, a stack, a norm, a clamp and a multiply per parameter;
// torch.isfinite(...).item() is a host read.  Here the whole set is ONE streaming pass: a workgroup walks chunks of
// GX_GUARD_CHUNK elements in a fixed grid-stride order (the segment of a chunk is found by bisecting the descriptors' work prefix,
// as gx_hist_multi does), 16-byte loads from the first 16-byte boundary of a chunk and element loads at its ragged ends, the
// squares added in fp64 into kGuardUnroll independent accumulators per thread, then thread -> wave -> workgroup into one partial
// per workgroup; a second one-workgroup launch adds the partials in order and writes the record.  No floating-point atomic and
// no hand-over between workgroups inside a launch: two calls on the same input write the same bits, and the workspace needs no
// clearing.
#include "gx_common.h"

namespace {

constexpr int kGuardThreads = 256;
constexpr int kGuardUnroll = 4;      // 16-byte loads in flight per thread, one fp64 accumulator each

typedef double f64x2 __attribute__((ext_vector_type(2)));
template <typename T> struct GuardVec;
template <> struct GuardVec<float> { typedef f32x4 type; };
template <> struct GuardVec<double> { typedef f64x2 type; };

static_assert(sizeof(GxGuardRecord) == GX_GUARD_RECORD_BYTES, "the record of include/genesis_hip.h");

// the last segment whose first chunk is <= w
__device__ __forceinline__ int guard_segment(const long long* __restrict__ table, int S, long long w) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * GX_GUARD_DESC_WORDS + GX_GUARD_D_WORK] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// where the 16-byte accesses of a chunk of n elements at p (aligned to its element only) begin and end
template <typename T>
__device__ __forceinline__ void guard_split(const T* p, int n, int& head, int& nv, int& rest0) {
    constexpr int V = 16 / (int)sizeof(T);
    const int to_boundary = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
    head = to_boundary < n ? to_boundary : n;
    nv = (n - head) / V;
    rest0 = head + nv * V;
}

template <typename T>
__device__ __forceinline__ void guard_scan(const T* __restrict__ p, int n, double (&acc)[kGuardUnroll]) {
    typedef typename GuardVec<T>::type Vec;
    constexpr int V = 16 / (int)sizeof(T);
    const int t = threadIdx.x;
    int head, nv, rest0;
    guard_split(p, n, head, nv, rest0);
    // the ragged ends (fewer than V elements each): thread t takes element t of the head and element t of the rest
    if (t < head) { const double x = (double)p[t]; acc[0] = fma(x, x, acc[0]); }
    if (t < n - rest0) { const double x = (double)p[rest0 + t]; acc[1] = fma(x, x, acc[1]); }
    const Vec* __restrict__ pv = reinterpret_cast<const Vec*>(p + head);
    for (int i0 = 0; i0 < nv; i0 += kGuardThreads * kGuardUnroll) {
        Vec q[kGuardUnroll];
#pragma unroll
        for (int u = 0; u < kGuardUnroll; ++u) {
            const int i = i0 + u * kGuardThreads + t;
            q[u] = Vec{};                                    // (+0 squared adds nothing and hides no NaN)
            if (i < nv) q[u] = pv[i];
        }
#pragma unroll
        for (int u = 0; u < kGuardUnroll; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) { const double x = (double)q[u][j]; acc[u] = fma(x, x, acc[u]); }
        }
    }
}

__global__ void __launch_bounds__(kGuardThreads)
guard_partial_kernel(const long long* __restrict__ table, int S, long long work, double* __restrict__ parts) {
    __shared__ double s_w[kGuardThreads / 64];
    const int t = threadIdx.x;
    double acc[kGuardUnroll];
#pragma unroll
    for (int u = 0; u < kGuardUnroll; ++u) acc[u] = 0.0;
    for (long long w = blockIdx.x; w < work; w += gridDim.x) {
        const long long* d = table + (size_t)guard_segment(table, S, w) * GX_GUARD_DESC_WORDS;
        const long long N = d[GX_GUARD_D_N], first = (w - d[GX_GUARD_D_WORK]) * GX_GUARD_CHUNK;
        const int n = (int)(N - first < GX_GUARD_CHUNK ? N - first : GX_GUARD_CHUNK);
        if (d[GX_GUARD_D_DTYPE] == GX_GUARD_FP32)
            guard_scan<float>(reinterpret_cast<const float*>(d[GX_GUARD_D_SRC]) + first, n, acc);
        else
            guard_scan<double>(reinterpret_cast<const double*>(d[GX_GUARD_D_SRC]) + first, n, acc);
    }
    // thread -> wave (xor butterfly: every lane ends with the same bits) -> workgroup, waves in order
    double a = gx_wave_sum_d((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((t & 63) == 0) s_w[t >> 6] = a;
    __syncthreads();
    if (t == 0) parts[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order, then wave, then workgroup; thread 0 writes the record
__global__ void __launch_bounds__(kGuardThreads)
guard_final_kernel(const double* __restrict__ parts, int nparts, const float* __restrict__ check, int n_check, float gscale,
                   double max_norm, int force_ok, GxGuardRecord* __restrict__ rec) {
    __shared__ double s_w[kGuardThreads / 64];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int i = t; i < nparts; i += kGuardThreads) a += parts[i];
    a = gx_wave_sum_d(a);
    if ((t & 63) == 0) s_w[t >> 6] = a;
    __syncthreads();
    if (t != 0) return;
    {
#pragma clang fp contract(off)
    const double S = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    bool finite = __builtin_isfinite(S);
    for (int k = 0; k < n_check; ++k) finite = finite && __builtin_isfinite(check[k]);
    const double norm = (double)gscale * sqrt(S);
    double c = 1.0;
    if (max_norm > 0.0) {
        c = max_norm / (norm + 1e-6);                        // torch.nn.utils.clip_grad_norm_
        c = c < 1.0 ? c : (c != c ? c : 1.0);                // torch.clamp(c, max=1.0): a NaN stays a NaN
    }
    const float coef = (float)c;
    rec->S = S;
    rec->norm = (float)norm;
    rec->coef = coef;
    rec->scale = gscale * coef;                              // ONE fp32 multiply: what the optimiser launch receives as gscale
    rec->ok = (force_ok || finite) ? 1 : 0;                  // (skipped: cumulative, owned by the guarded tail launches)
    }
}

template <typename T>
__device__ __forceinline__ void scale_chunk(T* p, int n, T c) {
    typedef typename GuardVec<T>::type Vec;
    constexpr int V = 16 / (int)sizeof(T);
    const int t = threadIdx.x;
    int head, nv, rest0;
    guard_split(p, n, head, nv, rest0);
    if (t < head) p[t] = p[t] * c;
    if (t < n - rest0) p[rest0 + t] = p[rest0 + t] * c;
    Vec* pv = reinterpret_cast<Vec*>(p + head);
    for (int i0 = 0; i0 < nv; i0 += kGuardThreads * kGuardUnroll) {
        Vec q[kGuardUnroll];
#pragma unroll
        for (int u = 0; u < kGuardUnroll; ++u) {
            const int i = i0 + u * kGuardThreads + t;
            if (i < nv) q[u] = pv[i];
        }
#pragma unroll
        for (int u = 0; u < kGuardUnroll; ++u) {
            const int i = i0 + u * kGuardThreads + t;
            if (i < nv) pv[i] = q[u] * c;
        }
    }
}

// every element times the record's coef, in the element's type; coef == 1: nothing is read or written
__global__ void __launch_bounds__(kGuardThreads)
scale_multi_kernel(const long long* __restrict__ table, int S, long long work, const GxGuardRecord* __restrict__ rec) {
    const float coef = rec->coef;
    if (coef == 1.f) return;
    for (long long w = blockIdx.x; w < work; w += gridDim.x) {
        const long long* d = table + (size_t)guard_segment(table, S, w) * GX_GUARD_DESC_WORDS;
        const long long N = d[GX_GUARD_D_N], first = (w - d[GX_GUARD_D_WORK]) * GX_GUARD_CHUNK;
        const int n = (int)(N - first < GX_GUARD_CHUNK ? N - first : GX_GUARD_CHUNK);
        if (d[GX_GUARD_D_DTYPE] == GX_GUARD_FP32)
            scale_chunk<float>(reinterpret_cast<float*>(d[GX_GUARD_D_SRC]) + first, n, coef);
        else
            scale_chunk<double>(reinterpret_cast<double*>(d[GX_GUARD_D_SRC]) + first, n, (double)coef);
    }
}

// the descriptor table as the host holds it: GX_EINVAL-style checks shared by the two entry points.  -> 0, or the message is set
int guard_check_table(const char* who, const long long* table_host, const long long* table_dev, long long table_words,
                      int n_segments, long long* work_out, double* bytes_out) {
    GX_CHECK_ARG(table_host && table_dev, "%s: null descriptor table", who);
    GX_CHECK_ARG(n_segments >= 1, "%s: n_segments = %d below 1", who, n_segments);
    GX_CHECK_ARG(table_words >= (long long)n_segments * GX_GUARD_DESC_WORDS, "%s: %d segments do not fit a table of %lld words", who,
                 n_segments, table_words);
    GX_CHECK_ARG((reinterpret_cast<uintptr_t>(table_dev) & 7) == 0, "%s: the device table must be 8-byte aligned", who);
    long long work = 0;
    double bytes = 0.0;
    for (int si = 0; si < n_segments; ++si) {
        const long long* d = table_host + (size_t)si * GX_GUARD_DESC_WORDS;
        const long long N = d[GX_GUARD_D_N], dtype = d[GX_GUARD_D_DTYPE];
        const uintptr_t src = (uintptr_t)d[GX_GUARD_D_SRC];
        GX_CHECK_ARG(dtype == GX_GUARD_FP32 || dtype == GX_GUARD_FP64, "%s: segment %d: unknown dtype %lld", who, si, dtype);
        GX_CHECK_ARG(N >= 1 && N < (1LL << 31), "%s: segment %d: N = %lld outside [1, 2^31)", who, si, N);
        GX_CHECK_ARG(src, "%s: segment %d: null source", who, si);
        GX_CHECK_ARG((src & (dtype == GX_GUARD_FP32 ? 3 : 7)) == 0, "%s: segment %d: source %#llx is not aligned to its %d-byte elements",
                     who, si, (unsigned long long)src, dtype == GX_GUARD_FP32 ? 4 : 8);
        GX_CHECK_ARG(d[GX_GUARD_D_WORK] == work, "%s: segment %d: WORK = %lld, the prefix is %lld", who, si, d[GX_GUARD_D_WORK], work);
        work += (N + GX_GUARD_CHUNK - 1) / GX_GUARD_CHUNK;
        bytes += (double)N * (dtype == GX_GUARD_FP32 ? 4 : 8);
    }
    GX_CHECK_ARG(work < (1LL << 31), "%s: %lld chunks are too many for one launch", who, work);
    *work_out = work;
    *bytes_out = bytes;
    return GX_OK;
}

}  // namespace

extern "C" {

size_t gx_grad_guard_ws_bytes(long long total_chunks) {
    const long long g = total_chunks < 1 ? 1 : (total_chunks < GX_GUARD_MAX_GRID ? total_chunks : GX_GUARD_MAX_GRID);
    return (size_t)g * sizeof(double);
}

int gx_grad_guard(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                  const float* check, int n_check, float gscale, double max_norm, int force_ok, void* record, void* ws,
                  size_t ws_bytes, gx_stream_t stream) {
    long long work = 0;
    double bytes = 0.0;
    const int rc = guard_check_table("gx_grad_guard", table_host, table_dev, table_words, n_segments, &work, &bytes);
    if (rc != GX_OK) return rc;
    GX_CHECK_ARG(record && ws, "gx_grad_guard: null record or workspace");
    GX_CHECK_ARG(((reinterpret_cast<uintptr_t>(record) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                 "gx_grad_guard: record and ws must be 8-byte aligned");
    GX_CHECK_ARG(n_check >= 0 && n_check <= GX_GUARD_MAX_CHECK && (n_check == 0 || check) && (reinterpret_cast<uintptr_t>(check) & 3) == 0,
                 "gx_grad_guard: n_check = %d outside [0, %d], or a null / misaligned check pointer", n_check, GX_GUARD_MAX_CHECK);
    GX_CHECK_ARG(ws_bytes >= gx_grad_guard_ws_bytes(work), "gx_grad_guard: workspace of %zu bytes, %zu needed (gx_grad_guard_ws_bytes)",
                 ws_bytes, gx_grad_guard_ws_bytes(work));
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)(work < GX_GUARD_MAX_GRID ? work : GX_GUARD_MAX_GRID);      // sized to the chip, not to N
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, bytes);
        hipLaunchKernelGGL(guard_partial_kernel, dim3(grid), dim3(kGuardThreads), 0, s, table_dev, n_segments, work, (double*)ws);
    }
    GX_CHECK_LAUNCH("gx_grad_guard");
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 8.0 * grid);
        hipLaunchKernelGGL(guard_final_kernel, dim3(1), dim3(kGuardThreads), 0, s, (const double*)ws, (int)grid, check, n_check, gscale,
                           max_norm, force_ok, (GxGuardRecord*)record);
    }
    GX_CHECK_LAUNCH("gx_grad_guard");
    return GX_OK;
}

int gx_scale_multi_guarded(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                           const void* record, gx_stream_t stream) {
    long long work = 0;
    double bytes = 0.0;
    const int rc = guard_check_table("gx_scale_multi_guarded", table_host, table_dev, table_words, n_segments, &work, &bytes);
    if (rc != GX_OK) return rc;
    GX_CHECK_ARG(record && (reinterpret_cast<uintptr_t>(record) & 7) == 0, "gx_scale_multi_guarded: null or misaligned record");
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)(work < GX_GUARD_MAX_GRID ? work : GX_GUARD_MAX_GRID);
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 2.0 * bytes);
        hipLaunchKernelGGL(scale_multi_kernel, dim3(grid), dim3(kGuardThreads), 0, s, table_dev, n_segments, work,
                           (const GxGuardRecord*)record);
    }
    GX_CHECK_LAUNCH("gx_scale_multi_guarded");
    return GX_OK;
}

}  // extern "C"
