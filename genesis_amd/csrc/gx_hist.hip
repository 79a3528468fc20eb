// TensorBoard histograms on the device (train.py:313-325 log_distributions, :340-345 log_grads_and_weights; contract:
// include/genesis_hip.h, gx_hist_multi).  tensorboardX's add_histogram copies every tensor to the host, widens it to fp64 and runs
// numpy.histogram over a table of edges, plus min / max / sum / dot: per logging event several hundred copies and synchronisations.
// Here ONE call histograms every queued tensor against the shared edge table.  A workgroup owns one chunk of GX_HIST_CHUNK elements
// of one segment (found by bisecting the descriptors' work prefix, as gx_vis_compose finds its grid): the edge table and the bin
// counts live in LDS (sized by the table: 19 KB for the 1549 default edges, 48 KB for 4096), a value's bin is a bisection over the
// table's own doubles, the counts are LDS integer atomics flushed (the non-zero ones) with global integer atomics.  min / max /
// sum / sum of squares and the three tallies go per thread -> wave -> workgroup into one partial per chunk; a second small launch
// adds a segment's partials in chunk order.  No floating-point atomic anywhere and no hand-over between workgroups inside a
// launch: two calls on the same input give the same bits.
#include "gx_common.h"

namespace {

constexpr int kHistThreads = 256;
constexpr int kHistUnroll = 4;      // 16-byte loads in flight per thread

typedef double f64x2 __attribute__((ext_vector_type(2)));

struct HistPart {      // one chunk's share of a segment: 64 bytes
    double mn, mx, sum, sq;
    unsigned long long nan, below, above, pad;
};

struct HistAcc {      // a thread's share of a chunk (at most GX_HIST_CHUNK / 256 values: the tallies fit 32 bits)
    double mn, mx, sum, sq;
    unsigned nan, below, above;
};

__device__ __forceinline__ double hist_wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double hist_wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ unsigned hist_wave_sum_u(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// J values of one thread: first the bisections of all of them side by side (independent chains of LDS reads: one value after the
// other leaves the thread waiting on one read at a time), then per value its statistics and its count.
// Bin by numpy's rule for explicit edges -- bin i holds e[i] <= v < e[i + 1], the last bin also v == e[last]; NaN, v < e[0] and
// v > e[last] fall in no bin (-0.0 compares as 0.0).  top: the largest power of two <= n_edges - 1.  on[j]: value j exists.
// All lanes of the wave whose value j exists count together: when they agree on the bin (a zero-filled bias, a zero gradient),
// ONE lane adds their number instead of 64 lanes queueing on one LDS word.
template <int J>
__device__ __forceinline__ void hist_values(const double (&v)[J], const bool (&on)[J], const double* __restrict__ e, int n_edges,
                                            int top, unsigned* __restrict__ cnt, HistAcc& a) {
    int pos[J];      // the last edge <= v (0 for a NaN and for a value below the table, which the classification takes out)
#pragma unroll
    for (int j = 0; j < J; ++j) pos[j] = 0;
    for (int s = top; s > 0; s >>= 1) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            // (the read is unconditional and stays inside the table: a read under a branch would wait for its own answer)
            const int m = pos[j] + s;
            const double edge = e[m < n_edges ? m : n_edges - 1];
            pos[j] = (m < n_edges) & (edge <= v[j]) ? m : pos[j];
        }
    }
    const double e_first = e[0], e_last = e[n_edges - 1];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        if (!on[j]) continue;
        const double x = v[j];
        int bin = -1;
        if (x != x) {
            ++a.nan;
        } else {
            a.mn = fmin(a.mn, x); a.mx = fmax(a.mx, x);
            a.sum += x; a.sq += x * x;
            if (x < e_first) ++a.below;
            else if (x > e_last) ++a.above;
            else bin = pos[j] == n_edges - 1 ? pos[j] - 1 : pos[j];
        }
        const int first = __builtin_amdgcn_readfirstlane(bin);
        if (__all(bin == first)) {
            if (first >= 0) {
                const unsigned long long active = __ballot(1);
                if ((int)(threadIdx.x & 63) == __ffsll((long long)active) - 1) atomicAdd(&cnt[first], (unsigned)__popcll(active));
            }
        } else if (bin >= 0) {
            atomicAdd(&cnt[bin], 1u);
        }
    }
}

template <typename T> struct HistVec;
template <> struct HistVec<float> { typedef f32x4 type; };
template <> struct HistVec<double> { typedef f64x2 type; };

// n values at p (aligned to its element only: a slice of a flat buffer): scalar loads up to the first 16-byte boundary, 16-byte
// loads from there, scalar loads for what is left
template <typename T>
__device__ __forceinline__ void hist_scan(const T* __restrict__ p, int n, const double* __restrict__ e, int n_edges, int top,
                                          unsigned* __restrict__ cnt, HistAcc& a) {
    typedef typename HistVec<T>::type Vec;
    constexpr int V = 16 / (int)sizeof(T);
    const int t = threadIdx.x;
    const int to_boundary = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
    const int head = to_boundary < n ? to_boundary : n;
    const int nv = (n - head) / V, rest0 = head + nv * V;
    {      // the ragged ends: thread t takes element t of the head and element t of the rest
        const bool on[2] = {t < head, t < n - rest0};
        const double v[2] = {on[0] ? (double)p[t] : 0.0, on[1] ? (double)p[rest0 + t] : 0.0};
        if (on[0] || on[1]) hist_values<2>(v, on, e, n_edges, top, cnt, a);
    }
    const Vec* __restrict__ pv = reinterpret_cast<const Vec*>(p + head);
    for (int i0 = 0; i0 < nv; i0 += kHistThreads * kHistUnroll) {
        double v[kHistUnroll * V];
        bool on[kHistUnroll * V];
#pragma unroll
        for (int u = 0; u < kHistUnroll; ++u) {
            const int i = i0 + u * kHistThreads + t;
            Vec q = {};
            if (i < nv) q = pv[i];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                v[u * V + j] = (double)q[j];
                on[u * V + j] = i < nv;
            }
        }
        if (i0 + t < nv) hist_values<kHistUnroll * V>(v, on, e, n_edges, top, cnt, a);
    }
}

__host__ __device__ constexpr size_t hist_lds_bytes(int n_edges) {
    return (kHistThreads / 64) * sizeof(HistPart) + (size_t)n_edges * sizeof(double) + (size_t)n_edges * sizeof(unsigned);
}

__global__ void __launch_bounds__(kHistThreads)
hist_chunk_kernel(const long long* __restrict__ table, int S, const double* __restrict__ edges, int n_edges, int top,
                  unsigned* __restrict__ counts, HistPart* __restrict__ parts) {
    // all LDS in the dynamic region, sized by the table (hist_lds_bytes): the waves' partials, the edges, the counts
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    HistPart* s_w = reinterpret_cast<HistPart*>(s_dyn);
    double* s_e = reinterpret_cast<double*>(s_dyn + (kHistThreads / 64) * sizeof(HistPart));
    unsigned* s_c = reinterpret_cast<unsigned*>(s_e + n_edges);
    const int t = threadIdx.x, nb = n_edges - 1;
    const long long w = blockIdx.x;
    int lo = 0, hi = S - 1;      // the last segment whose first chunk is <= w
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * GX_HIST_DESC_WORDS + GX_HIST_D_WORK] <= w) lo = mid; else hi = mid - 1;
    }
    const long long* d = table + (size_t)lo * GX_HIST_DESC_WORDS;
    for (int i = t; i < n_edges; i += kHistThreads) s_e[i] = edges[i];
    for (int i = t; i < nb; i += kHistThreads) s_c[i] = 0u;
    __syncthreads();
    const long long N = d[GX_HIST_D_N], first = (w - d[GX_HIST_D_WORK]) * GX_HIST_CHUNK;
    const int n = (int)(N - first < GX_HIST_CHUNK ? N - first : GX_HIST_CHUNK);
    HistAcc a;
    a.mn = __longlong_as_double(0x7ff0000000000000LL); a.mx = -a.mn; a.sum = 0.0; a.sq = 0.0;
    a.nan = a.below = a.above = 0u;
    if (d[GX_HIST_D_DTYPE] == GX_HIST_FP32)
        hist_scan<float>(reinterpret_cast<const float*>(d[GX_HIST_D_SRC]) + first, n, s_e, n_edges, top, s_c, a);
    else
        hist_scan<double>(reinterpret_cast<const double*>(d[GX_HIST_D_SRC]) + first, n, s_e, n_edges, top, s_c, a);
    // thread -> wave (xor butterflies: every lane ends with the same bits) -> workgroup, waves in order
    a.mn = hist_wave_min(a.mn); a.mx = hist_wave_max(a.mx);
    a.sum = gx_wave_sum_d(a.sum); a.sq = gx_wave_sum_d(a.sq);
    a.nan = hist_wave_sum_u(a.nan); a.below = hist_wave_sum_u(a.below); a.above = hist_wave_sum_u(a.above);
    if ((t & 63) == 0) {
        HistPart& p = s_w[t >> 6];
        p.mn = a.mn; p.mx = a.mx; p.sum = a.sum; p.sq = a.sq;
        p.nan = a.nan; p.below = a.below; p.above = a.above; p.pad = 0;
    }
    __syncthreads();
    if (t == 0) {
        HistPart r = s_w[0];
#pragma unroll
        for (int k = 1; k < kHistThreads / 64; ++k) {
            r.mn = fmin(r.mn, s_w[k].mn); r.mx = fmax(r.mx, s_w[k].mx);
            r.sum += s_w[k].sum; r.sq += s_w[k].sq;
            r.nan += s_w[k].nan; r.below += s_w[k].below; r.above += s_w[k].above;
        }
        parts[w] = r;
    }
    unsigned* out = counts + (size_t)lo * nb;
    for (int i = t; i < nb; i += kHistThreads) {
        const unsigned c = s_c[i];
        if (c) atomicAdd(&out[i], c);
    }
}

// one wave per segment: lane l adds the partials l, l + 64, ... in that order, then the lanes are folded
__global__ void __launch_bounds__(64)
hist_combine_kernel(const long long* __restrict__ table, const HistPart* __restrict__ parts, double* __restrict__ stats,
                    unsigned long long* __restrict__ tally) {
    const int seg = blockIdx.x, lane = threadIdx.x;
    const long long* d = table + (size_t)seg * GX_HIST_DESC_WORDS;
    const long long chunks = (d[GX_HIST_D_N] + GX_HIST_CHUNK - 1) / GX_HIST_CHUNK;
    const HistPart* p = parts + d[GX_HIST_D_WORK];
    double mn = __longlong_as_double(0x7ff0000000000000LL), mx = -mn, sum = 0.0, sq = 0.0;
    unsigned long long nan = 0, below = 0, above = 0;
    for (long long i = lane; i < chunks; i += 64) {
        mn = fmin(mn, p[i].mn); mx = fmax(mx, p[i].mx);
        sum += p[i].sum; sq += p[i].sq;
        nan += p[i].nan; below += p[i].below; above += p[i].above;
    }
    mn = hist_wave_min(mn); mx = hist_wave_max(mx);
    sum = gx_wave_sum_d(sum); sq = gx_wave_sum_d(sq);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nan += __shfl_xor(nan, off, 64); below += __shfl_xor(below, off, 64); above += __shfl_xor(above, off, 64);
    }
    if (lane == 0) {
        double* s = stats + (size_t)seg * 4;
        s[0] = mn; s[1] = mx; s[2] = sum; s[3] = sq;
        unsigned long long* y = tally + (size_t)seg * 3;
        y[0] = nan; y[1] = below; y[2] = above;
    }
}

}  // namespace

extern "C" {

size_t gx_hist_multi_ws_bytes(long long total_chunks) {
    return total_chunks > 0 ? (size_t)total_chunks * sizeof(HistPart) : 0;
}

int gx_hist_multi(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                  const double* edges, int n_edges, unsigned int* counts, double* stats, unsigned long long* tally, void* ws,
                  size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(table_host && table_dev && edges && counts && stats && tally && ws, "gx_hist_multi: null pointer");
    GX_CHECK_ARG(n_segments >= 1, "gx_hist_multi: n_segments = %d below 1", n_segments);
    GX_CHECK_ARG(table_words >= (long long)n_segments * GX_HIST_DESC_WORDS, "gx_hist_multi: %d segments do not fit a table of %lld words",
                 n_segments, table_words);
    GX_CHECK_ARG(n_edges >= 2 && n_edges <= GX_HIST_MAX_EDGES, "gx_hist_multi: n_edges = %d outside [2, %d]", n_edges, GX_HIST_MAX_EDGES);
    GX_CHECK_ARG(((reinterpret_cast<uintptr_t>(edges) | reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(tally) |
                   reinterpret_cast<uintptr_t>(ws)) & 7) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0,
                 "gx_hist_multi: edges, stats, tally and ws must be 8-byte aligned, counts 4-byte aligned");
    long long work = 0;
    double bytes = 0.0;
    for (int si = 0; si < n_segments; ++si) {
        const long long* d = table_host + (size_t)si * GX_HIST_DESC_WORDS;
        const long long N = d[GX_HIST_D_N], dtype = d[GX_HIST_D_DTYPE];
        const uintptr_t src = (uintptr_t)d[GX_HIST_D_SRC];
        GX_CHECK_ARG(dtype == GX_HIST_FP32 || dtype == GX_HIST_FP64, "gx_hist_multi: segment %d: unknown dtype %lld", si, dtype);
        GX_CHECK_ARG(N >= 1 && N < (1LL << 31), "gx_hist_multi: segment %d: N = %lld outside [1, 2^31)", si, N);
        GX_CHECK_ARG(src, "gx_hist_multi: segment %d: null source", si);
        GX_CHECK_ARG((src & (dtype == GX_HIST_FP32 ? 3 : 7)) == 0, "gx_hist_multi: segment %d: source %#llx is not aligned to its %d-byte elements",
                     si, (unsigned long long)src, dtype == GX_HIST_FP32 ? 4 : 8);
        GX_CHECK_ARG(d[GX_HIST_D_WORK] == work, "gx_hist_multi: segment %d: WORK = %lld, the prefix is %lld", si, d[GX_HIST_D_WORK], work);
        work += (N + GX_HIST_CHUNK - 1) / GX_HIST_CHUNK;
        bytes += (double)N * (dtype == GX_HIST_FP32 ? 4 : 8);
    }
    GX_CHECK_ARG(work < (1LL << 31), "gx_hist_multi: %lld chunks are too many for one launch", work);
    GX_CHECK_ARG(ws_bytes >= gx_hist_multi_ws_bytes(work), "gx_hist_multi: workspace of %zu bytes, %zu needed (gx_hist_multi_ws_bytes)",
                 ws_bytes, gx_hist_multi_ws_bytes(work));
    hipStream_t s = (hipStream_t)stream;
    const int nb = n_edges - 1;
    int top = 1;
    while (top * 2 <= nb) top *= 2;
    if (hipMemsetAsync(counts, 0, (size_t)n_segments * nb * sizeof(unsigned), s) != hipSuccess) {
        gx_set_error("gx_hist_multi: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
        return GX_ELAUNCH;
    }
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, bytes);
        hipLaunchKernelGGL(hist_chunk_kernel, dim3((unsigned)work), dim3(kHistThreads), hist_lds_bytes(n_edges), s, table_dev, n_segments, edges, n_edges, top,
                           counts, reinterpret_cast<HistPart*>(ws));
    }
    GX_CHECK_LAUNCH("gx_hist_multi");
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)work * sizeof(HistPart));
        hipLaunchKernelGGL(hist_combine_kernel, dim3((unsigned)n_segments), dim3(64), 0, s, table_dev, reinterpret_cast<const HistPart*>(ws),
                           stats, tally);
    }
    GX_CHECK_LAUNCH("gx_hist_multi");
    return GX_OK;
}

}  // extern "C"
