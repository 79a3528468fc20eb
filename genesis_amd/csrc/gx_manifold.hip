// Sample-quality metrics beside FID (genesis_amd/sample_quality.py): the all-pairs work of improved precision / recall
// (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and KID (Binkowski et al. 2018) over fp32 feature rows, in
// fp64, without an N x M matrix in memory.
//   gx_knn_radii        squared distance of every row to its k-th nearest other row
//   gx_manifold_counts  per query row: how many reference balls hold it; per reference row: does its ball hold any query
//   gx_kid_sums         per subset: the three kernel sums of the MMD^2 estimate with the cubic polynomial kernel
//
// One workgroup of 256 threads owns a 64 x 64 tile of (row of A) x (row of B) pairs; each thread a 4 x 4 micro-tile of fp64
// accumulators.  D is streamed through LDS as fp32 in chunks of 32, stored transposed ([d][row]) so that a thread reads the four
// rows of its micro-tile in one 16-byte LDS read, and converted to fp64 at use.  Per pair the D-sum is ONE sequential fma chain over
// d = 0 .. D-1 from 0 (a chunk's tail past D holds zeros in both operands, which leave the accumulator as it is), so d^2(a, b) has
// the same bits in every launch, at every tile position and in either argument order ((a - b)^2 == (b - a)^2 exactly), and identical
// rows give exactly 0.  No floating-point atomics anywhere: the integer counts use integer atomics, the KID sums a fixed tree.
#include "gx_common.h"

#include <limits.h>

namespace {

constexpr int kT = 64;          // tile side (rows of A, rows of B)
constexpr int kDK = 32;         // features per LDS chunk
constexpr int kMaxK = 8;        // neighbours kept per row
constexpr int kMaxD = 8192;
constexpr int kMaxRows = 1 << 21;      // rows per operand (the tile grid's y extent stays below 65536)

struct Stage { f32x4 a[kDK][kT / 4], b[kDK][kT / 4]; };       // [d][row]: 2 x 8 KB

// acc[i][j] (+)= sum_d f(A[ty*4 + i][d], B[tx*4 + j][d]); f = (a - b)^2 (DIFF) or a * b.  pa / pb: the row of A / B THIS thread
// stages (row t & 63 of the tile; null: a row past the end, staged as zeros).
template <bool DIFF>
__device__ __forceinline__ void tile_accumulate(const float* __restrict__ pa, const float* __restrict__ pb, int D, Stage& st,
                                                double (&acc)[4][4]) {
    const int t = threadIdx.x, lr = t & 63, lq = t >> 6, ty = t >> 4, tx = t & 15;
    float* sa = reinterpret_cast<float*>(st.a);
    float* sb = reinterpret_cast<float*>(st.b);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 ga[2], gb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int d = (lq + 4 * i) * 4;                      // D % 4 == 0: d < D covers d .. d + 3
        ga[i] = (pa && d < D) ? *reinterpret_cast<const f32x4*>(pa + d) : zero;
        gb[i] = (pb && d < D) ? *reinterpret_cast<const f32x4*>(pb + d) : zero;
    }
    for (int d0 = 0; d0 < D; d0 += kDK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sa[((lq + 4 * i) * 4 + j) * kT + lr] = ga[i][j];
                sb[((lq + 4 * i) * 4 + j) * kT + lr] = gb[i][j];
            }
        __syncthreads();
        if (d0 + kDK < D) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int d = d0 + kDK + (lq + 4 * i) * 4;
                ga[i] = (pa && d < D) ? *reinterpret_cast<const f32x4*>(pa + d) : zero;
                gb[i] = (pb && d < D) ? *reinterpret_cast<const f32x4*>(pb + d) : zero;
            }
        }
#pragma unroll 8
        for (int d = 0; d < kDK; ++d) {
            const f32x4 qa = st.a[d][ty], qb = st.b[d][tx];
            double va[4], vb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { va[i] = (double)qa[i]; vb[i] = (double)qb[i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (DIFF) {
                        const double df = va[i] - vb[j];
                        acc[i][j] = fma(df, df, acc[i][j]);
                    } else {
                        acc[i][j] = fma(va[i], vb[j], acc[i][j]);
                    }
                }
        }
    }
}

// keeps the kMaxK smallest values seen, ascending, with multiplicity (registers only: every index is a compile-time constant)
__device__ __forceinline__ void keep_smallest(double (&best)[kMaxK], double v) {
#pragma unroll
    for (int s = 0; s < kMaxK; ++s)
        if (v < best[s]) { const double o = best[s]; best[s] = v; v = o; }
}

// cand [tiles][k][N]: the k smallest d^2(x_i, x_j), j != i, of row i among the columns of each column tile
__global__ void __launch_bounds__(256)
knn_tile_kernel(const float* __restrict__ X, int N, int D, int k, double* __restrict__ cand) {
    __shared__ Stage st;
    __shared__ double tile[kT][kT];
    const int t = threadIdx.x, lr = t & 63, ty = t >> 4, tx = t & 15;
    const int i0 = blockIdx.y * kT, j0 = blockIdx.x * kT;
    const float* pa = i0 + lr < N ? X + (size_t)(i0 + lr) * D : nullptr;
    const float* pb = j0 + lr < N ? X + (size_t)(j0 + lr) * D : nullptr;
    double acc[4][4] = {};
    tile_accumulate<true>(pa, pb, D, st, acc);
    const double inf = __builtin_huge_val();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty * 4 + a, j = j0 + tx * 4 + c;
            tile[ty * 4 + a][tx * 4 + c] = (j < N && j != i) ? acc[a][c] : inf;      // self is excluded by index
        }
    __syncthreads();
    if (t < kT && i0 + t < N) {
        double best[kMaxK];
#pragma unroll
        for (int s = 0; s < kMaxK; ++s) best[s] = inf;
        for (int jj = 0; jj < kT; ++jj) keep_smallest(best, tile[t][(jj + t) & (kT - 1)]);     // (rotated: no bank conflict)
#pragma unroll
        for (int s = 0; s < kMaxK; ++s)
            if (s < k) cand[((size_t)blockIdx.x * k + s) * N + i0 + t] = best[s];
    }
}

__global__ void __launch_bounds__(256)
knn_merge_kernel(const double* __restrict__ cand, int N, int k, int tiles, double* __restrict__ radii2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double best[kMaxK];
#pragma unroll
    for (int s = 0; s < kMaxK; ++s) best[s] = __builtin_huge_val();
    const int n = tiles * k;
    for (int e = 0; e < n; ++e) keep_smallest(best, cand[(size_t)e * N + i]);
    double r = best[0];
#pragma unroll
    for (int s = 1; s < kMaxK; ++s)
        if (s == k - 1) r = best[s];
    radii2[i] = r;
}

// hits / covered are zero on entry (the host call clears them in front of this launch)
__global__ void __launch_bounds__(256)
manifold_counts_kernel(const float* __restrict__ Q, int M, const float* __restrict__ R, int N, int D,
                       const double* __restrict__ radii2, int* __restrict__ hits, int* __restrict__ covered) {
    __shared__ Stage st;
    const int t = threadIdx.x, lr = t & 63, ty = t >> 4, tx = t & 15;
    const int q0 = blockIdx.y * kT, r0 = blockIdx.x * kT;
    const float* pa = q0 + lr < M ? Q + (size_t)(q0 + lr) * D : nullptr;
    const float* pb = r0 + lr < N ? R + (size_t)(r0 + lr) * D : nullptr;
    double acc[4][4] = {};
    tile_accumulate<true>(pa, pb, D, st, acc);
    double rad[4];
    int any[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int i = r0 + tx * 4 + c;
        rad[c] = i < N ? radii2[i] : 0.0;
        any[c] = 0;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int j = q0 + ty * 4 + a;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int in = (j < M && r0 + tx * 4 + c < N && acc[a][c] <= rad[c]) ? 1 : 0;
            cnt += in;
            any[c] |= in;
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) cnt += __shfl_xor(cnt, off, 64);       // over the 16 column threads of the row
        if (tx == 0 && cnt > 0) atomicAdd(&hits[j], cnt);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int f = any[c];
        f |= __shfl_xor(f, 16, 64);                                                  // over the wave's 4 row threads
        f |= __shfl_xor(f, 32, 64);
        if ((ty & 3) == 0 && f) covered[r0 + tx * 4 + c] = 1;                         // (every writer stores the same 1)
    }
}

__device__ __forceinline__ int clamp_row(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// part [S][3][T * T]: tile (ta, tb) of sum kappa(a, b), kappa = (a . b / D + 1)^3, over the m x m pairs of subset s; 0: x with x,
// 1: y with y (both without the diagonal; kappa is symmetric bit for bit, so a tile below the diagonal is left to its mirror image,
// which counts twice), 2: x with y
__global__ void __launch_bounds__(256)
kid_tile_kernel(const float* __restrict__ X, int NX, const int* __restrict__ ix, const float* __restrict__ Y, int NY,
                const int* __restrict__ iy, int m, int D, int T, double* __restrict__ part) {
    __shared__ Stage st;
    __shared__ double red[4];
    const int t = threadIdx.x, lr = t & 63, ty = t >> 4, tx = t & 15;
    const int s = blockIdx.z / 3, which = blockIdx.z % 3;
    double* out = part + ((size_t)blockIdx.z * T + blockIdx.y) * T + blockIdx.x;
    if (which < 2 && blockIdx.x < blockIdx.y) {
        if (t == 0) *out = 0.0;
        return;
    }
    const float* A = which == 1 ? Y : X;
    const float* B = which == 0 ? X : Y;
    const int* ia = (which == 1 ? iy : ix) + (size_t)s * m;
    const int* ib = (which == 0 ? ix : iy) + (size_t)s * m;
    const int na = which == 1 ? NY : NX, nb = which == 0 ? NX : NY;
    const int a0 = blockIdx.y * kT, b0 = blockIdx.x * kT;
    const float* pa = a0 + lr < m ? A + (size_t)clamp_row(ia[a0 + lr], na) * D : nullptr;
    const float* pb = b0 + lr < m ? B + (size_t)clamp_row(ib[b0 + lr], nb) * D : nullptr;
    double acc[4][4] = {};
    tile_accumulate<false>(pa, pb, D, st, acc);
    const double dd = (double)D;
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = a0 + ty * 4 + a, q = b0 + tx * 4 + c;
            if (p < m && q < m && (which == 2 || p != q)) {
                const double v = acc[a][c] / dd + 1.0;
                sum += v * v * v;
            }
        }
    sum = gx_wave_sum_d(sum);                   // a fixed butterfly, then the four waves in order
    if ((t & 63) == 0) red[t >> 6] = sum;
    __syncthreads();
    if (t == 0) {
        const double r = ((red[0] + red[1]) + red[2]) + red[3];
        *out = (which < 2 && blockIdx.x > blockIdx.y) ? 2.0 * r : r;
    }
}

__global__ void __launch_bounds__(64)
kid_reduce_kernel(const double* __restrict__ part, int n, int per, double* __restrict__ sums) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double v = 0.0;
    for (int e = 0; e < per; ++e) v += part[(size_t)i * per + e];
    sums[i] = v;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

size_t gx_knn_radii_ws_bytes(int N, int k) {
    if (N < 1 || N > kMaxRows || k < 1 || k > kMaxK) return 0;
    return (size_t)gx_ceil_div(N, kT) * k * N * sizeof(double);
}

int gx_knn_radii(const float* X, int N, int D, int k, double* radii2, void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(X && radii2 && ws, "gx_knn_radii: null pointer");
    GX_CHECK_ARG(D >= 4 && D <= kMaxD && D % 4 == 0, "gx_knn_radii: D must be a multiple of 4 in [4, %d], not %d", kMaxD, D);
    GX_CHECK_ARG(N >= 1 && N <= kMaxRows, "gx_knn_radii: N must be in [1, %d], not %d", kMaxRows, N);
    GX_CHECK_ARG(k >= 1 && k <= kMaxK, "gx_knn_radii: k must be in [1, %d], not %d", kMaxK, k);
    GX_CHECK_ARG(k <= N - 1, "gx_knn_radii: k = %d needs at least k + 1 rows, have N = %d", k, N);
    GX_CHECK_ARG(aligned16(X) && aligned16(ws), "gx_knn_radii: X and ws must be 16-byte aligned");
    const size_t need = gx_knn_radii_ws_bytes(N, k);
    GX_CHECK_ARG(ws_bytes >= need, "gx_knn_radii: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int tiles = gx_ceil_div(N, kT);
    hipLaunchKernelGGL(knn_tile_kernel, dim3(tiles, tiles), dim3(256), 0, s, X, N, D, k, (double*)ws);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(gx_ceil_div(N, 256)), dim3(256), 0, s, (const double*)ws, N, k, tiles, radii2);
    GX_CHECK_LAUNCH("gx_knn_radii");
    return GX_OK;
}

int gx_manifold_counts(const float* Q, int M, const float* R, int N, int D, const double* radii2, int* hits, int* covered,
                       gx_stream_t stream) {
    GX_CHECK_ARG(Q && R && radii2 && hits && covered, "gx_manifold_counts: null pointer");
    GX_CHECK_ARG(D >= 4 && D <= kMaxD && D % 4 == 0, "gx_manifold_counts: D must be a multiple of 4 in [4, %d], not %d", kMaxD,
                 D);
    GX_CHECK_ARG(M >= 1 && M <= kMaxRows && N >= 1 && N <= kMaxRows, "gx_manifold_counts: M and N must be in [1, %d], not %d, %d",
                 kMaxRows, M, N);
    GX_CHECK_ARG(aligned16(Q) && aligned16(R), "gx_manifold_counts: Q and R must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(hits, 0, (size_t)M * sizeof(int), s) != hipSuccess ||
        hipMemsetAsync(covered, 0, (size_t)N * sizeof(int), s) != hipSuccess) {
        (void)hipGetLastError();
        gx_set_error("gx_manifold_counts: clearing the outputs failed");
        return GX_ELAUNCH;
    }
    hipLaunchKernelGGL(manifold_counts_kernel, dim3(gx_ceil_div(N, kT), gx_ceil_div(M, kT)), dim3(256), 0, s, Q, M, R, N, D,
                       radii2, hits, covered);
    GX_CHECK_LAUNCH("gx_manifold_counts");
    return GX_OK;
}

size_t gx_kid_sums_ws_bytes(int m, int S) {
    if (m < 2 || m > 64 * 1024 || S < 1 || S > 65535 / 3) return 0;
    const size_t T = (size_t)gx_ceil_div(m, kT);
    return (size_t)S * 3 * T * T * sizeof(double);
}

int gx_kid_sums(const float* X, int NX, const int* ix, const float* Y, int NY, const int* iy, int m, int D, int S, double* sums,
                void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(X && ix && Y && iy && sums && ws, "gx_kid_sums: null pointer");
    GX_CHECK_ARG(D >= 4 && D <= kMaxD && D % 4 == 0, "gx_kid_sums: D must be a multiple of 4 in [4, %d], not %d", kMaxD, D);
    GX_CHECK_ARG(NX >= 1 && NY >= 1, "gx_kid_sums: NX and NY must be at least 1, not %d, %d", NX, NY);
    GX_CHECK_ARG(m >= 2 && m <= 64 * 1024, "gx_kid_sums: m must be in [2, 65536], not %d", m);
    GX_CHECK_ARG(S >= 1 && S <= 65535 / 3, "gx_kid_sums: S must be in [1, %d], not %d", 65535 / 3, S);
    GX_CHECK_ARG(aligned16(X) && aligned16(Y) && aligned16(ws), "gx_kid_sums: X, Y and ws must be 16-byte aligned");
    const size_t need = gx_kid_sums_ws_bytes(m, S);
    GX_CHECK_ARG(ws_bytes >= need, "gx_kid_sums: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int T = gx_ceil_div(m, kT);
    hipLaunchKernelGGL(kid_tile_kernel, dim3(T, T, S * 3), dim3(256), 0, s, X, NX, ix, Y, NY, iy, m, D, T, (double*)ws);
    hipLaunchKernelGGL(kid_reduce_kernel, dim3(gx_ceil_div(S * 3, 64)), dim3(64), 0, s, (const double*)ws, S * 3, T * T, sums);
    GX_CHECK_LAUNCH("gx_kid_sums");
    return GX_OK;
}

}  // extern "C"
