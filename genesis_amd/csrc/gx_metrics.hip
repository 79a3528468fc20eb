// Segmentation metrics (validation / scripts/compute_seg_metrics.py): the contingency table of two integer label
// maps per image.  Both reference metrics are functions of it alone:
//   utils/misc.py:101-114  average_ari       -> sklearn.metrics.adjusted_rand_score(pred, gt) per image, whose
//                                               published algorithm works on the contingency matrix
//   utils/misc.py:173-235  average_segcover  -> iou(A == i, (B == j) & (A >= 0)) = n_ij / (a_i + b_j - n_ij)
// The reference does this on the host with per-image Python loops over numpy / boolean-mask passes (it dominates
// validation once the forward pass is fast); here one workgroup per image histograms its pixels into LDS with
// integer atomics (exact and order-independent) and the tiny [B, KA, KB+1] tables stay on the device.
#include "gx_common.h"

namespace {

// counts[b][i][j], i in [0,KA), j in [0,KB] -- column KB collects segB labels outside [0,KB); pixels whose segA label
// is outside [0,KA) (the reference's "ignore" regions, label < 0) are not counted at all.
__global__ void __launch_bounds__(256)
label_contingency_kernel(const long long* __restrict__ segA, const long long* __restrict__ segB, int HW, int KA,
                         int KB, int* __restrict__ counts) {
    extern __shared__ int hist[];
    const int cells = KA * (KB + 1);
    for (int i = threadIdx.x; i < cells; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const long long* a = segA + (size_t)blockIdx.x * HW;
    const long long* b = segB + (size_t)blockIdx.x * HW;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
        const long long la = a[p], lb = b[p];
        if (la >= 0 && la < KA) {
            const int j = (lb >= 0 && lb < KB) ? (int)lb : KB;
            atomicAdd(&hist[(int)la * (KB + 1) + j], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += blockDim.x) counts[(size_t)blockIdx.x * cells + i] = hist[i];
}

// ---- gx_seg_metrics: log-mask planes + instance map -> every score of the validation loop, one launch per batch -------------
// (contract: include/genesis_hip.h).  One workgroup per image: argmax over the K planes read in place, the [G, K] table in LDS,
// then wave 0 turns the table into the image's eight values, and the last workgroup to finish folds the batch into the running
// accumulators (the counter pattern of mse_rmse_kernel: fixed order, no float atomics).
struct SegPlanes { const float* p[32]; };      // plane k of image 0; image b lies image_stride floats further
enum { SEG_COUNTER = 0, SEG_BATCHES = 1, SEG_OVERFLOW = 2, SEG_CURSOR = 3 };      // words of `state`

// torch.argmax's order: a NaN ranks above every number and the first one wins; among equal numbers the lowest k wins
__device__ __forceinline__ void seg_take(float v, int k, float& best, int& bi) {
    if (best == best && (v > best || v != v)) { best = v; bi = k; }
}

__device__ __forceinline__ long long seg_wave_sum_ll(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// adjusted_rand_from_contingency (genesis_amd/metrics.py) on the integer sums of one table: n pixels, sum of squared cells,
// squared ground-truth marginals (sa2) and squared prediction marginals (sb2); every fp64 operation rounds on its own
__device__ __forceinline__ double seg_ari(long long n, long long ssq, long long sa2, long long sb2) {
#pragma clang fp contract(off)
    const long long tpi = ssq - n, fpi = sa2 - ssq, fni = sb2 - ssq, tni = n * n - fpi - fni - ssq;
    if (fni == 0 && fpi == 0) return 1.0;
    const double tp = (double)tpi, fp = (double)fpi, fn = (double)fni, tn = (double)tni;
    const double den = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn);
    return 2.0 * (tp * tn - fn * fp) / den;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
seg_metrics_kernel(SegPlanes planes, long long image_stride, const long long* __restrict__ inst, int B, int HW, int K, int G,
                   double* __restrict__ rows, double* __restrict__ acc, unsigned long long* __restrict__ state,
                   double* __restrict__ log, long long log_capacity) {
#pragma clang fp contract(off)
    extern __shared__ int hist[];      // [G][K]; the kernel's only LDS
    const int cells = G * K, b = blockIdx.x;
    for (int i = threadIdx.x; i < cells; i += 256) hist[i] = 0;
    __syncthreads();
    const long long* gt = inst + (size_t)b * HW;
    const size_t img = (size_t)b * (size_t)image_stride;
    unsigned over = 0;
    if (VEC) {
        for (int i = threadIdx.x; i < (HW >> 2); i += 256) {
            const f32x4 v0 = reinterpret_cast<const f32x4*>(planes.p[0] + img)[i];
            float best[4] = {v0[0], v0[1], v0[2], v0[3]};
            int bi[4] = {0, 0, 0, 0};
#pragma unroll 4
            for (int k = 1; k < K; ++k) {
                const f32x4 v = reinterpret_cast<const f32x4*>(planes.p[k] + img)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) seg_take(v[j], k, best[j], bi[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long g = gt[4 * i + j];
                if (g >= G) ++over;
                else if (g >= 0) atomicAdd(&hist[(int)g * K + bi[j]], 1);
            }
        }
    } else {
        for (int p = threadIdx.x; p < HW; p += 256) {
            float best = planes.p[0][img + p];
            int bi = 0;
#pragma unroll 4
            for (int k = 1; k < K; ++k) seg_take(planes.p[k][img + p], k, best, bi);
            const long long g = gt[p];
            if (g >= G) ++over;
            else if (g >= 0) atomicAdd(&hist[(int)g * K + bi], 1);
        }
    }
    if (over) atomicAdd(state + SEG_OVERFLOW, (unsigned long long)over);      // integer: exact in any order
    __syncthreads();
    if (threadIdx.x >= 64) return;      // (no barrier below)

    // ---- wave 0: marginals and scores.  Lane k holds the prediction marginal b_k, lane g - g0 the ground-truth row g.
    const int lane = threadIdx.x;
    int bk = 0, c0k = 0;
    if (lane < K) {
        for (int g = 0; g < G; ++g) bk += hist[g * K + lane];
        c0k = hist[lane];
    }
    long long n = 0, ssq = 0, sa2 = 0;      // this lane's rows; summed over the wave below
    long long a0 = 0, ssq0 = 0;             // row 0 (background) alone
    int present = 0;                        // rows with pixels
    // covering: the reference adds label after label, float32 -- kept in ascending order (every lane carries the same sums)
    float ms = 0.f, ss = 0.f, ms_fg = 0.f, ss_fg = 0.f;
    for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + lane;
        const bool valid = g < G;
        int a = 0;
        long long sq = 0;
        if (valid)
            for (int k = 0; k < K; ++k) { const int c = hist[g * K + k]; a += c; sq += (long long)c * c; }
        float best = 0.f;      // the reference's running maximum starts at 0; an empty union never wins it
        for (int k = 0; k < K; ++k) {
            const int bb = __shfl(bk, k, 64);
            if (valid) {
                const int c = hist[g * K + k], u = a + bb - c;
                const float iou = u == 0 ? 0.f : (float)c / (float)u;
                best = fmaxf(best, iou);
            }
        }
        n += a; ssq += sq; sa2 += (long long)a * a; present += a > 0;
        if (g0 == 0) { a0 = __shfl(a, 0, 64); ssq0 = __shfl(sq, 0, 64); }
        const int cnt = G - g0 < 64 ? G - g0 : 64;
        for (int l = 0; l < cnt; ++l) {
            const float bl = __shfl(best, l, 64), wl = (float)__shfl(a, l, 64) * bl;
            ms += bl; ss += wl;
            if (g0 + l > 0) { ms_fg += bl; ss_fg += wl; }
        }
    }
    n = seg_wave_sum_ll(n); ssq = seg_wave_sum_ll(ssq); sa2 = seg_wave_sum_ll(sa2);
    present = (int)seg_wave_sum_ll(present);
    const long long sb2 = seg_wave_sum_ll((long long)bk * bk);
    const long long sb2_fg = seg_wave_sum_ll((long long)(bk - c0k) * (bk - c0k));
    bool last = false;
    if (lane == 0) {
        const int present_fg = present - (a0 > 0);
        double* r = rows + (size_t)b * 8;
        r[0] = seg_ari(n, ssq, sa2, sb2);
        r[1] = seg_ari(n - a0, ssq - ssq0, sa2 - a0 * a0, sb2_fg);
        const long long n_fg = n - a0;
        r[2] = (double)(ms / (float)(present > 0 ? present : 1));
        r[3] = (double)(ms_fg / (float)(present_fg > 0 ? present_fg : 1));
        r[4] = (double)(ss / (float)(n > 0 ? n : 1));
        r[5] = (double)(ss_fg / (float)(n_fg > 0 ? n_fg : 1));
        r[6] = (double)n;
        r[7] = (double)present;
        __threadfence();
        last = atomicAdd(state + SEG_COUNTER, 1ull) == (unsigned long long)(B - 1);
    }
    if (!last) return;
    // ---- the batch step, by one thread in image order.  ARI: the fp64 sum over the images divided by B, the operations of the
    // reference's sum(list) / len(list) on Python floats.  Covering: a float32 mean where the reference has mean_sc.mean(0), but
    // NOT its operation order -- the per-image float32 values are summed in fp64 (exactly, for any B that fits a launch) and the
    // sum is rounded once to float32 before the float32 division, whereas torch adds in float32 in an order of its own.  The two
    // agree within float32 rounding of the sum (the tests' 2e-7 bar), not bit for bit.
    __threadfence();
    double m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < B; ++i)
        for (int c = 0; c < 8; ++c) m[c] += __builtin_nontemporal_load(rows + (size_t)i * 8 + c);
    for (int c = 0; c < 8; ++c) {
        const bool cover = c >= 2 && c < 6;
        const double mean = cover ? (double)((float)m[c] / (float)B) : m[c] / (double)B;
        // over batches the reference adds 0-dim float32 tensors for covering (sum(val) in train.py:567) and Python floats for ARI
        acc[c] = cover ? (double)((float)acc[c] + (float)mean) : acc[c] + mean;
    }
    state[SEG_BATCHES] += 1ull;
    if (log) {
        const long long cur = (long long)state[SEG_CURSOR];
        const long long room = log_capacity - cur, take = room < B ? room : (long long)B;
        for (long long i = 0; i < take; ++i)
            for (int c = 0; c < 8; ++c) log[(cur + i) * 8 + c] = __builtin_nontemporal_load(rows + (size_t)i * 8 + c);
        if (take > 0) state[SEG_CURSOR] = (unsigned long long)(cur + take);
    }
    state[SEG_COUNTER] = 0ull;      // ready for the next launch (graph replay)
}

}  // namespace

extern "C" {

int gx_label_contingency(const long long* segA, const long long* segB, int B, int HW, int KA, int KB, int* counts,
                         gx_stream_t stream) {
    GX_CHECK_ARG(segA && segB && counts, "gx_label_contingency: null pointer");
    GX_CHECK_ARG(B > 0 && HW > 0 && KA > 0 && KB > 0, "gx_label_contingency: bad dims");
    GX_CHECK_ARG((size_t)KA * (KB + 1) * sizeof(int) <= 64 * 1024, "gx_label_contingency: table exceeds 64 KiB of LDS");
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 16.0 * B * HW);
        hipLaunchKernelGGL(label_contingency_kernel, dim3(B), dim3(256), (size_t)KA * (KB + 1) * sizeof(int), s, segA,
                           segB, HW, KA, KB, counts);
    }
    GX_CHECK_LAUNCH("gx_label_contingency");
    return GX_OK;
}

int gx_seg_metrics(const float* base, long long plane_stride, long long image_stride, const float* const* planes,
                   const long long* instances, int B, int HW, int K, int max_labels, double* rows, double* acc,
                   unsigned long long* state, double* log, long long log_capacity, gx_stream_t stream) {
    GX_CHECK_ARG(K >= 1 && K <= 32, "gx_seg_metrics: K = %d outside [1, 32]", K);
    GX_CHECK_ARG((base != nullptr) != (planes != nullptr), "gx_seg_metrics: give either base (packed planes) or planes (a table)");
    GX_CHECK_ARG(instances && rows && acc && state, "gx_seg_metrics: null pointer");
    GX_CHECK_ARG(B > 0 && HW > 0 && HW < (1 << 30) && max_labels > 0, "gx_seg_metrics: bad dims");
    GX_CHECK_ARG(image_stride >= HW || B == 1, "gx_seg_metrics: image_stride %lld below HW %d", image_stride, HW);
    GX_CHECK_ARG(!base || plane_stride >= 0, "gx_seg_metrics: negative plane_stride");
    GX_CHECK_ARG(!log || log_capacity >= 0, "gx_seg_metrics: negative log_capacity");
    GX_CHECK_ARG((size_t)max_labels * K * sizeof(int) <= 64 * 1024, "gx_seg_metrics: table max_labels x K exceeds 64 KiB of LDS");
    SegPlanes T;
    uintptr_t bits = (uintptr_t)((unsigned long long)image_stride * sizeof(float));
    for (int k = 0; k < 32; ++k) {
        T.p[k] = k >= K ? nullptr : (base ? base + (size_t)k * (size_t)plane_stride : planes[k]);
        GX_CHECK_ARG(k >= K || T.p[k], "gx_seg_metrics: plane %d is null", k);
        bits |= reinterpret_cast<uintptr_t>(T.p[k]);
    }
    const bool vec = (HW & 3) == 0 && (bits & 15) == 0;      // every plane of every image on a 16-byte boundary
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)max_labels * K * sizeof(int);
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (4.0 * K + 8.0) * B * HW);
        if (vec)
            hipLaunchKernelGGL(seg_metrics_kernel<true>, dim3(B), dim3(256), lds, s, T, image_stride, instances, B, HW, K,
                               max_labels, rows, acc, state, log, log_capacity);
        else
            hipLaunchKernelGGL(seg_metrics_kernel<false>, dim3(B), dim3(256), lds, s, T, image_stride, instances, B, HW, K,
                               max_labels, rows, acc, state, log, log_capacity);
    }
    GX_CHECK_LAUNCH("gx_seg_metrics");
    return GX_OK;
}

}  // extern "C"
