// Per-slot feature pooling, the K-slot mixture likelihood, and the small 1x1 convolutions of the
// GENESIS-V2 path.  All HBM-bound streaming kernels: coalesced NCHW reads (consecutive lanes =
// consecutive pixels), wavefront shuffles + one LDS hop for the reductions, fixed reduction trees.
//
// Reference:
//   masked pooling   models/genesisv2_config.py:146-152   sum_hw(m_k * f) and sum_hw(m_k)
//   mixture / recon  models/genesisv2_config.py:212-223, models/monet_config.py:137-139 (log_softmax over K),
//                    models/genesis_config.py:273-286 (x_loss, no log-sum-exp trick)
//   1x1 convs        modules/blocks.py:175-178 (SemiConv: gate * conv1x1 + uv),
//                    models/genesisv2_config.py:99 (decoder_module.13: Conv2d(64, 4, 1))
#include "gx_common.h"

#include <cstdlib>

namespace {

constexpr int KMAX = 16;

__device__ __forceinline__ float block_sum_f(float v, float* red) {
    v = gx_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ double block_sum_dd(double v, double* red) {
    v = gx_wave_sum_d(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// ------------------------------------------------------------------ masked pooling
// S[b][k][c] = sum_p exp(log_m[k][b][p]) * f[b][c][p];   msum[b][k] = sum_p exp(log_m[k][b][p])
// grid (B, C/4): each block reduces 4 channels x K slots over the image.
constexpr int PCH = 4;
// KT: the slot count at compile time (0: run time): K x 5 double accumulators instead of 16 x 5, unguarded slot loops
template <int KT>
__global__ void __launch_bounds__(256)
maskpool_fwd_kernel(const float* __restrict__ f, const float* __restrict__ log_m, int B, int C, int HW, int Krt,
                    float* __restrict__ S, float* __restrict__ msum) {
    const int K = KT ? KT : Krt;
    constexpr int KMAX = KT ? KT : ::KMAX;
    __shared__ double wred[4][KMAX * (PCH + 1)];
    const int b = blockIdx.x, c0 = blockIdx.y * PCH;
    const size_t kstride = (size_t)B * HW;
    double acc[KMAX][PCH];
    double ms[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        ms[k] = 0.0;
#pragma unroll
        for (int c = 0; c < PCH; ++c) acc[k][c] = 0.0;
    }
    const float* fb = f + ((size_t)b * C + c0) * HW;
    if (gx_vec4_ok(HW, f, log_m)) {
        // 16-byte loads, 4 pixels per thread and iteration: 4x fewer serial load -> use steps (the loop is latency-bound);
        // the loads of iteration i + 1 are issued ahead of iteration i's sums (two register sets): at 64 x 64 a thread has four
        // iterations, each of which used to start with its 4 + K loads' full latency
        const int n4 = HW >> 2;
        f32x4 fv[2][PCH], lmv[2][KMAX];
#define GX_MP_LOAD(set_, p4_)                                                                                   \
        {                                                                                                       \
            _Pragma("unroll") for (int c = 0; c < PCH; ++c) {                                                   \
                if (c0 + c < C) fv[set_][c] = *reinterpret_cast<const f32x4*>(fb + (size_t)c * HW + 4 * (p4_)); \
                else { fv[set_][c][0] = 0.f; fv[set_][c][1] = 0.f; fv[set_][c][2] = 0.f; fv[set_][c][3] = 0.f; } \
            }                                                                                                   \
            _Pragma("unroll") for (int k = 0; k < KMAX; ++k)                                                    \
                if (k < K) lmv[set_][k] = *reinterpret_cast<const f32x4*>(log_m + k * kstride + (size_t)b * HW + 4 * (p4_)); \
        }
#define GX_MP_SUM(set_)                                                                                         \
        {                                                                                                       \
            /* (the products are rounded to fp32 BEFORE they are widened, like the reference's fp32 multiply: widening the  \
               operands once and using exact fp64 products is 5 us faster -- v_cvt_f64_f32 runs at a quarter of the fp64 \
               FMA rate -- but moves the pooled features' last bits, and with them a ReLU decision of the small golden   \
               case: z_head.3.weight 8e-4 from the fixture against its 5e-4 bar; measured and not kept) */            \
            _Pragma("unroll") for (int k = 0; k < KMAX; ++k) {                                                  \
                if (k < K) {                                                                                    \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                             \
                        const float m = expf(lmv[set_][k][e]);                                                  \
                        ms[k] += (double)m;                                                                     \
                        _Pragma("unroll") for (int c = 0; c < PCH; ++c) acc[k][c] += (double)(m * fv[set_][c][e]); \
                    }                                                                                           \
                }                                                                                               \
            }                                                                                                   \
        }
        int p4 = threadIdx.x;
        if (p4 < n4) GX_MP_LOAD(0, p4)
        while (p4 < n4) {
            const int q4 = p4 + (int)blockDim.x;
            if (q4 < n4) GX_MP_LOAD(1, q4)
            GX_MP_SUM(0)
            if (q4 >= n4) break;
            const int r4 = q4 + (int)blockDim.x;
            if (r4 < n4) GX_MP_LOAD(0, r4)
            GX_MP_SUM(1)
            p4 = r4;
        }
#undef GX_MP_LOAD
#undef GX_MP_SUM
    } else {
        for (int p = threadIdx.x; p < HW; p += blockDim.x) {
            float fv[PCH];
#pragma unroll
            for (int c = 0; c < PCH; ++c) fv[c] = (c0 + c < C) ? fb[(size_t)c * HW + p] : 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {
                    const float m = expf(log_m[k * kstride + (size_t)b * HW + p]);
                    ms[k] += (double)m;
#pragma unroll
                    for (int c = 0; c < PCH; ++c) acc[k][c] += (double)(m * fv[c]);
                }
            }
        }
    }
    // one multi-value block reduction (wave shuffles, a single LDS hop) instead of K * (PCH + 1) serial ones
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
#pragma unroll
            for (int c = 0; c < PCH; ++c) {
                const double v = gx_wave_sum_d(acc[k][c]);
                if (lane == 0) wred[wave][k * (PCH + 1) + c] = v;
            }
            const double v = gx_wave_sum_d(ms[k]);
            if (lane == 0) wred[wave][k * (PCH + 1) + PCH] = v;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * (PCH + 1); i += blockDim.x) {
        const double s = (wred[0][i] + wred[1][i]) + (wred[2][i] + wred[3][i]);
        const int k = i / (PCH + 1), c = i - k * (PCH + 1);
        if (c < PCH) {
            if (c0 + c < C) S[((size_t)b * K + k) * C + c0 + c] = (float)s;
        } else if (blockIdx.y == 0) {
            msum[(size_t)b * K + k] = (float)s;
        }
    }
}

// df[b][c][p]      = sum_k m_k[p] * gS[b][k][c]
// dlog_m[k][b][p]  = m_k[p] * (sum_c gS[b][k][c] * f[b][c][p] + gmsum[b][k])
// grid (B, HW/256): one thread per pixel; gS of the image staged in LDS.
__global__ void __launch_bounds__(256)
maskpool_bwd_kernel(const float* __restrict__ f, const float* __restrict__ log_m, const float* __restrict__ gS,
                    const float* __restrict__ gmsum, int B, int C, int HW, int K, float* __restrict__ df,
                    float* __restrict__ dlog_m) {
    extern __shared__ __attribute__((aligned(16))) float gsh[];  // [K][C]
    const int b = blockIdx.x;
    const int p = blockIdx.y * blockDim.x + threadIdx.x;
    for (int i = threadIdx.x; i < K * C; i += blockDim.x) gsh[i] = gS[(size_t)b * K * C + i];
    __syncthreads();
    if (p >= HW) return;
    const size_t kstride = (size_t)B * HW;
    float m[KMAX], a[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        m[k] = (k < K) ? expf(log_m[k * kstride + (size_t)b * HW + p]) : 0.f;
        a[k] = 0.f;
    }
    const float* fb = f + (size_t)b * C * HW + p;
    float* dfb = df + (size_t)b * C * HW + p;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {       // (8 independent loads in flight per thread)
        const float fv = fb[(size_t)c * HW];
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K) {
                const float g = gsh[k * C + c];
                a[k] += g * fv;
                d += m[k] * g;
            }
        }
        dfb[(size_t)c * HW] = d;
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) dlog_m[k * kstride + (size_t)b * HW + p] = m[k] * (a[k] + gmsum[(size_t)b * K + k]);
}

// 4 pixels per thread (16-byte accesses); the 4 waves of a workgroup share the same 256 pixels and split the channels
// (the per-pixel channel loop is a chain of dependent load -> store steps: a quarter of the channels per wave and 4x
// the waves in flight); their partial sum_c gS*f are combined through LDS in wave order.
template <int KT>      // (the slot count at compile time, 0: run time -- as maskpool_fwd_kernel: 2 x K float4 of state instead of 2 x 16)
__global__ void __launch_bounds__(256)
maskpool_bwd_vec_kernel(const float* __restrict__ f, const float* __restrict__ log_m, const float* __restrict__ gS,
                        const float* __restrict__ gmsum, int B, int C, int HW, int Krt, float* __restrict__ df,
                        float* __restrict__ dlog_m) {
    const int K = KT ? KT : Krt;
    constexpr int KMAX = KT ? KT : ::KMAX;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* gsh = sm;                                                    // [K][C]
    f32x4* ared = reinterpret_cast<f32x4*>(sm + ((K * C + 3) & ~3));    // [4 waves][K][64 lanes]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int p = (blockIdx.y * 64 + lane) * 4;
    for (int i = threadIdx.x; i < K * C; i += blockDim.x) gsh[i] = gS[(size_t)b * K * C + i];
    __syncthreads();
    const bool act = p < HW;
    const size_t kstride = (size_t)B * HW;
    f32x4 m[KMAX], a[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        a[k][0] = 0.f; a[k][1] = 0.f; a[k][2] = 0.f; a[k][3] = 0.f;
        m[k] = a[k];
        if (k < K && act) {
            const f32x4 lm = *reinterpret_cast<const f32x4*>(log_m + k * kstride + (size_t)b * HW + p);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[k][e] = expf(lm[e]);
        }
    }
    const int cper = (C + 3) / 4;
    const int cbeg = wave * cper, cend = (cbeg + cper < C) ? cbeg + cper : C;
    if (act) {
        const float* fb = f + (size_t)b * C * HW + p;
        float* dfb = df + (size_t)b * C * HW + p;
#pragma unroll 4
        for (int c = cbeg; c < cend; ++c) {
            const f32x4 fv = *reinterpret_cast<const f32x4*>(fb + (size_t)c * HW);
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {
                    const float g = gsh[k * C + c];
                    a[k] += g * fv;
                    d += m[k] * g;
                }
            }
            *reinterpret_cast<f32x4*>(dfb + (size_t)c * HW) = d;
        }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) ared[(wave * K + k) * 64 + lane] = a[k];
    __syncthreads();
    if (wave == 0 && act) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K) {
                const f32x4 t = (ared[(0 * K + k) * 64 + lane] + ared[(1 * K + k) * 64 + lane]) +
                                (ared[(2 * K + k) * 64 + lane] + ared[(3 * K + k) * 64 + lane]);
                *reinterpret_cast<f32x4*>(dlog_m + k * kstride + (size_t)b * HW + p) =
                    m[k] * (t + gmsum[(size_t)b * K + k]);
            }
        }
    }
}

// ------------------------------------------------------------------ mixture likelihood
// dec [K*B, 4, HW] slot-major (row k*B+b): channels 0..2 RGB pre-activation, 3 mask logit.
constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;

// KT: the slot count as a compile-time constant (0: run time, `Krt`).  With the K < KMAX guards of the unrolled slot loops folded
// away the 4 K + 3 loads of a pixel are independent instructions hipcc issues together; with run-time guards they are a chain of
// guarded loads (load - wait - branch), and this one-pixel-per-thread kernel at two waves per SIMD is bound by exactly that latency.
template <bool BWD, int KT>
__global__ void __launch_bounds__(256)
mixture_kernel(const float* __restrict__ x, const float* __restrict__ dec, int B, int HW, int Krt, float std_,
               int pixel_bound, float* __restrict__ recon, float* __restrict__ x_r, float* __restrict__ log_m_r,
               float* __restrict__ err_part, const float* __restrict__ g_err, float* __restrict__ ddec,
               const float* __restrict__ log_w, float* __restrict__ dlog_w, float std_first, int DC) {
    // DC = channels of `dec` per slot: 4 (RGB + mask logit) or 3 (GENESIS: RGB only, needs log_w)
    // log_w != NULL (MONet, models/monet_config.py:94-105): the mixing log-weights are the ATTENTION masks
    // [K,B,HW] instead of log_softmax(logits); the first slot may use its own pixel std (std_first).
    const int K = KT ? KT : Krt;
    constexpr int KMAX = KT ? KT : ::KMAX;          // (shadows the file's bound: the unrolled loops run to the actual slot count)
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int p = blockIdx.y * blockDim.x + threadIdx.x;
    double err = 0.0;
    if (p < HW) {
        float logit[KMAX];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < K) {
                logit[k] = (DC == 4) ? dec[(((size_t)k * B + b) * 4 + 3) * HW + p] : 0.f;
                mx = fmaxf(mx, logit[k]);
            } else {
                logit[k] = 0.f;
            }
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) se += expf(logit[k] - mx);
        const float lse = logf(se);
        float lm[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            lm[k] = (k < K) ? (logit[k] - mx) - lse : 0.f;   // torch log_softmax: (x - max) - log(sum exp(x - max))
            if (!BWD && k < K && log_m_r) log_m_r[((size_t)k * B + b) * HW + p] = lm[k];
            if (log_w && k < K) lm[k] = log_w[((size_t)k * B + b) * HW + p];
        }
        float dlogit[KMAX];
        if (BWD) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) dlogit[k] = 0.f;
        }
        const float ge = BWD ? g_err[b] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float xv = x[((size_t)b * 3 + c) * HW + p];
            float e[KMAX], mu[KMAX];
            float s = 0.f, rc = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {
                    const float raw = dec[(((size_t)k * B + b) * DC + c) * HW + p];
                    mu[k] = pixel_bound ? 1.f / (1.f + expf(-raw)) : raw;
                    const float dx = xv - mu[k];
                    const float sd = (k == 0) ? std_first : std_;
                    const float logn = -(dx * dx) / (2.f * sd * sd) - logf(sd) - LOG_SQRT_2PI;
                    e[k] = expf(lm[k] + logn);
                    s += e[k];
                    if (!BWD) {
                        x_r[(((size_t)k * B + b) * 3 + c) * HW + p] = mu[k];
                        rc += expf(lm[k]) * mu[k];
                    }
                } else { e[k] = 0.f; mu[k] = 0.f; }
            }
            if (!BWD) {
                err += (double)(-logf(s));
                recon[((size_t)b * 3 + c) * HW + p] = rc;
            } else {
                const float inv = 1.f / s;
#pragma unroll
                for (int k = 0; k < KMAX; ++k) {
                    if (k < K) {
                        const float w = e[k] * inv;                 // responsibility of slot k
                        dlogit[k] -= w;                             // d err / d log_m_r_k
                        const float sd = (k == 0) ? std_first : std_;
                        float gmu = -w * (xv - mu[k]) / (sd * sd);
                        if (pixel_bound) gmu *= mu[k] * (1.f - mu[k]);
                        ddec[(((size_t)k * B + b) * DC + c) * HW + p] = ge * gmu;
                    }
                }
            }
        }
        if (BWD) {
            // through log_softmax: d/d logit_j = g_j - softmax_j * sum_k g_k
            float gsum = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) if (k < K) gsum += dlogit[k];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (k < K) {
                    if (log_w) {
                        dlog_w[((size_t)k * B + b) * HW + p] = ge * dlogit[k];
                        if (DC == 4) ddec[(((size_t)k * B + b) * 4 + 3) * HW + p] = 0.f;
                    } else {
                        ddec[(((size_t)k * B + b) * 4 + 3) * HW + p] = ge * (dlogit[k] - expf(lm[k]) * gsum);
                    }
                }
            }
        }
    }
    if (!BWD) {
        const double s = block_sum_dd(err, red);
        if (threadIdx.x == 0) err_part[(size_t)b * gridDim.y + blockIdx.y] = (float)s;
    }
}

__global__ void row_sum_kernel(const float* __restrict__ part, int rows, int cols, float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
    for (int i = 0; i < cols; ++i) s += part[(size_t)r * cols + i];
    out[r] = (float)s;
}

// Input of a 1x1 conv that is still the PRE-norm tensor y of a GroupNorm+ReLU layer: relu(gn(y)) is formed on load
// (same expression as the norm kernels, gx_norm.hip) so that the normalised activation never exists in memory.
// mean == nullptr: plain input.
struct NormIn {
    const float* mean;    // [N*groups]
    const float* rstd;    // [N*groups]
    const float* gamma;   // [C]
    const float* beta;    // [C]
    int groups;
    int cpg;              // channels per group
};

__device__ __forceinline__ f32x4 norm_relu4(const NormIn& nin, f32x4 v, int n, int c) {
    const int g = n * nin.groups + c / nin.cpg;
    const float meanf = nin.mean[g], rstdf = nin.rstd[g], gm = nin.gamma[c], bt = nin.beta[c];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = (v[e] - meanf) * rstdf * gm + bt;
        o[e] = t > 0.f ? t : 0.f;
    }
    return o;
}

// ------------------------------------------------------------------ small 1x1 convolutions (Cout <= 8)
// y[n][co][p] = gate * (sum_ci w[co][ci] x[n][ci][p] + b[co]) + addend[co][p]
constexpr int COMAX = 8;
__global__ void __launch_bounds__(256)
conv1x1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                   const float* __restrict__ gate, const float* __restrict__ addend, int Cin, int Cout, int HW,
                   float* __restrict__ y) {
    const int n = blockIdx.x;
    const int p = blockIdx.y * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    float acc[COMAX];
#pragma unroll
    for (int co = 0; co < COMAX; ++co) acc[co] = 0.f;
    const float* xn = x + (size_t)n * Cin * HW + p;
    for (int ci = 0; ci < Cin; ++ci) {
        const float xv = xn[(size_t)ci * HW];
#pragma unroll
        for (int co = 0; co < COMAX; ++co)
            if (co < Cout) acc[co] += w[co * Cin + ci] * xv;
    }
    const float gt = gate ? *gate : 1.f;
#pragma unroll
    for (int co = 0; co < COMAX; ++co) {
        if (co < Cout) {
            float v = acc[co] + (bias ? bias[co] : 0.f);
            v = gate ? gt * v : v;
            if (addend) v += addend[(size_t)co * HW + p];
            y[((size_t)n * Cout + co) * HW + p] = v;
        }
    }
}

// 4 pixels per thread (16-byte accesses), channel loop unrolled by 8 so that 8 independent loads are in flight per
// thread: the op is a pure stream of x (Cin/Cout = 16x more bytes in than out).  The weights sit zero-padded to
// COMAX output channels in LDS (broadcast reads, no per-channel predicates in the loop).
__global__ void __launch_bounds__(256)
conv1x1_fwd_vec_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                       const float* __restrict__ gate, const float* __restrict__ addend, int Cin, int Cout, int HW,
                       float* __restrict__ y, const NormIn nin) {
    __shared__ __attribute__((aligned(16))) float ws[128 * COMAX];   // [ci][co], Cin <= 128
    for (int i = threadIdx.x; i < Cin * COMAX; i += blockDim.x) {
        const int ci = i / COMAX, co = i - ci * COMAX;
        ws[i] = co < Cout ? w[co * Cin + ci] : 0.f;
    }
    __syncthreads();
    const int n = blockIdx.x;
    const int p = (blockIdx.y * blockDim.x + threadIdx.x) * 4;
    if (p >= HW) return;
    f32x4 acc[COMAX];
#pragma unroll
    for (int co = 0; co < COMAX; ++co) { acc[co][0] = 0.f; acc[co][1] = 0.f; acc[co][2] = 0.f; acc[co][3] = 0.f; }
    const float* xn = x + (size_t)n * Cin * HW + p;
    int ci = 0;
    for (; ci + 8 <= Cin; ci += 8) {
        f32x4 xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = *reinterpret_cast<const f32x4*>(xn + (size_t)(ci + j) * HW);
        if (nin.mean) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = norm_relu4(nin, xv[j], n, ci + j);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(ws + (ci + j) * COMAX);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(ws + (ci + j) * COMAX + 4);
#pragma unroll
            for (int co = 0; co < 4; ++co) { acc[co] += w0[co] * xv[j]; acc[co + 4] += w1[co] * xv[j]; }
        }
    }
    for (; ci < Cin; ++ci) {
        f32x4 xv = *reinterpret_cast<const f32x4*>(xn + (size_t)ci * HW);
        if (nin.mean) xv = norm_relu4(nin, xv, n, ci);
#pragma unroll
        for (int co = 0; co < COMAX; ++co) acc[co] += ws[ci * COMAX + co] * xv;
    }
    const float gt = gate ? *gate : 1.f;
#pragma unroll
    for (int co = 0; co < COMAX; ++co) {
        if (co < Cout) {
            f32x4 v = acc[co] + (bias ? bias[co] : 0.f);
            if (gate) v = gt * v;
            if (addend) v += *reinterpret_cast<const f32x4*>(addend + (size_t)co * HW + p);
            *reinterpret_cast<f32x4*>(y + ((size_t)n * Cout + co) * HW + p) = v;
        }
    }
}

// dx[n][ci][p] = gate * sum_co w[co][ci] dy[n][co][p];  pb[blk][co] = sum_p dy[n][co][p] (ungated, per block)
// ACT: dx *= act'(actx) -- actx = the conv's INPUT, the output of a bias + ReLU (1) / ELU (2) layer whose backward this is
template <bool ACT>
__global__ void __launch_bounds__(256)
conv1x1_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ gate,
                     int Cin, int Cout, int HW, float* __restrict__ dx, float* __restrict__ pb,
                     const float* __restrict__ actx, int act, float* __restrict__ amax_parts) {
    __shared__ double red[4];
    float am = 0.f;               // ACT + an armed gx_amax_tap: largest |dx| this thread stores
    const int n = blockIdx.x;
    const int p = blockIdx.y * blockDim.x + threadIdx.x;
    const float gt = gate ? *gate : 1.f;
    float raw[COMAX], g[COMAX];
#pragma unroll
    for (int co = 0; co < COMAX; ++co) {
        raw[co] = (co < Cout && p < HW) ? dy[((size_t)n * Cout + co) * HW + p] : 0.f;
        g[co] = gt * raw[co];
    }
    if (p < HW) {
        float* dxn = dx + (size_t)n * Cin * HW + p;
        if constexpr (ACT) {
            const float* axn = actx + (size_t)n * Cin * HW + p;
#pragma unroll 4
            for (int ci = 0; ci < Cin; ++ci) {
                const float o = axn[(size_t)ci * HW];
                float s = 0.f;
#pragma unroll
                for (int co = 0; co < COMAX; ++co)
                    if (co < Cout) s += w[co * Cin + ci] * g[co];
                const float neg = act == 2 ? o + 1.f : 0.f;
                const float dv = s * (o > 0.f ? 1.f : neg);
                dxn[(size_t)ci * HW] = dv;
                am = fmaxf(am, fabsf(dv));
            }
        } else {
        for (int ci = 0; ci < Cin; ++ci) {
            float s = 0.f;
#pragma unroll
            for (int co = 0; co < COMAX; ++co)
                if (co < Cout) s += w[co * Cin + ci] * g[co];
            dxn[(size_t)ci * HW] = s;
        }
        }
    }
    const int blk = blockIdx.x * gridDim.y + blockIdx.y;
#pragma unroll
    for (int co = 0; co < COMAX; ++co) {
        if (co < Cout) {
            const double sum = block_sum_dd((double)raw[co], red);
            if (threadIdx.x == 0) pb[(size_t)blk * Cout + co] = (float)sum;
        }
    }
    if constexpr (ACT) {
        if (amax_parts) gx_block_amax_store(am, amax_parts, (unsigned)blk);      // (uniform)
    }
}

// Weight gradient of the small 1x1 conv on the fp32 matrix cores (v_mfma_f32_16x16x4_f32):
//   D[co (16, Cout <= 8 valid)][ci 16-tile] += A[co][k] * B[k][ci],  k = 4 pixel slots.
// HBM-bound (x is read exactly once).  Both operands go global -> registers: k slot q of a wave owns 16
// contiguous pixels of the wave's 64-pixel chunk, so each lane streams one channel row with 16-byte loads.
// pw[blk][co][ci] (ungated partial per block; the 4 waves of a block are combined through LDS).
template <int CIT>   // ci tiles of 16 (Cin <= 16*CIT)
__global__ void __launch_bounds__(256)
conv1x1_wgrad_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int Cin, int Cout,
                          int HW, float* __restrict__ pw) {
    __shared__ float red[4][16][16 * CIT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = lane & 15, q = lane >> 4;
    const int chunks_per_img = HW >> 6;
    const int nchunks = N * chunks_per_img;
    f32x4 acc[CIT];
#pragma unroll
    for (int t = 0; t < CIT; ++t) { acc[t][0] = 0.f; acc[t][1] = 0.f; acc[t][2] = 0.f; acc[t][3] = 0.f; }
    for (int c = blockIdx.x * 4 + wave; c < nchunks; c += gridDim.x * 4) {
        const int n = c / chunks_per_img;
        const int p0 = (c - n * chunks_per_img) * 64 + q * 16;
        f32x4 av[4], bv[CIT][4];
        const bool a_ok = row < Cout;
        const float* ap = dy + ((size_t)n * Cout + (a_ok ? row : 0)) * HW + p0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[i] = *reinterpret_cast<const f32x4*>(ap + 4 * i);
            if (!a_ok) { av[i][0] = 0.f; av[i][1] = 0.f; av[i][2] = 0.f; av[i][3] = 0.f; }
        }
#pragma unroll
        for (int t = 0; t < CIT; ++t) {
            const int ci = t * 16 + row;
            const bool b_ok = ci < Cin;
            const float* bp = x + ((size_t)n * Cin + (b_ok ? ci : 0)) * HW + p0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bv[t][i] = *reinterpret_cast<const f32x4*>(bp + 4 * i);
                if (!b_ok) { bv[t][i][0] = 0.f; bv[t][i][1] = 0.f; bv[t][i][2] = 0.f; bv[t][i][3] = 0.f; }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < CIT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][u], bv[t][i][u], acc[t], 0, 0, 0);
    }
    // C/D layout (16x16): col = lane & 15 (ci), row = (lane >> 4) * 4 + reg (co)
#pragma unroll
    for (int t = 0; t < CIT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][q * 4 + r][t * 16 + row] = acc[t][r];
    __syncthreads();
    for (int i = threadIdx.x; i < Cout * Cin; i += blockDim.x) {
        const int co = i / Cin, ci = i - co * Cin;
        pw[(size_t)blockIdx.x * Cout * Cin + i] = (red[0][co][ci] + red[1][co][ci]) + (red[2][co][ci] + red[3][co][ci]);
    }
}

// LDS-staged variant (Cin <= 64, H*W a multiple of 256).  The direct-from-global kernel above is bound by the
// MFMA operand layout: lanes of one load differ by channel (16 KB apart) and pixel slot, so every load instruction
// is a 64-line gather (2.2 TB/s on the 235 MB decoder activation).  Here a workgroup stages a 256-pixel tile of all
// channels with fully coalesced 16-byte loads (one channel row segment = 1 KiB per wave instruction; the next tile is
// prefetched into registers while the current one is consumed), and the MFMA fragments are read from LDS
// (row stride 260 floats: the 64 lanes of a fragment read spread over all banks twice = conflict-free).
// NORM: x is a pre-norm tensor (NormIn), normalised while it is staged; the kernel then also emits the bias
// gradient partials pb[block][co] = sum_p dy (the plain path gets them from the data-gradient kernel).
constexpr int C1_TP = 256, C1_LS = 260;
template <bool NORM>
__global__ void __launch_bounds__(256)
conv1x1_wgrad_lds_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int Cin, int Cout,
                         int HW, float* __restrict__ pw, const NormIn nin, float* __restrict__ pb) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* xs = sm;                       // [64][C1_LS]
    float* ds = sm + 64 * C1_LS;          // [8][C1_LS]
    float (*red)[16][64] = reinterpret_cast<float (*)[16][64]>(sm);   // epilogue re-uses the tile memory
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int idx = lane & 15, kq = lane >> 4;
    const int tiles_per_img = HW / C1_TP;
    const int ntiles = N * tiles_per_img;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { acc[t][0] = 0.f; acc[t][1] = 0.f; acc[t][2] = 0.f; acc[t][3] = 0.f; }
    f32x4 xr[16], dr[2];
    f32x4 dbs[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#define C1_LOAD(tile_)                                                                              \
    {                                                                                               \
        const int n_ = (tile_) / tiles_per_img;                                                     \
        const int p0_ = ((tile_) - n_ * tiles_per_img) * C1_TP + 4 * lane;                          \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                            \
            const int ch = wave + 4 * i;                                                            \
            if (ch < Cin) {                                                                         \
                xr[i] = *reinterpret_cast<const f32x4*>(x + ((size_t)n_ * Cin + ch) * HW + p0_);    \
                if (NORM) xr[i] = norm_relu4(nin, xr[i], n_, ch);                                   \
            } else { xr[i][0] = 0.f; xr[i][1] = 0.f; xr[i][2] = 0.f; xr[i][3] = 0.f; }              \
        }                                                                                           \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                             \
            const int co = wave + 4 * i;                                                            \
            if (co < Cout) dr[i] = *reinterpret_cast<const f32x4*>(dy + ((size_t)n_ * Cout + co) * HW + p0_); \
            else { dr[i][0] = 0.f; dr[i][1] = 0.f; dr[i][2] = 0.f; dr[i][3] = 0.f; }                \
        }                                                                                           \
    }
    int tile = blockIdx.x;
    if (tile < ntiles) C1_LOAD(tile)
    for (; tile < ntiles; tile += gridDim.x) {
        __syncthreads();                  // previous tile fully consumed
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<f32x4*>(xs + (wave + 4 * i) * C1_LS + 4 * lane) = xr[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(ds + (wave + 4 * i) * C1_LS + 4 * lane) = dr[i];
            if (NORM) dbs[i] += dr[i];
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) C1_LOAD(tile + gridDim.x)
        const float* ap = ds + (idx & 7) * C1_LS + 64 * wave + kq;
        const float* bp = xs + idx * C1_LS + 64 * wave + kq;
        const bool a_ok = idx < 8;
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const float a = a_ok ? ap[4 * st] : 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 16 * C1_LS + 4 * st], acc[t], 0, 0, 0);
        }
    }
#undef C1_LOAD
    if (NORM) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int co = wave + 4 * i;
            float v = (dbs[i][0] + dbs[i][1]) + (dbs[i][2] + dbs[i][3]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0 && co < Cout) pb[(size_t)blockIdx.x * Cout + co] = v;
        }
    }
    __syncthreads();
    // C/D layout (16x16): col = lane & 15 (ci), row = (lane >> 4) * 4 + reg (co)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][kq * 4 + r][t * 16 + idx] = acc[t][r];
    __syncthreads();
    for (int i = tid; i < Cout * Cin; i += blockDim.x) {
        const int co = i / Cin, ci = i - co * Cin;
        pw[(size_t)blockIdx.x * Cout * Cin + i] = (red[0][co][ci] + red[1][co][ci]) + (red[2][co][ci] + red[3][co][ci]);
    }
}

// raw = [dw_raw (Cout*Cin) | db_raw (Cout)] (ungated sums).  dgate = <w, dw_raw> + <b, db_raw>
// (since sum_p dy*(W x + b) = sum_ci w * (sum_p dy x) + b * sum_p dy); dw = gate*dw_raw; db = gate*db_raw.
__global__ void __launch_bounds__(256)
conv1x1_finalize_kernel(const float* __restrict__ raw, const float* __restrict__ w, const float* __restrict__ bias,
                        const float* __restrict__ gate, int Cin, int Cout, float* __restrict__ dw,
                        float* __restrict__ db, float* __restrict__ dgate) {
    __shared__ double red[4];
    const int npairs = Cout * Cin;
    const float gt = gate ? *gate : 1.f;
    double s = 0.0;
    for (int i = threadIdx.x; i < npairs; i += blockDim.x) {
        const float r = raw[i];
        dw[i] = gt * r;
        s += (double)r * w[i];
    }
    for (int i = threadIdx.x; i < Cout; i += blockDim.x) {
        const float r = raw[npairs + i];
        if (db) db[i] = gt * r;
        if (bias) s += (double)r * bias[i];
    }
    s = block_sum_dd(s, red);
    if (threadIdx.x == 0 && dgate) *dgate = (float)s;
}

// the two partial-sum tables of the 1x1-conv backward (weight pairs, bias) in one launch: blocks [0, n0) reduce
// part0 into out0, blocks [n0, n0 + n1) reduce part1 into out1
__global__ void __launch_bounds__(256)
col_sum2_kernel(const float* __restrict__ part0, int nblk0, int n0, float* __restrict__ out0,
                const float* __restrict__ part1, int nblk1, int n1, float* __restrict__ out1, int accumulate = 0) {
    __shared__ double red[4];
    const bool first = (int)blockIdx.x < n0;
    const int i = first ? blockIdx.x : blockIdx.x - n0;
    const float* part = first ? part0 : part1;
    const int nblk = first ? nblk0 : nblk1, n = first ? n0 : n1;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += blockDim.x) s += part[(size_t)b * n + i];
    s = block_sum_dd(s, red);
    if (threadIdx.x == 0) {
        float* out = first ? out0 : out1;
        if (out) out[i] = accumulate ? out[i] + (float)s : (float)s;      // (a parameter used again in the same iteration)
    }
}

}  // namespace

extern "C" {

int gx_maskpool_fwd(const float* f, const float* log_m, int B, int C, int H, int W, int K, float* S, float* msum,
                    gx_stream_t stream) {
    GX_CHECK_ARG(f && log_m && S && msum, "gx_maskpool_fwd: null pointer");
    GX_CHECK_ARG(B > 0 && C > 0 && K >= 1 && K <= KMAX && H > 0 && W > 0, "gx_maskpool_fwd: bad dims (K<=16)");
    {
        GxProf pf(KID_MASKPOOL_FWD, (hipStream_t)stream, 2.0 * B * K * C * H * W, 4.0 * B * H * W * (C + K));
#define GX_MP_FWD(KT_)                                                                                                 \
        hipLaunchKernelGGL(maskpool_fwd_kernel<KT_>, dim3(B, gx_ceil_div(C, PCH)), dim3(256), 0, (hipStream_t)stream, f,  \
                           log_m, B, C, H * W, K, S, msum)
        if (K == 7) GX_MP_FWD(7); else if (K == 5) GX_MP_FWD(5); else if (K == 11) GX_MP_FWD(11); else GX_MP_FWD(0);
#undef GX_MP_FWD
    }
    GX_CHECK_LAUNCH("gx_maskpool_fwd");
    return GX_OK;
}

int gx_maskpool_bwd(const float* f, const float* log_m, const float* gS, const float* gmsum, int B, int C, int H,
                    int W, int K, float* df, float* dlog_m, gx_stream_t stream) {
    GX_CHECK_ARG(f && log_m && gS && gmsum && df && dlog_m, "gx_maskpool_bwd: null pointer");
    GX_CHECK_ARG(B > 0 && C > 0 && K >= 1 && K <= KMAX && H > 0 && W > 0, "gx_maskpool_bwd: bad dims (K<=16)");
    const int HW = H * W;
    {
        GxProf pf(KID_MASKPOOL_BWD, (hipStream_t)stream, 4.0 * B * K * C * HW, 4.0 * B * HW * (2.0 * C + 2.0 * K));
        if (gx_vec4_ok(HW, f, log_m, df, dlog_m)) {
#define GX_MP_BWD(KT_)                                                                                                 \
            hipLaunchKernelGGL(maskpool_bwd_vec_kernel<KT_>, dim3(B, gx_ceil_div(HW, 256)), dim3(256),                \
                               (size_t)(((K * C + 3) & ~3) + 4 * K * 64 * 4) * sizeof(float), (hipStream_t)stream, f,   \
                               log_m, gS, gmsum, B, C, HW, K, df, dlog_m)
            if (K == 7) GX_MP_BWD(7); else if (K == 5) GX_MP_BWD(5); else if (K == 11) GX_MP_BWD(11); else GX_MP_BWD(0);
#undef GX_MP_BWD
        }
        else
            hipLaunchKernelGGL(maskpool_bwd_kernel, dim3(B, gx_ceil_div(HW, 256)), dim3(256),
                               (size_t)K * C * sizeof(float), (hipStream_t)stream, f, log_m, gS, gmsum, B, C, HW, K, df,
                               dlog_m);
    }
    GX_CHECK_LAUNCH("gx_maskpool_bwd");
    return GX_OK;
}

size_t gx_mixture_ws_bytes(int B, int H, int W) { return (size_t)B * gx_ceil_div(H * W, 256) * sizeof(float); }

static int mixture_fwd_impl(const float* x, const float* dec, const float* log_w, int dec_ch, int B, int H, int W, int K,
                            float std_first, float pixel_std, int pixel_bound, float* recon, float* x_r,
                            float* log_m_r, float* err, void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(x && dec && recon && x_r && err && ws, "gx_mixture_fwd: null pointer");
    GX_CHECK_ARG(B > 0 && K >= 1 && K <= KMAX && pixel_std > 0.f, "gx_mixture_fwd: bad dims (K<=16)");
    GX_CHECK_ARG(ws_bytes >= gx_mixture_ws_bytes(B, H, W), "gx_mixture_fwd: workspace too small");
    const int HW = H * W, nb = gx_ceil_div(HW, 256);
    hipStream_t s = (hipStream_t)stream;
    {
        // read x (3) + dec (4K); write recon (3), x_r (3K), log_m_r (K)
        GxProf pf(KID_MIXTURE_FWD, s, 0.0, 4.0 * B * HW * (6.0 + 8.0 * K));
#define GX_MIX_FWD(KT_)                                                                                                \
        hipLaunchKernelGGL((mixture_kernel<false, KT_>), dim3(B, nb), dim3(256), 0, s, x, dec, B, HW, K, pixel_std,       \
                           pixel_bound, recon, x_r, log_m_r, (float*)ws, (const float*)nullptr, (float*)nullptr,         \
                           log_w, (float*)nullptr, std_first, dec_ch)
        if (K == 7) GX_MIX_FWD(7); else if (K == 5) GX_MIX_FWD(5); else if (K == 11) GX_MIX_FWD(11); else GX_MIX_FWD(0);
#undef GX_MIX_FWD
    }
    GX_CHECK_LAUNCH("gx_mixture_fwd");
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 4.0 * B * nb);
        hipLaunchKernelGGL(row_sum_kernel, dim3(gx_ceil_div(B, 64)), dim3(64), 0, s, (const float*)ws, B, nb, err);
    }
    GX_CHECK_LAUNCH("gx_mixture_fwd(reduce)");
    return GX_OK;
}

static int mixture_bwd_impl(const float* x, const float* dec, const float* log_w, const float* g_err, int dec_ch,
                            int B, int H, int W, int K, float std_first, float pixel_std, int pixel_bound, float* ddec,
                            float* dlog_w, gx_stream_t stream) {
    GX_CHECK_ARG(x && dec && g_err && ddec, "gx_mixture_bwd: null pointer");
    GX_CHECK_ARG(B > 0 && K >= 1 && K <= KMAX && pixel_std > 0.f, "gx_mixture_bwd: bad dims (K<=16)");
    const int HW = H * W, nb = gx_ceil_div(HW, 256);
    {
        GxProf pf(KID_MIXTURE_BWD, (hipStream_t)stream, 0.0, 4.0 * B * HW * (3.0 + 8.0 * K));
#define GX_MIX_BWD(KT_)                                                                                                \
        hipLaunchKernelGGL((mixture_kernel<true, KT_>), dim3(B, nb), dim3(256), 0, (hipStream_t)stream, x, dec, B, HW, K,  \
                           pixel_std, pixel_bound, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,   \
                           g_err, ddec, log_w, dlog_w, std_first, dec_ch)
        if (K == 7) GX_MIX_BWD(7); else if (K == 5) GX_MIX_BWD(5); else if (K == 11) GX_MIX_BWD(11); else GX_MIX_BWD(0);
#undef GX_MIX_BWD
    }
    GX_CHECK_LAUNCH("gx_mixture_bwd");
    return GX_OK;
}

int gx_mixture_fwd(const float* x, const float* dec, int B, int H, int W, int K, float pixel_std, int pixel_bound,
                   float* recon, float* x_r, float* log_m_r, float* err, void* ws, size_t ws_bytes,
                   gx_stream_t stream) {
    GX_CHECK_ARG(log_m_r, "gx_mixture_fwd: null pointer");
    return mixture_fwd_impl(x, dec, nullptr, 4, B, H, W, K, pixel_std, pixel_std, pixel_bound, recon, x_r, log_m_r, err,
                            ws, ws_bytes, stream);
}

int gx_mixture_bwd(const float* x, const float* dec, const float* g_err, int B, int H, int W, int K,
                   float pixel_std, int pixel_bound, float* ddec, gx_stream_t stream) {
    return mixture_bwd_impl(x, dec, nullptr, g_err, 4, B, H, W, K, pixel_std, pixel_std, pixel_bound, ddec, nullptr,
                            stream);
}

int gx_mixture_w_fwd(const float* x, const float* dec, const float* log_w, int dec_ch, int B, int H, int W, int K,
                     float pixel_std1, float pixel_std2, int pixel_bound, float* recon, float* x_r, float* err,
                     void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(log_w && (dec_ch == 3 || dec_ch == 4), "gx_mixture_w_fwd: null pointer / dec_ch must be 3 or 4");
    return mixture_fwd_impl(x, dec, log_w, dec_ch, B, H, W, K, pixel_std1, pixel_std2, pixel_bound, recon, x_r, nullptr, err,
                            ws, ws_bytes, stream);
}

int gx_mixture_w_bwd(const float* x, const float* dec, const float* log_w, const float* g_err, int dec_ch, int B,
                     int H, int W, int K, float pixel_std1, float pixel_std2, int pixel_bound, float* ddec,
                     float* dlog_w, gx_stream_t stream) {
    GX_CHECK_ARG(log_w && dlog_w && (dec_ch == 3 || dec_ch == 4), "gx_mixture_w_bwd: null pointer / dec_ch");
    return mixture_bwd_impl(x, dec, log_w, g_err, dec_ch, B, H, W, K, pixel_std1, pixel_std2, pixel_bound, ddec, dlog_w,
                            stream);
}

int gx_conv1x1_fwd(const float* x, const float* w, const float* bias, const float* gate, const float* addend,
                   int N, int Cin, int Cout, int H, int W, float* y, gx_stream_t stream) {
    GX_CHECK_ARG(x && w && y, "gx_conv1x1_fwd: null pointer");
    GX_CHECK_ARG(N > 0 && Cin > 0 && Cout > 0 && Cout <= COMAX, "gx_conv1x1_fwd: Cout must be <= 8");
    const int HW = H * W;
    {
        GxProf pf(KID_CONV1X1_FWD, (hipStream_t)stream, 2.0 * N * Cin * Cout * HW, 4.0 * N * HW * (Cin + Cout));
        const bool vec = (HW % 4) == 0 && Cin <= 128 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 &&
                         (!addend || ((uintptr_t)addend % 16) == 0);
        if (vec)
            hipLaunchKernelGGL(conv1x1_fwd_vec_kernel, dim3(N, gx_ceil_div(HW, 1024)), dim3(256), 0,
                               (hipStream_t)stream, x, w, bias, gate, addend, Cin, Cout, HW, y,
                               NormIn{nullptr, nullptr, nullptr, nullptr, 1, 1});
        else
            hipLaunchKernelGGL(conv1x1_fwd_kernel, dim3(N, gx_ceil_div(HW, 256)), dim3(256), 0, (hipStream_t)stream, x,
                               w, bias, gate, addend, Cin, Cout, HW, y);
    }
    GX_CHECK_LAUNCH("gx_conv1x1_fwd");
    return GX_OK;
}

static int conv1x1_wgrad_blocks(int N, int HW) {
    const int nchunks = N * (HW / 64);
    int b = gx_ceil_div(nchunks, 4);
    return b > 1024 ? 1024 : (b < 1 ? 1 : b);
}

size_t gx_conv1x1_bwd_ws_bytes(int N, int Cin, int Cout, int H, int W) {
    const int HW = H * W;
    const size_t nblkw = conv1x1_wgrad_blocks(N, HW);
    const size_t nblkd = (size_t)N * gx_ceil_div(HW, 256);
    return (nblkw * Cout * Cin + nblkd * Cout + (size_t)Cout * Cin + Cout) * sizeof(float);
}

int gx_conv1x1_bwd(const float* x, const float* dy, const float* w, const float* bias, const float* gate, int N,
                   int Cin, int Cout, int H, int W, float* dx, float* dw, float* db, float* dgate, void* ws,
                   size_t ws_bytes, gx_stream_t stream) {
    return gx_conv1x1_bwd_ex(x, dy, w, bias, gate, N, Cin, Cout, H, W, dx, dw, db, dgate, 0, ws, ws_bytes, stream);
}

static int conv1x1_bwd_impl(const float* x, const float* dy, const float* w, const float* bias, const float* gate, int N,
                            int Cin, int Cout, int H, int W, float* dx, float* dw, float* db, float* dgate, int accumulate,
                            int act, float* dbx, void* ws, size_t ws_bytes, gx_stream_t stream);

int gx_conv1x1_bwd_ex(const float* x, const float* dy, const float* w, const float* bias, const float* gate, int N,
                      int Cin, int Cout, int H, int W, float* dx, float* dw, float* db, float* dgate, int accumulate,
                      void* ws, size_t ws_bytes, gx_stream_t stream) {
    return conv1x1_bwd_impl(x, dy, w, bias, gate, N, Cin, Cout, H, W, dx, dw, db, dgate, accumulate, 0, nullptr, ws, ws_bytes,
                            stream);
}

/* ... of a conv whose input x is the output of a bias + activation layer: dxa = dx * act'(x) in the data-gradient kernel and
 * that layer's bias gradient dbx [Cin] = sum_{n,hw} dxa (gx_bias_act_bwd without its pass) */
size_t gx_conv1x1_bwd_act_ws_bytes(int N, int Cin, int Cout, int H, int W) {
    return gx_round_up((long)gx_conv1x1_bwd_ws_bytes(N, Cin, Cout, H, W), 256) + (size_t)N * Cin * sizeof(float);
}
int gx_conv1x1_bwd_act(const float* x, const float* dy, const float* w, const float* bias, int N, int Cin, int Cout, int H,
                       int W, int act, float* dxa, float* dw, float* db, float* dbx, void* ws, size_t ws_bytes,
                       gx_stream_t stream) {
    GX_CHECK_ARG(act == 1 || act == 2, "gx_conv1x1_bwd_act: act must be 1 (ReLU) or 2 (ELU)");
    GX_CHECK_ARG(ws_bytes >= gx_conv1x1_bwd_act_ws_bytes(N, Cin, Cout, H, W), "gx_conv1x1_bwd_act: workspace too small");
    return conv1x1_bwd_impl(x, dy, w, bias, nullptr, N, Cin, Cout, H, W, dxa, dw, db, nullptr, 0, act, dbx, ws, ws_bytes, stream);
}

static int conv1x1_bwd_impl(const float* x, const float* dy, const float* w, const float* bias, const float* gate, int N,
                            int Cin, int Cout, int H, int W, float* dx, float* dw, float* db, float* dgate, int accumulate,
                            int act, float* dbx, void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(x && dy && w && dx && dw && ws, "gx_conv1x1_bwd: null pointer");
    GX_CHECK_ARG(!accumulate || !gate, "gx_conv1x1_bwd_ex: accumulate is for the plain (ungated) conv");
    GX_CHECK_ARG(N > 0 && Cin > 0 && Cout > 0 && Cout <= COMAX && Cin <= 128,
                 "gx_conv1x1_bwd: Cout must be <= 8 and Cin <= 128");
    GX_CHECK_ARG((gate == nullptr) == (dgate == nullptr), "gx_conv1x1_bwd: gate and dgate go together");
    const int HW = H * W;
    GX_CHECK_ARG(HW % 64 == 0, "gx_conv1x1_bwd: H*W must be a multiple of 64");
    GX_CHECK_ARG(ws_bytes >= gx_conv1x1_bwd_ws_bytes(N, Cin, Cout, H, W), "gx_conv1x1_bwd: workspace too small");
    const int nblkw = conv1x1_wgrad_blocks(N, HW);
    const int nblkd = N * gx_ceil_div(HW, 256);
    const int npairs = Cout * Cin;
    float* pw = (float*)ws;
    float* pb = pw + (size_t)nblkw * npairs;
    float* raw = pb + (size_t)nblkd * Cout;
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_CONV1X1_DGRAD, s, 2.0 * N * Cin * Cout * HW, 4.0 * N * HW * (Cin + Cout));
        if (act) {
            // (an armed gx_amax_tap: dxa's partial maxima for the canvas conv that reads it next -- the first data gradient of a
            //  BroadcastDecoder chain)
            float* ap = gx_amax_producer_out(dx, false, (unsigned)nblkd, (size_t)N * Cin * HW);
            hipLaunchKernelGGL(conv1x1_dgrad_kernel<true>, dim3(N, gx_ceil_div(HW, 256)), dim3(256), 0, s, dy, w, gate, Cin,
                               Cout, HW, dx, pb, x, act, ap);
        } else
            hipLaunchKernelGGL(conv1x1_dgrad_kernel<false>, dim3(N, gx_ceil_div(HW, 256)), dim3(256), 0, s, dy, w, gate, Cin,
                               Cout, HW, dx, pb, (const float*)nullptr, 0, (float*)nullptr);
    }
    GX_CHECK_LAUNCH("gx_conv1x1_bwd(dgrad)");
    {
        GxProf pf(KID_CONV1X1_WGRAD, s, 2.0 * N * Cin * Cout * HW, 4.0 * N * HW * (Cin + Cout));
        if (Cin <= 64 && (HW % C1_TP) == 0) {
            static bool attr_set = false;
            const size_t lds = (size_t)(64 + 8) * C1_LS * sizeof(float);
            if (!attr_set) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_wgrad_lds_kernel<false>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                attr_set = true;
            }
            hipLaunchKernelGGL(conv1x1_wgrad_lds_kernel<false>, dim3(nblkw), dim3(256), lds, s, x, dy, N, Cin, Cout,
                               HW, pw, NormIn{nullptr, nullptr, nullptr, nullptr, 1, 1}, (float*)nullptr);
        } else if (Cin <= 64)
            hipLaunchKernelGGL(conv1x1_wgrad_mfma_kernel<4>, dim3(nblkw), dim3(256), 0, s, x, dy, N, Cin, Cout, HW, pw);
        else
            hipLaunchKernelGGL(conv1x1_wgrad_mfma_kernel<8>, dim3(nblkw), dim3(256), 0, s, x, dy, N, Cin, Cout, HW, pw);
    }
    GX_CHECK_LAUNCH("gx_conv1x1_bwd(wgrad)");
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 4.0 * ((double)nblkw * npairs + (double)nblkd * Cout));
        if (!gate) {   // no gate: the column sums ARE dw and db
            hipLaunchKernelGGL(col_sum2_kernel, dim3(npairs + Cout), dim3(256), 0, s, (const float*)pw, nblkw, npairs,
                               dw, (const float*)pb, nblkd, Cout, db, accumulate ? 1 : 0);
        } else {       // dgate = <raw dw, w> + <raw db, bias> needs all sums: second launch
            hipLaunchKernelGGL(col_sum2_kernel, dim3(npairs + Cout), dim3(256), 0, s, (const float*)pw, nblkw, npairs,
                               raw, (const float*)pb, nblkd, Cout, raw + npairs);
            hipLaunchKernelGGL(conv1x1_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)raw, w, bias, gate,
                               Cin, Cout, dw, db, dgate);
        }
    }
    GX_CHECK_LAUNCH("gx_conv1x1_bwd(finalize)");
    if (dbx)
        return gx_chan_sums_launch(dx, N, Cin, HW, (float*)((char*)ws + gx_round_up((long)gx_conv1x1_bwd_ws_bytes(N, Cin, Cout, H, W), 256)),
                                   dbx, s);
    return GX_OK;
}

// ---- 1x1 conv on a GroupNorm+ReLU layer that is never materialised (decoder_module.12-13)
int gx_conv1x1_gn_fwd(const float* y_pre, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, int groups, const float* w, const float* bias, const float* gate,
                      const float* addend, int N, int Cin, int Cout, int H, int W, float* out, gx_stream_t stream) {
    GX_CHECK_ARG(y_pre && mean && rstd && gamma && beta && w && out, "gx_conv1x1_gn_fwd: null pointer");
    GX_CHECK_ARG(N > 0 && Cin > 0 && Cout > 0 && Cout <= COMAX && Cin <= 128 && groups > 0 && Cin % groups == 0,
                 "gx_conv1x1_gn_fwd: Cout <= 8, Cin <= 128, Cin %% groups == 0");
    const int HW = H * W;
    GX_CHECK_ARG((HW % 4) == 0 && ((uintptr_t)y_pre % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                     (!addend || ((uintptr_t)addend % 16) == 0),
                 "gx_conv1x1_gn_fwd: H*W %% 4 == 0 and 16-byte aligned tensors");
    {
        GxProf pf(KID_CONV1X1_FWD, (hipStream_t)stream, 2.0 * N * Cin * Cout * HW, 4.0 * N * HW * (Cin + Cout));
        hipLaunchKernelGGL(conv1x1_fwd_vec_kernel, dim3(N, gx_ceil_div(HW, 1024)), dim3(256), 0, (hipStream_t)stream,
                           y_pre, w, bias, gate, addend, Cin, Cout, HW, out,
                           NormIn{mean, rstd, gamma, beta, groups, Cin / groups});
    }
    GX_CHECK_LAUNCH("gx_conv1x1_gn_fwd");
    return GX_OK;
}

size_t gx_conv1x1_gn_wgrad_ws_bytes(int N, int Cin, int Cout, int H, int W) {
    const size_t nblkw = conv1x1_wgrad_blocks(N, H * W);
    return (nblkw + 1) * ((size_t)Cout * Cin + Cout) * sizeof(float);
}

int gx_conv1x1_gn_wgrad(const float* y_pre, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int groups, const float* g_out, const float* w, const float* bias,
                        const float* gate, int N, int Cin, int Cout, int H, int W, float* dw, float* db,
                        float* dgate, void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(y_pre && mean && rstd && gamma && beta && g_out && dw && ws, "gx_conv1x1_gn_wgrad: null pointer");
    GX_CHECK_ARG((gate == nullptr) == (dgate == nullptr) && (!gate || w),
                 "gx_conv1x1_gn_wgrad: gate, dgate (and w) go together");
    GX_CHECK_ARG(N > 0 && Cin > 0 && Cin <= 64 && Cout > 0 && Cout <= COMAX && groups > 0 && Cin % groups == 0,
                 "gx_conv1x1_gn_wgrad: Cout <= 8, Cin <= 64, Cin %% groups == 0");
    const int HW = H * W;
    GX_CHECK_ARG(HW % C1_TP == 0, "gx_conv1x1_gn_wgrad: H*W must be a multiple of 256");
    GX_CHECK_ARG(ws_bytes >= gx_conv1x1_gn_wgrad_ws_bytes(N, Cin, Cout, H, W), "gx_conv1x1_gn_wgrad: workspace too small");
    const int nblkw = conv1x1_wgrad_blocks(N, HW);
    const int npairs = Cout * Cin;
    float* pw = (float*)ws;
    float* pb = pw + (size_t)nblkw * npairs;
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_CONV1X1_WGRAD, s, 2.0 * N * Cin * Cout * HW, 4.0 * N * HW * (Cin + Cout));
        static bool attr_set = false;
        const size_t lds = (size_t)(64 + 8) * C1_LS * sizeof(float);
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1x1_wgrad_lds_kernel<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            attr_set = true;
        }
        hipLaunchKernelGGL(conv1x1_wgrad_lds_kernel<true>, dim3(nblkw), dim3(256), lds, s, y_pre, g_out, N, Cin, Cout,
                           HW, pw, NormIn{mean, rstd, gamma, beta, groups, Cin / groups}, pb);
    }
    GX_CHECK_LAUNCH("gx_conv1x1_gn_wgrad");
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 4.0 * (double)nblkw * (npairs + Cout));
        if (!gate) {
            hipLaunchKernelGGL(col_sum2_kernel, dim3(npairs + Cout), dim3(256), 0, s, (const float*)pw, nblkw, npairs,
                               dw, (const float*)pb, nblkw, Cout, db);
        } else {
            float* raw = pb + (size_t)nblkw * Cout;
            hipLaunchKernelGGL(col_sum2_kernel, dim3(npairs + Cout), dim3(256), 0, s, (const float*)pw, nblkw, npairs,
                               raw, (const float*)pb, nblkw, Cout, raw + npairs);
            hipLaunchKernelGGL(conv1x1_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)raw, w, bias, gate,
                               Cin, Cout, dw, db, dgate);
        }
    }
    GX_CHECK_LAUNCH("gx_conv1x1_gn_wgrad(reduce)");
    return GX_OK;
}

// Finishes the 1x1 conv's parameter gradients from the per-image partials gx_gn_relu_bwd_proj produced
// (wpart [N][Cout][Cin], bpart [N][Cout]): fixed-order sums over the images, then the gate handling of gx_conv1x1_bwd.
size_t gx_conv1x1_gn_wgrad_finish_ws_bytes(int Cin, int Cout) { return ((size_t)Cout * Cin + Cout) * sizeof(float); }

int gx_conv1x1_gn_wgrad_finish(const float* wpart, const float* bpart, int N, int Cin, int Cout, const float* w,
                               const float* bias, const float* gate, float* dw, float* db, float* dgate, void* ws,
                               size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(wpart && bpart && dw, "gx_conv1x1_gn_wgrad_finish: null pointer");
    GX_CHECK_ARG(N > 0 && Cin > 0 && Cout > 0 && Cout <= COMAX, "gx_conv1x1_gn_wgrad_finish: bad N/Cin/Cout");
    GX_CHECK_ARG((gate == nullptr) == (dgate == nullptr) && (!gate || (w && ws)),
                 "gx_conv1x1_gn_wgrad_finish: gate, dgate (and w, ws) go together");
    GX_CHECK_ARG(!gate || ws_bytes >= gx_conv1x1_gn_wgrad_finish_ws_bytes(Cin, Cout),
                 "gx_conv1x1_gn_wgrad_finish: workspace too small");
    const int npairs = Cout * Cin;
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 4.0 * (double)N * (npairs + Cout));
        if (!gate) {
            hipLaunchKernelGGL(col_sum2_kernel, dim3(npairs + Cout), dim3(256), 0, s, wpart, N, npairs, dw, bpart, N,
                               Cout, db);
        } else {
            float* raw = (float*)ws;
            hipLaunchKernelGGL(col_sum2_kernel, dim3(npairs + Cout), dim3(256), 0, s, wpart, N, npairs, raw, bpart, N,
                               Cout, raw + npairs);
            hipLaunchKernelGGL(conv1x1_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)raw, w, bias, gate,
                               Cin, Cout, dw, db, dgate);
        }
    }
    GX_CHECK_LAUNCH("gx_conv1x1_gn_wgrad_finish");
    return GX_OK;
}

}  // extern "C"
