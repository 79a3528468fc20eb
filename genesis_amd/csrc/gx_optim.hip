// Optimiser-side kernels of the training step: fused flat-buffer Adam and the GECO multiplier update.
//
// Reference: train.py:174-175,262-263 (torch.optim.Adam(lr=1e-4), betas (0.9, 0.999), eps 1e-8, no weight
// decay) and utils/geco.py:35-51.  Both read their step-dependent scalars from device memory so a whole
// training step can be replayed from a HIP graph without host round-trips (the reference's
// `constraint.item()` at geco.py:45 is a device->host sync every iteration).
#include "gx_common.h"
#include "gx_philox.h"

namespace {

// p, g, m, v: flat buffers of n elements.  step: device int64 counter, already incremented for this
// update (t >= 1).  gscale multiplies the gradient first (1/world_size for data-parallel averaging).
template <typename T, bool ZERO_G = false>
__device__ __forceinline__ void adam_body(T* __restrict__ p, T* __restrict__ g, T* __restrict__ m, T* __restrict__ v,
                                          size_t n, const int64_t* __restrict__ step, double lr, double b1, double b2,
                                          double eps, float gscale, unsigned block, unsigned nblocks) {
    // hyper-parameters arrive as doubles and every derived constant is formed in double before it is rounded to T,
    // as torch.optim.Adam does with its Python floats (1 - 0.999 in fp32 is 4.7e-5 off the fp64 value it uses)
    const double t = (double)(*step);
    const double bc1 = 1.0 - pow(b1, t);
    const double bc2 = 1.0 - pow(b2, t);
    const T step_size = (T)(lr / bc1);
    const T bc2_sqrt = (T)sqrt(bc2);
    const T one_m_b1 = (T)(1.0 - b1), one_m_b2 = (T)(1.0 - b2), b2_t = (T)b2, eps_t = (T)eps;
    for (size_t i = (size_t)block * blockDim.x + threadIdx.x; i < n; i += (size_t)nblocks * blockDim.x) {
        // Where a product is fused into a sum is WRITTEN here (fma) and nowhere left to the compiler: left to contract as it
        // pleased, it fused v b2 + (g g)(1 - b2) one way with ZERO_G and the other way without, and the launch the trainer uses
        // (ZERO_G) differed from gx_adam_step in the last bit of the fp64 v (tests/test_step_tail_gpu.py::test_adam_pair).  The
        // forms below are the ones the trainer's launch has always computed; gx_adam_step now computes them too.  The fp32 and
        // the fp64 form differ (and g gscale enters m unrounded but v rounded) for that reason alone: a run continued from a
        // checkpoint, or compared with an earlier one, keeps its bits.  Neither is more accurate than the other.
#pragma clang fp contract(off)
        const T gs = (T)gscale, gr = g[i], mo = m[i];
        const T gi = gr * gs;
        if (ZERO_G) g[i] = (T)0;                                   // the next iteration accumulates into a clean bucket
        const T d = fma(gr, gs, -mo);                              // g gscale - m, the product unrounded
        T mi, vi;
        if constexpr (sizeof(T) == 4) {
            mi = mo + d * one_m_b1;                                // torch: exp_avg.lerp_(grad, 1 - beta1)
            vi = (gi * gi) * one_m_b2 + v[i] * b2_t;               // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
        } else {
            mi = fma(one_m_b1, d, mo);
            vi = fma(one_m_b2, gi * gi, b2_t * v[i]);
        }
        const T denom = sqrt(vi) / bc2_sqrt + eps_t;
        p[i] = fma(-step_size, mi / denom, p[i]);
        m[i] = mi;
        v[i] = vi;
    }
}

template <typename T>
__global__ void __launch_bounds__(256)
adam_kernel(T* __restrict__ p, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, size_t n,
            const int64_t* __restrict__ step, double lr, double b1, double b2, double eps, float gscale) {
    adam_body<T, false>(p, const_cast<T*>(g), m, v, n, step, lr, b1, b2, eps, gscale, blockIdx.x, gridDim.x);
}

// the fp32 and the fp64 parameter groups in one launch (blocks [0, nb32) / [nb32, gridDim.x)), optionally zeroing the
// gradients they consumed: the tail of a training step is this launch and the GECO / step-counter one
struct AdamGroup { void* p; void* g; void* m; void* v; size_t n; };
template <bool ZERO_G>
__global__ void __launch_bounds__(256)
adam_pair_kernel(const AdamGroup a, const AdamGroup b, unsigned nb32, const int64_t* __restrict__ step, double lr,
                 double b1, double b2, double eps, float gscale) {
    if (blockIdx.x < nb32)
        adam_body<float, ZERO_G>((float*)a.p, (float*)a.g, (float*)a.m, (float*)a.v, a.n, step, lr, b1, b2, eps, gscale,
                                 blockIdx.x, nb32);
    else
        adam_body<double, ZERO_G>((double*)b.p, (double*)b.g, (double*)b.m, (double*)b.v, b.n, step, lr, b1, b2, eps,
                                  gscale, blockIdx.x - nb32, gridDim.x - nb32);
}

// Guarded form (gx_adam_step_pair_guarded): gscale is the gradient guard's `scale` (1/world times the clip coefficient) read from
// its device record; a record that is not `ok` (a non-finite gradient, err or kl) leaves p, m and v alone and only zeroes the
// gradients -- the launch and its grid are those of adam_pair_kernel, the body is adam_body itself.
template <typename T>
__device__ __forceinline__ void zero_body(T* __restrict__ g, size_t n, unsigned block, unsigned nblocks) {
    for (size_t i = (size_t)block * blockDim.x + threadIdx.x; i < n; i += (size_t)nblocks * blockDim.x) g[i] = (T)0;
}
template <bool ZERO_G>
__global__ void __launch_bounds__(256)
adam_pair_guarded_kernel(const AdamGroup a, const AdamGroup b, unsigned nb32, const int64_t* __restrict__ step, double lr,
                         double b1, double b2, double eps, const GxGuardRecord* __restrict__ rec) {
    const bool f32 = blockIdx.x < nb32;
    if (!rec->ok) {
        if (ZERO_G) {
            if (f32) zero_body<float>((float*)a.g, a.n, blockIdx.x, nb32);
            else zero_body<double>((double*)b.g, b.n, blockIdx.x - nb32, gridDim.x - nb32);
        }
        return;
    }
    const float gscale = rec->scale;
    if (f32)
        adam_body<float, ZERO_G>((float*)a.p, (float*)a.g, (float*)a.m, (float*)a.v, a.n, step, lr, b1, b2, eps, gscale,
                                 blockIdx.x, nb32);
    else
        adam_body<double, ZERO_G>((double*)b.p, (double*)b.g, (double*)b.m, (double*)b.v, b.n, step, lr, b1, b2, eps,
                                  gscale, blockIdx.x - nb32, gridDim.x - nb32);
}

// torch.optim.RMSprop(lr) defaults (alpha 0.99, eps 1e-8, no momentum, not centred; train.py:171-172) and
// torch.optim.SGD(lr, momentum 0.9) (train.py:175-176): one state buffer `m` (square average / momentum buffer, zero-initialised:
// mu * 0 + g reproduces torch's buf = grad at the first step).  KIND 1 = RMSprop, 2 = SGD with momentum.
template <typename T, int KIND, bool ZERO_G>
__device__ __forceinline__ void simple_opt_body(T* __restrict__ p, T* __restrict__ g, T* __restrict__ m, size_t n, double lr,
                                                double hp, double eps, float gscale, unsigned block, unsigned nblocks) {
    const T lr_t = (T)lr, hp_t = (T)hp, one_m = (T)(1.0 - hp), eps_t = (T)eps;
    for (size_t i = (size_t)block * blockDim.x + threadIdx.x; i < n; i += (size_t)nblocks * blockDim.x) {
        const T gi = g[i] * (T)gscale;
        if (ZERO_G) g[i] = (T)0;
        if (KIND == 1) {
            const T sq = m[i] * hp_t + gi * gi * one_m;            // square_avg.mul_(alpha).addcmul_(g, g, 1 - alpha)
            m[i] = sq;
            p[i] = p[i] - lr_t * (gi / (sqrt(sq) + eps_t));        // p.addcdiv_(g, sqrt(square_avg) + eps, -lr)
        } else {
            const T buf = m[i] * hp_t + gi;                        // buf.mul_(momentum).add_(g)
            m[i] = buf;
            p[i] = p[i] - lr_t * buf;
        }
    }
}
template <int KIND, bool ZERO_G>
__global__ void __launch_bounds__(256)
simple_opt_pair_kernel(const AdamGroup a, const AdamGroup b, unsigned nb32, int64_t* __restrict__ step, double lr, double hp,
                       double eps, float gscale) {
    (void)step;
    if (blockIdx.x < nb32)
        simple_opt_body<float, KIND, ZERO_G>((float*)a.p, (float*)a.g, (float*)a.m, a.n, lr, hp, eps, gscale, blockIdx.x, nb32);
    else
        simple_opt_body<double, KIND, ZERO_G>((double*)b.p, (double*)b.g, (double*)b.m, b.n, lr, hp, eps, gscale,
                                              blockIdx.x - nb32, gridDim.x - nb32);
}

template <int KIND, bool ZERO_G>
__global__ void __launch_bounds__(256)
simple_opt_pair_guarded_kernel(const AdamGroup a, const AdamGroup b, unsigned nb32, double lr, double hp, double eps,
                               const GxGuardRecord* __restrict__ rec) {
    const bool f32 = blockIdx.x < nb32;
    if (!rec->ok) {
        if (ZERO_G) {
            if (f32) zero_body<float>((float*)a.g, a.n, blockIdx.x, nb32);
            else zero_body<double>((double*)b.g, b.n, blockIdx.x - nb32, gridDim.x - nb32);
        }
        return;
    }
    const float gscale = rec->scale;
    if (f32)
        simple_opt_body<float, KIND, ZERO_G>((float*)a.p, (float*)a.g, (float*)a.m, a.n, lr, hp, eps, gscale, blockIdx.x, nb32);
    else
        simple_opt_body<double, KIND, ZERO_G>((double*)b.p, (double*)b.g, (double*)b.m, b.n, lr, hp, eps, gscale,
                                              blockIdx.x - nb32, gridDim.x - nb32);
}

// ---- extended forms (gx_adam_step_pair_ex / gx_optimiser_step_pair_ex): the learning rate from a schedule evaluated on the
//      device from the step counter, an exponential moving average of the parameters, an optional guard record.  The launch and
//      its grid are those of the kernels above and the arithmetic on p, m, v is adam_body / simple_opt_body itself, called with
//      the rate this launch computed.
struct GxSched { int kind; int n_ms; double base, W, s0, T, eta_min, gamma; long long ms[GX_SCHED_MAX_MILESTONES]; const double* lr_dev; };
struct GxEma { float* e32; double* e64; double decay; int warmup; };

// t = *step after the increment (>= 1), k = t - 1.  The closed forms of torch's SequentialLR([LinearLR, X]) at last_epoch = k, in
// fp64, every operation in the order genesis_amd/schedule.py: LRSchedule.value writes it (no contraction).  The cosine is HELD at
// eta_min from j = T on (torch's CosineAnnealingLR is periodic there).
__device__ __forceinline__ double sched_lr(const GxSched& sc, long long t) {
#pragma clang fp contract(off)
    if (sc.kind == GX_SCHED_DEVICE) return *sc.lr_dev;         // the host's own rule: no warm-up factor on top
    const double k = (double)(t - 1);
    if (k < sc.W) return sc.base * (sc.s0 + ((1.0 - sc.s0) * k) / sc.W);
    const double j = k - sc.W;
    switch (sc.kind) {
    case GX_SCHED_COSINE: {
        if (j >= sc.T) return sc.eta_min;
        return sc.eta_min + ((sc.base - sc.eta_min) * (1.0 + cos((M_PI * j) / sc.T))) / 2.0;
    }
    case GX_SCHED_EXPONENTIAL: return sc.base * pow(sc.gamma, j);
    case GX_SCHED_STEP: {
        int c = 0;
        for (int i = 0; i < sc.n_ms; ++i) c += (double)sc.ms[i] <= j ? 1 : 0;
        return sc.base * pow(sc.gamma, (double)c);
    }
    default: return sc.base;
    }
}

__device__ __forceinline__ double ema_decay_at(const GxEma& em, long long t) {
#pragma clang fp contract(off)
    if (!em.warmup) return em.decay;
    const double w = (1.0 + (double)t) / (10.0 + (double)t);   // the num_updates rule of tf.train.ExponentialMovingAverage
    return w < em.decay ? w : em.decay;
}

// e' = e + w (p' - e), every operation rounded in T: p' is what the optimiser body above just stored from this very thread
template <typename T>
__device__ __forceinline__ void ema_body(const T* __restrict__ p, T* __restrict__ e, size_t n, T w, unsigned block,
                                         unsigned nblocks) {
    for (size_t i = (size_t)block * blockDim.x + threadIdx.x; i < n; i += (size_t)nblocks * blockDim.x) {
        // written like adam_body's comment asks: the subtraction and the product-sum are two roundings each, never an fma
#pragma clang fp contract(off)
        const T eo = e[i];
        const T d = p[i] - eo;
        const T wd = w * d;
        e[i] = eo + wd;
    }
}

// what both _ex kernels do before their body: the verdict, the gradient scale, the rate, the EMA weight, the tail record.
// -> false: a skipped step (only the gradients are zeroed by the caller)
__device__ __forceinline__ bool ex_prologue(const GxGuardRecord* __restrict__ rec, const int64_t* __restrict__ step,
                                            const GxSched& sc, const GxEma& em, float& gscale, double& lr, double& decay_t,
                                            double* __restrict__ tail) {
    if (rec) {
        if (!rec->ok) return false;
        gscale = rec->scale;
    }
    const long long t = (long long)*step;
    lr = sched_lr(sc, t);
    decay_t = em.e32 ? ema_decay_at(em, t) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { tail[0] = lr; tail[1] = decay_t; }
    return true;
}

template <bool ZERO_G>
__global__ void __launch_bounds__(256)
adam_pair_ex_kernel(const AdamGroup a, const AdamGroup b, unsigned nb32, const int64_t* __restrict__ step, const GxSched sc,
                    double b1, double b2, double eps, float gscale, const GxGuardRecord* __restrict__ rec, const GxEma em,
                    double* __restrict__ tail) {
    const bool f32 = blockIdx.x < nb32;
    double lr, decay_t;
    if (!ex_prologue(rec, step, sc, em, gscale, lr, decay_t, tail)) {
        if (ZERO_G) {
            if (f32) zero_body<float>((float*)a.g, a.n, blockIdx.x, nb32);
            else zero_body<double>((double*)b.g, b.n, blockIdx.x - nb32, gridDim.x - nb32);
        }
        return;
    }
    if (f32) {
        adam_body<float, ZERO_G>((float*)a.p, (float*)a.g, (float*)a.m, (float*)a.v, a.n, step, lr, b1, b2, eps, gscale,
                                 blockIdx.x, nb32);
        if (em.e32) ema_body<float>((const float*)a.p, em.e32, a.n, (float)(1.0 - decay_t), blockIdx.x, nb32);
    } else {
        adam_body<double, ZERO_G>((double*)b.p, (double*)b.g, (double*)b.m, (double*)b.v, b.n, step, lr, b1, b2, eps,
                                  gscale, blockIdx.x - nb32, gridDim.x - nb32);
        if (em.e32) ema_body<double>((const double*)b.p, em.e64, b.n, 1.0 - decay_t, blockIdx.x - nb32, gridDim.x - nb32);
    }
}

template <int KIND, bool ZERO_G>
__global__ void __launch_bounds__(256)
simple_opt_pair_ex_kernel(const AdamGroup a, const AdamGroup b, unsigned nb32, const int64_t* __restrict__ step, const GxSched sc,
                          double hp, double eps, float gscale, const GxGuardRecord* __restrict__ rec, const GxEma em,
                          double* __restrict__ tail) {
    const bool f32 = blockIdx.x < nb32;
    double lr, decay_t;
    if (!ex_prologue(rec, step, sc, em, gscale, lr, decay_t, tail)) {
        if (ZERO_G) {
            if (f32) zero_body<float>((float*)a.g, a.n, blockIdx.x, nb32);
            else zero_body<double>((double*)b.g, b.n, blockIdx.x - nb32, gridDim.x - nb32);
        }
        return;
    }
    if (f32) {
        simple_opt_body<float, KIND, ZERO_G>((float*)a.p, (float*)a.g, (float*)a.m, a.n, lr, hp, eps, gscale, blockIdx.x, nb32);
        if (em.e32) ema_body<float>((const float*)a.p, em.e32, a.n, (float)(1.0 - decay_t), blockIdx.x, nb32);
    } else {
        simple_opt_body<double, KIND, ZERO_G>((double*)b.p, (double*)b.g, (double*)b.m, b.n, lr, hp, eps, gscale,
                                              blockIdx.x - nb32, gridDim.x - nb32);
        if (em.e32) ema_body<double>((const double*)b.p, em.e64, b.n, 1.0 - decay_t, blockIdx.x - nb32, gridDim.x - nb32);
    }
}

// gx_ema_multi: the same e + w (p - e) over a descriptor table of (p, ema, n, dtype, work offset) segments in chunks of
// GX_EMA_CHUNK elements, a capped grid walking the chunks with its stride (the table convention of gx_grad_guard)
__device__ __forceinline__ int ema_segment(const long long* __restrict__ table, int S, long long w) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * GX_EMA_DESC_WORDS + GX_EMA_D_WORK] <= w) lo = mid; else hi = mid - 1;
    }
    return lo;
}
template <typename T>
__device__ __forceinline__ void ema_chunk(const T* __restrict__ p, T* __restrict__ e, int n, T w) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma clang fp contract(off)
        const T eo = e[i];
        const T d = p[i] - eo;
        const T wd = w * d;
        e[i] = eo + wd;
    }
}
__global__ void __launch_bounds__(256)
ema_multi_kernel(const long long* __restrict__ table, int S, long long work, const int64_t* __restrict__ step, const GxEma em,
                 double* __restrict__ decay_used) {
    const double decay_t = ema_decay_at(em, (long long)*step);
    if (decay_used && blockIdx.x == 0 && threadIdx.x == 0) *decay_used = decay_t;
    const double w = 1.0 - decay_t;
    for (long long c = blockIdx.x; c < work; c += gridDim.x) {
        const long long* d = table + (size_t)ema_segment(table, S, c) * GX_EMA_DESC_WORDS;
        const long long N = d[GX_EMA_D_N], first = (c - d[GX_EMA_D_WORK]) * GX_EMA_CHUNK;
        const int n = (int)(N - first < GX_EMA_CHUNK ? N - first : GX_EMA_CHUNK);
        if (d[GX_EMA_D_DTYPE] == GX_EMA_FP32)
            ema_chunk<float>(reinterpret_cast<const float*>(d[GX_EMA_D_SRC]) + first, reinterpret_cast<float*>(d[GX_EMA_D_DST]) + first,
                             n, (float)w);
        else
            ema_chunk<double>(reinterpret_cast<const double*>(d[GX_EMA_D_SRC]) + first,
                              reinterpret_cast<double*>(d[GX_EMA_D_DST]) + first, n, w);
    }
}

// the host's schedule words (GX_SCHED_*) -> the kernel's descriptor; GX_EINVAL-style checks.  -> 0, or the message is set
int sched_from_words(const char* who, const double* w, const double* lr_dev, GxSched* out) {
    GX_CHECK_ARG(w, "%s: null schedule descriptor", who);
    const double kind = w[GX_SCHED_KIND], base = w[GX_SCHED_BASE], W = w[GX_SCHED_WARMUP], s0 = w[GX_SCHED_START];
    const double T = w[GX_SCHED_T], eta_min = w[GX_SCHED_ETA_MIN], gamma = w[GX_SCHED_GAMMA], nm = w[GX_SCHED_N_MILESTONES];
    GX_CHECK_ARG(kind == GX_SCHED_CONSTANT || kind == GX_SCHED_COSINE || kind == GX_SCHED_EXPONENTIAL || kind == GX_SCHED_STEP ||
                 kind == GX_SCHED_DEVICE, "%s: unknown schedule kind %g", who, kind);
    GX_CHECK_ARG(__builtin_isfinite(base), "%s: the base rate %g is not finite", who, base);
    GX_CHECK_ARG(W >= 0.0 && W < 9007199254740992.0 && W == (double)(long long)W, "%s: warm-up length W = %g is not a whole number >= 0", who, W);
    GX_CHECK_ARG(s0 > 0.0 && s0 <= 1.0, "%s: warm-up start factor s0 = %g outside (0, 1]", who, s0);
    if (kind == GX_SCHED_COSINE) {
        GX_CHECK_ARG(T > 0.0 && T < 9007199254740992.0 && T == (double)(long long)T, "%s: cosine length T = %g is not a whole number > 0", who, T);
        GX_CHECK_ARG(__builtin_isfinite(eta_min), "%s: eta_min %g is not finite", who, eta_min);
    }
    if (kind == GX_SCHED_EXPONENTIAL || kind == GX_SCHED_STEP)
        GX_CHECK_ARG(gamma > 0.0 && __builtin_isfinite(gamma), "%s: gamma = %g is not a positive finite number", who, gamma);
    int n_ms = 0;
    if (kind == GX_SCHED_STEP) {
        GX_CHECK_ARG(nm >= 0.0 && nm <= (double)GX_SCHED_MAX_MILESTONES && nm == (double)(int)nm,
                     "%s: %g milestones, at most %d are held", who, nm, GX_SCHED_MAX_MILESTONES);
        n_ms = (int)nm;
        for (int i = 0; i < n_ms; ++i) {
            const double m = w[GX_SCHED_MILESTONE0 + i];
            GX_CHECK_ARG(m >= 0.0 && m < 9007199254740992.0 && m == (double)(long long)m, "%s: milestone %d = %g is not a whole number >= 0", who, i, m);
            GX_CHECK_ARG(i == 0 || m >= w[GX_SCHED_MILESTONE0 + i - 1], "%s: milestones are not in ascending order (milestone %d = %g)", who, i, m);
        }
    }
    GX_CHECK_ARG(kind != GX_SCHED_DEVICE || (lr_dev && (reinterpret_cast<uintptr_t>(lr_dev) & 7) == 0),
                 "%s: the device schedule needs an 8-byte aligned lr_dev", who);
    GxSched sc{};
    sc.kind = (int)kind; sc.n_ms = n_ms; sc.base = base; sc.W = W; sc.s0 = s0; sc.T = T; sc.eta_min = eta_min; sc.gamma = gamma;
    for (int i = 0; i < n_ms; ++i) sc.ms[i] = (long long)w[GX_SCHED_MILESTONE0 + i];
    sc.lr_dev = lr_dev;
    *out = sc;
    return GX_OK;
}

int ema_check(const char* who, const float* ema32, const double* ema64, size_t n64, double decay, GxEma* out) {
    GX_CHECK_ARG(ema32 || !ema64, "%s: ema64 without ema32", who);
    if (ema32) {
        GX_CHECK_ARG(n64 == 0 || ema64, "%s: null ema64 with an fp64 group of %zu elements", who, n64);
        GX_CHECK_ARG((reinterpret_cast<uintptr_t>(ema32) & 3) == 0 && (reinterpret_cast<uintptr_t>(ema64) & 7) == 0,
                     "%s: an EMA buffer is not aligned to its elements", who);
        GX_CHECK_ARG(decay >= 0.0 && decay < 1.0, "%s: decay = %g outside [0, 1)", who, decay);
    }
    out->e32 = const_cast<float*>(ema32); out->e64 = const_cast<double*>(ema64); out->decay = decay;
    return GX_OK;
}

// beta of the fixed-beta objective with linear warm-up (train.py:252-258): beta * iter / (0.2 * train_iter) clamped to
// [0, beta]; iter = the device step counter BEFORE this iteration's increment
__global__ void beta_warmup_kernel(const int64_t* __restrict__ step, float beta, float warm_iters, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float b = beta * (float)(*step) / warm_iters;
    *out = fminf(fmaxf(b, 0.f), beta);
}

// train.py:244-246: mse_b = mean over (c, h, w) of (x - recon)^2, rmse_b = sqrt(mse_b); out = (mean_b mse_b, mean_b rmse_b).
// One workgroup per image, then the last workgroup to finish (a counter) averages: fixed order, no float atomics.
__global__ void __launch_bounds__(256)
mse_rmse_kernel(const float* __restrict__ x, const float* __restrict__ r, int B, int n, float* __restrict__ per_image,
                unsigned* __restrict__ counter, float* __restrict__ out) {
    __shared__ double red[4];
    __shared__ bool last;
    const int b = blockIdx.x;
    const float* xb = x + (size_t)b * n;
    const float* rb = r + (size_t)b * n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { const float d = xb[i] - rb[i]; s += (double)d * d; }
    s = gx_wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        per_image[b] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / n);
        __threadfence();
        last = atomicAdd(counter, 1u) == (unsigned)(B - 1);
    }
    __syncthreads();
    if (last && threadIdx.x == 0) {
        __threadfence();
        double m = 0.0, rm = 0.0;
        for (int i = 0; i < B; ++i) { const float v = __builtin_nontemporal_load(per_image + i); m += v; rm += sqrtf(v); }
        out[0] = (float)(m / B); out[1] = (float)(rm / B);
        *counter = 0u;                                     // ready for the next launch (graph replay)
    }
}

// ---- the step's noise in one launch: counter-based (Philox4x32-10), keyed by (seed, the device-side step counter): a
//      replayed HIP graph draws fresh numbers every step without the framework's graph-RNG bookkeeping (two offset fills
//      and one launch per tensor).  Element i of tensor t: counter (i / 4, t, step) -> four 32-bit words.
__global__ void __launch_bounds__(256)
philox_noise_kernel(float* __restrict__ u, long long nu, float* __restrict__ z, long long nz, unsigned long long seed,
                    const long long* __restrict__ step) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // one Philox call = 4 outputs
    const long long qu = (nu + 3) >> 2, qz = (nz + 3) >> 2;
    if (q >= qu + qz) return;
    const unsigned long long st = step ? (unsigned long long)*step : 0ull;
    const bool normal = q >= qu;
    const long long i4 = normal ? q - qu : q;
    unsigned w[4];
    philox4x32_10((unsigned)i4, (unsigned)(i4 >> 32) ^ (normal ? 0x80000000u : 0u), (unsigned)st, (unsigned)(st >> 32),
                  (unsigned)seed, (unsigned)(seed >> 32), w);
    float v[4];
    if (!normal) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)(w[e] >> 8) * 5.9604644775390625e-8f;              // [0, 1): 24 bits
    } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) {                                                               // Box-Muller, two pairs
            const float u1 = ((float)(w[2 * e] >> 8) + 1.f) * 5.9604644775390625e-8f;                // (0, 1]
            const float th = (float)(w[2 * e + 1] >> 8) * (6.283185307179586f * 5.9604644775390625e-8f);
            const float r = sqrtf(-2.f * logf(u1));
            v[2 * e] = r * cosf(th); v[2 * e + 1] = r * sinf(th);
        }
    }
    float* dst = normal ? z : u;
    const long long n = normal ? nz : nu;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * i4 + e < n) dst[4 * i4 + e] = v[e];
}

__global__ void step_inc_kernel(int64_t* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1;
}
// guarded: a record that is not `ok` keeps the counter and counts one skipped step instead
__global__ void step_inc_guarded_kernel(int64_t* step, GxGuardRecord* __restrict__ rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (rec->ok) *step += 1; else rec->skipped += 1;
}

// state = {beta, err_ema, initialised (0/1)}.  err: device scalar (batch-mean reconstruction error of
// THIS step, already averaged over ranks).  utils/geco.py:39-49.
__device__ __forceinline__ void geco_body(float* __restrict__ state, const float* __restrict__ err, float goal,
                                          float step_size, float alpha, float speedup, int use_speedup,
                                          float beta_min, float beta_max, int64_t* __restrict__ step) {
    if (step) *step += 1;          // the optimiser's step counter rides along (gx_geco_update_step)
    const float e = *err;
    float ema = state[1];
    if (state[2] == 0.f) { ema = e; state[2] = 1.f; }
    else ema = (1.0f - alpha) * e + alpha * ema;
    const float constraint = goal - ema;
    float factor;
    if (use_speedup && constraint > 0.f) factor = expf(speedup * step_size * constraint);
    else factor = expf(step_size * constraint);
    float beta = factor * state[0];
    beta = fminf(fmaxf(beta, beta_min), beta_max);
    state[0] = beta;
    state[1] = ema;
}
__global__ void geco_update_kernel(float* __restrict__ state, const float* __restrict__ err, float goal,
                                   float step_size, float alpha, float speedup, int use_speedup,
                                   float beta_min, float beta_max, int64_t* __restrict__ step) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    geco_body(state, err, goal, step_size, alpha, speedup, use_speedup, beta_min, beta_max, step);
}
// guarded (gx_geco_update_step_guarded): a record that is not `ok` keeps the state and the counter and counts one skipped step
__global__ void geco_update_guarded_kernel(float* __restrict__ state, const float* __restrict__ err, float goal,
                                           float step_size, float alpha, float speedup, int use_speedup, float beta_min,
                                           float beta_max, int64_t* __restrict__ step, GxGuardRecord* __restrict__ rec) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!rec->ok) { rec->skipped += 1; return; }
    geco_body(state, err, goal, step_size, alpha, speedup, use_speedup, beta_min, beta_max, step);
}

}  // namespace

extern "C" {

int gx_adam_step(void* p, const void* g, void* m, void* v, size_t n, int is_f64, int64_t* step, double lr,
                 double beta1, double beta2, double eps, float grad_scale, gx_stream_t stream) {
    GX_CHECK_ARG(p && g && m && v && step, "gx_adam_step: null pointer");
    if (n == 0) return GX_OK;
    hipStream_t s = (hipStream_t)stream;
    size_t blocks = (n + 1023) / 1024;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    {
        GxProf pf(KID_ADAM, s, 0.0, (is_f64 ? 8.0 : 4.0) * 7.0 * (double)n);  // read p,g,m,v; write p,m,v
        if (is_f64)
            hipLaunchKernelGGL(adam_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, s, (double*)p,
                               (const double*)g, (double*)m, (double*)v, n, (const int64_t*)step, lr, beta1, beta2,
                               eps, grad_scale);
        else
            hipLaunchKernelGGL(adam_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (float*)p,
                               (const float*)g, (float*)m, (float*)v, n, (const int64_t*)step, lr, beta1, beta2, eps,
                               grad_scale);
    }
    GX_CHECK_LAUNCH("gx_adam_step");
    return GX_OK;
}

/* nu uniform [0, 1) numbers into u and nz standard-normal numbers into z (either may be empty), a function of (seed, *step,
 * position) only: torch.rand / torch.randn of a training step (modules/attention.py:177-178 rand_pixel,
 * models/genesisv2_config.py:157 rsample) in one graph-replayable launch; step may be NULL (= 0). */
int gx_philox_noise(float* u, long long nu, float* z, long long nz, unsigned long long seed, const int64_t* step,
                    gx_stream_t stream) {
    GX_CHECK_ARG(nu >= 0 && nz >= 0 && (nu == 0 || u) && (nz == 0 || z), "gx_philox_noise: bad arguments");
    const long long calls = ((nu + 3) >> 2) + ((nz + 3) >> 2);
    if (calls == 0) return GX_OK;
    hipLaunchKernelGGL(philox_noise_kernel, dim3((unsigned)((calls + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, nu, z, nz,
                       seed, (const long long*)step);
    GX_CHECK_LAUNCH("gx_philox_noise");
    return GX_OK;
}

int gx_step_increment(int64_t* step, gx_stream_t stream) {
    GX_CHECK_ARG(step, "gx_step_increment: null pointer");
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step);
    GX_CHECK_LAUNCH("gx_step_increment");
    return GX_OK;
}

int gx_geco_update(float* state, const float* err, float goal, float step_size, float alpha, float speedup,
                   int use_speedup, float beta_min, float beta_max, gx_stream_t stream) {
    GX_CHECK_ARG(state && err, "gx_geco_update: null pointer");
    {
        GxProf pf(KID_GECO, (hipStream_t)stream, 0.0, 16.0);
        hipLaunchKernelGGL(geco_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, err, goal, step_size,
                           alpha, speedup, use_speedup, beta_min, beta_max, (int64_t*)nullptr);
    }
    GX_CHECK_LAUNCH("gx_geco_update");
    return GX_OK;
}

/* gx_geco_update + gx_step_increment in one launch */
int gx_geco_update_step(float* state, const float* err, float goal, float step_size, float alpha, float speedup,
                        int use_speedup, float beta_min, float beta_max, int64_t* step, gx_stream_t stream) {
    GX_CHECK_ARG(state && err && step, "gx_geco_update_step: null pointer");
    {
        GxProf pf(KID_GECO, (hipStream_t)stream, 0.0, 24.0);
        hipLaunchKernelGGL(geco_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, err, goal, step_size,
                           alpha, speedup, use_speedup, beta_min, beta_max, step);
    }
    GX_CHECK_LAUNCH("gx_geco_update_step");
    return GX_OK;
}

/* The other optimisers of train.py:170-176 on the same flat buffers: kind 1 = torch.optim.RMSprop(lr) (alpha 0.99, eps 1e-8),
 * kind 2 = torch.optim.SGD(lr, momentum 0.9); m = their one state buffer (square average / momentum buffer). */
int gx_optimiser_step_pair(int kind, float* p32, float* g32, float* m32, size_t n32, double* p64, double* g64, double* m64,
                           size_t n64, int64_t* step, double lr, double hp, double eps, float grad_scale, int zero_grads,
                           gx_stream_t stream) {
    GX_CHECK_ARG(kind == 1 || kind == 2, "gx_optimiser_step_pair: kind must be 1 (RMSprop) or 2 (SGD with momentum)");
    GX_CHECK_ARG(p32 && g32 && m32 && n32 > 0, "gx_optimiser_step_pair: null pointer / empty fp32 group");
    GX_CHECK_ARG(n64 == 0 || (p64 && g64 && m64), "gx_optimiser_step_pair: null fp64 pointer");
    hipStream_t s = (hipStream_t)stream;
    size_t nb32 = (n32 + 1023) / 1024, nb64 = n64 ? (n64 + 1023) / 1024 : 0;
    if (nb32 > 2048) nb32 = 2048;
    if (nb64 > 256) nb64 = 256;
    const AdamGroup a{p32, g32, m32, nullptr, n32}, b{p64, g64, m64, nullptr, n64};
    const dim3 grid((unsigned)(nb32 + nb64));
    {
        GxProf pf(KID_ADAM, s, 0.0, 4.0 * 5.0 * (double)n32 + 8.0 * 5.0 * (double)n64);
#define GX_OPT(K, Z) hipLaunchKernelGGL((simple_opt_pair_kernel<K, Z>), grid, dim3(256), 0, s, a, b, (unsigned)nb32, step, lr, hp, eps, grad_scale)
        if (kind == 1) { if (zero_grads) GX_OPT(1, true); else GX_OPT(1, false); }
        else { if (zero_grads) GX_OPT(2, true); else GX_OPT(2, false); }
#undef GX_OPT
    }
    GX_CHECK_LAUNCH("gx_optimiser_step_pair");
    return GX_OK;
}

int gx_beta_warmup(const int64_t* step, float beta, float warm_iters, float* out, gx_stream_t stream) {
    GX_CHECK_ARG(step && out && warm_iters > 0.f, "gx_beta_warmup: bad arguments");
    hipLaunchKernelGGL(beta_warmup_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, beta, warm_iters, out);
    GX_CHECK_LAUNCH("gx_beta_warmup");
    return GX_OK;
}

size_t gx_mse_rmse_ws_bytes(int B) { return ((size_t)B + 4) * sizeof(float); }
int gx_mse_rmse(const float* x, const float* recon, int B, int n, float* out, void* ws, size_t ws_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(x && recon && out && ws && B > 0 && n > 0, "gx_mse_rmse: bad arguments");
    GX_CHECK_ARG(ws_bytes >= gx_mse_rmse_ws_bytes(B), "gx_mse_rmse: workspace too small");
    unsigned* counter = (unsigned*)ws;                 // must be zero before the FIRST launch (the kernel re-zeroes it)
    float* per_image = (float*)ws + 4;
    {
        GxProf pf(KID_SMALL_REDUCE, (hipStream_t)stream, 0.0, 8.0 * (double)B * n);
        hipLaunchKernelGGL(mse_rmse_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, recon, B, n, per_image, counter, out);
    }
    GX_CHECK_LAUNCH("gx_mse_rmse");
    return GX_OK;
}

/* gx_adam_step on an fp32 group and an fp64 group (n64 may be 0) in one launch; zero_grads != 0: the gradients are
 * zeroed as they are consumed (replaces the bucket's zero-fill launch at the start of the next iteration) */
int gx_adam_step_pair(float* p32, float* g32, float* m32, float* v32, size_t n32, double* p64, double* g64,
                      double* m64, double* v64, size_t n64, int64_t* step, double lr, double beta1, double beta2,
                      double eps, float grad_scale, int zero_grads, gx_stream_t stream) {
    GX_CHECK_ARG(p32 && g32 && m32 && v32 && step && n32 > 0, "gx_adam_step_pair: null pointer / empty fp32 group");
    GX_CHECK_ARG(n64 == 0 || (p64 && g64 && m64 && v64), "gx_adam_step_pair: null fp64 pointer");
    hipStream_t s = (hipStream_t)stream;
    size_t nb32 = (n32 + 1023) / 1024, nb64 = n64 ? (n64 + 1023) / 1024 : 0;
    if (nb32 > 2048) nb32 = 2048;
    if (nb64 > 256) nb64 = 256;
    const AdamGroup a{p32, g32, m32, v32, n32}, b{p64, g64, m64, v64, n64};
    {
        GxProf pf(KID_ADAM, s, 0.0, 4.0 * 7.0 * (double)n32 + 8.0 * 7.0 * (double)n64);
        if (zero_grads)
            hipLaunchKernelGGL(adam_pair_kernel<true>, dim3((unsigned)(nb32 + nb64)), dim3(256), 0, s, a, b, (unsigned)nb32,
                               (const int64_t*)step, lr, beta1, beta2, eps, grad_scale);
        else
            hipLaunchKernelGGL(adam_pair_kernel<false>, dim3((unsigned)(nb32 + nb64)), dim3(256), 0, s, a, b, (unsigned)nb32,
                               (const int64_t*)step, lr, beta1, beta2, eps, grad_scale);
    }
    GX_CHECK_LAUNCH("gx_adam_step_pair");
    return GX_OK;
}

/* ---- the guarded tail: the same launches with the gradient guard's device record (gx_grad_guard) in place of the host's
 *      grad_scale.  ok: exactly what the unguarded entry point does when its grad_scale is the record's `scale`; not ok: parameters,
 *      optimiser state, step counter and GECO state keep their bits, the gradients are still zeroed with zero_grads, and the
 *      GECO / step-counter launch adds 1 to the record's `skipped`. */
#define GX_CHECK_RECORD(name) \
    GX_CHECK_ARG(record && (reinterpret_cast<uintptr_t>(record) & 7) == 0, name ": null or misaligned guard record")

int gx_step_increment_guarded(int64_t* step, void* record, gx_stream_t stream) {
    GX_CHECK_ARG(step, "gx_step_increment_guarded: null pointer");
    GX_CHECK_RECORD("gx_step_increment_guarded");
    hipLaunchKernelGGL(step_inc_guarded_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, (GxGuardRecord*)record);
    GX_CHECK_LAUNCH("gx_step_increment_guarded");
    return GX_OK;
}

int gx_geco_update_step_guarded(float* state, const float* err, float goal, float step_size, float alpha, float speedup,
                                int use_speedup, float beta_min, float beta_max, int64_t* step, void* record,
                                gx_stream_t stream) {
    GX_CHECK_ARG(state && err && step, "gx_geco_update_step_guarded: null pointer");
    GX_CHECK_RECORD("gx_geco_update_step_guarded");
    {
        GxProf pf(KID_GECO, (hipStream_t)stream, 0.0, 24.0);
        hipLaunchKernelGGL(geco_update_guarded_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, err, goal, step_size,
                           alpha, speedup, use_speedup, beta_min, beta_max, step, (GxGuardRecord*)record);
    }
    GX_CHECK_LAUNCH("gx_geco_update_step_guarded");
    return GX_OK;
}

int gx_adam_step_pair_guarded(float* p32, float* g32, float* m32, float* v32, size_t n32, double* p64, double* g64,
                              double* m64, double* v64, size_t n64, int64_t* step, double lr, double beta1, double beta2,
                              double eps, const void* record, int zero_grads, gx_stream_t stream) {
    GX_CHECK_ARG(p32 && g32 && m32 && v32 && step && n32 > 0, "gx_adam_step_pair_guarded: null pointer / empty fp32 group");
    GX_CHECK_ARG(n64 == 0 || (p64 && g64 && m64 && v64), "gx_adam_step_pair_guarded: null fp64 pointer");
    GX_CHECK_RECORD("gx_adam_step_pair_guarded");
    hipStream_t s = (hipStream_t)stream;
    size_t nb32 = (n32 + 1023) / 1024, nb64 = n64 ? (n64 + 1023) / 1024 : 0;
    if (nb32 > 2048) nb32 = 2048;
    if (nb64 > 256) nb64 = 256;
    const AdamGroup a{p32, g32, m32, v32, n32}, b{p64, g64, m64, v64, n64};
    const GxGuardRecord* rec = (const GxGuardRecord*)record;
    {
        GxProf pf(KID_ADAM, s, 0.0, 4.0 * 7.0 * (double)n32 + 8.0 * 7.0 * (double)n64);
        if (zero_grads)
            hipLaunchKernelGGL(adam_pair_guarded_kernel<true>, dim3((unsigned)(nb32 + nb64)), dim3(256), 0, s, a, b, (unsigned)nb32,
                               (const int64_t*)step, lr, beta1, beta2, eps, rec);
        else
            hipLaunchKernelGGL(adam_pair_guarded_kernel<false>, dim3((unsigned)(nb32 + nb64)), dim3(256), 0, s, a, b, (unsigned)nb32,
                               (const int64_t*)step, lr, beta1, beta2, eps, rec);
    }
    GX_CHECK_LAUNCH("gx_adam_step_pair_guarded");
    return GX_OK;
}

int gx_optimiser_step_pair_guarded(int kind, float* p32, float* g32, float* m32, size_t n32, double* p64, double* g64,
                                   double* m64, size_t n64, int64_t* step, double lr, double hp, double eps, const void* record,
                                   int zero_grads, gx_stream_t stream) {
    (void)step;
    GX_CHECK_ARG(kind == 1 || kind == 2, "gx_optimiser_step_pair_guarded: kind must be 1 (RMSprop) or 2 (SGD with momentum)");
    GX_CHECK_ARG(p32 && g32 && m32 && n32 > 0, "gx_optimiser_step_pair_guarded: null pointer / empty fp32 group");
    GX_CHECK_ARG(n64 == 0 || (p64 && g64 && m64), "gx_optimiser_step_pair_guarded: null fp64 pointer");
    GX_CHECK_RECORD("gx_optimiser_step_pair_guarded");
    hipStream_t s = (hipStream_t)stream;
    size_t nb32 = (n32 + 1023) / 1024, nb64 = n64 ? (n64 + 1023) / 1024 : 0;
    if (nb32 > 2048) nb32 = 2048;
    if (nb64 > 256) nb64 = 256;
    const AdamGroup a{p32, g32, m32, nullptr, n32}, b{p64, g64, m64, nullptr, n64};
    const dim3 grid((unsigned)(nb32 + nb64));
    const GxGuardRecord* rec = (const GxGuardRecord*)record;
    {
        GxProf pf(KID_ADAM, s, 0.0, 4.0 * 5.0 * (double)n32 + 8.0 * 5.0 * (double)n64);
#define GX_OPT(K, Z) hipLaunchKernelGGL((simple_opt_pair_guarded_kernel<K, Z>), grid, dim3(256), 0, s, a, b, (unsigned)nb32, lr, hp, eps, rec)
        if (kind == 1) { if (zero_grads) GX_OPT(1, true); else GX_OPT(1, false); }
        else { if (zero_grads) GX_OPT(2, true); else GX_OPT(2, false); }
#undef GX_OPT
    }
    GX_CHECK_LAUNCH("gx_optimiser_step_pair_guarded");
    return GX_OK;
}
#undef GX_CHECK_RECORD

/* ---- the extended tail (include/genesis_hip.h): schedule, EMA, optional guard record, tail record -- still one launch */
#define GX_CHECK_EX(name)                                                                                                       \
    GX_CHECK_ARG((reinterpret_cast<uintptr_t>(record) & 7) == 0, name ": misaligned guard record");                            \
    GX_CHECK_ARG(tail && (reinterpret_cast<uintptr_t>(tail) & 7) == 0, name ": null or misaligned tail record");               \
    GxSched sc;                                                                                                                 \
    GxEma em{};                                                                                                                 \
    if (int rc = sched_from_words(name, sched, lr_dev, &sc)) return rc;                                                         \
    if (int rc = ema_check(name, ema32, ema64, n64, ema_decay, &em)) return rc;                                                 \
    em.warmup = ema_warmup != 0

int gx_adam_step_pair_ex(float* p32, float* g32, float* m32, float* v32, size_t n32, double* p64, double* g64, double* m64,
                         double* v64, size_t n64, int64_t* step, const double* sched, const double* lr_dev, double beta1,
                         double beta2, double eps, float grad_scale, const void* record, float* ema32, double* ema64,
                         double ema_decay, int ema_warmup, double* tail, int zero_grads, gx_stream_t stream) {
    GX_CHECK_ARG(p32 && g32 && m32 && v32 && step && n32 > 0, "gx_adam_step_pair_ex: null pointer / empty fp32 group");
    GX_CHECK_ARG(n64 == 0 || (p64 && g64 && m64 && v64), "gx_adam_step_pair_ex: null fp64 pointer");
    GX_CHECK_EX("gx_adam_step_pair_ex");
    hipStream_t s = (hipStream_t)stream;
    size_t nb32 = (n32 + 1023) / 1024, nb64 = n64 ? (n64 + 1023) / 1024 : 0;
    if (nb32 > 2048) nb32 = 2048;
    if (nb64 > 256) nb64 = 256;
    const AdamGroup a{p32, g32, m32, v32, n32}, b{p64, g64, m64, v64, n64};
    const GxGuardRecord* rec = (const GxGuardRecord*)record;
    const double per = em.e32 ? 10.0 : 8.0;                 // read p,g,m,v; write p,m,v,g [; re-read p, read and write the EMA]
    {
        GxProf pf(KID_ADAM, s, 0.0, 4.0 * per * (double)n32 + 8.0 * per * (double)n64);
        if (zero_grads)
            hipLaunchKernelGGL(adam_pair_ex_kernel<true>, dim3((unsigned)(nb32 + nb64)), dim3(256), 0, s, a, b, (unsigned)nb32,
                               (const int64_t*)step, sc, beta1, beta2, eps, grad_scale, rec, em, tail);
        else
            hipLaunchKernelGGL(adam_pair_ex_kernel<false>, dim3((unsigned)(nb32 + nb64)), dim3(256), 0, s, a, b, (unsigned)nb32,
                               (const int64_t*)step, sc, beta1, beta2, eps, grad_scale, rec, em, tail);
    }
    GX_CHECK_LAUNCH("gx_adam_step_pair_ex");
    return GX_OK;
}

int gx_optimiser_step_pair_ex(int kind, float* p32, float* g32, float* m32, size_t n32, double* p64, double* g64, double* m64,
                              size_t n64, int64_t* step, const double* sched, const double* lr_dev, double hp, double eps,
                              float grad_scale, const void* record, float* ema32, double* ema64, double ema_decay,
                              int ema_warmup, double* tail, int zero_grads, gx_stream_t stream) {
    GX_CHECK_ARG(kind == 1 || kind == 2, "gx_optimiser_step_pair_ex: kind must be 1 (RMSprop) or 2 (SGD with momentum)");
    GX_CHECK_ARG(p32 && g32 && m32 && step && n32 > 0, "gx_optimiser_step_pair_ex: null pointer / empty fp32 group");
    GX_CHECK_ARG(n64 == 0 || (p64 && g64 && m64), "gx_optimiser_step_pair_ex: null fp64 pointer");
    GX_CHECK_EX("gx_optimiser_step_pair_ex");
    hipStream_t s = (hipStream_t)stream;
    size_t nb32 = (n32 + 1023) / 1024, nb64 = n64 ? (n64 + 1023) / 1024 : 0;
    if (nb32 > 2048) nb32 = 2048;
    if (nb64 > 256) nb64 = 256;
    const AdamGroup a{p32, g32, m32, nullptr, n32}, b{p64, g64, m64, nullptr, n64};
    const dim3 grid((unsigned)(nb32 + nb64));
    const GxGuardRecord* rec = (const GxGuardRecord*)record;
    const double per = em.e32 ? 8.0 : 6.0;
    {
        GxProf pf(KID_ADAM, s, 0.0, 4.0 * per * (double)n32 + 8.0 * per * (double)n64);
#define GX_OPT(K, Z) hipLaunchKernelGGL((simple_opt_pair_ex_kernel<K, Z>), grid, dim3(256), 0, s, a, b, (unsigned)nb32, \
                                        (const int64_t*)step, sc, hp, eps, grad_scale, rec, em, tail)
        if (kind == 1) { if (zero_grads) GX_OPT(1, true); else GX_OPT(1, false); }
        else { if (zero_grads) GX_OPT(2, true); else GX_OPT(2, false); }
#undef GX_OPT
    }
    GX_CHECK_LAUNCH("gx_optimiser_step_pair_ex");
    return GX_OK;
}
#undef GX_CHECK_EX

int gx_ema_multi(const long long* table_host, const long long* table_dev, long long table_words, int n_segments,
                 const int64_t* step, double decay, int warmup, double* decay_used, gx_stream_t stream) {
    const char* who = "gx_ema_multi";
    GX_CHECK_ARG(table_host && table_dev, "%s: null descriptor table", who);
    GX_CHECK_ARG(n_segments >= 1, "%s: n_segments = %d below 1", who, n_segments);
    GX_CHECK_ARG(table_words >= (long long)n_segments * GX_EMA_DESC_WORDS, "%s: %d segments do not fit a table of %lld words", who,
                 n_segments, table_words);
    GX_CHECK_ARG((reinterpret_cast<uintptr_t>(table_dev) & 7) == 0, "%s: the device table must be 8-byte aligned", who);
    GX_CHECK_ARG(step && (reinterpret_cast<uintptr_t>(step) & 7) == 0, "%s: null or misaligned step counter", who);
    GX_CHECK_ARG((reinterpret_cast<uintptr_t>(decay_used) & 7) == 0, "%s: misaligned decay_used", who);
    GX_CHECK_ARG(decay >= 0.0 && decay < 1.0, "%s: decay = %g outside [0, 1)", who, decay);
    long long work = 0;
    double bytes = 0.0;
    for (int si = 0; si < n_segments; ++si) {
        const long long* d = table_host + (size_t)si * GX_EMA_DESC_WORDS;
        const long long N = d[GX_EMA_D_N], dtype = d[GX_EMA_D_DTYPE];
        const uintptr_t src = (uintptr_t)d[GX_EMA_D_SRC], dst = (uintptr_t)d[GX_EMA_D_DST];
        GX_CHECK_ARG(dtype == GX_EMA_FP32 || dtype == GX_EMA_FP64, "%s: segment %d: unknown dtype %lld", who, si, dtype);
        GX_CHECK_ARG(N >= 1 && N < (1LL << 31), "%s: segment %d: N = %lld outside [1, 2^31)", who, si, N);
        GX_CHECK_ARG(src && dst, "%s: segment %d: null source or destination", who, si);
        GX_CHECK_ARG(((src | dst) & (dtype == GX_EMA_FP32 ? 3 : 7)) == 0, "%s: segment %d: source %#llx or destination %#llx is not aligned to its %d-byte elements",
                     who, si, (unsigned long long)src, (unsigned long long)dst, dtype == GX_EMA_FP32 ? 4 : 8);
        GX_CHECK_ARG(d[GX_EMA_D_WORK] == work, "%s: segment %d: WORK = %lld, the prefix is %lld", who, si, d[GX_EMA_D_WORK], work);
        work += (N + GX_EMA_CHUNK - 1) / GX_EMA_CHUNK;
        bytes += (double)N * (dtype == GX_EMA_FP32 ? 4 : 8);
    }
    GX_CHECK_ARG(work < (1LL << 31), "%s: %lld chunks are too many for one launch", who, work);
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)(work < GX_EMA_MAX_GRID ? work : GX_EMA_MAX_GRID);
    GxEma em{nullptr, nullptr, decay, warmup != 0};
    {
        GxProf pf(KID_ADAM, s, 0.0, 3.0 * bytes);
        hipLaunchKernelGGL(ema_multi_kernel, dim3(grid), dim3(256), 0, s, table_dev, n_segments, work, step, em, decay_used);
    }
    GX_CHECK_LAUNCH("gx_ema_multi");
    return GX_OK;
}

}  // extern "C"
