// TensorBoard image grids on the device (train.py:423-476 visualise_outputs; contract: include/genesis_hip.h, gx_vis_compose).
// The reference makes every grid with torchvision's make_grid after exp / cat / argmax launches of its own and a Python loop
// over the labels for the colours, and hands each to the writer with a transfer and a sync.  Here ONE launch writes every grid
// of a forward pass -- padding included -- into one atlas that goes to the host in one copy.  The kernel is a gather / scatter
// with no reuse: no LDS, no atomics but the overflow counter; a thread finds its grid by bisecting the descriptors' work
// prefix.  Work items of a grid: first its source vectors (or elements), then -- for the descriptor that owns the padding -- one
// per grid pixel, of which those outside the image cells write the pad value and the others leave at once.
#include "gx_common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct VisGrid {      // a descriptor, decoded
    const long long* d;
    int kind, n, C, H, W, K, mode, cell0, n_geom;
    int p, xmaps, ymaps, Hg, Wg;      // the geometry make_grid derives
    float pad_value;
    long long dst;
};

__device__ __forceinline__ VisGrid vis_decode(const long long* __restrict__ d) {
    VisGrid g;
    g.d = d;
    g.kind = (int)d[GX_VIS_D_KIND]; g.n = (int)d[GX_VIS_D_N]; g.C = (int)d[GX_VIS_D_C];
    g.H = (int)d[GX_VIS_D_H]; g.W = (int)d[GX_VIS_D_W]; g.K = (int)d[GX_VIS_D_K];
    g.mode = (int)d[GX_VIS_D_MODE]; g.cell0 = (int)d[GX_VIS_D_CELL0]; g.n_geom = (int)d[GX_VIS_D_N_GEOM];
    const int nrow = (int)d[GX_VIS_D_NROW];
    g.p = g.n_geom == 1 ? 0 : (int)d[GX_VIS_D_PADDING];
    g.xmaps = nrow < g.n_geom ? nrow : g.n_geom;
    g.ymaps = (g.n_geom + g.xmaps - 1) / g.xmaps;
    g.Hg = g.ymaps * (g.H + g.p) + g.p;
    g.Wg = g.xmaps * (g.W + g.p) + g.p;
    g.pad_value = __int_as_float((int)(unsigned)(d[GX_VIS_D_PAD_VALUE] & 0xffffffffLL));
    g.dst = d[GX_VIS_D_DST];
    return g;
}

__device__ __forceinline__ unsigned char vis_u8(float v) {      // rint(clamp(v, 0, 1) 255), half to even; a NaN gives 0
    return (unsigned char)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
}

template <int J> __device__ __forceinline__ void vis_load(const float* __restrict__ p, float (&v)[J]);
template <> __device__ __forceinline__ void vis_load<1>(const float* __restrict__ p, float (&v)[1]) { v[0] = p[0]; }
template <> __device__ __forceinline__ void vis_load<4>(const float* __restrict__ p, float (&v)[4]) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
}

// torch.argmax's order (gx_metrics.hip: seg_take)
__device__ __forceinline__ void vis_take(float v, int k, float& best, int& bi) {
    if (best == best && (v > best || v != v)) { best = v; bi = k; }
}

// palette colour of a label into v[.][j]; -> 1 if the label lies beyond the palette
__device__ __forceinline__ unsigned vis_colour(long long label, const unsigned char* __restrict__ palette, int P, float& r,
                                               float& g, float& b) {
    r = g = b = 0.f;
    if (label < 0) return 0;
    if (label >= P) return 1;
    r = (float)palette[3 * label]; g = (float)palette[3 * label + 1]; b = (float)palette[3 * label + 2];
    return 0;
}

// J pixels o[j] (pixel index inside the grid) of three channels -> the atlas
template <int J>
__device__ __forceinline__ void vis_store(const VisGrid& g, float* __restrict__ atlas, const int (&o)[J], const float (&v)[3][J],
                                          bool bytes) {
    if (g.mode == GX_VIS_U8_HWC) {
        unsigned char* out = reinterpret_cast<unsigned char*>(atlas + g.dst);
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(size_t)o[j] * 3 + c] = bytes ? (unsigned char)v[c][j] : vis_u8(v[c][j]);
        return;
    }
    const long long plane = (long long)g.Hg * g.Wg;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* out = atlas + g.dst + c * plane;
        if (J == 1) {
            out[o[0]] = v[c][0];
        } else {
#pragma unroll
            for (int j = 0; j + 1 < J; j += 2) {
                // two neighbours of one row on an 8-byte boundary (the atlas itself is 16-byte aligned): one store
                if (o[j + 1] == o[j] + 1 && ((g.dst + c * plane + o[j]) & 1) == 0) {
                    f32x2 q; q[0] = v[c][j]; q[1] = v[c][j + 1];
                    *reinterpret_cast<f32x2*>(out + o[j]) = q;
                } else {
                    out[o[j]] = v[c][j];
                    out[o[j + 1]] = v[c][j + 1];
                }
            }
        }
    }
}

// source item `it` of grid g: J consecutive pixels of one image
template <int J>
__device__ __forceinline__ void vis_source(const VisGrid& g, long long it, const long long* __restrict__ table,
                                           const unsigned char* __restrict__ palette, int P, float* __restrict__ atlas,
                                           unsigned* __restrict__ counter) {
    const int HW = g.H * g.W, per_image = HW / J;
    const int i = (int)(it / per_image), p0 = (int)(it - (long long)i * per_image) * J;
    const int cell = g.cell0 + i, cy = cell / g.xmaps, cx = cell - cy * g.xmaps;
    int o[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int p = p0 + j, row = p / g.W, col = p - row * g.W;
        o[j] = (cy * (g.H + g.p) + g.p + row) * g.Wg + cx * (g.W + g.p) + g.p + col;
    }
    const long long* d = g.d;
    float v[3][J];
    bool bytes = false;
    switch (g.kind) {
    case GX_VIS_COPY: {
        const float* src = reinterpret_cast<const float*>(d[GX_VIS_D_SRC0]) + (size_t)i * d[GX_VIS_D_STRIDE0] + p0;
        vis_load<J>(src, v[0]);
        if (g.C == 3) {
            vis_load<J>(src + HW, v[1]);
            vis_load<J>(src + 2 * (size_t)HW, v[2]);
        } else {
#pragma unroll
            for (int j = 0; j < J; ++j) v[1][j] = v[2][j] = v[0][j];
        }
        break;
    }
    case GX_VIS_EXP: {
        const float* src = reinterpret_cast<const float*>(d[GX_VIS_D_SRC0]) + (size_t)i * d[GX_VIS_D_STRIDE0] + p0;
        float m[J];
        vis_load<J>(src, m);
#pragma unroll
        for (int j = 0; j < J; ++j) v[0][j] = v[1][j] = v[2][j] = expf(m[j]);
        break;
    }
    case GX_VIS_EXP_MUL: {
#pragma clang fp contract(off)
        const float* x = reinterpret_cast<const float*>(d[GX_VIS_D_SRC0]) + (size_t)i * d[GX_VIS_D_STRIDE0] + p0;
        const float* ms = reinterpret_cast<const float*>(d[GX_VIS_D_SRC1]) + (size_t)i * d[GX_VIS_D_STRIDE1] + p0;
        float m[J];
        vis_load<J>(ms, m);
        vis_load<J>(x, v[0]);
        vis_load<J>(x + HW, v[1]);
        vis_load<J>(x + 2 * (size_t)HW, v[2]);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float e = expf(m[j]);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][j] = v[c][j] * e;
        }
        break;
    }
    case GX_VIS_LABEL_COLOUR: {
        const long long* src = reinterpret_cast<const long long*>(d[GX_VIS_D_SRC0]) + (size_t)i * d[GX_VIS_D_STRIDE0] + p0;
        unsigned over = 0;
#pragma unroll
        for (int j = 0; j < J; ++j) over += vis_colour(src[j], palette, P, v[0][j], v[1][j], v[2][j]);
        if (over) atomicAdd(counter, over);
        bytes = true;
        break;
    }
    case GX_VIS_ARGMAX_COLOUR: {
        const bool packed = d[GX_VIS_D_PACKED] != 0;
        const float* base = reinterpret_cast<const float*>(d[GX_VIS_D_SRC0]);
        const long long* ptrs = table + (packed ? 0 : d[GX_VIS_D_SRC1]);
        const size_t off = (size_t)i * d[GX_VIS_D_STRIDE0] + p0;
        float best[J];
        int bi[J];
        vis_load<J>((packed ? base : reinterpret_cast<const float*>(ptrs[0])) + off, best);
#pragma unroll
        for (int j = 0; j < J; ++j) bi[j] = 0;
        for (int k = 1; k < g.K; ++k) {
            const float* pk = packed ? base + (size_t)k * d[GX_VIS_D_STRIDE1] : reinterpret_cast<const float*>(ptrs[k]);
            float m[J];
            vis_load<J>(pk + off, m);
#pragma unroll
            for (int j = 0; j < J; ++j) vis_take(m[j], k, best[j], bi[j]);
        }
        unsigned over = 0;
#pragma unroll
        for (int j = 0; j < J; ++j) over += vis_colour(bi[j], palette, P, v[0][j], v[1][j], v[2][j]);
        if (over) atomicAdd(counter, over);
        bytes = true;
        break;
    }
    default:      // GX_VIS_FILL
#pragma unroll
        for (int j = 0; j < J; ++j) v[0][j] = v[1][j] = v[2][j] = g.pad_value;
        break;
    }
    vis_store<J>(g, atlas, o, v, bytes);
}

__global__ void __launch_bounds__(256)
vis_compose_kernel(const long long* __restrict__ table, int G, long long total, const unsigned char* __restrict__ palette, int P,
                   float* __restrict__ atlas, unsigned* __restrict__ counter) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    int lo = 0, hi = G - 1;      // the last grid whose first work item is <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * GX_VIS_DESC_WORDS + GX_VIS_D_WORK] <= t) lo = mid; else hi = mid - 1;
    }
    const long long* d = table + (size_t)lo * GX_VIS_DESC_WORDS;
    const VisGrid g = vis_decode(d);
    const long long it = t - d[GX_VIS_D_WORK], items = d[GX_VIS_D_ITEMS];
    if (it < items) {
        if (d[GX_VIS_D_VEC]) vis_source<4>(g, it, table, palette, P, atlas, counter);
        else vis_source<1>(g, it, table, palette, P, atlas, counter);
        return;
    }
    // the padding: pixel q of the grid, unless it lies in one of the cells 0 .. n_geom - 1
    const int q = (int)(it - items), y = q / g.Wg, x = q - y * g.Wg;
    const int yy = y - g.p, xx = x - g.p;
    if (yy >= 0 && xx >= 0) {
        const int cy = yy / (g.H + g.p), cx = xx / (g.W + g.p);
        if (yy - cy * (g.H + g.p) < g.H && xx - cx * (g.W + g.p) < g.W && cy < g.ymaps && cx < g.xmaps &&
            cy * g.xmaps + cx < g.n_geom)
            return;
    }
    const int o[1] = {q};
    const float v[3][1] = {{g.pad_value}, {g.pad_value}, {g.pad_value}};
    vis_store<1>(g, atlas, o, v, false);
}

}  // namespace

extern "C" {

int gx_vis_compose(const long long* table_host, const long long* table_dev, long long table_words, int n_grids,
                   const unsigned char* palette, int P, float* atlas, long long atlas_words, gx_stream_t stream) {
    GX_CHECK_ARG(table_host && table_dev && atlas, "gx_vis_compose: null pointer");
    GX_CHECK_ARG(n_grids >= 1 && table_words >= (long long)n_grids * GX_VIS_DESC_WORDS, "gx_vis_compose: %d grids do not fit a table of %lld words",
                 n_grids, table_words);
    GX_CHECK_ARG(atlas_words >= 1 && (reinterpret_cast<uintptr_t>(atlas) & 15) == 0, "gx_vis_compose: the atlas must be 16-byte aligned and hold its counter");
    GX_CHECK_ARG(P >= 0 && P <= 256, "gx_vis_compose: palette of %d entries (at most 256)", P);
    long long work = 0;
    for (int gi = 0; gi < n_grids; ++gi) {
        const long long* d = table_host + (size_t)gi * GX_VIS_DESC_WORDS;
        const long long kind = d[GX_VIS_D_KIND], n = d[GX_VIS_D_N], C = d[GX_VIS_D_C], H = d[GX_VIS_D_H], W = d[GX_VIS_D_W];
        const long long K = d[GX_VIS_D_K], nrow = d[GX_VIS_D_NROW], padding = d[GX_VIS_D_PADDING], mode = d[GX_VIS_D_MODE];
        const long long vec = d[GX_VIS_D_VEC], cell0 = d[GX_VIS_D_CELL0], n_geom = d[GX_VIS_D_N_GEOM], own = d[GX_VIS_D_OWN_PAD];
        const long long s0 = d[GX_VIS_D_STRIDE0], s1 = d[GX_VIS_D_STRIDE1];
        const uintptr_t a0 = (uintptr_t)d[GX_VIS_D_SRC0], a1 = (uintptr_t)d[GX_VIS_D_SRC1];
        GX_CHECK_ARG(kind >= GX_VIS_COPY && kind <= GX_VIS_FILL, "gx_vis_compose: grid %d: unknown kind %lld", gi, kind);
        GX_CHECK_ARG(mode == GX_VIS_FP32_CHW || mode == GX_VIS_U8_HWC, "gx_vis_compose: grid %d: unknown mode %lld", gi, mode);
        GX_CHECK_ARG(nrow >= 1, "gx_vis_compose: grid %d: nrow = %lld below 1", gi, nrow);
        GX_CHECK_ARG(padding >= 0 && padding < (1 << 15), "gx_vis_compose: grid %d: padding = %lld is negative or too large", gi, padding);
        GX_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && n_geom >= 1 && n_geom < (1 << 20) && cell0 >= 0 && cell0 + n <= n_geom,
                     "gx_vis_compose: grid %d: bad dims n = %lld, H = %lld, W = %lld, cells %lld + %lld of %lld", gi, n, H, W, cell0, n, n_geom);
        GX_CHECK_ARG(kind != GX_VIS_COPY || C == 1 || C == 3, "gx_vis_compose: grid %d: C = %lld is neither 1 nor 3", gi, C);
        GX_CHECK_ARG(kind != GX_VIS_ARGMAX_COLOUR || (K >= 1 && K <= 32), "gx_vis_compose: grid %d: K = %lld outside [1, 32]", gi, K);
        GX_CHECK_ARG((vec == 0 || vec == 1) && (own == 0 || own == 1), "gx_vis_compose: grid %d: VEC and OWN_PAD are flags", gi);
        GX_CHECK_ARG(s0 >= 0 && s1 >= 0, "gx_vis_compose: grid %d: negative stride", gi);
        const long long p = n_geom == 1 ? 0 : padding, xmaps = nrow < n_geom ? nrow : n_geom, ymaps = (n_geom + xmaps - 1) / xmaps;
        const long long Hg = ymaps * (H + p) + p, Wg = xmaps * (W + p) + p, HW = H * W;
        GX_CHECK_ARG(HW < (1LL << 30) && 3 * Hg * Wg < (1LL << 31), "gx_vis_compose: grid %d: %lld x %lld pixels are too many", gi, Hg, Wg);
        const long long words = mode == GX_VIS_FP32_CHW ? 3 * Hg * Wg : (3 * Hg * Wg + 3) / 4;
        GX_CHECK_ARG(d[GX_VIS_D_DST] >= 0 && d[GX_VIS_D_DST] + words <= atlas_words - 1,
                     "gx_vis_compose: grid %d: words [%lld, %lld) pass the atlas (%lld words and the counter)", gi, d[GX_VIS_D_DST],
                     d[GX_VIS_D_DST] + words, atlas_words - 1);
        const bool colour = kind == GX_VIS_LABEL_COLOUR || kind == GX_VIS_ARGMAX_COLOUR;
        GX_CHECK_ARG(!colour || palette, "gx_vis_compose: grid %d: a colour kind without a palette", gi);
        // sources, and whether 16-byte loads are legal where the descriptor asks for them
        bool vec_ok = (HW & 3) == 0;
        const bool packed = d[GX_VIS_D_PACKED] != 0;
        if (kind == GX_VIS_ARGMAX_COLOUR && !packed) {
            GX_CHECK_ARG(d[GX_VIS_D_SRC1] >= (long long)n_grids * GX_VIS_DESC_WORDS && d[GX_VIS_D_SRC1] + K <= table_words,
                         "gx_vis_compose: grid %d: pointer table at word %lld outside the table", gi, d[GX_VIS_D_SRC1]);
            for (int k = 0; k < K; ++k) {
                const uintptr_t a = (uintptr_t)table_host[d[GX_VIS_D_SRC1] + k];
                GX_CHECK_ARG(a, "gx_vis_compose: grid %d: plane %d is null", gi, k);
                vec_ok = vec_ok && (a & 15) == 0;
            }
        } else if (kind != GX_VIS_FILL) {
            GX_CHECK_ARG(a0, "gx_vis_compose: grid %d: null source", gi);
            if (kind != GX_VIS_LABEL_COLOUR) vec_ok = vec_ok && (a0 & 15) == 0;
            if (kind == GX_VIS_ARGMAX_COLOUR) vec_ok = vec_ok && (K == 1 || (s1 & 3) == 0);
        }
        if (kind == GX_VIS_EXP_MUL) {
            GX_CHECK_ARG(a1, "gx_vis_compose: grid %d: null mask source", gi);
            vec_ok = vec_ok && (a1 & 15) == 0 && (n == 1 || (s1 & 3) == 0);
        }
        if (kind != GX_VIS_FILL && kind != GX_VIS_LABEL_COLOUR) vec_ok = vec_ok && (n == 1 || (s0 & 3) == 0);
        GX_CHECK_ARG(!vec || vec_ok, "gx_vis_compose: grid %d: VEC set, but H W = %lld, the image bases or their strides rule 16-byte loads out", gi, HW);
        GX_CHECK_ARG(d[GX_VIS_D_ITEMS] == (vec ? n * HW / 4 : n * HW), "gx_vis_compose: grid %d: ITEMS = %lld does not match n H W", gi, d[GX_VIS_D_ITEMS]);
        GX_CHECK_ARG(d[GX_VIS_D_WORK] == work, "gx_vis_compose: grid %d: WORK = %lld, the prefix is %lld", gi, d[GX_VIS_D_WORK], work);
        work += d[GX_VIS_D_ITEMS] + (own ? Hg * Wg : 0);
    }
    GX_CHECK_ARG(work > 0 && (work + 255) / 256 < (1LL << 31), "gx_vis_compose: %lld work items", work);
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 8.0 * (double)work);
        hipLaunchKernelGGL(vis_compose_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, table_dev, n_grids, work, palette, P,
                           atlas, reinterpret_cast<unsigned*>(atlas + atlas_words - 1));
    }
    GX_CHECK_LAUNCH("gx_vis_compose");
    return GX_OK;
}

}  // extern "C"
