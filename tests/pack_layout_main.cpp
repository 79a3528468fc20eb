// Host check of the packed-weight descriptor (genesis_amd/csrc/gx_pack.h): packs seeded random weights with the functions the
// pack kernels use and checks, for every (view, form) the library produces and channel counts that pad in both directions,
//   1. no two (m, k, t, piece) of the padded range share a word;
//   2. every word lies inside gx_pack_bytes, the trailer too, and no word is the trailer;
//   3. the packing decodes (pieces summed, scale undone) to the source weight of the view -- stated here as plain index arithmetic
//      on w, independently of gx_pack_weight_value -- to the precision of the form; padding decodes to zero;
//   4. gx_pack_valid accepts exactly the pairs listed here.
// Prints one line per failure and "pack layout: N cases, 0 failures" at the end; exit status 1 on any failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gx_pack.h"

static int g_fail = 0;
static void fail(const char* what, GxPack p, int Co, int Ci, int m, int k, int t, double got, double want, double tol) {
    if (++g_fail <= 40)
        printf("FAIL %s: view %d form %d Co %d Ci %d (m %d k %d t %d) got %.17g want %.17g tol %.3g\n", what, (int)p.view,
               (int)p.form, Co, Ci, m, k, t, got, want, tol);
}

static uint32_t g_rng = 12345u;
static float rnd() {      // uniform in (-1, 1), every mantissa bit in use
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)((int32_t)g_rng) * (1.f / 2147483648.f);
}

// the views, restated: which weight element is Wp(t, k, m)?  M, K: the real output / reduction channel counts
static bool view_swaps(GxPackView v) {       // m runs over Ci (the weight's second dimension), k over Co
    return v == GX_VIEW_C3_DGRAD || v == GX_VIEW_DT_DGRAD || v == GX_VIEW_WINO_DGRAD || v == GX_VIEW_C5_FLIP;
}
static double src3(const std::vector<float>& w, int Ci, int co, int ci, int kh, int kw) { return w[(((size_t)co * Ci + ci) * 3 + kh) * 3 + kw]; }
static double src5(const std::vector<float>& w, int D1, int d0, int d1, int kh, int kw) { return w[(((size_t)d0 * D1 + d1) * 5 + kh) * 5 + kw]; }
static double source(const std::vector<float>& w, GxPackView v, int Co, int Ci, int m, int k, int t) {
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    switch (v) {
        case GX_VIEW_C3_FWD: return src3(w, Ci, m, k, t / 3, t % 3);                        // w [co = m][ci = k]
        case GX_VIEW_C3_DGRAD: return src3(w, Ci, k, m, 2 - t / 3, 2 - t % 3);              // w [co = k][ci = m], rotated by 180 degrees
        case GX_VIEW_DT_ROW0: return src5(w, Co, k, m, 2 * (t / 5), t % 5);                 // w [ci = k][co = m], even kernel rows
        case GX_VIEW_DT_ROW1: return src5(w, Co, k, m, 2 * (t / 5) + 1, t % 5);             // ... odd kernel rows
        case GX_VIEW_DT_DGRAD: return src5(w, Co, m, k, t / 5, t % 5);                      // w [ci = m][co = k]
        case GX_VIEW_C5: return src5(w, Ci, m, k, t / 5, t % 5);                            // w [Co = M][Ci = K]
        case GX_VIEW_C5_FLIP: return src5(w, Ci, k, m, 4 - t / 5, 4 - t % 5);               // w [Co = K][Ci = M], rotated by 180 degrees
        default: {                                                                          // (G g G^T)[xi][nu], t = 4 xi + nu, in fp64
            const int xi = t >> 2, nu = t & 3;
            double u = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const double g = v == GX_VIEW_WINO_FWD ? src3(w, Ci, m, k, a, b) : src3(w, Ci, k, m, 2 - a, 2 - b);
                    u += G[xi][a] * g * G[nu][b];
                }
            return u;
        }
    }
}

static double half_of(uint32_t word, int hi, bool fp16) {
    const unsigned short h = (unsigned short)(hi ? word >> 16 : word & 0xffffu);
    if (fp16) return (double)(float)__builtin_bit_cast(_Float16, h);
    return (double)(float)__builtin_bit_cast(__bf16, h);
}

static void run_case(GxPack p, int Co, int Ci) {
    const bool swap = view_swaps(p.view);
    const int M = swap ? Ci : Co, K = swap ? Co : Ci;
    const int NT = gx_pack_taps(p.view), np = gx_pack_pieces(p.form);
    // the call sites' padding: output channels to 64, reduction channels to the chunk of the kernel family
    const int Mpad = (M + 63) / 64 * 64, Kpad = gx_pack_pipe16(p.form) ? (K + 15) / 16 * 16 : (K + 7) / 8 * 8;
    std::vector<float> w((size_t)Co * Ci * gx_pack_src_elems(p.view));
    float amax = 0.f;
    for (float& x : w) { x = rnd(); amax = fmaxf(amax, fabsf(x)); }

    const size_t bytes = gx_pack_bytes(p, Kpad, Mpad), nwords = bytes / 4;
    const uint32_t kSentinel = 0x7fc5a5a5u;       // (a NaN in fp32, and its upper half a NaN in bf16 and fp16: no pack writes it)
    std::vector<uint32_t> wp(nwords, kSentinel);
    std::vector<unsigned char> owner(nwords, 0);

    // 2. the trailer
    size_t trailer_word = (size_t)-1;
    if (gx_pack_has_trailer(p.form)) {
        const size_t off = gx_pack_trailer_off(p, Kpad, Mpad);
        if (off % 4 != 0 || off + 4 > bytes) { fail("trailer outside the packing", p, Co, Ci, 0, 0, 0, (double)off, (double)bytes, 0); return; }
        trailer_word = off / 4;
        memcpy(&wp[trailer_word], &amax, 4);      // (what the amax launch ahead of the pack leaves there)
    }
    // 1. + 2. destinations
    for (int t = 0; t < NT; ++t)
        for (int k = 0; k < Kpad; k += np ? 2 : 1)
            for (int m = 0; m < Mpad; ++m)
                for (int q = 0; q < (np ? np : 1); ++q) {
                    const size_t d = gx_pack_word(p, m, k, t, q, Kpad, Mpad);
                    if (d >= nwords) { fail("word outside the packing", p, Co, Ci, m, k, t, (double)d, (double)nwords, 0); return; }
                    if (d == trailer_word) fail("word on the trailer", p, Co, Ci, m, k, t, (double)d, 0, 0);
                    if (owner[d]++) fail("word written twice", p, Co, Ci, m, k, t, (double)d, 0, 0);
                }
    // pack, exactly as pack_elements (gx_conv.hip) does
    const int f16_exp = gx_pack_scale_exp(p, reinterpret_cast<const float*>(wp.data()), Kpad, Mpad);
    for (int idx = 0; idx < NT * Kpad * Mpad; ++idx)
        gx_pack_store(w.data(), reinterpret_cast<float*>(wp.data()), p, Co, Ci, idx % Mpad, (idx / Mpad) % Kpad, idx / (Mpad * Kpad), Kpad,
                      Mpad, f16_exp);
    // the store wrote the words gx_pack_word names, and no others
    for (size_t d = 0; d < nwords; ++d)
        if (d != trailer_word && (wp[d] != kSentinel) != (owner[d] != 0)) fail("store and gx_pack_word disagree", p, Co, Ci, 0, 0, 0, (double)d, owner[d], 0);
    if (gx_pack_has_trailer(p.form)) {
        // the scale puts bound * amax into [2^14, 2^15): every scaled value is below fp16's largest, 65504
        const double top = ldexp((double)gx_pack_amax_bound(p.view) * amax, f16_exp);
        if (!(top >= 16384.0 && top < 32768.0)) fail("scale", p, Co, Ci, 0, 0, 0, top, 16384.0, 0);
    }

    // 3. decode
    // u = 2^-24, the unit roundoff of fp32.  The Winograd operand is computed in fp32: each of the two 1-D transforms is two
    // additions and an exact halving.  Stage 1: sums <= 3 amax, so <= 0.5 * 2 * u * 3 amax = 3 u amax of rounding.  Stage 2: its
    // three inputs carry that error (0.5 * 3 * 3 u amax = 4.5 u amax) and its own sums are <= 4.5 amax (0.5 * 2 * u * 4.5 amax):
    // 9 u amax in all; 10 u amax covers the second-order terms.  Every other view copies a weight: exact.
    const double u = ldexp(1.0, -24);
    const double e32 = gx_pack_wino(p.view) ? 10.0 * u * amax : 0.0;
    for (int t = 0; t < NT; ++t)
        for (int k = 0; k < Kpad; ++k)
            for (int m = 0; m < Mpad; ++m) {
                const bool real = m < M && k < K;
                const double want = real ? source(w, p.view, Co, Ci, m, k, t) : 0.0;
                double got = 0.0, tol;
                if (np == 0) {
                    got = (double)__builtin_bit_cast(float, wp[gx_pack_word(p, m, k, t, 0, Kpad, Mpad)]);
                    tol = 0.0;                      // fp32 forms: the value itself
                } else {
                    for (int q = 0; q < np; ++q)
                        got += half_of(wp[gx_pack_word(p, m, k & ~1, t, q, Kpad, Mpad)], k & 1, p.form == GX_FORM_F16X2);
                    const double a = fabs(want) + e32;        // bound on the magnitude of the fp32 value that was split
                    if (p.form == GX_FORM_BF16X3) {
                        // a bf16 piece keeps 8 significant bits: rounding to nearest leaves a remainder <= 2^-8 of the value, which
                        // fp32 holds exactly; three pieces in a row leave <= 2^-24 of the value: 24 significant bits
                        tol = ldexp(a, -24);
                    } else if (p.form == GX_FORM_F16X2) {
                        // s = v * 2^e <= 2^15 in magnitude.  hi = fp16(s) keeps 11 significant bits (s in fp16's normal range:
                        // remainder <= 2^-11 |s|); lo = fp16(s - hi) keeps 11 more where s - hi is normal, >= 2^-14 (remainder
                        // <= 2^-22 |s|: 22 significant bits), and is within half a subnormal step, 2^-25, where it is not
                        got = ldexp(got, -f16_exp);
                        tol = ldexp(fmax(ldexp(a, f16_exp - 22), ldexp(1.0, -25)), -f16_exp);
                    } else {
                        // one bf16 piece: 8 significant bits, remainder <= 2^-8 of the value
                        tol = ldexp(a, -8);
                    }
                }
                if (real) tol += e32;
                if (!(fabs(got - want) <= tol)) fail(real ? "decode" : "padding not zero", p, Co, Ci, m, k, t, got, want, tol);
            }
}

int main() {
    // 4. the pairs the library produces: every view in the tap fp32 form and the three 16-bit-pipe forms; the k-quad fp32 form
    // for the conv3x3 and the transposed conv; the tap bf16 form for everything but the Winograd operands
    static const bool kValid[GX_VIEW_COUNT][GX_FORM_COUNT] = {
        /* C3_FWD     */ {1, 1, 1, 1, 1, 1},
        /* C3_DGRAD   */ {1, 1, 1, 1, 1, 1},
        /* DT_ROW0    */ {1, 1, 1, 1, 1, 1},
        /* DT_ROW1    */ {1, 1, 1, 1, 1, 1},
        /* DT_DGRAD   */ {1, 1, 1, 1, 1, 1},
        /* WINO_FWD   */ {1, 0, 1, 1, 1, 0},
        /* WINO_DGRAD */ {1, 0, 1, 1, 1, 0},
        /* C5         */ {1, 0, 1, 1, 1, 1},
        /* C5_FLIP    */ {1, 0, 1, 1, 1, 1},
    };
    for (int v = 0; v <= GX_VIEW_COUNT + 1; ++v)
        for (int f = 0; f <= GX_FORM_COUNT + 1; ++f) {
            const GxPack p{(GxPackView)v, (GxPackForm)f};
            const bool want = v < GX_VIEW_COUNT && f < GX_FORM_COUNT && kValid[v][f];
            if (gx_pack_valid(p) != want) fail("gx_pack_valid", p, 0, 0, 0, 0, 0, gx_pack_valid(p), want, 0);
        }
    if (!(GxPack{GX_VIEW_C5, GX_FORM_F16X2} == GxPack{GX_VIEW_C5, GX_FORM_F16X2}) ||
        GxPack{GX_VIEW_C5, GX_FORM_F16X2} == GxPack{GX_VIEW_C5_FLIP, GX_FORM_F16X2} ||
        GxPack{GX_VIEW_C5, GX_FORM_F16X2} == GxPack{GX_VIEW_C5, GX_FORM_BF16X3})
        fail("operator==", GxPack{GX_VIEW_C5, GX_FORM_F16X2}, 0, 0, 0, 0, 0, 0, 0, 0);

    // channel counts from {7, 16, 24, 40, 72}: below and above a 64-channel tile, multiples and non-multiples of 8 and 16
    static const int kChannels[][2] = {{7, 7}, {7, 16}, {16, 7}, {24, 40}, {40, 24}, {16, 72}, {72, 16}, {72, 72}};
    int cases = 0;
    for (int v = 0; v < GX_VIEW_COUNT; ++v)
        for (int f = 0; f < GX_FORM_COUNT; ++f) {
            const GxPack p{(GxPackView)v, (GxPackForm)f};
            if (!gx_pack_valid(p)) continue;
            for (const auto& c : kChannels) { run_case(p, c[0], c[1]); ++cases; }
        }
    printf("pack layout: %d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
