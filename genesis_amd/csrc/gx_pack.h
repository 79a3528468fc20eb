// Packed conv weights: which view of which weight tensor, in which layout and piece form -- one descriptor, and the only place
// where the facts of a packing (taps, pieces, size, trailer, destination word, value, piece split) are written down.
// Host and device; needs nothing else of the library, so a host program can pack with the very functions the kernels use.
//
// Every conv family packs its weight through launch_pack (gx_conv.hip): Wp(t, k, m), k = reduction channel padded to Kpad,
// m = output channel padded to Mpad, zero filled.  Who reads what:
//
//   view \ form    TAP_F32             KQ_F32            BF16X3 / F16X2 / BF16X1 (16-bit matrix pipe)        TAP_BF16X1
//   C3_FWD/_DGRAD  tapconv_body M_C3   gx_kq.hip Q_C3    gx_kq.hip Q_C3H (<= 32 output channels, 32-ch tiles) tapconv_body M_C3
//   DT_ROW0/_ROW1  tapconv_dt_kernel   gx_kq.hip QCfgDT  gx_kq.hip QCfgDTH                                    tapconv_dt_kernel
//   DT_DGRAD       tapconv_body M_DG   gx_kq.hip Q_DG    gx_kq.hip Q_DGH (taps grouped by parity plane)       tapconv_body M_DG
//   WINO_FWD/_DGRAD gx_wino.hip fp32   --                gx_wino.hip wino_conv_h_kernel                       --
//   C5 / C5_FLIP   tapconv_body M_C5   --                gx_kq.hip Q_C5H                                      tapconv_body M_C5
//
//   TAP_F32     fp32 [t][k][m] (the Winograd views: the operand order of gx_wino_u_slot); the fp32 matrix pipe
//   KQ_F32      fp32, k-quad order (gx_kq_w_slot): 16-byte k-contiguous operand reads
//   BF16X3      every weight as three bf16 pieces hi | mid | lo, two channels per 32-bit word: family mode 1 (gx_kq_precision,
//               gx_wino_precision), and the Winograd layers of gx_matmul_precision 1 whose input's maxima are not known
//   F16X2       two fp16 pieces of w * 2^e; e from the weight tensor's largest magnitude, which the amax launch ahead of the
//               pack leaves in the packing's TRAILER (one float): gx_matmul_precision 1, the default
//   BF16X1      one bf16 piece, w rounded to nearest even, in the one-piece layouts: gx_matmul_precision 2
//   TAP_BF16X1  one bf16 piece in the tap-conv layout [t][k / 8][m][8 ch] -- the 8 channels of (t, m) are one 16-byte vector,
//               a lane's A operand: gx_tapconv_precision 3
// In the 16-bit forms the thread of an even k writes the words of (k, k + 1), the odd one nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum GxPackView : uint8_t {
    GX_VIEW_C3_FWD = 0,     // conv3x3 forward        W[co][ci][3][3] -> m = co, k = ci, t = kh*3 + kw
    GX_VIEW_C3_DGRAD,       // conv3x3 data gradient  W[co][ci][3][3] -> m = ci, k = co, t = (kh, kw) reads W[..][2-kh][2-kw]
    GX_VIEW_DT_ROW0,        // transposed conv 5x5 s2, output rows of parity 0: W[ci][co][5][5] -> m = co, k = ci, t = khi*5 + kw, kh = 2 khi
    GX_VIEW_DT_ROW1,        // ... of parity 1: kh = 2 khi + 1
    GX_VIEW_DT_DGRAD,       // its data gradient      W[ci][co][5][5] -> m = ci, k = co, t = kh*5 + kw
    GX_VIEW_WINO_FWD,       // Winograd F(2x2,3x3) operand U = G g G^T of the conv3x3 forward, t = position
    GX_VIEW_WINO_DGRAD,     // ... of its data gradient
    GX_VIEW_C5,             // 5x5 stride 1, cross-correlation: w [Co = M][Ci = K][5][5]
    GX_VIEW_C5_FLIP,        // 5x5 stride 1, true convolution with the channel roles swapped: w [Co = K][Ci = M][5][5]
    GX_VIEW_COUNT
};
enum GxPackForm : uint8_t { GX_FORM_TAP_F32 = 0, GX_FORM_KQ_F32, GX_FORM_BF16X3, GX_FORM_F16X2, GX_FORM_BF16X1, GX_FORM_TAP_BF16X1, GX_FORM_COUNT };
struct GxPack { GxPackView view; GxPackForm form; };
__host__ __device__ __forceinline__ bool operator==(GxPack a, GxPack b) { return a.view == b.view && a.form == b.form; }

__host__ __device__ __forceinline__ bool gx_pack_wino(GxPackView v) { return v == GX_VIEW_WINO_FWD || v == GX_VIEW_WINO_DGRAD; }
// taps (Winograd: positions) of a view -- the packing's t range
__host__ __device__ __forceinline__ int gx_pack_taps(GxPackView v) {
    switch (v) {
        case GX_VIEW_C3_FWD: case GX_VIEW_C3_DGRAD: return 9;
        case GX_VIEW_DT_ROW0: return 15;
        case GX_VIEW_DT_ROW1: return 10;
        case GX_VIEW_WINO_FWD: case GX_VIEW_WINO_DGRAD: return 16;
        default: return 25;
    }
}
// floats of the source weight per channel pair: 3 x 3 or 5 x 5
__host__ __device__ __forceinline__ int gx_pack_src_elems(GxPackView v) { return (v <= GX_VIEW_C3_DGRAD || gx_pack_wino(v)) ? 9 : 25; }
// the forms of the 16-bit matrix pipe (gx_kq.hip's and gx_wino.hip's bf16 / fp16 kernels): reduction channels in chunks of 16
__host__ __device__ __forceinline__ bool gx_pack_pipe16(GxPackForm f) { return f == GX_FORM_BF16X3 || f == GX_FORM_F16X2 || f == GX_FORM_BF16X1; }
// pieces per value (0: a plain fp32 word)
__host__ __device__ __forceinline__ int gx_pack_pieces(GxPackForm f) {
    return f == GX_FORM_BF16X3 ? 3 : (f == GX_FORM_F16X2 ? 2 : ((f == GX_FORM_BF16X1 || f == GX_FORM_TAP_BF16X1) ? 1 : 0));
}
// the fp16 form: its scale needs the weight tensor's largest magnitude, kept in the packing's trailer ...
__host__ __device__ __forceinline__ bool gx_pack_has_trailer(GxPackForm f) { return f == GX_FORM_F16X2; }
// ... times this bound on |packed value| / max |w| (the Winograd operands U = G g G^T: |U| <= 2.25 max |g|)
__host__ __device__ __forceinline__ float gx_pack_amax_bound(GxPackView v) { return gx_pack_wino(v) ? 2.25f : 1.f; }
// does the library produce this pair?  (no k-quad or tap-bf16 Winograd operands, no k-quad 5 x 5 stride 1)
__host__ __device__ __forceinline__ bool gx_pack_valid(GxPack p) {
    if (p.view >= GX_VIEW_COUNT || p.form >= GX_FORM_COUNT) return false;
    if (p.form == GX_FORM_KQ_F32) return p.view <= GX_VIEW_DT_DGRAD;
    if (p.form == GX_FORM_TAP_BF16X1) return !gx_pack_wino(p.view);
    return true;
}

// ---- Winograd F(2x2,3x3) weight operand (gx_wino.hip; also produced by the packed-weight cache of gx_conv.hip) ----
// (G g G^T)[xi][nu], p = 4 xi + nu, for output channel m / reduction channel k.  mode 0: g = w[m][k] (forward);
// mode 1: g = w[k][m] rotated by 180 degrees (data gradient).  w is [Co][Ci][3][3].
__host__ __device__ __forceinline__ float gx_wino_u_value(const float* __restrict__ w, int mode, int Co, int Ci, int m, int k,
                                                          int p) {
    const int Mact = mode == 0 ? Co : Ci, Kact = mode == 0 ? Ci : Co;
    if (m >= Mact || k >= Kact) return 0.f;
    const int xi = p >> 2, nu = p & 3;
    float t[3];   // row xi of G g
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        float g0, g1, g2;
        if (mode == 0) {
            const float* q = w + ((size_t)m * Ci + k) * 9 + b;
            g0 = q[0]; g1 = q[3]; g2 = q[6];
        } else {
            const float* q = w + ((size_t)k * Ci + m) * 9 + (2 - b);
            g0 = q[6]; g1 = q[3]; g2 = q[0];
        }
        t[b] = xi == 0 ? g0 : (xi == 1 ? 0.5f * (g0 + g1 + g2) : (xi == 2 ? 0.5f * (g0 - g1 + g2) : g2));
    }
    return nu == 0 ? t[0] : (nu == 1 ? 0.5f * (t[0] + t[1] + t[2]) : (nu == 2 ? 0.5f * (t[0] - t[1] + t[2]) : t[2]));
}
// position of U(p, k, m) in the conv kernel's operand order:
// [m tile][chunk of 8 k][position][lane = 32 ((k >> 2) & 1) + (m & 31)][2 (k & 3) + ((m >> 5) & 1)]
// (lane half h of the chunk's MFMA j multiplies channel 4 h + j: the B operand's four values are one 16-byte LDS read)
__host__ __device__ __forceinline__ size_t gx_wino_u_slot(int m, int k, int p, int Kpad) {
    const size_t base = ((size_t)(m >> 6) * (Kpad >> 3) + (k >> 3)) * 16 + p;
    return base * 512 + (size_t)((((((k >> 2) & 1) << 5) | (m & 31)) << 3) | ((k & 3) << 1) | ((m >> 5) & 1));
}
// The same operands for the bf16 matrix pipe (gx_wino.hip: wino_conv_h_kernel): every U value as three bf16 pieces, chunks of 16
// reduction channels.  32-bit word (two channels k even, k + 1) of piece `piece` of position p:
// [m tile 64][chunk k >> 4][position 16][piece 3][m half (m >> 5) & 1][lane = 32 ((k >> 3) & 1) + (m & 31)][(k & 7) >> 1]
// -- a wave's A operand of (position, piece, m half) is 1 KB, lane-linear: one 16-byte load per lane.
// (NP = 1: the one-piece form, gx_wino_precision(3) -- one bf16 piece per value, positions 2 KB apart instead of 6 KB)
__host__ __device__ __forceinline__ size_t gx_wino_h_word(int m, int k, int p, int piece, int Kpad16, int NP = 3) {
    return ((((((size_t)(m >> 6) * (Kpad16 >> 4) + (k >> 4)) * 16 + p) * NP + piece) * 2 + ((m >> 5) & 1)) * 256) +
           (size_t)((((k >> 3) & 1) * 32 + (m & 31)) * 4 + ((k & 7) >> 1));
}

// ---- k-quad tap convolutions (gx_kq.hip): 16-byte k-contiguous MFMA operand reads for the chip-filling layers ----
// packed-weight layout [m tile 64][chunk of 8 k][tap, phase-major][quad (k >> 2) & 1][m & 63][k & 3]
// tap order: the [t] order of the views above, except the transposed conv's data gradient (25 taps, t = kh*5+kw),
// whose taps are grouped by parity plane (kh & 1, kw & 1): planes of 9, 6, 6, 4 taps, (kh / 2, kw / 2) row-major inside
__host__ __device__ __forceinline__ int gx_kq_dg_tap_slot(int t) {
    const int kh = t / 5, kw = t % 5;
    const int pa = kh & 1, pb = kw & 1;
    const int p = pa * 2 + pb;
    const int base = p == 0 ? 0 : (p == 1 ? 9 : (p == 2 ? 15 : 21));
    return base + (kh >> 1) * (3 - pb) + (kw >> 1);
}
__host__ __device__ __forceinline__ size_t gx_kq_w_slot(int m, int k, int tslot, int NT, int Kpad) {
    return ((((size_t)(m >> 6) * (Kpad >> 3) + (k >> 3)) * NT + tslot) * 2 + ((k >> 2) & 1)) * 256 + (m & 63) * 4 + (k & 3);
}
// ... on the 16-bit matrix pipe: 32-bit word of element (m, k even, k + 1) of piece `piece` of tap t:
// [channel tile][16-channel chunk][tap][piece][octet][64 output channels][8 channels], two channels per word
// (NP: pieces per value -- 3 bf16 ones, 2 fp16 ones or 1 bf16 one)
__host__ __device__ __forceinline__ size_t gx_kq_h_word(int m, int k, int t, int piece, int NT, int K, int NP = 3) {
    return ((((size_t)(m >> 6) * (K >> 4) + (k >> 4)) * NT + t) * NP + piece) * 512 + (((k >> 3) & 1) * 64 + (m & 63)) * 4 + ((k & 7) >> 1);
}
// ... the conv3x3 of <= 32-output-channel layers (gx_kq.hip Q_C3H): 32 output channels per channel tile
__host__ __device__ __forceinline__ size_t gx_kq_h32_word(int m, int k, int t, int piece, int NT, int K, int NP = 3) {
    return ((((size_t)(m >> 5) * (K >> 4) + (k >> 4)) * NT + t) * NP + piece) * 256 + (((k >> 3) & 1) * 32 + (m & 31)) * 4 + ((k & 7) >> 1);
}
// A 16-bit-pipe packing is laid out for three pieces of 2 KB per (tap, chunk, tile), + 16 KB of slack (the kernels copy whole
// phases); the trailer -- the weight tensor's largest magnitude, written by the amax launch that precedes the pack, read by the
// pack and by the conv kernels -- is the float 64 bytes before the end of that slack.  Byte offset of that float:
__host__ __device__ __forceinline__ size_t gx_kq_h_amax_off(int K, int M, int nt) {
    return (size_t)((M + 63) / 64) * (K / 16) * nt * 6144 + 16384 - 64;
}
__host__ __device__ __forceinline__ int gx_f16_scale_exp(float amax) {     // amax * 2^e in [2^14, 2^15); 0 / inf / nan: e = 0
    if (!(amax > 0.f) || amax > 3.0e38f) return 0;
    int ex;
    (void)frexpf(amax, &ex);
    return 15 - ex;
}

// ---- the descriptor's facts ----
__host__ __device__ __forceinline__ size_t gx_pack_trailer_off(GxPack p, int Kpad, int Mpad) {
    return gx_kq_h_amax_off(Kpad, Mpad, gx_pack_taps(p.view));
}
// bytes of the packing (what a cache entry allocates; the 16-bit-pipe forms: the three-piece size whatever the piece count)
__host__ __device__ __forceinline__ size_t gx_pack_bytes(GxPack p, int Kpad, int Mpad) {
    if (gx_pack_pipe16(p.form)) return gx_pack_trailer_off(p, Kpad, Mpad) + 64;
    return (size_t)gx_pack_taps(p.view) * Kpad * Mpad * (p.form == GX_FORM_TAP_BF16X1 ? 2 : sizeof(float));
}
// 32-bit word of the packing that holds (m, k, t): the fp32 value, or piece `piece` of channels (k even, k + 1)
__host__ __device__ __forceinline__ size_t gx_pack_word(GxPack p, int m, int k, int t, int piece, int Kpad, int Mpad) {
    const int NT = gx_pack_taps(p.view), np = gx_pack_pieces(p.form);
    const int tslot = p.view == GX_VIEW_DT_DGRAD ? gx_kq_dg_tap_slot(t) : t;     // (the k-quad and 16-bit-pipe kernels' tap order)
    switch (p.form) {
        case GX_FORM_TAP_F32:
            return gx_pack_wino(p.view) ? gx_wino_u_slot(m, k, t, Kpad) : ((size_t)t * Kpad + k) * Mpad + m;
        case GX_FORM_KQ_F32:
            return gx_kq_w_slot(m, k, tslot, NT, Kpad);
        case GX_FORM_TAP_BF16X1:
            return (((size_t)t * (Kpad >> 3) + (k >> 3)) * Mpad + m) * 4 + ((k & 7) >> 1);
        default:
            // (the Winograd fp16 form keeps the three-piece spacing: its kernel shares the bf16 x 3 kernel's addressing)
            if (gx_pack_wino(p.view)) return gx_wino_h_word(m, k, t, piece, Kpad, p.form == GX_FORM_BF16X1 ? 1 : 3);
            if (p.view <= GX_VIEW_C3_DGRAD) return gx_kq_h32_word(m, k, t, piece, NT, Kpad, np);
            return gx_kq_h_word(m, k, tslot, piece, NT, Kpad, np);
    }
}

// the packed value Wp(t, k, m) of a view of w (Co, Ci: the weight tensor's leading dimensions); zero in the padding
__host__ __device__ __forceinline__ float gx_pack_weight_value(const float* __restrict__ w, GxPackView view, int Co, int Ci, int m,
                                                               int k, int t) {
    float v = 0.f;
    switch (view) {
        case GX_VIEW_C3_FWD:
            if (m < Co && k < Ci) v = w[((size_t)m * Ci + k) * 9 + t];
            break;
        case GX_VIEW_C3_DGRAD:
            if (m < Ci && k < Co) v = w[((size_t)k * Ci + m) * 9 + (8 - t)];
            break;
        case GX_VIEW_DT_ROW0: case GX_VIEW_DT_ROW1: {
            const int kh = 2 * (t / 5) + (view - GX_VIEW_DT_ROW0), kw = t % 5;
            if (m < Co && k < Ci) v = w[((size_t)k * Co + m) * 25 + kh * 5 + kw];
            break;
        }
        case GX_VIEW_DT_DGRAD:
            if (m < Ci && k < Co) v = w[((size_t)m * Co + k) * 25 + t];
            break;
        case GX_VIEW_C5:
            if (m < Co && k < Ci) v = w[((size_t)m * Ci + k) * 25 + t];
            break;
        case GX_VIEW_C5_FLIP:
            if (k < Co && m < Ci) v = w[((size_t)k * Ci + m) * 25 + (24 - t)];
            break;
        default:
            v = gx_wino_u_value(w, view - GX_VIEW_WINO_FWD, Co, Ci, m, k, t);
    }
    return v;
}
// a value's pieces, as 16-bit patterns: bf16 hi | mid | lo (each the rounded remainder of the ones before), fp16 hi | lo of
// v * 2^f16_exp, or the one bf16 nearest v
__host__ __device__ __forceinline__ void gx_pack_split(float v, GxPackForm form, int f16_exp, unsigned short pc[3]) {
    pc[1] = pc[2] = 0;
    if (form == GX_FORM_F16X2) {
        const float ws = ldexpf(v, f16_exp);
        const _Float16 h = (_Float16)ws;
        pc[0] = __builtin_bit_cast(unsigned short, h);
        pc[1] = __builtin_bit_cast(unsigned short, (_Float16)(ws - (float)h));
        return;
    }
    const __bf16 h = (__bf16)v;
    pc[0] = __builtin_bit_cast(unsigned short, h);
    if (form != GX_FORM_BF16X3) return;
    const float r1 = v - (float)h;
    const __bf16 mm = (__bf16)r1;
    pc[1] = __builtin_bit_cast(unsigned short, mm);
    pc[2] = __builtin_bit_cast(unsigned short, (__bf16)(r1 - (float)mm));
}
// the fp16 form's scale exponent, from the trailer (0 for every other form)
__host__ __device__ __forceinline__ int gx_pack_scale_exp(GxPack p, const float* wp, int Kpad, int Mpad) {
    if (!gx_pack_has_trailer(p.form)) return 0;
    return gx_f16_scale_exp(gx_pack_amax_bound(p.view) *
                            *reinterpret_cast<const float*>(reinterpret_cast<const char*>(wp) + gx_pack_trailer_off(p, Kpad, Mpad)));
}
// packs element (m, k, t) of the padded range into wp
__host__ __device__ __forceinline__ void gx_pack_store(const float* __restrict__ w, float* __restrict__ wp, GxPack p, int Co, int Ci,
                                                       int m, int k, int t, int Kpad, int Mpad, int f16_exp) {
    const int np = gx_pack_pieces(p.form);
    if (np == 0) {
        wp[gx_pack_word(p, m, k, t, 0, Kpad, Mpad)] = gx_pack_weight_value(w, p.view, Co, Ci, m, k, t);
        return;
    }
    if (k & 1) return;
    unsigned short pc[2][3];
#pragma unroll
    for (int e = 0; e < 2; ++e) gx_pack_split(gx_pack_weight_value(w, p.view, Co, Ci, m, k + e, t), p.form, f16_exp, pc[e]);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (q >= np) break;
        const unsigned wd = (unsigned)pc[0][q] | ((unsigned)pc[1][q] << 16);
        wp[gx_pack_word(p, m, k, t, q, Kpad, Mpad)] = __builtin_bit_cast(float, wd);
    }
}
