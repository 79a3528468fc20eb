// Loose image files on the device (genesis_amd/imagefile.py): the pixel half of JPEG and PNG decoding and Pillow's
// resize-then-crop for a batch whose frames each have their OWN size, sampling class and channel count.  What a frame is and
// where its bytes lie comes from a per-frame descriptor table of 64-bit words (include/genesis_hip.h, GX_JPEGR_* / GX_PNGR_* /
// GX_RSR_*), handed over the way gx_png_pack's is: the host copy is checked word by word before anything is launched, the
// device copy is what the kernels read.  A batch costs four launches whatever it holds:
//   gx_jpeg_decode_ragged      two launches.  (1) blocks -> planes: eight lanes per 8 x 8 block exactly as in gx_jpeg.hip
//                              (dequantise, column pass, row pass, one 8-byte store), kJpegrBlocksPerWg blocks a workgroup, the
//                              padded uint8 planes going to a scratch arena in global memory.  (2) planes -> pixels: a workgroup
//                              per kJpegrTileH x kJpegrTileW tile of a frame, a thread per pixel: chroma_at + ycc_to_rgb.
//                              Why two launches and not one with the chroma halo recomputed per band: DESIGN.md.
//   gx_png_unfilter_ragged     one launch, one workgroup per frame: png_unfilter_frame (gx_png_unfilter.h), the kernel of
//                              gx_png_unfilter, with C chosen per workgroup from the table.
//   gx_u8_resample_ragged_f32chw  one launch: Pillow's two-pass 8-bit BILINEAR of the WHOLE frame to (h', w'), of which only the
//                              output window's rows and columns are computed; fp32 CHW = byte / 255.
// The arithmetic is shared, not copied: gx_jpeg_pixel.h, gx_png_unfilter.h.
#include "gx_common.h"
#include "gx_jpeg_pixel.h"
#include "gx_png_unfilter.h"

namespace {

constexpr int kMaxDim = kGxImageMaxDim;

// the last frame whose first workgroup (word `field` of its descriptor) is <= wg
__device__ __forceinline__ int frame_of(const long long* __restrict__ table, int n, int words, int field, long long wg) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * words + field] <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- JPEG ------------------------------------------------------------------------------------------------------------------------
constexpr int kGroups = 32;             // 8-lane groups of a workgroup of 256
constexpr int kTileRow = 9;             // words per row of a group's transpose tile (gx_jpeg.hip)
constexpr int kTileWords = 8 * kTileRow;
static_assert(GX_JPEGR_BLOCKS_PER_WG % kGroups == 0, "a workgroup takes whole trips of kGroups blocks");
static_assert(GX_JPEGR_TILE_H * GX_JPEGR_TILE_W % 256 == 0, "a pixel tile is a whole number of passes of 256 threads");

struct JpegrGeom {
    int bw0, bh0, bwc, bhc;             // blocks per row / column of the luma and chroma planes (chroma: 0 for a grey frame)
    int cw, ch;                         // real extent of a chroma plane
    long long nb0, nbc;                 // blocks of the luma plane, of one chroma plane
};

__host__ __device__ inline JpegrGeom jpegr_geom(int H, int W, int ncomp, int sampling) {
    JpegrGeom g;
    const int hs = sampling ? 2 : 1, vs = sampling == 2 ? 2 : 1;
    const int mcux = (W + 8 * hs - 1) / (8 * hs), mcuy = (H + 8 * vs - 1) / (8 * vs);
    g.bw0 = mcux * hs;
    g.bh0 = mcuy * vs;
    g.bwc = ncomp == 3 ? mcux : 0;
    g.bhc = ncomp == 3 ? mcuy : 0;
    g.cw = (W + hs - 1) / hs;
    g.ch = (H + vs - 1) / vs;
    g.nb0 = (long long)g.bw0 * g.bh0;
    g.nbc = (long long)g.bwc * g.bhc;
    return g;
}

__global__ void __launch_bounds__(256)
jpegr_idct_kernel(const long long* __restrict__ table, int n, const short* __restrict__ coef, const unsigned short* __restrict__ qtab,
                  unsigned char* __restrict__ scratch) {
    __shared__ int tiles[kGroups * kTileWords];
    const int f = frame_of(table, n, GX_JPEGR_DESC_WORDS, GX_JPEGR_D_WG0_IDCT, blockIdx.x);
    const long long* d = table + (size_t)f * GX_JPEGR_DESC_WORDS;
    const JpegrGeom g = jpegr_geom((int)d[GX_JPEGR_D_H], (int)d[GX_JPEGR_D_W], (int)d[GX_JPEGR_D_NCOMP], (int)d[GX_JPEGR_D_SAMPLING]);
    const int nb0 = (int)g.nb0, nbc = (int)g.nbc, nb = nb0 + 2 * nbc;
    const short* fcoef = coef + d[GX_JPEGR_D_COEF];
    const unsigned short* fq = qtab + d[GX_JPEGR_D_QTAB];
    unsigned char* plane0 = scratch + d[GX_JPEGR_D_PLANES];
    unsigned char* plane1 = plane0 + (size_t)nb0 * 64;
    unsigned char* plane2 = plane1 + (size_t)nbc * 64;
    const int pitch0 = g.bw0 * 8, pitchc = g.bwc * 8;
    const int base = (int)(blockIdx.x - d[GX_JPEGR_D_WG0_IDCT]) * GX_JPEGR_BLOCKS_PER_WG;

    const int grp = threadIdx.x >> 3, j = threadIdx.x & 7;
    int* tile = tiles + grp * kTileWords;
    for (int first = 0; first < GX_JPEGR_BLOCKS_PER_WG; first += kGroups) {       // the same trip count for every thread (barriers inside)
        const int blk = base + first + grp;
        const bool on = blk < nb;
        const int c = blk < nb0 ? 0 : (blk < nb0 + nbc ? 1 : 2);
        int v[8];
        if (on) {
            const uint4 cw = *(const uint4*)(fcoef + (size_t)blk * 64 + j * 8);
            const uint4 qw = *(const uint4*)(fq + c * 64 + j * 8);
            const unsigned cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                tile[j * kTileRow + 2 * i] = (int)(short)(cs[i] & 0xffffu) * (int)(qs[i] & 0xffffu);
                tile[j * kTileRow + 2 * i + 1] = (int)(short)(cs[i] >> 16) * (int)(qs[i] >> 16);
            }
        }
        __syncthreads();
        if (on) {                                                 // lane j: column j
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = tile[i * kTileRow + j];
            idct8(v, 11);
#pragma unroll
            for (int i = 0; i < 8; ++i) tile[i * kTileRow + j] = v[i];
        }
        __syncthreads();
        if (on) {                                                 // lane j: row j
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = tile[j * kTileRow + i];
            idct8(v, 18);
            unsigned lo = 0, hi = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo |= (unsigned)clamp8(v[i] + 128) << (8 * i);
                hi |= (unsigned)clamp8(v[4 + i] + 128) << (8 * i);
            }
            const int k = c == 0 ? blk : (c == 1 ? blk - nb0 : blk - nb0 - nbc);
            const int bw = c == 0 ? g.bw0 : g.bwc, pitch = c == 0 ? pitch0 : pitchc;
            const int by = k / bw, bx = k - by * bw;
            unsigned char* p = (c == 0 ? plane0 : (c == 1 ? plane1 : plane2)) + (size_t)(by * 8 + j) * pitch + bx * 8;
            *(uint2*)p = make_uint2(lo, hi);
        }
        // (the next trip's first write to the tile is to row j, which this lane alone has just read)
    }
}

__global__ void __launch_bounds__(256)
jpegr_pixel_kernel(const long long* __restrict__ table, int n, const unsigned char* __restrict__ scratch, unsigned char* __restrict__ dst) {
    const int f = frame_of(table, n, GX_JPEGR_DESC_WORDS, GX_JPEGR_D_WG0_PIX, blockIdx.x);
    const long long* d = table + (size_t)f * GX_JPEGR_DESC_WORDS;
    const int H = (int)d[GX_JPEGR_D_H], W = (int)d[GX_JPEGR_D_W], ncomp = (int)d[GX_JPEGR_D_NCOMP], sampling = (int)d[GX_JPEGR_D_SAMPLING];
    const JpegrGeom g = jpegr_geom(H, W, ncomp, sampling);
    const unsigned char* plane0 = scratch + d[GX_JPEGR_D_PLANES];
    const unsigned char* plane1 = plane0 + (size_t)g.nb0 * 64;
    const unsigned char* plane2 = plane1 + (size_t)g.nbc * 64;
    const int pitch0 = g.bw0 * 8, pitchc = g.bwc * 8;
    unsigned char* out = dst + d[GX_JPEGR_D_DST];
    const int local = (int)(blockIdx.x - d[GX_JPEGR_D_WG0_PIX]);
    const int tiles_w = (W + GX_JPEGR_TILE_W - 1) / GX_JPEGR_TILE_W;
    const int ty = local / tiles_w, tx = local - ty * tiles_w;
#pragma unroll
    for (int k = 0; k < GX_JPEGR_TILE_H * GX_JPEGR_TILE_W / 256; ++k) {
        const int i = k * 256 + threadIdx.x;
        const int y = ty * GX_JPEGR_TILE_H + i / GX_JPEGR_TILE_W, x = tx * GX_JPEGR_TILE_W + i % GX_JPEGR_TILE_W;
        if (y < H && x < W) {
            const int yy = plane0[(size_t)y * pitch0 + x];
            const size_t at = (size_t)y * W + x;
            if (ncomp == 1) {
                out[at] = (unsigned char)yy;
            } else {
                const int cb = chroma_at(plane1, pitchc, g.cw, g.ch, sampling, y, x) - 128;
                const int cr = chroma_at(plane2, pitchc, g.cw, g.ch, sampling, y, x) - 128;
                int r, gg, b;
                ycc_to_rgb(yy, cb, cr, &r, &gg, &b);
                out[3 * at] = (unsigned char)r;
                out[3 * at + 1] = (unsigned char)gg;
                out[3 * at + 2] = (unsigned char)b;
            }
        }
    }
}

// ---- PNG -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPngThreads)
pngr_unfilter_kernel(const long long* __restrict__ table, const unsigned char* __restrict__ filtered, unsigned char* __restrict__ dst) {
    __shared__ unsigned char carry[kMaxDim * 4];          // the last row of the previous band
    __shared__ unsigned char edge[2][kPngWaves][4];
    const long long* d = table + (size_t)blockIdx.x * GX_PNGR_DESC_WORDS;
    const int H = (int)d[GX_PNGR_D_H], W = (int)d[GX_PNGR_D_W], C = (int)d[GX_PNGR_D_C];      // uniform over the workgroup
    const unsigned char* src = filtered + d[GX_PNGR_D_SRC];
    unsigned char* out = dst + d[GX_PNGR_D_DST];
    if (C == 1) png_unfilter_frame<1>(src, out, nullptr, 0, H, W, carry, edge);
    else if (C == 3) png_unfilter_frame<3>(src, out, nullptr, 0, H, W, carry, edge);
    else png_unfilter_frame<4>(src, out, nullptr, 0, H, W, carry, edge);
}

// ---- resize, then crop -----------------------------------------------------------------------------------------------------------
constexpr int kPilBits = 22;            // gx_feed.hip
constexpr int kRsrInter = 32768;        // bytes of the uint8 intermediate per workgroup
constexpr int kRsrMaxBand = 8;          // output rows of a band, at most
constexpr int kRsrMaxOut = 1024;        // S_h and S_w, at most: a band of ONE row of any frame then fits the intermediate (rsr_plan_frame)

__device__ __forceinline__ unsigned char pil_clip8(int acc) {
    acc >>= kPilBits;
    return (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// One workgroup per band of R output rows of a frame's window.
//   Pass 1: the horizontal taps of every source row the band's vertical taps touch, for the window's columns only, read from the
//   frame in global memory (a frame is read about 1 + 2 / scale times over all bands, from L2) into the uint8 intermediate.
//   Pass 2: the vertical taps from the intermediate, written as fp32 planes with x fastest.
// hb / vb are the bounds of the WINDOW's columns / rows (the host hands over the table rows from left' / top' on), so a
// pass whose size does not change meets the identity rows (1, 0) of Pillow's table and copies.
// Every index a table supplies is clamped to the frame and to the intermediate before it is used.
__global__ void __launch_bounds__(256)
rsr_kernel(const long long* __restrict__ table, int n, const unsigned char* __restrict__ src, const int* __restrict__ tables,
           float* __restrict__ dst, int Sh, int Sw) {
    __shared__ unsigned char inter[kRsrInter];
    const int b = frame_of(table, n, GX_RSR_DESC_WORDS, GX_RSR_D_WG0, blockIdx.x);
    const long long* d = table + (size_t)b * GX_RSR_DESC_WORDS;
    const int Hs = (int)d[GX_RSR_D_HS], Ws = (int)d[GX_RSR_D_WS], C = (int)d[GX_RSR_D_C];
    const int Cc = C == 1 ? 1 : 3;                                         // channels computed: alpha is dropped, grey replicated below
    const int R = (int)d[GX_RSR_D_R], kh = (int)d[GX_RSR_D_KH], kv = (int)d[GX_RSR_D_KV];
    const int* hb = tables + d[GX_RSR_D_HB];
    const int* hw = tables + d[GX_RSR_D_HW];
    const int* vb = tables + d[GX_RSR_D_VB];
    const int* vw = tables + d[GX_RSR_D_VW];
    const unsigned char* frame = src + d[GX_RSR_D_SRC];
    const int band = (int)(blockIdx.x - d[GX_RSR_D_WG0]);
    const int y0 = band * R, y1 = min(y0 + R, Sh);
    const int nx = Sw;
    const int rowb = nx * Cc;
    const int r0 = min(max(vb[2 * y0], 0), Hs - 1);
    const int nr = min(min(vb[2 * (y1 - 1)] + vb[2 * (y1 - 1) + 1] - r0, Hs - r0), kRsrInter / rowb);
    for (int i = threadIdx.x; i < nr * rowb; i += blockDim.x) {
        const int r = i / rowb, rem = i - r * rowb;
        const int xo = rem / Cc, c = rem - xo * Cc;
        const int first = min(max(hb[2 * xo], 0), Ws - 1);
        const int taps = min(min(hb[2 * xo + 1], kh), Ws - first);
        const unsigned char* q = frame + ((size_t)(r0 + r) * Ws + first) * C + c;
        const int* w = hw + (size_t)xo * kh;
        int acc = 1 << (kPilBits - 1);
        for (int t = 0; t < taps; ++t) acc += (int)q[t * C] * w[t];
        inter[i] = pil_clip8(acc);
    }
    __syncthreads();
    const int ny = y1 - y0;
    const size_t plane = (size_t)Sh * Sw;
    float* out = dst + (size_t)b * 3 * plane;
    for (int i = threadIdx.x; i < Cc * ny * nx; i += blockDim.x) {
        const int x = i % nx, yc = i / nx;
        const int yl = yc % ny, c = yc / ny;
        const int y = y0 + yl;
        const int first = vb[2 * y] - r0, taps = min(vb[2 * y + 1], kv);
        const int* w = vw + (size_t)y * kv;
        int acc = 1 << (kPilBits - 1);
        for (int t = 0; t < taps; ++t) {
            const int r = first + t;
            if (r >= 0 && r < nr) acc += (int)inter[r * rowb + x * Cc + c] * w[t];
        }
        const float v = (float)pil_clip8(acc) / 255.0f;          // a true division, as in gx_feed.hip
        const size_t at = (size_t)y * Sw + x;
        if (Cc == 1) {
            out[at] = v;
            out[plane + at] = v;
            out[2 * plane + at] = v;
        } else {
            out[c * plane + at] = v;
        }
    }
}

// Rows of a band of one frame: kRsrMaxBand, fewer while the bound on the band's source rows times the window's row of
// intermediate bytes does not fit; 0 when not even one row fits.  For a square window of side S one row always fits: its taps span
// at most 2 * Hs / H2 + 2 source rows with H2 >= S (4 when the frame grows), so at most 3 * (2 * kMaxDim + 2 * S) bytes.
static_assert(3 * (2 * kMaxDim + 2 * kRsrMaxOut) <= kRsrInter, "a band of one output row of a square window must fit the intermediate");
int rsr_plan_frame(int Hs, int H2, int C, int Sh, int Sw) {
    const int Cc = C == 1 ? 1 : 3;
    int R = Sh < kRsrMaxBand ? Sh : kRsrMaxBand;
    while (R > 1 && (size_t)gx_pil_band_rows(Hs, H2, R) * Sw * Cc > (size_t)kRsrInter) --R;
    return (size_t)gx_pil_band_rows(Hs, H2, R) * Sw * Cc <= (size_t)kRsrInter ? R : 0;
}

int rsr_check_frame(const char* who, int i, const long long* d, long long src_bytes, long long tables_values, int Sh, int Sw) {
    const long long Hs = d[GX_RSR_D_HS], Ws = d[GX_RSR_D_WS], C = d[GX_RSR_D_C], H2 = d[GX_RSR_D_H2], W2 = d[GX_RSR_D_W2];
    GX_CHECK_ARG(Hs >= 1 && Hs <= kMaxDim && Ws >= 1 && Ws <= kMaxDim, "%s: frame %d: H = %lld, W = %lld outside [1, %d]", who, i, Hs, Ws, kMaxDim);
    GX_CHECK_ARG(C == 1 || C == 3 || C == 4, "%s: frame %d: C = %lld is not 1, 3 or 4", who, i, C);
    GX_CHECK_ARG(H2 >= Sh && W2 >= Sw && H2 <= (1 << 24) && W2 <= (1 << 24),
                 "%s: frame %d: the resized frame %lld x %lld does not hold the %d x %d window", who, i, W2, H2, Sw, Sh);
    GX_CHECK_ARG(d[GX_RSR_D_SRC] >= 0 && d[GX_RSR_D_SRC] + Hs * Ws * C <= src_bytes, "%s: frame %d: SRC = %lld, its %lld bytes end outside the %lld of src",
                 who, i, d[GX_RSR_D_SRC], Hs * Ws * C, src_bytes);
    const int kh = gx_pil_bilinear_ksize((int)Ws, (int)W2), kv = gx_pil_bilinear_ksize((int)Hs, (int)H2);
    GX_CHECK_ARG(d[GX_RSR_D_KH] == kh && d[GX_RSR_D_KV] == kv, "%s: frame %d: table ksize (%lld, %lld) is not that of %lld -> %lld, %lld -> %lld", who, i,
                 d[GX_RSR_D_KH], d[GX_RSR_D_KV], Ws, W2, Hs, H2);
    const long long need[4] = {2LL * Sw, (long long)Sw * kh, 2LL * Sh, (long long)Sh * kv};
    const int field[4] = {GX_RSR_D_HB, GX_RSR_D_HW, GX_RSR_D_VB, GX_RSR_D_VW};
    for (int k = 0; k < 4; ++k)
        GX_CHECK_ARG(d[field[k]] >= 0 && d[field[k]] + need[k] <= tables_values, "%s: frame %d: table word %d = %lld, its %lld values end outside the %lld of tables",
                     who, i, field[k], d[field[k]], need[k], tables_values);
    return GX_OK;
}

}  // namespace

extern "C" {

int gx_jpeg_decode_ragged(const long long* table_host, const long long* table_dev, int n_frames, const short* coef, long long coef_values,
                          const unsigned short* qtab, long long qtab_values, unsigned char* scratch, long long scratch_bytes,
                          unsigned char* dst_u8, long long dst_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(table_host && table_dev && coef && qtab && scratch && dst_u8, "gx_jpeg_decode_ragged: null pointer");
    GX_CHECK_ARG(n_frames >= 1, "gx_jpeg_decode_ragged: n_frames = %d below 1", n_frames);
    GX_CHECK_ARG(((uintptr_t)coef % 16) == 0 && ((uintptr_t)qtab % 16) == 0 && ((uintptr_t)scratch % 16) == 0,
                 "gx_jpeg_decode_ragged: coef, qtab and scratch must be 16-byte aligned");
    long long wg_idct = 0, wg_pix = 0;
    double bytes = 0.0;
    for (int i = 0; i < n_frames; ++i) {
        const long long* d = table_host + (size_t)i * GX_JPEGR_DESC_WORDS;
        const long long H = d[GX_JPEGR_D_H], W = d[GX_JPEGR_D_W], nc = d[GX_JPEGR_D_NCOMP], sampling = d[GX_JPEGR_D_SAMPLING];
        GX_CHECK_ARG(H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim, "gx_jpeg_decode_ragged: frame %d: H = %lld, W = %lld outside [1, %d]", i, H, W,
                     kMaxDim);
        GX_CHECK_ARG(nc == 1 || nc == 3, "gx_jpeg_decode_ragged: frame %d: %lld components (1 or 3)", i, nc);
        GX_CHECK_ARG(sampling >= 0 && sampling <= 2 && (nc == 3 || sampling == 0), "gx_jpeg_decode_ragged: frame %d: bad sampling class %lld", i, sampling);
        const JpegrGeom g = jpegr_geom((int)H, (int)W, (int)nc, (int)sampling);
        const long long nb = g.nb0 + 2 * g.nbc;
        GX_CHECK_ARG(d[GX_JPEGR_D_COEF] >= 0 && d[GX_JPEGR_D_COEF] % 8 == 0 && d[GX_JPEGR_D_COEF] + nb * 64 <= coef_values,
                     "gx_jpeg_decode_ragged: frame %d: COEF = %lld (a multiple of 8), its %lld values end outside the %lld of coef", i,
                     d[GX_JPEGR_D_COEF], nb * 64, coef_values);
        GX_CHECK_ARG(d[GX_JPEGR_D_QTAB] >= 0 && d[GX_JPEGR_D_QTAB] % 8 == 0 && d[GX_JPEGR_D_QTAB] + 192 <= qtab_values,
                     "gx_jpeg_decode_ragged: frame %d: QTAB = %lld (a multiple of 8), its 192 values end outside the %lld of qtab", i,
                     d[GX_JPEGR_D_QTAB], qtab_values);
        GX_CHECK_ARG(d[GX_JPEGR_D_PLANES] >= 0 && d[GX_JPEGR_D_PLANES] % 16 == 0 && d[GX_JPEGR_D_PLANES] + nb * 64 <= scratch_bytes,
                     "gx_jpeg_decode_ragged: frame %d: PLANES = %lld (a multiple of 16), its %lld bytes end outside the %lld of scratch", i,
                     d[GX_JPEGR_D_PLANES], nb * 64, scratch_bytes);
        GX_CHECK_ARG(d[GX_JPEGR_D_DST] >= 0 && d[GX_JPEGR_D_DST] + H * W * nc <= dst_bytes,
                     "gx_jpeg_decode_ragged: frame %d: DST = %lld, its %lld bytes end outside the %lld of dst_u8", i, d[GX_JPEGR_D_DST], H * W * nc,
                     dst_bytes);
        GX_CHECK_ARG(d[GX_JPEGR_D_WG0_IDCT] == wg_idct && d[GX_JPEGR_D_WG0_PIX] == wg_pix,
                     "gx_jpeg_decode_ragged: frame %d: WG0 = (%lld, %lld), the prefixes are (%lld, %lld)", i, d[GX_JPEGR_D_WG0_IDCT],
                     d[GX_JPEGR_D_WG0_PIX], wg_idct, wg_pix);
        wg_idct += (nb + GX_JPEGR_BLOCKS_PER_WG - 1) / GX_JPEGR_BLOCKS_PER_WG;
        wg_pix += ((H + GX_JPEGR_TILE_H - 1) / GX_JPEGR_TILE_H) * ((W + GX_JPEGR_TILE_W - 1) / GX_JPEGR_TILE_W);
        bytes += (double)nb * 64;
    }
    GX_CHECK_ARG(wg_idct < (1LL << 31) && wg_pix < (1LL << 31), "gx_jpeg_decode_ragged: too many blocks for one launch");
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 3.0 * bytes);
        hipLaunchKernelGGL(jpegr_idct_kernel, dim3((unsigned)wg_idct), dim3(256), 0, s, table_dev, n_frames, coef, qtab, scratch);
    }
    GX_CHECK_LAUNCH("gx_jpeg_decode_ragged (blocks to planes)");
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, 4.0 * bytes);
        hipLaunchKernelGGL(jpegr_pixel_kernel, dim3((unsigned)wg_pix), dim3(256), 0, s, table_dev, n_frames, (const unsigned char*)scratch, dst_u8);
    }
    GX_CHECK_LAUNCH("gx_jpeg_decode_ragged (planes to pixels)");
    return GX_OK;
}

int gx_png_unfilter_ragged(const long long* table_host, const long long* table_dev, int n_frames, const unsigned char* filtered,
                           long long filtered_bytes, unsigned char* dst_u8, long long dst_bytes, gx_stream_t stream) {
    GX_CHECK_ARG(table_host && table_dev && filtered && dst_u8, "gx_png_unfilter_ragged: null pointer");
    GX_CHECK_ARG(n_frames >= 1, "gx_png_unfilter_ragged: n_frames = %d below 1", n_frames);
    double bytes = 0.0;
    for (int i = 0; i < n_frames; ++i) {
        const long long* d = table_host + (size_t)i * GX_PNGR_DESC_WORDS;
        const long long H = d[GX_PNGR_D_H], W = d[GX_PNGR_D_W], C = d[GX_PNGR_D_C];
        GX_CHECK_ARG(H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim, "gx_png_unfilter_ragged: frame %d: H = %lld, W = %lld outside [1, %d]", i, H, W,
                     kMaxDim);
        GX_CHECK_ARG(C == 1 || C == 3 || C == 4, "gx_png_unfilter_ragged: frame %d: C = %lld is not 1, 3 or 4", i, C);
        GX_CHECK_ARG(d[GX_PNGR_D_SRC] >= 0 && d[GX_PNGR_D_SRC] + H * (1 + W * C) <= filtered_bytes,
                     "gx_png_unfilter_ragged: frame %d: SRC = %lld, its %lld bytes end outside the %lld of filtered", i, d[GX_PNGR_D_SRC],
                     H * (1 + W * C), filtered_bytes);
        GX_CHECK_ARG(d[GX_PNGR_D_DST] >= 0 && d[GX_PNGR_D_DST] + H * W * C <= dst_bytes,
                     "gx_png_unfilter_ragged: frame %d: DST = %lld, its %lld bytes end outside the %lld of dst_u8", i, d[GX_PNGR_D_DST], H * W * C,
                     dst_bytes);
        bytes += (double)H * (1 + 2 * W * C);
    }
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, bytes);
        hipLaunchKernelGGL(pngr_unfilter_kernel, dim3((unsigned)n_frames), dim3(kPngThreads), 0, s, table_dev, filtered, dst_u8);
    }
    GX_CHECK_LAUNCH("gx_png_unfilter_ragged");
    return GX_OK;
}

int gx_u8_resample_ragged_plan(long long* table_host, int n_frames, int S_h, int S_w, long long* workgroups) {
    GX_CHECK_ARG(table_host && workgroups, "gx_u8_resample_ragged_plan: null pointer");
    GX_CHECK_ARG(n_frames >= 1, "gx_u8_resample_ragged_plan: n_frames = %d below 1", n_frames);
    GX_CHECK_ARG(S_h >= 1 && S_w >= 1 && S_h <= kRsrMaxOut && S_w <= kRsrMaxOut, "gx_u8_resample_ragged_plan: bad output size %d x %d (1 .. %d)", S_h, S_w, kRsrMaxOut);
    long long wg = 0;
    for (int i = 0; i < n_frames; ++i) {
        long long* d = table_host + (size_t)i * GX_RSR_DESC_WORDS;
        const long long Hs = d[GX_RSR_D_HS], H2 = d[GX_RSR_D_H2], C = d[GX_RSR_D_C];
        GX_CHECK_ARG(Hs >= 1 && Hs <= kMaxDim && H2 >= S_h && H2 <= (1 << 24) && (C == 1 || C == 3 || C == 4),
                     "gx_u8_resample_ragged_plan: frame %d: H = %lld -> %lld with C = %lld", i, Hs, H2, C);
        const int R = rsr_plan_frame((int)Hs, (int)H2, (int)C, S_h, S_w);
        GX_CHECK_ARG(R >= 1, "gx_u8_resample_ragged_plan: frame %d: %lld -> %lld rows with a %d x %d window exceeds the kernel's band buffer", i, Hs,
                     H2, S_w, S_h);
        d[GX_RSR_D_R] = R;
        d[GX_RSR_D_WG0] = wg;
        wg += gx_ceil_div(S_h, R);
    }
    *workgroups = wg;
    return GX_OK;
}

int gx_u8_resample_ragged_f32chw(const long long* table_host, const long long* table_dev, int n_frames, const unsigned char* src,
                                 long long src_bytes, const int* tables, long long tables_values, float* dst, int S_h, int S_w,
                                 gx_stream_t stream) {
    GX_CHECK_ARG(table_host && table_dev && src && tables && dst, "gx_u8_resample_ragged_f32chw: null pointer");
    GX_CHECK_ARG(n_frames >= 1, "gx_u8_resample_ragged_f32chw: n_frames = %d below 1", n_frames);
    GX_CHECK_ARG(S_h >= 1 && S_w >= 1 && S_h <= kRsrMaxOut && S_w <= kRsrMaxOut, "gx_u8_resample_ragged_f32chw: bad output size %d x %d (1 .. %d)", S_h, S_w, kRsrMaxOut);
    GX_CHECK_ARG(((uintptr_t)tables % 4) == 0 && ((uintptr_t)dst % 4) == 0, "gx_u8_resample_ragged_f32chw: tables and dst must be 4-byte aligned");
    long long wg = 0;
    double bytes = 0.0;
    for (int i = 0; i < n_frames; ++i) {
        const long long* d = table_host + (size_t)i * GX_RSR_DESC_WORDS;
        const int rc = rsr_check_frame("gx_u8_resample_ragged_f32chw", i, d, src_bytes, tables_values, S_h, S_w);
        if (rc != GX_OK) return rc;
        const int R = rsr_plan_frame((int)d[GX_RSR_D_HS], (int)d[GX_RSR_D_H2], (int)d[GX_RSR_D_C], S_h, S_w);
        GX_CHECK_ARG(R >= 1 && d[GX_RSR_D_R] == R && d[GX_RSR_D_WG0] == wg,
                     "gx_u8_resample_ragged_f32chw: frame %d: (R, WG0) = (%lld, %lld), gx_u8_resample_ragged_plan gives (%d, %lld)", i,
                     d[GX_RSR_D_R], d[GX_RSR_D_WG0], R, wg);
        wg += gx_ceil_div(S_h, R);
        bytes += (double)d[GX_RSR_D_HS] * d[GX_RSR_D_WS] * d[GX_RSR_D_C];
    }
    GX_CHECK_ARG(wg < (1LL << 31), "gx_u8_resample_ragged_f32chw: grid too large");
    hipStream_t s = (hipStream_t)stream;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, bytes + 12.0 * n_frames * S_h * S_w);
        hipLaunchKernelGGL(rsr_kernel, dim3((unsigned)wg), dim3(256), 0, s, table_dev, n_frames, src, tables, dst, S_h, S_w);
    }
    GX_CHECK_LAUNCH("gx_u8_resample_ragged_f32chw");
    return GX_OK;
}

}  // extern "C"
