// Device half of the JPEG decoder (genesis_amd/jpeg.py; host half: gx_jpeg.cpp): quantised DCT coefficients -> the fp32
// NCHW batch the model consumes, in one launch.  Reference: third_party/tf_gqn/gqn_tfr_provider.py:141-143
// (tf.image.decode_jpeg, convert_image_dtype) and datasets/gqn_config.py:141-145 (moveaxis, F.interpolate).  The
// arithmetic is libjpeg's default decoding path, restated from its definition (include/genesis_hip.h), bit for bit:
// the 13-bit fixed-point inverse DCT on columns then rows, triangle-filter chroma upsampling, 16-bit fixed-point colour
// conversion.
//   one workgroup of 256 threads per frame; the three uint8 component planes (padded to whole MCUs) live in LDS
//   stage 1  eight lanes per 8x8 block, 32 blocks at a time: lane j loads coefficient row j and quantiser row j (16 bytes
//            each), multiplies, and the block is transposed through a per-group LDS tile (rows of 9 words: conflict-free
//            both ways) so that lane x runs the column pass of column x; a second trip through the tile gives lane y row y
//            for the row pass, whose eight samples go to the plane as one 8-byte store
//   stage 2  a thread per output pixel, x fastest: nearest source pixel, chroma upsampled from the planes, colour, scale,
//            and one coalesced fp32 store per channel plane
// B = 32 frames of 64 x 64 occupy 32 of the chip's 256 CUs whatever the layout: the aim is one short launch.
#include "gx_common.h"
#include "gx_jpeg_pixel.h"      // idct8, clamp8, chroma_at, ycc_to_rgb: shared with gx_imagefile.hip

#include <math.h>

namespace {

constexpr int kMaxDim = 128;
constexpr int kPitchPad = 8;            // bytes added to a plane's row: rows of one block fall on different banks
constexpr int kGroups = 32;             // 8-lane groups of the workgroup
constexpr int kTileRow = 9;             // words per row of a group's transpose tile
constexpr int kTileWords = 8 * kTileRow;

struct JpegGeom {
    int bw0, bh0, bwc, bhc;             // blocks per row / column of the luma and chroma planes
    int pitch0, pitchc, size0, sizec;   // bytes
    int cw, ch;                         // real extent of a chroma plane
};

__host__ __device__ inline JpegGeom jpeg_geom(int H, int W, int sampling) {
    JpegGeom g;
    const int hs = sampling ? 2 : 1, vs = sampling == 2 ? 2 : 1;
    const int mcux = (W + 8 * hs - 1) / (8 * hs), mcuy = (H + 8 * vs - 1) / (8 * vs);
    g.bw0 = mcux * hs;
    g.bh0 = mcuy * vs;
    g.bwc = mcux;
    g.bhc = mcuy;
    g.pitch0 = g.bw0 * 8 + kPitchPad;
    g.pitchc = g.bwc * 8 + kPitchPad;
    g.size0 = g.pitch0 * g.bh0 * 8;
    g.sizec = g.pitchc * g.bhc * 8;
    g.cw = (W + hs - 1) / hs;
    g.ch = (H + vs - 1) / vs;
    return g;
}

inline size_t jpeg_lds_bytes(const JpegGeom& g) { return (size_t)g.size0 + 2 * (size_t)g.sizec + kGroups * kTileWords * sizeof(int); }

// s = min(floor(d * scale), in - 1) with scale = in / out in fp32: F.interpolate's nearest source index (gx_feed.hip)
__device__ __forceinline__ int nearest_src(int d, float scale, int in) {
    const int s = (int)floorf((float)d * scale);
    return s < in - 1 ? s : in - 1;
}

__global__ void __launch_bounds__(256)
jpeg_decode_kernel(const short* __restrict__ coef, const unsigned short* __restrict__ qtab, float* __restrict__ dst_f32,
                   unsigned char* __restrict__ dst_u8, int H, int W, int sampling, int Sh, int Sw) {
    extern __shared__ uint4 jpeg_lds[];
    const JpegGeom g = jpeg_geom(H, W, sampling);
    unsigned char* plane0 = (unsigned char*)jpeg_lds;
    unsigned char* plane1 = plane0 + g.size0;
    unsigned char* plane2 = plane1 + g.sizec;
    int* tiles = (int*)(plane2 + g.sizec);
    const int frame = blockIdx.x;
    const int nb0 = g.bw0 * g.bh0, nbc = g.bwc * g.bhc, nb = nb0 + 2 * nbc;
    const short* fcoef = coef + (size_t)frame * nb * 64;
    const unsigned short* fq = qtab + (size_t)frame * 192;

    // ---- stage 1: blocks -> planes
    const int grp = threadIdx.x >> 3, j = threadIdx.x & 7;
    int* tile = tiles + grp * kTileWords;
    for (int first = 0; first < nb; first += kGroups) {           // the same trip count for every thread (barriers inside)
        const int blk = first + grp;
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
        if (on) {                                                 // lane j: column j, rows in v[]; only this lane touches it
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
            const int bw = c == 0 ? g.bw0 : g.bwc, pitch = c == 0 ? g.pitch0 : g.pitchc;
            const int by = k / bw, bx = k - by * bw;
            unsigned char* p = (c == 0 ? plane0 : (c == 1 ? plane1 : plane2)) + (by * 8 + j) * pitch + bx * 8;
            *(uint2*)p = make_uint2(lo, hi);
        }
        // (the next trip's first write to the tile is to row j, which this lane alone has just read)
    }
    __syncthreads();

    // ---- stage 2: planes -> pixels
    auto rgb_at = [&](int y, int x, int* r, int* gg, int* b) {
        const int yy = plane0[y * g.pitch0 + x];
        const int cb = chroma_at(plane1, g.pitchc, g.cw, g.ch, sampling, y, x) - 128;
        const int cr = chroma_at(plane2, g.pitchc, g.cw, g.ch, sampling, y, x) - 128;
        ycc_to_rgb(yy, cb, cr, r, gg, b);
    };
    if (dst_f32) {
        const float sh = (float)H / (float)Sh, sw = (float)W / (float)Sw;
        const int npix = Sh * Sw;
        float* out = dst_f32 + (size_t)frame * 3 * npix;
        for (int i = threadIdx.x; i < npix; i += blockDim.x) {
            const int oy = i / Sw, ox = i - oy * Sw;
            int r, gg, b;
            rgb_at(nearest_src(oy, sh, H), nearest_src(ox, sw, W), &r, &gg, &b);
            out[i] = (float)r * (1.0f / 255.0f);                  // convert_image_dtype's multiplication, not a division
            out[npix + i] = (float)gg * (1.0f / 255.0f);
            out[2 * npix + i] = (float)b * (1.0f / 255.0f);
        }
    }
    if (dst_u8) {
        unsigned char* out = dst_u8 + (size_t)frame * H * W * 3;
        for (int i = threadIdx.x; i < H * W; i += blockDim.x) {
            const int y = i / W, x = i - y * W;
            int r, gg, b;
            rgb_at(y, x, &r, &gg, &b);
            out[3 * i] = (unsigned char)r;
            out[3 * i + 1] = (unsigned char)gg;
            out[3 * i + 2] = (unsigned char)b;
        }
    }
}

}  // namespace

extern "C" {

int gx_jpeg_decode_f32chw(const short* coef, const unsigned short* qtab, float* dst_f32, unsigned char* dst_u8, int B, int H, int W,
                          int sampling, int S_h, int S_w, gx_stream_t stream) {
    GX_CHECK_ARG(coef && qtab, "gx_jpeg_decode_f32chw: null pointer");
    GX_CHECK_ARG(dst_f32 || dst_u8, "gx_jpeg_decode_f32chw: no output (dst_f32 and dst_u8 are both null)");
    GX_CHECK_ARG(((uintptr_t)coef % 16) == 0 && ((uintptr_t)qtab % 16) == 0, "gx_jpeg_decode_f32chw: coef and qtab must be 16-byte aligned");
    GX_CHECK_ARG(B > 0 && H > 0 && W > 0, "gx_jpeg_decode_f32chw: bad dims");
    GX_CHECK_ARG(H <= kMaxDim && W <= kMaxDim, "gx_jpeg_decode_f32chw: a %d x %d frame is larger than the %d x %d the kernel decodes", W,
                 H, kMaxDim, kMaxDim);
    GX_CHECK_ARG(sampling >= 0 && sampling <= 2, "gx_jpeg_decode_f32chw: bad sampling class %d", sampling);
    GX_CHECK_ARG(!dst_f32 || (S_h > 0 && S_w > 0 && S_h <= 8192 && S_w <= 8192), "gx_jpeg_decode_f32chw: bad output size %d x %d", S_h,
                 S_w);
    const JpegGeom g = jpeg_geom(H, W, sampling);
    const size_t lds = jpeg_lds_bytes(g);
    GX_CHECK_ARG(lds <= 65536, "gx_jpeg_decode_f32chw: %zu bytes of LDS", lds);
    hipStream_t s = (hipStream_t)stream;
    {
        const double blocks = (double)g.bw0 * g.bh0 + 2.0 * g.bwc * g.bhc;
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, B * (blocks * 128 + 384 + (dst_f32 ? 12.0 * S_h * S_w : 0.0) + (dst_u8 ? 3.0 * H * W : 0.0)));
        hipLaunchKernelGGL(jpeg_decode_kernel, dim3((unsigned)B), dim3(256), lds, s, coef, qtab, dst_f32, dst_u8, H, W, sampling, S_h,
                           S_w);
    }
    GX_CHECK_LAUNCH("gx_jpeg_decode_f32chw");
    return GX_OK;
}

}  // extern "C"
