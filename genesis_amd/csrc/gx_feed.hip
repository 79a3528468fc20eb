// Input side of the training step: uint8 HWC frames as the datasets store them -> the fp32 NCHW batch
// in [0,1] the model consumes, on the device.  Reference: datasets/multid_config.py:131-135 (transforms.ToTensor(): HWC
// uint8 -> CHW float32 / 255; F.interpolate(size=img_size), default mode 'nearest', when the stored size differs),
// datasets/multi_object_config.py:176-186 (np.moveaxis(img, 3, 1); torch.FloatTensor(img) / 255.; F.interpolate).
// There the conversion runs on the host per sample and the fp32 batch (4x the bytes) crosses PCIe (train.py:218-220);
// here the uint8 frames cross PCIe and one HBM-bound launch converts them.
#include "gx_common.h"

#include <math.h>
#include <vector>

namespace {

// dst[b][c][y][x] = src[b][sy][sx][c] / 255 with the 'nearest' source index of F.interpolate:
// s = min(floor(d * (float)in / out), in - 1)  (ATen nearest_neighbor_compute_source_index, scale = in / out in fp32)
__global__ void __launch_bounds__(256)
u8hwc_to_f32chw_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int B, int Hs, int Ws, int C,
                       int H, int W) {
    const size_t total = (size_t)B * C * H * W;
    const float sh = (float)Hs / (float)H, sw = (float)Ws / (float)W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const int b = (int)(i / ((size_t)W * H * C));
        int sy = (int)floorf((float)y * sh), sx = (int)floorf((float)x * sw);
        sy = sy < Hs - 1 ? sy : Hs - 1;
        sx = sx < Ws - 1 ? sx : Ws - 1;
        const unsigned char v = src[(((size_t)b * Hs + sy) * Ws + sx) * C + c];
        dst[i] = (float)v / 255.0f;          // a true division, as ToTensor's .div(255) is
    }
}

// The same index rule inside a crop window (top, left, Hc, Wc) of the stored frame: the resample sees the window as the
// whole image (np_img_centre_crop, then F.interpolate).  With the full-frame window it computes what the kernel above does.
__global__ void __launch_bounds__(256)
u8hwc_crop_nearest_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int B, int Hs, int Ws, int C,
                          int top, int left, int Hc, int Wc, int H, int W) {
    const size_t total = (size_t)B * C * H * W;
    const float sh = (float)Hc / (float)H, sw = (float)Wc / (float)W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const int b = (int)(i / ((size_t)W * H * C));
        int sy = (int)floorf((float)y * sh), sx = (int)floorf((float)x * sw);
        sy = sy < Hc - 1 ? sy : Hc - 1;
        sx = sx < Wc - 1 ? sx : Wc - 1;
        const unsigned char v = src[(((size_t)b * Hs + top + sy) * Ws + left + sx) * C + c];
        dst[i] = (float)v / 255.0f;
    }
}

// Pillow's 8-bit fixed-point resampler (ImagingResample, BILINEAR filter): what torchvision's Resize does to a PIL image.
// Per axis a table of `count` taps from `first` with int32 weights of 22 fractional bits (gx_pil_bilinear_coeffs, computed
// on the host in double as Pillow does).  Horizontal pass first, into a uint8 intermediate; then the vertical pass on it.
// Each sum starts at 1 << 21 (round half up) and is shifted right by 22 and clamped to [0, 255] (Pillow's clip8).
constexpr int kPilBits = 22;
constexpr int kResampleInter = 16384;   // bytes of the uint8 intermediate per workgroup
constexpr int kResampleStage = 32768;   // bytes of staged source rows per workgroup (the host sizes band and tile to fit both)

__device__ __forceinline__ unsigned char pil_clip8(int acc) {
    acc >>= kPilBits;
    return (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// One workgroup per (output-row band of R rows, output-column tile of tw columns, image), bands fastest.  The band needs
// the source rows from the first tap of its first row to the last tap of its last row, and of those the columns from the
// first tap of the tile's first column to the last tap of its last (all monotone in the output index).
//   Stage: those rows' bytes into LDS with aligned 16-byte loads, a row at a pitch of whole 16-byte chunks.  A row's first
//   byte sits at any offset (left * C and Ws * C are arbitrary), so the chunks start at its 16-byte boundary and the row
//   begins `off` bytes into its LDS row; only chunks holding a byte of the row are read (never a page the row does not touch).
//   Pass 1: every (source row, tile column, channel) of the uint8 intermediate from the staged rows.
//   Pass 2: the vertical taps from the intermediate, written as [C][rows][tw] fp32 with x fastest (coalesced row stores).
__global__ void __launch_bounds__(256)
u8hwc_pil_bilinear_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int Hs, int Ws, int C, int top,
                          int left, int H, int W, int R, int tw, int nbands, int ntiles, const int* __restrict__ hb,
                          const int* __restrict__ hw, int kh, const int* __restrict__ vb, const int* __restrict__ vw, int kv) {
    __shared__ uint4 stage4[kResampleStage / 16];
    __shared__ unsigned char inter[kResampleInter];
    const unsigned char* stage = (const unsigned char*)stage4;
    const int band = blockIdx.x % nbands, tile = (blockIdx.x / nbands) % ntiles, b = blockIdx.x / (nbands * ntiles);
    const int y0 = band * R, y1 = min(y0 + R, H);
    const int x0 = tile * tw, x1 = min(x0 + tw, W), nx = x1 - x0;
    const int r0 = vb[2 * y0], c0 = hb[2 * x0];
    const int sb = (hb[2 * (x1 - 1)] + hb[2 * (x1 - 1) + 1] - c0) * C;   // source bytes of one row the tile reads
    const int nch = (sb + 30) / 16;                                       // 16-byte chunks of a staged row, any offset
    const int rowb = nx * C;                                              // bytes of one intermediate row
    // the host's bounds on rows and columns make the min a no-op; it keeps every LDS write in bounds whatever the tables say
    const int nr = min(vb[2 * (y1 - 1)] + vb[2 * (y1 - 1) + 1] - r0, min(kResampleInter / rowb, kResampleStage / (16 * nch)));
    const size_t pitch = (size_t)Ws * C;
    const unsigned char* rows = src + ((size_t)b * Hs + top + r0) * pitch + (size_t)(left + c0) * C;
    for (int i = threadIdx.x; i < nr * nch; i += blockDim.x) {
        const int r = i / nch, k = i - r * nch;
        const uintptr_t p = (uintptr_t)(rows + r * pitch);
        if (16 * k < (int)(p & 15) + sb) stage4[i] = *(const uint4*)((p & ~(uintptr_t)15) + 16 * (uintptr_t)k);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nr * rowb; i += blockDim.x) {
        const int r = i / rowb, rem = i - r * rowb;
        const int xo = x0 + rem / C, c = rem % C;
        const int first = hb[2 * xo] - c0, n = hb[2 * xo + 1];
        const int off = (int)((uintptr_t)(rows + r * pitch) & 15);
        const unsigned char* q = stage + r * 16 * nch + off + first * C + c;
        const int* w = hw + (size_t)xo * kh;
        int acc = 1 << (kPilBits - 1);
        for (int t = 0; t < n; ++t) acc += (int)q[t * C] * w[t];
        inter[i] = pil_clip8(acc);
    }
    __syncthreads();
    const int ny = y1 - y0;
    for (int i = threadIdx.x; i < C * ny * nx; i += blockDim.x) {
        const int x = i % nx, yc = i / nx;
        const int yl = yc % ny, c = yc / ny;
        const int y = y0 + yl;
        const int first = vb[2 * y] - r0, n = vb[2 * y + 1];
        const int* w = vw + (size_t)y * kv;
        int acc = 1 << (kPilBits - 1);
        for (int t = 0; t < n; ++t) {
            const int r = first + t;
            if (r < nr) acc += (int)inter[r * rowb + x * C + c] * w[t];
        }
        dst[(((size_t)b * C + c) * H + y) * W + x0 + x] = (float)pil_clip8(acc) / 255.0f;
    }
}

// Instance label maps: int [B, Hs, Ws] -> int64 [B, 1, H, W], nearest inside the crop window with F.interpolate's index
// rule.  The reference moves labels through fp32 (FloatTensor, F.interpolate, .long()); that round trip is the identity on
// every value an fp32 holds exactly, which this copy is.
// s = min(floor(d * scale), in - 1) with scale = in / out in fp32: the source index of output index d on one axis.
__device__ __forceinline__ int nearest_src_index(int d, float scale, int in) {
    const int s = (int)floorf((float)d * scale);
    return s < in - 1 ? s : in - 1;
}

template <typename T>
__global__ void __launch_bounds__(256)
labels_crop_nearest_kernel(const T* __restrict__ src, long long* __restrict__ dst, int B, int Hs, int Ws, int top, int left,
                           int Hc, int Wc, int H, int W) {
    const size_t total = (size_t)B * H * W;
    const float sh = (float)Hc / (float)H, sw = (float)Wc / (float)W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int b = (int)(i / ((size_t)W * H));
        const int sy = nearest_src_index(y, sh, Hc), sx = nearest_src_index(x, sw, Wc);
        dst[i] = (long long)src[((size_t)b * Hs + top + sy) * Ws + left + sx];
    }
}

// Entity-mask stacks -> instance maps (datasets/multi_object_config.py:188-203): the reference writes o + 1 wherever
// mask[o] == 255, for o = background_entities .. E - 1 in order, so the highest such o wins; 0 where there is none.  Fused
// with the crop window and the nearest resample of the kernel above (the same index rule), int64 out.  Byte (b, o, y, x) sits
// at b * E * Hs * Ws + o * es + (y * Ws + x) * ps: [E, Hs, Ws] stacks (es = Hs * Ws, ps = 1) and [Hs, Ws, E] stacks (es = 1,
// ps = E: Multi-dSprites, which the reference transposes on the host) are read in place.  Entities are visited from the top
// down and a pixel stops at its first hit.  Lanes walk x: planar stacks read a plane's row contiguously, interleaved ones
// read E adjacent bytes a lane, so the wave's lines are fully used over the entity loop.
__global__ void __launch_bounds__(256)
entity_masks_to_labels_kernel(const unsigned char* __restrict__ masks, long long* __restrict__ dst, int B, int E, int Hs, int Ws,
                              long long es, long long ps, int bg, int top, int left, int Hc, int Wc, int H, int W) {
    const size_t total = (size_t)B * H * W;
    const float sh = (float)Hc / (float)H, sw = (float)Wc / (float)W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int b = (int)(i / ((size_t)W * H));
        const int sy = nearest_src_index(y, sh, Hc), sx = nearest_src_index(x, sw, Wc);
        const unsigned char* p = masks + (size_t)b * E * Hs * Ws + ((size_t)(top + sy) * Ws + left + sx) * (size_t)ps;
        int label = 0;
        for (int o = E - 1; o >= bg; --o)
            if (p[(size_t)o * (size_t)es] == 255) {
                label = o + 1;
                break;
            }
        dst[i] = (long long)label;
    }
}

// The same map of a planar stack without a resample (H = Hc, W = Wc), 16 pixels of a row a thread: one aligned 16-byte load
// per entity plane (a wave reads 1 KB of a plane's rows per instruction) and eight 16-byte stores.  The host takes this path
// only when every row segment starts on a 16-byte boundary: both bases, Hs * Ws, Ws, left and Wc all multiples of 16.
__global__ void __launch_bounds__(256)
entity_masks_to_labels_rows16_kernel(const unsigned char* __restrict__ masks, long long* __restrict__ dst, int B, int E, int Hs,
                                     int Ws, int bg, int top, int left, int H, int W) {
    const int wq = W / 16;
    const size_t total = (size_t)B * H * wq, plane = (size_t)Hs * Ws;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xq = (int)(i % wq);
        const int y = (int)((i / wq) % H);
        const int b = (int)(i / ((size_t)wq * H));
        const unsigned char* p = masks + (size_t)b * E * plane + (size_t)(top + y) * Ws + left + 16 * xq;
        unsigned char lab[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) lab[j] = 0;
        for (int o = bg; o < E; ++o) {                 // ascending, the later entity overwrites: the reference's order
            const uint4 v = *(const uint4*)(p + (size_t)o * plane);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == 255u) lab[j] = (unsigned char)(o + 1);
        }
        longlong2* q = (longlong2*)(dst + ((size_t)b * H + y) * W + 16 * xq);
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = make_longlong2((long long)lab[2 * j], (long long)lab[2 * j + 1]);
    }
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter (support 1), in double on the host.  Kept out of
// FMA contraction so that the doubles are the ones Pillow's own build computes.
int pil_bilinear_ksize(int in, int out) {
    double filterscale = (double)in / out;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(1.0 * filterscale) * 2 + 1;
}

void pil_bilinear_coeffs(int in, int out, int ksize, int* bounds, int* weights, double* k) {
#pragma clang fp contract(off)
    const double scale = (double)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            const double w = t < 1.0 ? 1.0 - t : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < ksize; ++x) {
            double v = x < xmax ? k[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            weights[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << kPilBits)) : (int)(0.5 + v * (1 << kPilBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// Upper bound on the source rows a band of R output rows spans: first tap >= c0 - support - 0.5, last tap + 1 <=
// c1 + support + 0.5 with c1 - c0 = (R - 1) * scale.
int pil_band_rows(int in, int out, int R) {
    const double scale = (double)in / out, support = scale < 1.0 ? 1.0 : scale;
    const int b = (int)floor((R - 1) * scale + 2.0 * support) + 2;
    return b < in ? b : in;
}

}  // namespace

extern "C" {

int gx_u8hwc_to_f32chw(const unsigned char* src, float* dst, int B, int Hs, int Ws, int C, int H, int W,
                       gx_stream_t stream) {
    GX_CHECK_ARG(src && dst, "gx_u8hwc_to_f32chw: null pointer");
    GX_CHECK_ARG(B > 0 && Hs > 0 && Ws > 0 && C > 0 && H > 0 && W > 0, "gx_u8hwc_to_f32chw: bad dims");
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)B * C * H * W;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * Hs * Ws * C + 4.0 * total);
        hipLaunchKernelGGL(u8hwc_to_f32chw_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, B, Hs, Ws, C, H, W);
    }
    GX_CHECK_LAUNCH("gx_u8hwc_to_f32chw");
    return GX_OK;
}

}  // extern "C"

int gx_pil_band_rows(int in, int out, int R) { return pil_band_rows(in, out, R); }      // gx_common.h: for gx_imagefile.hip

extern "C" {

int gx_pil_bilinear_ksize(int in, int out) {
    if (in <= 0 || out <= 0) return 0;
    return pil_bilinear_ksize(in, out);
}

int gx_pil_bilinear_coeffs(int in, int out, int ksize, int* bounds, int* weights) {
    GX_CHECK_ARG(bounds && weights, "gx_pil_bilinear_coeffs: null pointer");
    GX_CHECK_ARG(in > 0 && out > 0, "gx_pil_bilinear_coeffs: bad sizes (in %d, out %d)", in, out);
    GX_CHECK_ARG(ksize == pil_bilinear_ksize(in, out), "gx_pil_bilinear_coeffs: ksize %d, expected gx_pil_bilinear_ksize() = %d",
                 ksize, pil_bilinear_ksize(in, out));
    std::vector<double> k((size_t)ksize);
    pil_bilinear_coeffs(in, out, ksize, bounds, weights, k.data());
    return GX_OK;
}

int gx_u8hwc_resample_f32chw(const unsigned char* src, float* dst, int B, int Hs, int Ws, int C, int top, int left, int Hc,
                             int Wc, int H, int W, int mode, const int* hbounds, const int* hweights, int hksize,
                             const int* vbounds, const int* vweights, int vksize, gx_stream_t stream) {
    GX_CHECK_ARG(src && dst, "gx_u8hwc_resample_f32chw: null pointer");
    GX_CHECK_ARG(B > 0 && Hs > 0 && Ws > 0 && C > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0, "gx_u8hwc_resample_f32chw: bad dims");
    GX_CHECK_ARG(top >= 0 && left >= 0 && top + Hc <= Hs && left + Wc <= Ws,
                 "gx_u8hwc_resample_f32chw: crop window (%d, %d, %d, %d) outside the %d x %d frame", top, left, Hc, Wc, Hs, Ws);
    GX_CHECK_ARG(mode == GX_RESAMPLE_NEAREST || mode == GX_RESAMPLE_PIL_BILINEAR, "gx_u8hwc_resample_f32chw: bad mode %d", mode);
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)B * C * H * W;
    if (mode == GX_RESAMPLE_NEAREST) {
        size_t blocks = (total + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * Hc * Wc * C + 4.0 * total);
        hipLaunchKernelGGL(u8hwc_crop_nearest_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, B, Hs, Ws, C, top,
                           left, Hc, Wc, H, W);
    } else {
        GX_CHECK_ARG(hbounds && hweights && vbounds && vweights, "gx_u8hwc_resample_f32chw: bilinear needs the coefficient tables");
        GX_CHECK_ARG(hksize == pil_bilinear_ksize(Wc, W) && vksize == pil_bilinear_ksize(Hc, H),
                     "gx_u8hwc_resample_f32chw: table ksize (%d, %d) is not that of %d -> %d, %d -> %d", hksize, vksize, Wc, W, Hc, H);
        // column tile: at most 768 intermediate bytes a row; band: up to 8 output rows.  Both shrink (the band first) until
        // the bounds on the band's source rows and the tile's source columns fit the staging and intermediate buffers.
        auto fits = [&](int R, int tw) {
            const size_t rows = (size_t)pil_band_rows(Hc, H, R), cols = (size_t)pil_band_rows(Wc, W, tw);
            return rows * tw * C <= (size_t)kResampleInter && rows * ((cols * C + 30) / 16) * 16 <= (size_t)kResampleStage;
        };
        int tw = W, R = 8;
        while (tw > 1 && tw * C > 768) tw = (tw + 1) / 2;
        while (!fits(R, tw) && (R > 1 || tw > 1)) {
            if (R > 1) --R;
            else tw = (tw + 1) / 2;
        }
        GX_CHECK_ARG(fits(R, tw), "gx_u8hwc_resample_f32chw: %d x %d -> %d x %d with %d channels exceeds the kernel's band buffers",
                     Hc, Wc, H, W, C);
        const int nbands = gx_ceil_div(H, R), ntiles = gx_ceil_div(W, tw);
        GX_CHECK_ARG((size_t)nbands * ntiles * B < (1u << 31), "gx_u8hwc_resample_f32chw: grid too large");
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * Hc * Wc * C + 4.0 * total);
        hipLaunchKernelGGL(u8hwc_pil_bilinear_kernel, dim3((unsigned)(nbands * ntiles * B)), dim3(256), 0, s, src, dst, Hs, Ws,
                           C, top, left, H, W, R, tw, nbands, ntiles, hbounds, hweights, hksize, vbounds, vweights, vksize);
    }
    GX_CHECK_LAUNCH("gx_u8hwc_resample_f32chw");
    return GX_OK;
}

int gx_labels_crop_nearest(const void* src, int dtype, long long* dst, int B, int Hs, int Ws, int top, int left, int Hc, int Wc,
                           int H, int W, gx_stream_t stream) {
    GX_CHECK_ARG(src && dst, "gx_labels_crop_nearest: null pointer");
    GX_CHECK_ARG(B > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0, "gx_labels_crop_nearest: bad dims");
    GX_CHECK_ARG(top >= 0 && left >= 0 && top + Hc <= Hs && left + Wc <= Ws,
                 "gx_labels_crop_nearest: crop window (%d, %d, %d, %d) outside the %d x %d frame", top, left, Hc, Wc, Hs, Ws);
    GX_CHECK_ARG(dtype == GX_LABEL_U8 || dtype == GX_LABEL_I32 || dtype == GX_LABEL_I64, "gx_labels_crop_nearest: bad dtype %d",
                 dtype);
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)B * H * W;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const int esz = dtype == GX_LABEL_U8 ? 1 : (dtype == GX_LABEL_I32 ? 4 : 8);
    GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * Hc * Wc * esz + 8.0 * total);
    if (dtype == GX_LABEL_U8)
        hipLaunchKernelGGL(labels_crop_nearest_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, s,
                           (const unsigned char*)src, dst, B, Hs, Ws, top, left, Hc, Wc, H, W);
    else if (dtype == GX_LABEL_I32)
        hipLaunchKernelGGL(labels_crop_nearest_kernel<int>, dim3((unsigned)blocks), dim3(256), 0, s, (const int*)src, dst, B,
                           Hs, Ws, top, left, Hc, Wc, H, W);
    else
        hipLaunchKernelGGL(labels_crop_nearest_kernel<long long>, dim3((unsigned)blocks), dim3(256), 0, s,
                           (const long long*)src, dst, B, Hs, Ws, top, left, Hc, Wc, H, W);
    GX_CHECK_LAUNCH("gx_labels_crop_nearest");
    return GX_OK;
}

int gx_entity_masks_to_labels(const unsigned char* masks, long long* dst, int B, int E, int Hs, int Ws, long long entity_stride,
                              long long pixel_stride, int background_entities, int top, int left, int Hc, int Wc, int H, int W,
                              gx_stream_t stream) {
    GX_CHECK_ARG(masks && dst, "gx_entity_masks_to_labels: null pointer");
    GX_CHECK_ARG(B > 0 && E > 0 && E < 255 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0,
                 "gx_entity_masks_to_labels: bad dims");
    GX_CHECK_ARG(top >= 0 && left >= 0 && top + Hc <= Hs && left + Wc <= Ws,
                 "gx_entity_masks_to_labels: crop window (%d, %d, %d, %d) outside the %d x %d frame", top, left, Hc, Wc, Hs, Ws);
    GX_CHECK_ARG(background_entities >= 0, "gx_entity_masks_to_labels: bad background_entities %d", background_entities);
    const long long plane = (long long)Hs * Ws;
    GX_CHECK_ARG(entity_stride > 0 && pixel_stride > 0 && entity_stride <= (long long)E * plane && pixel_stride <= (long long)E * plane &&
                     (E - 1) * entity_stride + (plane - 1) * pixel_stride < (long long)E * plane,
                 "gx_entity_masks_to_labels: entity stride %lld and pixel stride %lld reach outside a frame's %d x %d x %d bytes",
                 entity_stride, pixel_stride, E, Hs, Ws);
    hipStream_t s = (hipStream_t)stream;
    const bool planar = entity_stride == plane && pixel_stride == 1;
    const bool rows16 = planar && H == Hc && W == Wc && ((uintptr_t)masks % 16) == 0 && ((uintptr_t)dst % 16) == 0 && plane % 16 == 0 && Ws % 16 == 0 &&
                        left % 16 == 0 && Wc % 16 == 0;
    const size_t total = rows16 ? (size_t)B * H * (W / 16) : (size_t)B * H * W;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const int ne = E > background_entities ? E - background_entities : 0;
    GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * Hc * Wc * ne + 8.0 * B * H * W);
    if (rows16)
        hipLaunchKernelGGL(entity_masks_to_labels_rows16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, masks, dst, B, E, Hs, Ws,
                           background_entities, top, left, H, W);
    else
        hipLaunchKernelGGL(entity_masks_to_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, s, masks, dst, B, E, Hs, Ws,
                           entity_stride, pixel_stride, background_entities, top, left, Hc, Wc, H, W);
    GX_CHECK_LAUNCH("gx_entity_masks_to_labels");
    return GX_OK;
}

}  // extern "C"
