// Device half of the PNG decoder (genesis_amd/png.py): undoes the five scanline filters of a batch of inflated frames
// (gx_png.cpp: gx_png_inflate) in ONE launch.
//
// Byte (r, x) of a frame depends on (r, x - C), (r - 1, x) and (r - 1, x - C); Average and Paeth are not associative, so a
// row is serial in x and the rows are serial in r.  What is parallel is the skewed wavefront and the C byte lanes of a
// pixel: one workgroup per frame, thread (r, c) = one (row, channel byte) of a BAND of kThreads / C rows, and at step t
// thread (r, c) reconstructs pixel column t - r.  Its three neighbours are then
//   a  its own value of the step before (a register),
//   b  the value thread (r - 1, c) -- C lanes down -- produced the step before: one cross-lane move inside a wave, and
//      across a wave boundary C bytes through LDS (double-buffered, so ONE barrier per step),
//   c  the b of its own step before (a register).
// A band takes W + rows - 1 steps.  Frames taller than a band run band after band; the last row of a band is handed to the
// next one through one row of LDS (W * C <= 16 KB: the kMaxDim bound), so dst_u8 may be NULL.  The frame itself stays
// in global / L2-resident memory: the filtered bytes of the next kAhead steps are loaded a chunk ahead of their use.
#include "gx_common.h"
#include "gx_png_unfilter.h"      // the reconstruction of one frame: shared with gx_imagefile.hip

namespace {

constexpr int kMaxDim = kGxPngMaxDim;  // W and H (gx_common.h): carry[] below is kMaxDim * C bytes of LDS
constexpr int kThreads = kPngThreads;
constexpr int kWaves = kPngWaves;

template <int C>
__global__ void __launch_bounds__(kThreads) png_unfilter_kernel(const unsigned char* __restrict__ filtered,
                                                                unsigned char* __restrict__ dst_u8,
                                                                unsigned char* __restrict__ dst_plane0, int plane_rule, int H, int W) {
    __shared__ unsigned char carry[kMaxDim * C];          // the last row of the previous band
    __shared__ unsigned char edge[2][kWaves][4];          // the last C lanes of every wave, of the step before
    const size_t stride = 1 + (size_t)W * C;
    png_unfilter_frame<C>(filtered + (size_t)blockIdx.x * H * stride, dst_u8 ? dst_u8 + (size_t)blockIdx.x * H * W * C : nullptr,
                          dst_plane0 ? dst_plane0 + (size_t)blockIdx.x * H * W : nullptr, plane_rule, H, W, carry, edge);
}

}  // namespace

extern "C" {

int gx_png_unfilter(const unsigned char* filtered, unsigned char* dst_u8, unsigned char* dst_plane0, int plane_rule, int B, int H,
                    int W, int C, gx_stream_t stream) {
    GX_CHECK_ARG(filtered, "gx_png_unfilter: null pointer");
    GX_CHECK_ARG(dst_u8 || dst_plane0, "gx_png_unfilter: no output (dst_u8 and dst_plane0 are both null)");
    GX_CHECK_ARG(B > 0 && H > 0 && W > 0, "gx_png_unfilter: bad dims");
    GX_CHECK_ARG(H <= kMaxDim && W <= kMaxDim, "gx_png_unfilter: a %d x %d frame is larger than the %d x %d the kernel takes", W, H,
                 kMaxDim, kMaxDim);
    GX_CHECK_ARG(C == 1 || C == 3 || C == 4, "gx_png_unfilter: C must be 1, 3 or 4, not %d", C);
    GX_CHECK_ARG(plane_rule >= 0 && plane_rule <= 2, "gx_png_unfilter: bad plane rule %d", plane_rule);
    hipStream_t s = (hipStream_t)stream;
    const int rows = H < kThreads / C ? H : kThreads / C;
    const dim3 block((unsigned)gx_round_up(rows * C, 64));
    {
        GxProf pf(KID_SMALL_REDUCE, s, 0.0, (double)B * H * ((1.0 + (double)W * C) + (dst_u8 ? (double)W * C : 0.0) + (dst_plane0 ? W : 0.0)));
        if (C == 1)
            hipLaunchKernelGGL(png_unfilter_kernel<1>, dim3((unsigned)B), block, 0, s, filtered, dst_u8, dst_plane0, plane_rule, H, W);
        else if (C == 3)
            hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3((unsigned)B), block, 0, s, filtered, dst_u8, dst_plane0, plane_rule, H, W);
        else
            hipLaunchKernelGGL(png_unfilter_kernel<4>, dim3((unsigned)B), block, 0, s, filtered, dst_u8, dst_plane0, plane_rule, H, W);
    }
    GX_CHECK_LAUNCH("gx_png_unfilter");
    return GX_OK;
}

}  // extern "C"
