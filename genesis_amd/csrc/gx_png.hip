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

namespace {

constexpr int kMaxDim = kGxPngMaxDim;  // W and H (gx_common.h): carry[] below is kMaxDim * C bytes of LDS
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kAhead = 8;              // steps whose filtered bytes are in flight

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);         // ties: a, then b, then c
}

__device__ __forceinline__ unsigned char plane_value(int v, int rule) {
    if (rule == 1)      // third_party/shapestacks/segmentation_utils.py:38-41 + .long(): imread's float in [0, 1], / 32, truncated
        return (unsigned char)(int)(((float)v / 255.0f) / 32.0f);
    return (unsigned char)(rule == 2 ? (v >> 5) : v);
}

template <int C>
__global__ void __launch_bounds__(kThreads) png_unfilter_kernel(const unsigned char* __restrict__ filtered,
                                                                unsigned char* __restrict__ dst_u8,
                                                                unsigned char* __restrict__ dst_plane0, int plane_rule, int H, int W) {
    constexpr int kBand = kThreads / C;
    __shared__ unsigned char carry[kMaxDim * C];          // the last row of the previous band
    __shared__ unsigned char edge[2][kWaves][4];          // the last C lanes of every wave, of the step before
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid / C, ch = tid - r * C;
    const size_t stride = 1 + (size_t)W * C;
    const unsigned char* src = filtered + (size_t)blockIdx.x * H * stride;
    unsigned char* out = dst_u8 ? dst_u8 + (size_t)blockIdx.x * H * W * C : nullptr;
    unsigned char* plane = dst_plane0 ? dst_plane0 + (size_t)blockIdx.x * H * W : nullptr;

    for (int row0 = 0; row0 < H; row0 += kBand) {
        const int rows = min(kBand, H - row0);
        const bool mine = r < rows;
        const int row = row0 + r;
        const unsigned char* line = src + (size_t)(mine ? row : 0) * stride;
        const int filter = mine ? line[0] : 0;
        const unsigned char* raw = line + 1 + ch;
        int a = 0, b_prev = 0, cur = 0;
        const int steps = W + rows - 1;
        int ahead[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead; ++j) {
            const int x = j - r;
            ahead[j] = (mine && x >= 0 && x < W) ? raw[x * C] : 0;
        }
        for (int t0 = 0; t0 < steps; t0 += kAhead) {
            int now[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) now[j] = ahead[j];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {                 // the next chunk's bytes: in flight during this chunk's steps
                const int x = t0 + kAhead + j - r;
                ahead[j] = (mine && x >= 0 && x < W) ? raw[x * C] : 0;
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const int t = t0 + j;
                if (t < steps) {                               // uniform over the workgroup
                    const int x = t - r;
                    int b = __shfl_up(cur, C, 64);             // thread (r - 1, ch)'s value of step t - 1: (row - 1, x)
                    if (lane < C && wave > 0) b = edge[(t + 1) & 1][wave - 1][lane];
                    const bool on = mine && x >= 0 && x < W;
                    if (on) {
                        if (r == 0) b = row0 ? carry[x * C + ch] : 0;
                        const int c = x ? b_prev : 0;
                        const int left = x ? a : 0;
                        int pred = 0;
                        if (filter == 1) pred = left;
                        else if (filter == 2) pred = b;
                        else if (filter == 3) pred = (left + b) >> 1;
                        else if (filter == 4) pred = paeth(left, b, c);
                        cur = (now[j] + pred) & 255;
                        a = cur;
                        b_prev = b;
                        if (out) out[((size_t)row * W + x) * C + ch] = (unsigned char)cur;
                        if (plane && ch == 0) plane[(size_t)row * W + x] = plane_value(cur, plane_rule);
                    }
                    if (lane >= 64 - C) edge[t & 1][wave][lane - (64 - C)] = (unsigned char)cur;
                    // the row this band hands to the next one; column x of it is read (by row 0, at step x) before it is
                    // rewritten (by the last row, at step x + rows - 1), with this barrier in between
                    if (on && r == rows - 1 && row0 + rows < H) carry[x * C + ch] = (unsigned char)cur;
                    __syncthreads();
                }
            }
        }
    }
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
