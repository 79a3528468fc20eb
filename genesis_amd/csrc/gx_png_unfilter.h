// The skewed-wavefront reconstruction of ONE inflated PNG frame by one workgroup (the method: gx_png.hip), shared by
// gx_png_unfilter (one geometry per launch, gx_png.hip) and gx_png_unfilter_ragged (a geometry per frame, gx_imagefile.hip).
// One definition, so that the two cannot drift apart.  Device code only.
#pragma once

namespace {

constexpr int kPngThreads = 1024;
constexpr int kPngWaves = kPngThreads / 64;
constexpr int kPngAhead = 8;              // steps whose filtered bytes are in flight

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

// src: the frame's H * (1 + W * C) filtered bytes; out [H, W, C] and / or plane [H, W] (either may be null); carry: W * C bytes of
// LDS (the last row of the previous band); edge: the last C lanes of every wave, of the step before.  Every thread of the
// workgroup calls it (barriers inside), whatever the block size up to kPngThreads.
template <int C>
__device__ __forceinline__ void png_unfilter_frame(const unsigned char* __restrict__ src, unsigned char* __restrict__ out,
                                                   unsigned char* __restrict__ plane, int plane_rule, int H, int W,
                                                   unsigned char* carry, unsigned char (*edge)[kPngWaves][4]) {
    constexpr int kBand = kPngThreads / C;
    constexpr int kAhead = kPngAhead;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid / C, ch = tid - r * C;
    const size_t stride = 1 + (size_t)W * C;

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
