// The pixel arithmetic of baseline JPEG decoding (libjpeg's default path, include/genesis_hip.h), shared by the two kernels that
// decode: gx_jpeg.hip (one workgroup per frame, planes in LDS) and gx_imagefile.hip (frames of any size, planes in global memory).
// One definition, so that the two cannot drift apart.  Device code only.
#pragma once

namespace {

// One 8-point pass.  Unsigned arithmetic: a valid stream stays far inside 32 bits, a hostile one wraps instead of
// overflowing a signed int.
__device__ __forceinline__ void idct8(int (&v)[8], int shift) {
    typedef unsigned int u32;
    const u32 v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5], v6 = v[6], v7 = v[7];
    u32 z1 = (v2 + v6) * 4433u;
    const u32 t2 = z1 - v6 * 15137u, t3 = z1 + v2 * 6270u;
    const u32 t0 = (v0 + v4) << 13, t1 = (v0 - v4) << 13;
    const u32 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    u32 a = v7, b = v5, c = v3, d = v1;
    z1 = a + d;
    u32 z2 = b + c, z3 = a + c, z4 = b + d;
    const u32 z5 = (z3 + z4) * 9633u;
    a *= 2446u;
    b *= 16819u;
    c *= 25172u;
    d *= 12299u;
    z1 *= (u32)-7373;
    z2 *= (u32)-20995;
    z3 = z3 * (u32)-16069 + z5;
    z4 = z4 * (u32)-3196 + z5;
    a += z1 + z3;
    b += z2 + z4;
    c += z2 + z3;
    d += z1 + z4;
    const u32 r = 1u << (shift - 1);
    v[0] = (int)(t10 + d + r) >> shift;
    v[1] = (int)(t11 + c + r) >> shift;
    v[2] = (int)(t12 + b + r) >> shift;
    v[3] = (int)(t13 + a + r) >> shift;
    v[4] = (int)(t13 - a + r) >> shift;
    v[5] = (int)(t12 - b + r) >> shift;
    v[6] = (int)(t11 - c + r) >> shift;
    v[7] = (int)(t10 - d + r) >> shift;
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The chroma sample of stored pixel (y, x): the plane's own sample (4:4:4), or the triangle-filter upsampling of h2v1 /
// h2v2.  A neighbour outside the plane's real extent cw x ch is the edge sample itself, never the MCU padding.
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pitch, int cw, int ch, int sampling, int y, int x) {
    if (sampling == 0) return p[y * pitch + x];
    const int i = x >> 1;
    if (sampling == 1) {
        const unsigned char* r = p + y * pitch;
        const int c = r[i];
        if (x & 1) return i == cw - 1 ? c : (3 * c + r[i + 1] + 2) >> 2;
        return i == 0 ? c : (3 * c + r[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    const int fr = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
    const unsigned char* near = p + r * pitch;
    const unsigned char* far = p + fr * pitch;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

// libjpeg's 16-bit fixed-point YCbCr -> RGB; cb and cr already minus 128
__device__ __forceinline__ void ycc_to_rgb(int yy, int cb, int cr, int* r, int* g, int* b) {
    *r = clamp8(yy + ((91881 * cr + 32768) >> 16));
    *b = clamp8(yy + ((116130 * cb + 32768) >> 16));
    *g = clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
}

}  // namespace
