// FID on the device (genesis_amd/fid.py): the forward pass of pytorch_fid's "FID Inception" (torchvision's Inception-v3
// with the FID patches, BatchNorm folded into the conv weights on the host) and the streaming fp64 moments of its features.
//   gx_fid_preprocess      the reference's PNG round trip (uint8(255 x) / 255) + bilinear 299 x 299 + 2x - 1, NCHW -> NHWC
//   gx_fid_conv_bias_relu  implicit-GEMM conv forward on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32: exact fp32
//                          products), NHWC, any kh, kw, stride and padding; up to three destinations along N (stacked
//                          sibling convs), each a channel slice of its own tensor
//   gx_fid_pool            3 x 3 max-pool (s2 valid / s1 p1), 3 x 3 avg-pool s1 p1 (count_include_pad=False), global average
//   gx_fid_moments         sum f and sum f f^T over a batch, added into fp64 buffers
// Every output element is reduced in an order fixed by the layer's shape alone (no split-K, no atomics, no choice made
// from the batch size): an image's features, and the moments, are bit-identical whatever batch they are computed in.
#include "gx_common.h"

#include <limits.h>

namespace {

constexpr int kFidSide = 299;

// ---- preprocess ---------------------------------------------------------------------------------------------------
// np.uint8(255 * x) (float32 product, truncated; clamped first) then float32(u8) / 255; quantise == 0: x as is
__device__ __forceinline__ float fid_quant(float x, int quantise) {
    if (!quantise) return x;
    float v = __fmul_rn(255.f, x);
    v = fminf(fmaxf(v, 0.f), 255.f);          // (NaN -> 0)
    return __fdiv_rn((float)(int)v, 255.f);
}

// torch's CPU upsample_bilinear2d index / weight rule (align_corners=False; ATen/native/UpSample.h), in float and with
// the contractions its x86 FMA builds make (measured bit-exact against them: tests/test_fid_gpu.py):
// src = max(fma(scale, i + 0.5, -0.5), 0); i0 = min(floor(src), in - 1); l1 = clamp(src - i0, 0, 1); l0 = 1 - l1
__device__ __forceinline__ void fid_src_index(int i, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
    if (in == kFidSide) {            // (torch copies when the sizes agree)
        i0 = i1 = i; l0 = 1.f; l1 = 0.f;
        return;
    }
    float r = __fmaf_rn(scale, __fadd_rn((float)i, 0.5f), -0.5f);
    if (r < 0.f) r = 0.f;
    i0 = min((int)floorf(r), in - 1);
    l1 = fminf(fmaxf(__fsub_rn(r, (float)i0), 0.f), 1.f);
    l0 = __fsub_rn(1.f, l1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// a w_a + b w_b as torch's two-tap Interpolate computes it: fma(a, w_a, b * w_b)
__device__ __forceinline__ float fid_lerp(float a, float wa, float b, float wb) {
    return __fmaf_rn(a, wa, __fmul_rn(b, wb));
}

__global__ void __launch_bounds__(256)
fid_preprocess_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int quantise, float sh,
                      float sw) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= B * kFidSide * kFidSide) return;
    const int ow = p % kFidSide, oh = (p / kFidSide) % kFidSide, b = p / (kFidSide * kFidSide);
    int h0, h1, w0, w1;
    float lh0, lh1, lw0, lw1;
    fid_src_index(oh, H, sh, h0, h1, lh0, lh1);
    fid_src_index(ow, W, sw, w0, w1, lw0, lw1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* pl = x + ((size_t)b * 3 + c) * H * W;
        const float v00 = fid_quant(pl[(size_t)h0 * W + w0], quantise), v01 = fid_quant(pl[(size_t)h0 * W + w1], quantise);
        const float v10 = fid_quant(pl[(size_t)h1 * W + w0], quantise), v11 = fid_quant(pl[(size_t)h1 * W + w1], quantise);
        // along width inside each source row, then along height
        const float v = fid_lerp(fid_lerp(v00, lw0, v01, lw1), lh0, fid_lerp(v10, lw0, v11, lw1), lh1);
        y[(size_t)p * 3 + c] = __fsub_rn(__fmul_rn(2.f, v), 1.f);
    }
}

// ---- implicit-GEMM convolution --------------------------------------------------------------------------------------
// C[m][n] = sum_k A[m][k] B[k][n]: m = (image, oh, ow), n = output channel, k = (r, s, c) with c fastest (NHWC: a k chunk of
// 16 lies inside one tap when Cin % 16 == 0).  Workgroup tile 128 x 64, four waves of 64 x 32 (4 x 2 MFMA tiles of
// 16 x 16); k chunks of 16 staged in LDS, the next chunk's global loads in flight during the current chunk's MFMAs.
// The MFMA's k slot g of step q holds k = 4 g + q, so a lane reads its A and B values of a chunk as one 16-byte LDS word.
constexpr int kBM = 128, kBN = 64, kBK = 16, kLS = 20;   // LDS row stride (floats): 80 bytes keeps 16-byte alignment

struct FidDst { float* p; int ctot, c0, n; };

template <bool VEC>
__global__ void __launch_bounds__(256)
fid_conv_kernel(const float* __restrict__ x, int H, int W, int Cin, const float* __restrict__ wp,
                const float* __restrict__ bias, int N, int K, int Kpad, int kw, int st, int ph, int pw, int Ho, int Wo,
                int M, FidDst d0, FidDst d1, FidDst d2) {
    __shared__ __attribute__((aligned(16))) float As[kBM * kLS];
    __shared__ __attribute__((aligned(16))) float Bs[kBN * kLS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
    const int kq = (t & 3) * 4;
    int ihb[2], iwb[2];
    size_t xb[2];
    bool ok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + (t >> 2) + 64 * i;
        ok[i] = m < M;
        const int mm = ok[i] ? m : 0;
        const int ow = mm % Wo, q = mm / Wo, oh = q % Ho, n = q / Ho;
        ihb[i] = oh * st - ph;
        iwb[i] = ow * st - pw;
        xb[i] = (size_t)n * H * W * Cin;
    }
    const float* wrow = wp + (size_t)(n0 + (t >> 2)) * Kpad + kq;    // weights [Npad][Kpad], zero-padded
    f32x4 ra[2], rb;
    auto load = [&](int kc) {
        rb = *reinterpret_cast<const f32x4*>(wrow + kc);
        if (VEC) {
            const int rs = kc / Cin, c = kc - rs * Cin + kq, r = rs / kw, s = rs - r * kw;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ih = ihb[i] + r, iw = iwb[i] + s;
                if (ok[i] && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                    ra[i] = *reinterpret_cast<const f32x4*>(x + xb[i] + ((size_t)ih * W + iw) * Cin + c);
                else
                    ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kk = kc + kq + j;
                    float v = 0.f;
                    if (ok[i] && kk < K) {
                        const int rs = kk / Cin, c = kk - rs * Cin, r = rs / kw, s = rs - r * kw;
                        const int ih = ihb[i] + r, iw = iwb[i] + s;
                        if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                            v = x[xb[i] + ((size_t)ih * W + iw) * Cin + c];
                    }
                    ra[i][j] = v;
                }
        }
    };
    f32x4 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = wv & 1, wn = wv >> 1, li = lane & 15, g = lane >> 4;
    load(0);
    for (int kc = 0; kc < Kpad; kc += kBK) {
        __syncthreads();
        *reinterpret_cast<f32x4*>(&As[(t >> 2) * kLS + kq]) = ra[0];
        *reinterpret_cast<f32x4*>(&As[((t >> 2) + 64) * kLS + kq]) = ra[1];
        *reinterpret_cast<f32x4*>(&Bs[(t >> 2) * kLS + kq]) = rb;
        __syncthreads();
        if (kc + kBK < Kpad) load(kc + kBK);
        f32x4 av[4], bv[2];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = *reinterpret_cast<const f32x4*>(&As[(wm * 64 + a * 16 + li) * kLS + 4 * g]);
#pragma unroll
        for (int b = 0; b < 2; ++b) bv[b] = *reinterpret_cast<const f32x4*>(&Bs[(wn * 32 + b * 16 + li) * kLS + 4 * g]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a][q], bv[b][q], acc[a][b], 0, 0, 0);
    }
    // epilogue: C/D map of the 16 x 16 form: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int n = n0 + wn * 32 + b * 16 + li;
        if (n >= N) continue;
        const FidDst& d = n < d0.n ? d0 : (n < d0.n + d1.n ? d1 : d2);
        const int nc = n < d0.n ? n : (n < d0.n + d1.n ? n - d0.n : n - d0.n - d1.n);
        const float bn = bias[n];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * 64 + a * 16 + 4 * g + r;
                if (m < M) d.p[(size_t)m * d.ctot + d.c0 + nc] = fmaxf(acc[a][b][r] + bn, 0.f);
            }
    }
}

// ---- pools (NHWC input [B, H, W, C], output into channels [c0, c0 + C) of a Ctot-channel tensor) -------------------
__global__ void __launch_bounds__(256)
fid_pool_kernel(const float* __restrict__ x, int H, int W, int C, int mode, int Ho, int Wo, float* __restrict__ y,
                int yct, int yc0, int total) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const int c = p % C;
    int q = p / C;
    const int ow = q % Wo;
    q /= Wo;
    const int oh = q % Ho, b = q / Ho;
    const float* xb = x + (size_t)b * H * W * C + c;
    float v;
    if (mode == GX_FID_GLOBAL_AVGPOOL) {
        float s = 0.f;
        for (int i = 0; i < H * W; ++i) s += xb[(size_t)i * C];
        v = s / (float)(H * W);
    } else {
        const int hs = mode == GX_FID_MAXPOOL_S2 ? 2 * oh : oh - 1, ws = mode == GX_FID_MAXPOOL_S2 ? 2 * ow : ow - 1;
        const int h0 = max(hs, 0), h1 = min(hs + 3, H), w0 = max(ws, 0), w1 = min(ws + 3, W);
        if (mode == GX_FID_AVGPOOL_S1P1) {
            float s = 0.f;
            for (int h = h0; h < h1; ++h)
                for (int w = w0; w < w1; ++w) s += xb[((size_t)h * W + w) * C];
            v = s / (float)((h1 - h0) * (w1 - w0));
        } else {
            v = -INFINITY;
            for (int h = h0; h < h1; ++h)
                for (int w = w0; w < w1; ++w) v = fmaxf(v, xb[((size_t)h * W + w) * C]);
        }
    }
    y[(((size_t)b * Ho + oh) * Wo + ow) * yct + yc0 + c] = v;
}

// ---- moments: sum[i] += sum_b f[b][i], sumsq[i][j] += sum_b f[b][i] f[b][j] in fp64, images in order ----------------
// (an fp32 x fp32 product is exact in fp64: only the additions round, and each entry adds its images one after the
// other, first to last -- the same bits however the images are split into batches)
__global__ void __launch_bounds__(256)
fid_moments_kernel(const float* __restrict__ f, int B, int D, double* __restrict__ S) {
    __shared__ float fi[32][64], fj[32][64];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty * 4 + a, j = j0 + tx * 4 + c;
            acc[a][c] = (i < D && j < D) ? S[(size_t)i * D + j] : 0.0;
        }
    for (int b0 = 0; b0 < B; b0 += 32) {
        const int nb = min(32, B - b0);
        __syncthreads();
        for (int e = t; e < 32 * 64; e += 256) {
            const int bb = e >> 6, k = e & 63;
            const bool in = bb < nb;
            fi[bb][k] = (in && i0 + k < D) ? f[(size_t)(b0 + bb) * D + i0 + k] : 0.f;
            fj[bb][k] = (in && j0 + k < D) ? f[(size_t)(b0 + bb) * D + j0 + k] : 0.f;
        }
        __syncthreads();
        for (int bb = 0; bb < nb; ++bb) {
            double vi[4], vj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) vi[a] = (double)fi[bb][ty * 4 + a];
#pragma unroll
            for (int c = 0; c < 4; ++c) vj[c] = (double)fj[bb][tx * 4 + c];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] = fma(vi[a], vj[c], acc[a][c]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty * 4 + a, j = j0 + tx * 4 + c;
            if (i < D && j < D) S[(size_t)i * D + j] = acc[a][c];
        }
}

__global__ void __launch_bounds__(256)
fid_sum_kernel(const float* __restrict__ f, int B, int D, double* __restrict__ s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D) return;
    double v = s[i];
    for (int b = 0; b < B; ++b) v += (double)f[(size_t)b * D + i];
    s[i] = v;
}

}  // namespace

extern "C" {

int gx_fid_preprocess(const float* x, float* y, int B, int H, int W, int quantise, gx_stream_t stream) {
    GX_CHECK_ARG(x && y, "gx_fid_preprocess: null pointer");
    GX_CHECK_ARG(B > 0 && H > 0 && W > 0, "gx_fid_preprocess: bad dims");
    GX_CHECK_ARG((long long)B * kFidSide * kFidSide <= INT_MAX - 256, "gx_fid_preprocess: batch too large (%d)", B);
    const int total = B * kFidSide * kFidSide;
    hipLaunchKernelGGL(fid_preprocess_kernel, dim3(gx_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, B,
                       H, W, quantise, (float)H / (float)kFidSide, (float)W / (float)kFidSide);
    GX_CHECK_LAUNCH("gx_fid_preprocess");
    return GX_OK;
}

int gx_fid_conv_bias_relu(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, int kh, int kw,
                          int stride, int ph, int pw, float* d0, int d0_ctot, int d0_c0, int n0, float* d1, int d1_ctot,
                          int d1_c0, int n1, float* d2, int d2_ctot, int d2_c0, int n2, gx_stream_t stream) {
    GX_CHECK_ARG(x && w && bias && d0, "gx_fid_conv_bias_relu: null pointer");
    GX_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && kh > 0 && kw > 0 && stride > 0 && ph >= 0 && pw >= 0,
                 "gx_fid_conv_bias_relu: bad dims");
    GX_CHECK_ARG(n0 > 0 && n1 >= 0 && n2 >= 0 && (n1 > 0 || n2 == 0), "gx_fid_conv_bias_relu: bad part sizes");
    GX_CHECK_ARG(d0_c0 >= 0 && d0_c0 + n0 <= d0_ctot, "gx_fid_conv_bias_relu: destination 0 slice out of range");
    GX_CHECK_ARG(n1 == 0 || (d1 && d1_c0 >= 0 && d1_c0 + n1 <= d1_ctot),
                 "gx_fid_conv_bias_relu: destination 1 slice out of range");
    GX_CHECK_ARG(n2 == 0 || (d2 && d2_c0 >= 0 && d2_c0 + n2 <= d2_ctot),
                 "gx_fid_conv_bias_relu: destination 2 slice out of range");
    const int Hp = H + 2 * ph - kh, Wp = W + 2 * pw - kw;
    GX_CHECK_ARG(Hp >= 0 && Wp >= 0, "gx_fid_conv_bias_relu: kernel larger than the padded input");
    const int Ho = Hp / stride + 1, Wo = Wp / stride + 1;
    const long long M = (long long)B * Ho * Wo;
    const long long K = (long long)kh * kw * Cin;
    GX_CHECK_ARG(M <= INT_MAX - kBM && K <= INT_MAX / 2, "gx_fid_conv_bias_relu: problem too large");
    const int N = n0 + n1 + n2, Kpad = gx_round_up((int)K, kBK);
    const FidDst D0{d0, d0_ctot, d0_c0, n0}, D1{d1, d1_ctot, d1_c0, n1}, D2{d2, d2_ctot, d2_c0, n2};
    const bool vec = Cin % kBK == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const dim3 grid(gx_ceil_div((int)M, kBM), gx_ceil_div(N, kBN));
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(fid_conv_kernel<true>, grid, dim3(256), 0, s, x, H, W, Cin, w, bias, N, (int)K, Kpad, kw, stride,
                           ph, pw, Ho, Wo, (int)M, D0, D1, D2);
    else
        hipLaunchKernelGGL(fid_conv_kernel<false>, grid, dim3(256), 0, s, x, H, W, Cin, w, bias, N, (int)K, Kpad, kw, stride,
                           ph, pw, Ho, Wo, (int)M, D0, D1, D2);
    GX_CHECK_LAUNCH("gx_fid_conv_bias_relu");
    return GX_OK;
}

int gx_fid_pool(const float* x, int B, int H, int W, int C, int mode, float* y, int y_ctot, int y_c0,
                gx_stream_t stream) {
    GX_CHECK_ARG(x && y, "gx_fid_pool: null pointer");
    GX_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, "gx_fid_pool: bad dims");
    GX_CHECK_ARG(mode >= GX_FID_MAXPOOL_S2 && mode <= GX_FID_GLOBAL_AVGPOOL, "gx_fid_pool: unknown mode %d", mode);
    GX_CHECK_ARG(y_c0 >= 0 && y_c0 + C <= y_ctot, "gx_fid_pool: destination slice out of range");
    GX_CHECK_ARG(mode != GX_FID_MAXPOOL_S2 || (H >= 3 && W >= 3), "gx_fid_pool: input smaller than the window");
    int Ho = H, Wo = W;
    if (mode == GX_FID_MAXPOOL_S2) { Ho = (H - 3) / 2 + 1; Wo = (W - 3) / 2 + 1; }
    if (mode == GX_FID_GLOBAL_AVGPOOL) { Ho = 1; Wo = 1; }
    const long long total = (long long)B * Ho * Wo * C;
    GX_CHECK_ARG(total <= INT_MAX - 256, "gx_fid_pool: problem too large");
    hipLaunchKernelGGL(fid_pool_kernel, dim3(gx_ceil_div((int)total, 256)), dim3(256), 0, (hipStream_t)stream, x, H, W, C,
                       mode, Ho, Wo, y, y_ctot, y_c0, (int)total);
    GX_CHECK_LAUNCH("gx_fid_pool");
    return GX_OK;
}

int gx_fid_moments(const float* feats, int B, int D, double* sum, double* sumsq, gx_stream_t stream) {
    GX_CHECK_ARG(feats && sum && sumsq, "gx_fid_moments: null pointer");
    GX_CHECK_ARG(B > 0 && D > 0 && D <= 65536, "gx_fid_moments: bad dims");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fid_sum_kernel, dim3(gx_ceil_div(D, 256)), dim3(256), 0, s, feats, B, D, sum);
    hipLaunchKernelGGL(fid_moments_kernel, dim3(gx_ceil_div(D, 64), gx_ceil_div(D, 64)), dim3(256), 0, s, feats, B, D,
                       sumsq);
    GX_CHECK_LAUNCH("gx_fid_moments");
    return GX_OK;
}

}  // extern "C"
