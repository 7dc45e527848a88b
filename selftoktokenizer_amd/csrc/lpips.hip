// LPIPS (AlexNet backbone, v0.1 linear layers) on the device (include/selftok_hip_ext.h): an fp32 convolution on the f32-input MFMA, a
// 3 x 3 / 2 max-pool, the input stage and the fp64 distance stage.  selftoktokenizer_amd/lpips.py (LPIPS_DEFINITION, LpipsNet) chains
// them; tests/lpips_cases.py restates the arithmetic of record in torch-CPU fp64 / numpy.  Activations are channels-last fp32
// [N, H, W, C]; both images of a pair go through the network as one batch of 2B (recon images first, then the originals).
//
// Convolution (cross-correlation, zero padding) -- the arithmetic of record of lpips_conv_kernel:
//   k = (kh * KW + kw) * Cin + ci (kernel row, kernel column, input channel), a_k the input pixel of tap k or an exact +0.0f where the
//   tap falls into the padding, w_k = weight[co, ci, kh, kw].  The taps are dealt to EIGHT chains: chain j (0 .. 7) takes the taps with
//   (k mod 16) in {2j, 2j + 1}, ascending, c_j = fmaf(a_k, w_k, c_j) from +0.0f -- one accumulator of v_mfma_f32_32x32x2_f32 each, whose
//   result is bit for bit that k-ordered fmaf chain.  Then
//       out[n, oy, ox, co] = act((((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7))) + bias[co])
//   in fp32, the bias added LAST with one addition, then the optional ReLU (v < 0 ? 0 : v, so a NaN stays a NaN).  K is padded with zero
//   taps (a = w = +0.0f) up to a multiple of 16, which leaves every chain's bits alone.  Why eight chains and not one: a single chain of
//   K = 3456 non-negative-input products (conv4) has 2.2 - 3.6 x the rms error of torch's fp32 CPU convolution against fp64, outside
//   the project's standing gate (2 x rms); eight chains of K / 8 have 0.4 - 1.5 x.  Every output element walks
//   the same taps in the same order wherever it falls in a tile and whatever else is in the batch: a function of its own image alone.
// Implicit GEMM: rows = the N * OH * OW output pixels, columns = Cout, depth = K.  One workgroup (256 threads, 4 waves) owns a 64 x 64
// tile, each wave one 32 x 32 accumulator.  Per 16-deep step the im2col tile (64 rows x 16 taps, gathered with a predicate: a padding
// tap or a row past the end is never loaded) and the weight tile (16 x 64 of the packed [KP][CoutP] image, zero-padded by the packer)
// are fetched into registers while the previous step's MFMAs run, then stored k-major to LDS: 2 * 16 * 68 * 4 = 8704 bytes.
// Cin % 4 == 0 gathers one float4 per thread and step; otherwise (conv1, Cin = 3) four scalar taps.
//
// Distance stage: per pixel n = sqrt(sum_c f_c^2) + 1e-10 for each image, sum_c w_c (f0_c / n0 - f1_c / n1)^2, fp64 throughout and every
// operation rounded on its own (pragma below and -ffp-contract=off).  One wave owns a pixel: lane l adds channels l, l + 64, ...
// ascending, a butterfly adds the 64 lanes; a wave adds its 16 pixels of a 64-pixel tile in ascending order, the four waves are added
// as (w0 + w1) + (w2 + w3); the finish adds a pair's tiles in index order and divides by the pixel count.  No atomics.
#include "common.h"
#include "conv_f32_shared.h"
#include "u8_shared.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

using conv_f32::BM; using conv_f32::BN; using conv_f32::KT; using conv_f32::NT; using conv_f32::ConvArgs; using conv_f32::out_side;
constexpr int MIN_SIDE = 31;

// the convolution of record: conv_f32_shared.h's tile body (__builtin_amdgcn_mfma_f32_32x32x2f32), shared with csrc/fid.hip
template <bool VEC>
__global__ void __launch_bounds__(NT) lpips_conv_kernel(ConvArgs a)
{
    conv_f32::conv_tile<VEC>(a);
}

// channels-last 3 x 3 stride 2 max-pool, floor mode, no padding: every window lies inside the image.  A NaN wins (torch's rule).
__global__ void __launch_bounds__(NT) lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int PH, int PW, long total)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long p = i / C;
    const int px = (int)(p % PW); p /= PW;
    const int py = (int)(p % PH);
    const long n = p / PH;
    const float* src = in + (((size_t)n * H + 2 * py) * W + 2 * px) * C + c;
    float m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float v = src[((size_t)dy * W + dx) * C];
            if (v > m || v != v) m = v;
        }
    out[i] = m;
}

struct InputArgs {
    const void* recon; const void* orig; float* out;
    int B, H, W, orig_signed, quantize;
    long total;                                                   // 2B * H * W * 3
};

// [B, 3, H, W] recon (in [0, 1]) and orig -> out [2B, H, W, 3]: the scaling layer's output, images 0 .. B-1 = recon, B .. 2B-1 = orig
template <bool RB, bool OB>
__global__ void __launch_bounds__(NT) lpips_input_kernel(InputArgs a)
{
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= a.total) return;
    const int c = (int)(i % 3);
    long p = i / 3;
    const long hw = (long)a.H * a.W;
    const long pix = p % hw;
    const long n = p / hw;
    const bool is_orig = n >= a.B;
    const size_t at = ((size_t)(is_orig ? n - a.B : n) * 3 + c) * hw + pix;
    float x;
    if (!is_orig) {
        const float v = RB ? bf16_to_f32(((const unsigned short*)a.recon)[at]) : ((const float*)a.recon)[at];
        if (a.quantize) x = (float)to_u8_one<RB>(v) / 255.0f * 2.0f - 1.0f;
        else x = v * 2.0f - 1.0f;
    } else {
        const float v = OB ? bf16_to_f32(((const unsigned short*)a.orig)[at]) : ((const float*)a.orig)[at];
        if (a.quantize) {
            const float o = a.orig_signed ? (v + 1.0f) / 2.0f : v;
            x = (float)to_u8_one<false>(o) / 255.0f * 2.0f - 1.0f;
        } else x = a.orig_signed ? v : v * 2.0f - 1.0f;
    }
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    a.out[i] = (x - shift) / scale;
}

constexpr int DT = 64;                                            // pixels per distance tile, 16 per wave

__device__ __forceinline__ double wave_sum_f64(double v)         // butterfly: every lane ends with the same bits
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// grid (tiles, B): feat [2B, npix, C]; ws[b * tiles + tile] = the tile's sum over its pixels
__global__ void __launch_bounds__(NT) lpips_dist_kernel(const float* __restrict__ feat, const float* __restrict__ w, double* __restrict__ ws, int B, int npix, int C)
{
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, tile = blockIdx.x;
    const float* f0 = feat + (size_t)b * npix * C;
    const float* f1 = feat + (size_t)(b + B) * npix * C;
    double acc = 0.0;
    for (int j = 0; j < DT / 4; ++j) {
        const int p = tile * DT + wave * (DT / 4) + j;            // uniform in the wave
        if (p >= npix) break;
        const float* p0 = f0 + (size_t)p * C;
        const float* p1 = f1 + (size_t)p * C;
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double x = (double)p0[c], y = (double)p1[c];
            s0 += x * x; s1 += y * y;
        }
        const double n0 = sqrt(wave_sum_f64(s0)) + 1e-10, n1 = sqrt(wave_sum_f64(s1)) + 1e-10;
        double t = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double d = (double)p0[c] / n0 - (double)p1[c] / n1;
            t += (double)w[c] * (d * d);
        }
        acc += wave_sum_f64(t);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ws[(size_t)b * gridDim.x + tile] = (part[0] + part[1]) + (part[2] + part[3]);
}

// one thread per pair: its tiles in index order, the spatial mean, added to out[b] when `accumulate`
__global__ void __launch_bounds__(64) lpips_dist_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int B, int tiles, double npix, int accumulate)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += ws[(size_t)b * tiles + i];
    const double v = s / npix;
    out[b] = accumulate ? out[b] + v : v;
}

bool fail(const char* msg) { set_last_error(msg); return false; }

bool conv_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* OH, int* OW)
{
    char msg[256];
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0 || pad >= KH || pad >= KW) {
        snprintf(msg, sizeof msg, "lpips_conv2d: need N, H, W, Cin, Cout, KH, KW, stride >= 1 and 0 <= pad < KH, KW, got N %d, %d x %d, Cin %d, Cout %d, %d x %d, stride %d, pad %d",
                 N, H, W, Cin, Cout, KH, KW, stride, pad);
        return fail(msg);
    }
    *OH = out_side(H, KH, stride, pad); *OW = out_side(W, KW, stride, pad);
    if (*OH < 1 || *OW < 1) {
        snprintf(msg, sizeof msg, "lpips_conv2d: %d x %d input has no output pixel under a %d x %d kernel with pad %d", H, W, KH, KW, pad);
        return fail(msg);
    }
    const long lim = 1l << 31;
    const long kk = (long)KH * KW;
    if (kk >= lim / Cin || (long)H * W >= lim / Cin || (long)N >= lim / ((long)H * W * Cin) || (long)*OH * *OW >= lim / Cout ||
        (long)N >= lim / ((long)*OH * *OW * Cout) || ((kk * Cin + KT - 1) / KT * KT) >= lim / ((Cout + BN - 1) / BN * BN)) {
        snprintf(msg, sizeof msg, "lpips_conv2d: input, output and packed weight element counts must stay below 2^31, got N %d, %d x %d, Cin %d, Cout %d, %d x %d",
                 N, H, W, Cin, Cout, KH, KW);
        return fail(msg);
    }
    return true;
}

}  // namespace
}  // namespace selftok

using namespace selftok;

extern "C" {

size_t selftok_lpips_conv2d_packed_floats(int Cin, int Cout, int KH, int KW)
{
    if (Cin < 1 || Cout < 1 || KH < 1 || KW < 1) { set_last_error("lpips_conv2d_packed_floats: need Cin, Cout, KH, KW >= 1"); return 0; }
    const long KP = ((long)KH * KW * Cin + KT - 1) / KT * KT, CP = ((long)Cout + BN - 1) / BN * BN;
    if (KP >= (1l << 31) / CP) { set_last_error("lpips_conv2d_packed_floats: the packed weight must stay below 2^31 elements"); return 0; }
    return (size_t)(KP * CP);
}

int selftok_lpips_conv2d_f32(const float* in, const float* packed, const float* bias, float* out, int N, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, int relu, hipStream_t stream)
{
    if (!in || !packed || !out) { set_last_error("lpips_conv2d: null pointer"); return SELFTOK_EINVAL; }
    int OH, OW;
    if (!conv_plan(N, H, W, Cin, Cout, KH, KW, stride, pad, &OH, &OW)) return SELFTOK_EINVAL;
    if (((uintptr_t)in & 15) != 0 || ((uintptr_t)packed & 15) != 0 || ((uintptr_t)out & 3) != 0 || ((uintptr_t)bias & 3) != 0) {
        set_last_error("lpips_conv2d: in and packed must be 16-byte aligned, out and bias 4-byte aligned"); return SELFTOK_EINVAL;
    }
    ConvArgs a{in, packed, bias, out, H, W, Cin, OH, OW, Cout, (Cout + BN - 1) / BN * BN, KH, KW, stride, pad, pad, KH * KW * Cin,
               (KH * KW * Cin + KT - 1) / KT * KT, relu != 0, Cout, 0, (long)N * OH * OW};
    const dim3 grid((unsigned)((a.M + BM - 1) / BM), (unsigned)(a.CoutP / BN));
    if (grid.y > 65535u) { set_last_error("lpips_conv2d: Cout above 64 * 65535"); return SELFTOK_EINVAL; }
    if (Cin % 4 == 0) hipLaunchKernelGGL(lpips_conv_kernel<true>, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(lpips_conv_kernel<false>, grid, dim3(NT), 0, stream, a);
    return check_launch("lpips_conv_kernel");
}

int selftok_lpips_maxpool3s2_f32(const float* in, float* out, int N, int H, int W, int C, hipStream_t stream)
{
    if (!in || !out) { set_last_error("lpips_maxpool3s2: null pointer"); return SELFTOK_EINVAL; }
    char msg[200];
    if (N < 1 || C < 1 || H < 3 || W < 3) {
        snprintf(msg, sizeof msg, "lpips_maxpool3s2: need N, C >= 1 and H, W >= 3 (one window), got N %d, %d x %d, C %d", N, H, W, C); set_last_error(msg); return SELFTOK_EINVAL;
    }
    const long lim = 1l << 31;
    if ((long)H * W >= lim / C || (long)N >= lim / ((long)H * W * C)) {
        snprintf(msg, sizeof msg, "lpips_maxpool3s2: N * H * W * C must stay below 2^31, got N %d, %d x %d, C %d", N, H, W, C); set_last_error(msg); return SELFTOK_EINVAL;
    }
    const int PH = (H - 3) / 2 + 1, PW = (W - 3) / 2 + 1;
    const long total = (long)N * PH * PW * C;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, in, out, H, W, C, PH, PW, total);
    return check_launch("lpips_pool_kernel");
}

int selftok_lpips_input(const void* recon, int recon_bf16, const void* orig, int orig_bf16, int orig_signed, int quantize, float* out,
                        int B, int H, int W, hipStream_t stream)
{
    if (!recon || !orig || !out) { set_last_error("lpips_input: null pointer"); return SELFTOK_EINVAL; }
    char msg[200];
    if (B < 1 || H < MIN_SIDE || W < MIN_SIDE) {
        snprintf(msg, sizeof msg, "lpips_input: need B >= 1 and H, W >= 31 (one pixel at every tap), got B %d, %d x %d", B, H, W); set_last_error(msg); return SELFTOK_EINVAL;
    }
    const long hw = (long)H * W;
    if (hw >= (1l << 31) / 6 || (long)B > ((1l << 31) - 1) / (6 * hw)) {
        snprintf(msg, sizeof msg, "lpips_input: 2B * 3 * H * W must stay below 2^31, got B %d, %d x %d", B, H, W); set_last_error(msg); return SELFTOK_EINVAL;
    }
    InputArgs a{recon, orig, out, B, H, W, orig_signed != 0, quantize != 0, 6l * B * hw};
    const dim3 grid((unsigned)((a.total + NT - 1) / NT));
    if (recon_bf16 && orig_bf16) hipLaunchKernelGGL((lpips_input_kernel<true, true>), grid, dim3(NT), 0, stream, a);
    else if (recon_bf16) hipLaunchKernelGGL((lpips_input_kernel<true, false>), grid, dim3(NT), 0, stream, a);
    else if (orig_bf16) hipLaunchKernelGGL((lpips_input_kernel<false, true>), grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL((lpips_input_kernel<false, false>), grid, dim3(NT), 0, stream, a);
    return check_launch("lpips_input_kernel");
}

size_t selftok_lpips_distance_workspace_bytes(int B, int npix)
{
    char msg[160];
    if (B < 1 || npix < 1 || B > 65535) {
        snprintf(msg, sizeof msg, "lpips_distance: need 1 <= B <= 65535 and npix >= 1, got B %d, npix %d", B, npix); set_last_error(msg); return 0;
    }
    return (size_t)B * (size_t)(((long)npix + DT - 1) / DT) * sizeof(double);     // in long: npix may be anything up to INT_MAX here
}

int selftok_lpips_distance(const float* feat, const float* w, double* out, void* workspace, size_t workspace_bytes, int B, int npix, int C,
                           int accumulate, hipStream_t stream)
{
    if (!feat || !w || !out || !workspace) { set_last_error("lpips_distance: null pointer"); return SELFTOK_EINVAL; }
    const size_t need = selftok_lpips_distance_workspace_bytes(B, npix);
    if (!need) return SELFTOK_EINVAL;
    char msg[160];
    if (C < 1 || (long)npix >= (1l << 31) / C || 2l * B >= (1l << 31) / ((long)npix * C)) {
        snprintf(msg, sizeof msg, "lpips_distance: need C >= 1 and 2B * npix * C below 2^31, got B %d, npix %d, C %d", B, npix, C); set_last_error(msg); return SELFTOK_EINVAL;
    }
    if (workspace_bytes < need) { set_last_error("lpips_distance: workspace smaller than selftok_lpips_distance_workspace_bytes"); return SELFTOK_EINVAL; }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)out & 7) != 0) { set_last_error("lpips_distance: workspace and out must be 8-byte aligned"); return SELFTOK_EINVAL; }
    const int tiles = (int)(((long)npix + DT - 1) / DT);
    hipLaunchKernelGGL(lpips_dist_kernel, dim3(tiles, B), dim3(NT), 0, stream, feat, w, (double*)workspace, B, npix, C);
    hipLaunchKernelGGL(lpips_dist_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, (const double*)workspace, out, B, tiles, (double)npix, accumulate != 0);
    return check_launch("lpips_distance kernels");
}

}  // extern "C"
