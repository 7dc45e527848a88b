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
// Cin % 4 == 0 gathers one float4 per thread and step; otherwise (conv1, Cin = 3) four scalar taps.  The tile body and the entry's host side
// (refusals, ConvArgs, grid) are csrc/conv_f32_shared.h's; the max-pool is csrc/pool_shared.h's body, the input stage's pixel conversion csrc/u8_shared.h's.
//
// Distance stage: per pixel n = sqrt(sum_c f_c^2) + 1e-10 for each image, sum_c w_c (f0_c / n0 - f1_c / n1)^2, fp64 throughout and every
// operation rounded on its own (pragma below and -ffp-contract=off).  One wave owns a pixel: lane l adds channels l, l + 64, ...
// ascending, a butterfly adds the 64 lanes; a wave adds its 16 pixels of a 64-pixel tile in ascending order, the four waves are added
// as (w0 + w1) + (w2 + w3); the finish adds a pair's tiles in index order and divides by the pixel count.  No atomics.
#include "common.h"
#include "conv_f32_shared.h"
#include "pool_shared.h"
#include "u8_shared.h"
#include "selftok_hip_ext.h"
#include <stdio.h>

#pragma clang fp contract(off)

namespace selftok {
namespace {

using conv_f32::BN; using conv_f32::KT; using conv_f32::NT; using conv_f32::ConvArgs;
constexpr int MIN_SIDE = 31;

// the convolution of record: conv_f32_shared.h's tile body (__builtin_amdgcn_mfma_f32_32x32x2f32), shared with csrc/fid.hip
template <bool VEC>
__global__ void __launch_bounds__(NT) lpips_conv_kernel(ConvArgs a)
{
    conv_f32::conv_tile<VEC>(a);
}

// channels-last 3 x 3 stride 2 max-pool, floor mode, no padding: pool_shared.h's body (a NaN wins, torch's rule)
__global__ void __launch_bounds__(NT) lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int PH, int PW, long total)
{
    pool::pool_element<3, 2, 0, false>(in, out, H, W, C, PH, PW, C, 0, total);
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
        const float v = load_px<RB>(a.recon, at);
        if (a.quantize) x = (float)px_u8<RB>(v, false) / 255.0f * 2.0f - 1.0f;
        else x = v * 2.0f - 1.0f;
    } else {
        const float v = load_px<OB>(a.orig, at);
        if (a.quantize) x = (float)px_u8<false>(v, a.orig_signed) / 255.0f * 2.0f - 1.0f;
        else x = a.orig_signed ? v : v * 2.0f - 1.0f;
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
    ConvArgs a;
    dim3 grid;
    if (!conv_f32::conv_plan("lpips_conv2d", in, packed, bias, out, N, H, W, Cin, Cout, KH, KW, stride, pad, pad, Cout, 0, relu, &a, &grid)) return SELFTOK_EINVAL;
    if (Cin % 4 == 0) hipLaunchKernelGGL(lpips_conv_kernel<true>, grid, dim3(NT), 0, stream, a);
    else hipLaunchKernelGGL(lpips_conv_kernel<false>, grid, dim3(NT), 0, stream, a);
    return check_launch("lpips_conv_kernel");
}

int selftok_lpips_maxpool3s2_f32(const float* in, float* out, int N, int H, int W, int C, hipStream_t stream)
{
    int PH, PW;
    long total;
    if (!pool::check<3, 2, 0>("lpips_maxpool3s2", in, out, N, H, W, C, C, 0, &PH, &PW, &total)) return SELFTOK_EINVAL;
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
